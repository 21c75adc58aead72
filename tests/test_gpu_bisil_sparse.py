"""The bisilhouette of sparse views on the device: resnmtf_bisil_sparse against resnmtf_bisil on a dense handle holding
the same fp32 values (bitwise), against the plain restatement (bisil_ref), reproducibility, the refusals,
res_nmtf_inner(score_bisil=True, bisil_sparse=True) on a mixed view list and apply_resnmtf's k sweep on sparse views.

Shapes: 150 x 90 -- the row side pads its 150 members to 192 (three 64-wide tiles, the last ragged) and clusters drawn at
p = 0.45 give about 40 features (a second 32-feature LDS stage with a ragged end) -- and a small 40 x 30."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import bisil_ref as B
import resnmtf_amd
from resnmtf_amd import api, naming
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "manhattan", "cosine")
ATOL = 1e-9            # the bar of test_gpu_bisil.py::test_silhouettes_match_restatement
ZERO_ROW, DENSE_ROW, ZERO_COL = 3, 7, 5


def _data(n, m, density, seed):
    """x = where(u > thr, u, 0) with about ``density`` stored, then an all-zero row, a dense row and an all-zero column
    (the dense row stores every entry but the one in that column)."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, m))
    x = np.where(u > 1.0 - density, u, 0.0)
    x[ZERO_ROW, :] = 0.0
    x[DENSE_ROW, :] = 0.5 + 0.5 * u[DENSE_ROW, :]
    x[:, ZERO_COL] = 0.0
    return x


def _clusters(n, m, K, seed, p=0.45):
    """Independent draws at p (overlapping); for K >= 5 bicluster 3 has no rows and bicluster 2 one row.  The zero row
    and the dense row are members and the zero column is a feature of bicluster 0."""
    rng = np.random.default_rng(seed)
    rc = (rng.random((n, K)) < p).astype(np.float64)
    cc = (rng.random((m, K)) < p).astype(np.float64)
    if K >= 5:
        rc[:, 3] = 0.0
        rc[:, 2] = 0.0
        rc[rng.integers(n), 2] = 1.0
    rc[[ZERO_ROW, DENSE_ROW], 0] = 1.0
    cc[ZERO_COL, 0] = 1.0
    return rc, cc


CONFIGS = [  # (n, m, stored share, K, membership probability)
    (150, 90, 0.03, 5, 0.45),
    (150, 90, 0.30, 5, 0.45),
    (150, 90, 0.30, 1, 0.45),
    (150, 90, 0.03, 64, 0.12),     # (K = 64: smaller biclusters keep the restatement's loops short; U is still every row)
    (40, 30, 0.30, 5, 0.45),
    (40, 30, 0.30, 64, 0.25),
]


@functools.lru_cache(maxsize=None)
def _case(ci):
    """One configuration's data and device results, computed once: per metric the sparse handle's silhouettes (twice)
    and the dense handle's, both uploads pre-processed (each stores f32(x))."""
    n, m, density, K, p = CONFIGS[ci]
    x = _data(n, m, density, 40 + ci)
    rc, cc = _clusters(n, m, K, 80 + ci, p)
    xs = sp.csc_matrix(x)
    out = {"x32": x.astype(np.float32).astype(np.float64), "rc": rc, "cc": cc, "sparse": {}, "again": {}, "dense": {}}
    with Engine([n], [m], [2], nnz=[xs.nnz]) as es, Engine([n], [m], [2]) as ed:
        es.set_view_sparse(0, xs, pre_processed=True)
        ed.set_view(0, x)
        for metric in METRICS:
            out["sparse"][metric] = es.bisil_sparse(0, rc, cc, metric)
            out["again"][metric] = es.bisil_sparse(0, rc, cc, metric)
            out["dense"][metric] = ed.bisil(0, rc, cc, metric)
    return out


def test_data_has_the_edge_lines():
    n, m, density = CONFIGS[0][:3]
    x = _data(n, m, density, 40)
    assert not x[ZERO_ROW].any() and not x[:, ZERO_COL].any()
    assert np.count_nonzero(x[DENSE_ROW]) == m - 1
    assert 0.02 < np.count_nonzero(np.delete(x, DENSE_ROW, 0)) / x.size < 0.04
    rc, cc = _clusters(n, m, 5, 80)
    assert rc[:, 3].sum() == 0 and rc[:, 2].sum() == 1 and cc.sum(0).min() > 32


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_bitwise_equal_to_the_dense_path(ci, metric):
    c = _case(ci)
    (rs, cs), (dr, dc) = c["sparse"][metric], c["dense"][metric]
    assert np.array_equal(rs, dr)
    assert np.array_equal(cs, dc)
    if CONFIGS[ci][3] > 1:
        assert rs.any() and cs.any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_silhouettes_match_restatement(ci, metric):
    c = _case(ci)
    rs, cs = c["sparse"][metric]
    wr, wc = B.silhouettes(c["x32"], c["rc"], c["cc"], metric)
    print(f"config {CONFIGS[ci]} {metric}: max |d row| {np.abs(rs - wr).max():.3e}, max |d col| {np.abs(cs - wc).max():.3e}")
    np.testing.assert_allclose(rs, wr, rtol=0, atol=ATOL)
    np.testing.assert_allclose(cs, wc, rtol=0, atol=ATOL)


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_two_calls_are_bitwise_equal(ci):
    c = _case(ci)
    for metric in METRICS:
        a, b = c["sparse"][metric], c["again"][metric]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_refusals():
    n, m = 40, 30
    x = _data(n, m, 0.3, 1)
    rc, cc = _clusters(n, m, 4, 2)
    xs = sp.csc_matrix(x)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                          # noqa: E731
    rs = np.zeros((n, 4), order="F"); cs = np.zeros((m, 4), order="F")
    rcf, ccf = np.asfortranarray(rc), np.asfortranarray(cc)
    with Engine([n], [m], [2]) as e:
        e.set_view(0, x)
        with pytest.raises(ResnmtfError, match="resnmtf_bisil") as ei:              # a dense view
            e.bisil_sparse(0, rc, cc)
        assert ei.value.code == 5
        dense_codes = [e._lib.resnmtf_bisil(e._h, 0, 4, dp(rcf), dp(ccf), 3, dp(rs), dp(cs)),      # unknown metric
                       e._lib.resnmtf_bisil(e._h, 1, 4, dp(rcf), dp(ccf), 0, dp(rs), dp(cs)),      # bad view
                       e._lib.resnmtf_bisil(e._h, 0, 4, None, dp(ccf), 0, dp(rs), dp(cs))]         # NULL
        dense_errors = []
        half = rc.copy(); half[0, 0] = 0.5
        for bad_rc, bad_cc in ((rc[:, :0], cc[:, :0]), (np.ones((n, 65)), np.ones((m, 65))), (half, cc)):
            with pytest.raises(ResnmtfError) as ei:
                e.bisil(0, bad_rc, bad_cc)
            dense_errors.append((ei.value.code, str(ei.value)))
    with Engine([n], [m], [2], nnz=[xs.nnz]) as e:
        with pytest.raises(ResnmtfError, match="no data") as ei:                    # nothing uploaded yet
            e.bisil_sparse(0, rc, cc)
        assert ei.value.code == 5
        e.set_view_sparse(0, xs, pre_processed=True)
        assert [e._lib.resnmtf_bisil_sparse(e._h, 0, 4, dp(rcf), dp(ccf), 3, dp(rs), dp(cs)),
                e._lib.resnmtf_bisil_sparse(e._h, 1, 4, dp(rcf), dp(ccf), 0, dp(rs), dp(cs)),
                e._lib.resnmtf_bisil_sparse(e._h, 0, 4, None, dp(ccf), 0, dp(rs), dp(cs))] == dense_codes == [1, 1, 1]
        for (bad_rc, bad_cc), (code, text) in zip(((rc[:, :0], cc[:, :0]), (np.ones((n, 65)), np.ones((m, 65))), (half, cc)),
                                                  dense_errors):
            with pytest.raises(ResnmtfError) as ei:
                e.bisil_sparse(0, bad_rc, bad_cc)
            assert (ei.value.code, str(ei.value)) == (code, text) and code == 1
        with pytest.raises(ResnmtfError, match="sparse") as ei:                     # the dense entry point, as before
            e.bisil(0, rc, cc)
        assert ei.value.code == 5


def test_workspace_too_large_is_an_error():
    """A 300000 x 300000 view with one bicluster holding everything: the restricted block would be 300000 x 300032
    floats (360 GB, more than the device has).  Refused before any allocation, with the bytes in the message."""
    n = m = 300000
    idx = np.arange(m)
    xs = sp.csc_matrix((np.ones(m), (idx, idx)), shape=(n, m))
    with Engine([n], [m], [2], nnz=[xs.nnz]) as e:
        e.set_view_sparse(0, xs, pre_processed=True)
        with pytest.raises(ResnmtfError, match=r"\d+ bytes asked for") as ei:
            e.bisil_sparse(0, np.ones((n, 1)), np.ones((m, 1)))
        assert ei.value.code == 4
        asked = int(str(ei.value).split(" bytes asked for")[0].split()[-1])
        assert asked >= n * 300032 * 4
        rs, cs = e.bisil_sparse(0, np.ones((n, 1)), np.zeros((m, 1)))               # the handle still works (inactive: zeros)
        assert not rs.any() and not cs.any()


def _blocks(seed, n, m, k, noise=0.05):
    """k planted blocks of height 1 + noise, on disjoint row and column ranges."""
    rng = np.random.default_rng(seed)
    rl = np.arange(n) * k // n; cl = np.arange(m) * k // m
    return (rl[:, None] == cl[None, :]) * 1.0 + noise * rng.random((n, m))


def test_res_nmtf_inner_scores_a_mixed_view_list():
    x1 = _blocks(1, 60, 40, 3); x1[x1 < 0.5] = 0.0          # sparse view: the blocks only
    x2 = _blocks(2, 60, 30, 3)                              # dense view, rows shared with view 0
    data = naming.check_data([sp.csc_matrix(x1), x2])
    rn, cn = naming.give_names(data, None, None, None, None)
    kw = dict(k_vec=[3, 3], spurious=False, row_names=rn, col_names=cn, seed=5, n_iters=30, score_bisil=True)
    with pytest.raises(NotImplementedError, match="sparse"):                        # without the opt-in: as before
        api.res_nmtf_inner(data, naming.shared_names(rn), naming.shared_names(cn), **kw)
    for metric in ("euclidean", "cosine"):
        res = api.res_nmtf_inner(data, naming.shared_names(rn), naming.shared_names(cn), distance=metric,
                                 bisil_sparse=True, **kw)
        x32 = [np.asarray(d.toarray() if sp.issparse(d) else d).astype(np.float32).astype(np.float64) for d in data]
        want = B.bisil(x32, res["row_clusters"], res["col_clusters"], metric)
        print(f"{metric}: bisil {res['bisil']!r}, restated {want!r}")
        assert res["bisil"] == pytest.approx(want, abs=ATOL)
        assert res["bisil"] != 0.0


def planted(seed):
    """test-resnmtf.R:38-52: three 60 x 60 blocks of height 10 + 0.1 |N(0, 1)| (as in test_gpu_bisil.py)."""
    rng = np.random.default_rng(seed)
    rc = np.zeros((180, 3)); cc = np.zeros((180, 3))
    for i in range(3):
        rc[i * 60:(i + 1) * 60, i] = 1
        cc[i * 60:(i + 1) * 60, i] = 1
    return rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + 0.1 * np.abs(rng.normal(size=(180, 180)))


def test_k_sweep_on_sparse_views():
    data = []
    for seed in (1, 2):
        x = planted(seed)
        data.append(sp.csc_matrix(np.where(x > 0.2, x, 0.0)))        # the blocks and the noise above two sigma
    kw = dict(k_max=5, spurious=False, stability=False, k_sweep=True, return_sweep=True, seed=3, n_iters=40)
    with pytest.raises(NotImplementedError, match="sparse"):          # without the opt-in: as before
        resnmtf_amd.apply_resnmtf(data, **kw)
    res = resnmtf_amd.apply_resnmtf(data, bisil_sparse=True, **kw)
    sweep = res["k_sweep"]
    print("k sweep on sparse views:", sweep)
    assert sweep["k"][:3] == [3, 4, 5]
    assert np.isfinite(sweep["bisil"]).all()
    k = sweep["k"][int(np.argmax(sweep["bisil"]))]
    assert [f.shape[1] for f in res["output_f"]] == [k, k]
    assert res["bisil"] == max(sweep["bisil"])
    x32 = [d.toarray().astype(np.float32).astype(np.float64) for d in naming.check_data(data)]
    want = B.bisil(x32, res["row_clusters"], res["col_clusters"], "euclidean")
    print(f"bisil {res['bisil']!r}, restated {want!r}")
    assert res["bisil"] == pytest.approx(want, abs=ATOL)
