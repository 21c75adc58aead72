"""The bisilhouette on the device: resnmtf_bisil against the plain restatement (bisil_ref) on the device's own fp32
copy of the data, bitwise reproducibility, the refusals, res_nmtf_inner(score_bisil=True) and the reference's test
"resnmtf runs with k not specified" (tests/testthat/test-resnmtf.R:123-135) through apply_resnmtf(k_sweep=True)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import bisil_ref as B
import resnmtf_amd
from resnmtf_amd import api, bisil, naming
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _clusters(rng, n, m, K, p, empty=(), singleton=()):
    rc = (rng.random((n, K)) < p).astype(np.float64)
    cc = (rng.random((m, K)) < p).astype(np.float64)
    for j in empty:
        rc[:, j] = 0.0
    for j in singleton:
        rc[:, j] = 0.0
        rc[rng.integers(n), j] = 1.0
    return rc, cc


def _view(rng, n, m):
    return rng.random((n, m)) ** 2


CASES = [  # (n, m, K, membership probability, empty biclusters, singleton biclusters)
    (77, 45, 1, 0.5, (), ()),
    (150, 97, 3, 0.3, (), ()),            # overlapping (independent draws)
    (201, 130, 17, 0.15, (4, 9), (2,)),
    (130, 97, 64, 0.06, (0, 33), (5,)),
]


@pytest.mark.parametrize("metric", ["euclidean", "manhattan", "cosine"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_silhouettes_match_restatement(case, metric):
    n, m, K, p, empty, single = CASES[case]
    rng = np.random.default_rng(100 + case)
    x = _view(rng, n, m)
    if metric == "cosine":
        x[3, :] = 0.0                      # a zero row: zero norms on every column set
    rc, cc = _clusters(rng, n, m, K, p, empty, single)
    with Engine([n], [m], [2]) as e:
        e.set_view(0, x)
        xd = e.get_view(0)
        rs, cs = e.bisil(0, rc, cc, metric)
    wr, wc = B.silhouettes(xd, rc, cc, metric)
    np.testing.assert_allclose(rs, wr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(cs, wc, rtol=0, atol=1e-9)
    assert bisil.view_score(rc, cc, rs, cs) == pytest.approx(B.view_score(rc, cc, wr, wc), abs=1e-9)


def test_two_calls_are_bitwise_equal():
    rng = np.random.default_rng(7)
    x = _view(rng, 300, 140)
    rc, cc = _clusters(rng, 300, 140, 20, 0.2)
    with Engine([300], [140], [2]) as e:
        e.set_view(0, x)
        for metric in ("euclidean", "manhattan", "cosine"):
            a = e.bisil(0, rc, cc, metric)
            b = e.bisil(0, rc, cc, metric)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_c2_shape_euclidean_spot_checks():
    """c2's shape (10000 x 2000), k = 3 planted blocks with overlap: every member's silhouette is computed on the
    device; 48 members per side are recomputed by the restatement."""
    rng = np.random.default_rng(11)
    n, m, K = 10000, 2000, 3
    rl = rng.integers(0, K, n); cl = rng.integers(0, K, m)
    rc = np.eye(K)[rl]; cc = np.eye(K)[cl]
    rc[rng.random(n) < 0.05, 0] = 1.0                    # some rows in two biclusters
    x = 0.2 * rng.random((n, m)) + 2.0 * (np.eye(K)[rl] @ np.eye(K)[cl].T)
    with Engine([n], [m], [2]) as e:
        e.set_view(0, x)
        xd = e.get_view(0)
        rs, cs = e.bisil(0, rc, cc, "euclidean")
    rows, cols = B.index_sets(rc, cc)
    for k in range(K):
        for i in rng.choice(rows[k], 16, replace=False):
            assert abs(rs[i, k] - B.member_silhouette(xd, rows, cols, k, i, "euclidean")) < 1e-9
        for j in rng.choice(cols[k], 16, replace=False):
            assert abs(cs[j, k] - B.member_silhouette(xd.T, cols, rows, k, j, "euclidean")) < 1e-9
    assert (rs[rc == 0] == 0).all() and (cs[cc == 0] == 0).all()
    assert bisil.view_score(rc, cc, rs, cs) > 0.5        # planted blocks separate well


def test_refusals():
    rng = np.random.default_rng(3)
    x = _view(rng, 40, 30)
    rc, cc = _clusters(rng, 40, 30, 4, 0.4)
    with Engine([40], [30], [2]) as e:
        e.set_view(0, x)
        for bad_rc, bad_cc in ((rc[:, :0], cc[:, :0]), (np.ones((40, 65)), np.ones((30, 65)))):
            with pytest.raises(ResnmtfError, match="k must be in") as ei:
                e.bisil(0, bad_rc, bad_cc)
            assert ei.value.code == 1
        half = rc.copy(); half[0, 0] = 0.5
        with pytest.raises(ResnmtfError, match="0 or 1"):
            e.bisil(0, half, cc)
        two = cc.copy(); two[1, 1] = 2.0
        with pytest.raises(ResnmtfError, match="0 or 1"):
            e.bisil(0, rc, two)
        rs = np.zeros((40, 4), order="F"); cs = np.zeros((30, 4), order="F")
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                          # noqa: E731
        rcf, ccf = np.asfortranarray(rc), np.asfortranarray(cc)
        assert e._lib.resnmtf_bisil(e._h, 0, 4, dp(rcf), dp(ccf), 3, dp(rs), dp(cs)) == 1     # unknown metric
        assert e._lib.resnmtf_bisil(e._h, 1, 4, dp(rcf), dp(ccf), 0, dp(rs), dp(cs)) == 1     # bad view
        assert e._lib.resnmtf_bisil(e._h, 0, 4, None, dp(ccf), 0, dp(rs), dp(cs)) == 1        # NULL
    xs = sp.csc_matrix(np.where(x > 0.3, x, 0.0))
    with Engine([40], [30], [2], nnz=[xs.nnz]) as e:
        e.set_view_sparse(0, xs, pre_processed=True)
        with pytest.raises(ResnmtfError, match="sparse") as ei:
            e.bisil(0, rc, cc)
        assert ei.value.code == 5


def planted(seed):
    """test-resnmtf.R:38-52: three 60 x 60 blocks of height 10 + 0.1 |N(0, 1)|."""
    rng = np.random.default_rng(seed)
    rc = np.zeros((180, 3)); cc = np.zeros((180, 3))
    for i in range(3):
        rc[i * 60:(i + 1) * 60, i] = 1
        cc[i * 60:(i + 1) * 60, i] = 1
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + 0.1 * np.abs(rng.normal(size=(180, 180)))
    return x, rc, cc


def test_k_not_specified():
    """test-resnmtf.R:123-135 ("resnmtf runs with k not specified"), through the k sweep."""
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    data = [x1, x2]
    res = resnmtf_amd.apply_resnmtf(data, k_max=5, spurious=False, stability=False, k_sweep=True, return_sweep=True,
                                    seed=3)
    assert len(res["output_f"]) == 2 and res["output_f"][0].shape == (180, 3)
    for v in range(2):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))
    sweep = res["k_sweep"]
    assert sweep["k"][:3] == [3, 4, 5]
    assert res["bisil"] == max(sweep["bisil"])
    assert sweep["k"][int(np.argmax(sweep["bisil"]))] == 3
    # the same k and seed through res_nmtf_inner(score_bisil=True)
    rn, cn = naming.give_names(data, None, None, None, None)
    one = api.res_nmtf_inner(naming.check_data(data), naming.shared_names(rn), naming.shared_names(cn), k_vec=[3, 3],
                             spurious=False, row_names=rn, col_names=cn, seed=3 + 3, score_bisil=True)
    assert one["bisil"] == res["bisil"]
    for key in ("Error", "lambda", "mu"):
        assert key in res
    # the default leaves bisil unset
    assert api.res_nmtf_inner(naming.check_data(data), naming.shared_names(rn), naming.shared_names(cn), k_vec=[3, 3],
                              spurious=False, row_names=rn, col_names=cn, seed=6, n_iters=5)["bisil"] is None
