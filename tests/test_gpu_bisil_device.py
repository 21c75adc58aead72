"""The bisilhouette from cluster matrices in device memory (resnmtf_bisil_device) and the steps after
the loop without downloads (post_on_device=True).

The silhouettes are compared with Engine.bisil / Engine.bisil_sparse on the same clusters on bytes, the returned score
with bisil.view_score (NumPy) of the host entry's silhouettes with ==: the reference is never the code under test.
Shapes are the smallest that reach every form: k = 1, 17 and 64 (bit 63), |U| on both sides of the 64-wide tile, member
counts on both sides of NumPy's 8-entry and 128-entry summation edges."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import resnmtf_amd
from resnmtf_amd import _lib, api, bisil, naming, spurious
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "manhattan", "cosine")
DEV = torch.device("cuda", 0)


def _members(rng, n, count):
    col = np.zeros(n)
    col[rng.choice(n, count, replace=False)] = 1.0
    return col


def _with_union(n, m, K, union, seed):
    """K biclusters whose rows have a union of exactly ``union`` points (every one active)."""
    rng = np.random.default_rng(seed)
    rc = np.zeros((n, K)); cc = (rng.random((m, K)) < 0.4).astype(np.float64)
    pts = np.sort(rng.choice(n, union, replace=False))
    rc[pts, rng.integers(K, size=union)] = 1.0
    rc[pts[:K], np.arange(K)] = 1.0                        # (no bicluster without a row)
    rc[pts[::7], 0] = 1.0                                   # (overlaps)
    cc[rng.integers(m, size=K), np.arange(K)] = 1.0
    assert (rc.sum(1) > 0).sum() == union
    return rc, cc


def _case(name):
    """(x, rc, cc) of one dense case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "k5_edges":                                  # an empty bicluster, a singleton, two overlapping, points in none
        n, m, K = 150, 90, 5
        rc = (rng.random((n, K)) < 0.3).astype(np.float64); cc = (rng.random((m, K)) < 0.3).astype(np.float64)
        rc[:, 3] = 0.0
        rc[:, 2] = 0.0; rc[17, 2] = 1.0
        rc[:40, 0] = 1.0; rc[20:60, 1] = 1.0
        rc[140:] = 0.0; cc[80:] = 0.0
    elif name == "k1":
        n, m, K = 70, 130, 1
        rc = (rng.random((n, K)) < 0.5).astype(np.float64); cc = (rng.random((m, K)) < 0.5).astype(np.float64)
    elif name == "k17":
        n, m, K = 200, 64, 17
        rc = (rng.random((n, K)) < 0.2).astype(np.float64); cc = (rng.random((m, K)) < 0.2).astype(np.float64)
    elif name == "k64":                                     # bicluster 63 active: the top bit of the membership word
        n, m, K = 130, 70, 64
        rc = (rng.random((n, K)) < 0.1).astype(np.float64); cc = (rng.random((m, K)) < 0.1).astype(np.float64)
        rc[5:9, 63] = 1.0; cc[3:6, 63] = 1.0
    elif name.startswith("union"):
        n, m, K = 200, 50, 3
        rc, cc = _with_union(n, m, K, int(name[5:]), 7)
    elif name == "numpy_edges":                             # member counts on NumPy's summation edges
        n, m = 330, 40
        counts = (7, 8, 9, 128, 129, 300)
        K = len(counts)
        rc = np.stack([_members(rng, n, c) for c in counts], axis=1)
        cc = np.stack([_members(rng, m, c) for c in (7, 8, 9, 12, 5, 30)], axis=1)
    else:
        raise KeyError(name)
    x = rng.random((n, m)) * (rng.random((n, m)) < 0.8)
    return x, rc, cc


CASES = ("k5_edges", "k1", "k17", "k64", "union64", "union65", "union128", "numpy_edges")


def _forms(a, stream):
    """``a`` as the four kinds of tensor, each produced on ``stream`` (a NaN fill first: a read that does not wait for the
    stream sees it): fp64 contiguous, fp32 viewed transposed, fp16, bf16 sliced with a row stride of 2."""
    host = torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    n, k = a.shape
    with torch.cuda.stream(stream):
        src = host.to(DEV, non_blocking=True)
        f64 = torch.full((n, k), float("nan"), dtype=torch.float64, device=DEV); f64.copy_(src)
        f32t = torch.full((k, n), float("nan"), dtype=torch.float32, device=DEV); f32t.copy_(src.T)
        f16 = torch.full((n, k), float("nan"), dtype=torch.float16, device=DEV); f16.copy_(src)
        wide = torch.full((2 * n, k), float("nan"), dtype=torch.bfloat16, device=DEV); wide[::2].copy_(src)
    return {"f64": f64, "f32T": f32t.T, "f16": f16, "bf16_strided": wide[::2]}


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", CASES)
def test_bitwise_against_the_host_entry_dense(name):
    x, rc, cc = _case(name)
    n, m = x.shape
    side = torch.cuda.Stream(DEV)
    probe = _forms(rc, side)
    assert probe["f32T"].stride(0) == 1 and probe["bf16_strided"].stride(0) == 2 * rc.shape[1] and probe["f64"].is_contiguous()
    with Engine([n], [m], [2]) as e:
        e.set_view(0, x)
        for metric in METRICS:
            want_r, want_c = e.bisil(0, rc, cc, metric)
            want = bisil.view_score(rc, cc, want_r, want_c)
            for form in ("f64", "f32T", "f16", "bf16_strided"):
                with torch.cuda.stream(side):
                    trc, tcc = _forms(rc, side)[form], _forms(cc, side)[form]
                    rs, cs, score = e.bisil_device(0, trc, tcc, metric)
                assert rs.dtype == torch.float64 and tuple(rs.shape) == rc.shape and rs.stride() == (1, n)
                print(f"{name} {metric} {form}: score {score!r}, view_score {want!r}")
                assert _bytes(rs.T) == np.ascontiguousarray(want_r.T).tobytes(), (metric, form)
                assert _bytes(cs.T) == np.ascontiguousarray(want_c.T).tobytes(), (metric, form)
                assert score == want, (metric, form)
        if rc.shape[1] > 1 and name != "k1":
            assert want != 0.0


def _sparse_data(n, m, density, seed):
    """About ``density`` stored, an all-zero member row (3), a dense row (7) and an all-zero column (5)."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, m))
    x = np.where(u > 1.0 - density, u, 0.0)
    x[3, :] = 0.0
    x[7, :] = 0.5 + 0.5 * u[7, :]
    x[:, 5] = 0.0
    return x


@pytest.mark.parametrize("n,m,density", [(150, 90, 0.03), (40, 30, 0.30)])
def test_sparse_views_bitwise(n, m, density):
    x = _sparse_data(n, m, density, 40 + n)
    rng = np.random.default_rng(80 + n)
    K = 5
    rc = (rng.random((n, K)) < 0.45).astype(np.float64); cc = (rng.random((m, K)) < 0.45).astype(np.float64)
    rc[:, 3] = 0.0
    rc[:, 2] = 0.0; rc[11, 2] = 1.0
    rc[[3, 7], 0] = 1.0; cc[5, 0] = 1.0
    xs = sp.csc_matrix(x)
    trc, tcc = torch.as_tensor(rc, device=DEV), torch.as_tensor(cc, device=DEV)
    with Engine([n], [m], [2], nnz=[xs.nnz]) as es, Engine([n], [m], [2]) as ed:
        es.set_view_sparse(0, xs, pre_processed=True)
        ed.set_view(0, x)
        for metric in METRICS:
            want_r, want_c = es.bisil_sparse(0, rc, cc, metric)
            want = bisil.view_score(rc, cc, want_r, want_c)
            rs, cs, score = es.bisil_device(0, trc, tcc, metric)
            dr, dc, dscore = ed.bisil_device(0, trc, tcc, metric)
            for got_r, got_c in ((rs, cs), (dr, dc)):
                assert _bytes(got_r.T) == np.ascontiguousarray(want_r.T).tobytes(), metric
                assert _bytes(got_c.T) == np.ascontiguousarray(want_c.T).tobytes(), metric
            assert score == want and dscore == want and want != 0.0, metric


def test_degenerate_cases():
    x, rc, cc = _case("k5_edges")
    n, m = x.shape
    with Engine([n], [m], [2]) as e:
        e.set_view(0, x)
        # no active bicluster: rows without columns
        none_r, none_c = rc.copy(), np.zeros_like(cc)
        rs, cs, score = e.bisil_device(0, torch.as_tensor(none_r, device=DEV), torch.as_tensor(none_c, device=DEV))
        assert score == 0.0 and not rs.any().item() and not cs.any().item()
        assert e.bisil_device(0, torch.as_tensor(none_r, device=DEV), torch.as_tensor(none_c, device=DEV),
                              silhouettes=False) == (None, None, 0.0)
        # exactly one active bicluster: score 0, the silhouettes of the host route
        one_r, one_c = np.zeros_like(rc), np.zeros_like(cc)
        one_r[:, 1] = rc[:, 1]; one_c[:, 1] = cc[:, 1]; one_r[:, 4] = rc[:, 4]
        want_r, want_c = e.bisil(0, one_r, one_c)
        rs, cs, score = e.bisil_device(0, torch.as_tensor(one_r, device=DEV), torch.as_tensor(one_c, device=DEV))
        assert score == 0.0 == bisil.view_score(one_r, one_c, want_r, want_c)
        assert _bytes(rs.T) == np.ascontiguousarray(want_r.T).tobytes() and _bytes(cs.T) == np.ascontiguousarray(want_c.T).tobytes()
        # silhouettes=False returns the same score; two calls are bitwise equal
        trc, tcc = torch.as_tensor(rc, device=DEV), torch.as_tensor(cc, device=DEV)
        a = e.bisil_device(0, trc, tcc, "cosine")
        b = e.bisil_device(0, trc, tcc, "cosine")
        only = e.bisil_device(0, trc, tcc, "cosine", silhouettes=False)
        assert only[0] is None and only[1] is None and only[2] == a[2] == b[2] and a[2] != 0.0
        assert _bytes(a[0]) == _bytes(b[0]) and _bytes(a[1]) == _bytes(b[1])


def _sentinels(n, m, k):
    return torch.full((k, n), 7.0, dtype=torch.float64, device=DEV).T, torch.full((k, m), 7.0, dtype=torch.float64, device=DEV).T


def _untouched(out):
    return all(bool((t == 7.0).all().item()) for t in out)


def test_refusals_leave_the_outputs_untouched():
    n, m, K = 40, 30, 4
    rng = np.random.default_rng(3)
    x = rng.random((n, m))
    rc = (rng.random((n, K)) < 0.5).astype(np.float64); cc = (rng.random((m, K)) < 0.5).astype(np.float64)
    trc, tcc = torch.as_tensor(rc, device=DEV), torch.as_tensor(cc, device=DEV)
    with Engine([n], [m], [2]) as e:
        e.set_view(0, x)
        for bad in (0.5, 2.0, float("nan")):
            for bad_r, bad_c, text in ((True, False, "row_clusters entries must be 0 or 1"),
                                       (False, True, "col_clusters entries must be 0 or 1"),
                                       (True, True, "row_clusters entries must be 0 or 1")):
                r2, c2 = trc.clone(), tcc.clone()
                if bad_r:
                    r2[n - 1, K - 1] = bad
                if bad_c:
                    c2[0, 0] = bad
                out = _sentinels(n, m, K)
                with pytest.raises(ResnmtfError, match=text) as ei:
                    e.bisil_device(0, r2, c2, out=out)
                assert ei.value.code == 1 and _untouched(out), (bad, bad_r, bad_c)
        # -0.0 is 0
        r2 = trc.clone(); r2[r2 == 0] = -0.0
        a, b = e.bisil_device(0, r2, tcc), e.bisil_device(0, trc, tcc)
        assert a[2] == b[2] and _bytes(a[0]) == _bytes(b[0]) and _bytes(a[1]) == _bytes(b[1])
        # straight at the C entry: a host pointer, k = 0, k = 65, a bad metric, NULL descriptors
        out = _sentinels(n, m, K)
        score = C.c_double(-1.0)
        host = np.asfortranarray(rc)
        dm = lambda t: _lib.DeviceMatrix(t.data_ptr(), _lib.DTYPE_F64, int(t.stride(0)), int(t.stride(1)))       # noqa: E731
        on_host = _lib.DeviceMatrix(host.ctypes.data, _lib.DTYPE_F64, 1, n)

        def call(k, d_r, d_c, metric):
            rc_ = e._lib.resnmtf_bisil_device(e._h, 0, k, None if d_r is None else C.byref(d_r), C.byref(d_c), metric,
                                              C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), C.byref(score), None)
            return rc_, (e._lib.resnmtf_last_error(e._h) or b"").decode()

        for args, text in (((K, on_host, dm(tcc), 0), "not device memory"), ((0, dm(trc), dm(tcc), 0), r"k must be in \[1, 64\]"),
                           ((65, dm(trc), dm(tcc), 0), r"k must be in \[1, 64\]"), ((K, dm(trc), dm(tcc), 3), "metric must be"),
                           ((K, None, dm(tcc), 0), "NULL"),
                           ((K, _lib.DeviceMatrix(trc.data_ptr(), 9, K, 1), dm(tcc), 0), "unknown dtype"),
                           ((K, _lib.DeviceMatrix(trc.data_ptr(), _lib.DTYPE_F64, -K, 1), dm(tcc), 0), "negative strides")):
            code, msg = call(*args)
            assert code == 1 and re.search(text, msg), (args[0], msg)
            assert _untouched(out) and score.value == -1.0
        with pytest.raises(ResnmtfError, match=r"k must be in \[1, 64\]"):
            e.bisil_device(0, torch.ones((n, 65), device=DEV), torch.ones((m, 65), device=DEV))
        with pytest.raises(ValueError, match="distance"):
            e.bisil_device(0, trc, tcc, "chebyshev")
        # wrong shapes, a host matrix, an integer tensor: Python errors before any device call
        with pytest.raises(ValueError, match="row clusters must be 40 x k"):
            e.bisil_device(0, trc[:-1], tcc)
        with pytest.raises(ValueError, match="column clusters of shape"):
            e.bisil_device(0, trc, tcc[:, :-1])
        with pytest.raises(ValueError, match="lives on cpu"):
            e.bisil_device(0, trc.cpu(), tcc)
        with pytest.raises(TypeError, match="torch.Tensors"):
            e.bisil_device(0, rc, tcc)
        with pytest.raises(ValueError, match="fp64, fp32, fp16 or bf16"):
            e.bisil_device(0, trc.long(), tcc)
    with Engine([n], [m], [2]) as e:                      # a view without data
        out = _sentinels(n, m, K)
        with pytest.raises(ResnmtfError, match="no data") as ei:
            e.bisil_device(0, trc, tcc, out=out)
        assert ei.value.code == 5 and _untouched(out)


def test_a_tensor_on_another_device_is_refused():
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    n, m, K = 40, 30, 4
    other = torch.device("cuda", 1)
    with Engine([n], [m], [2]) as e:
        e.set_view(0, np.random.default_rng(0).random((n, m)))
        with pytest.raises(ValueError, match="lives on cuda:1"):
            e.bisil_device(0, torch.ones((n, K), device=other, dtype=torch.float64), torch.ones((m, K), device=DEV, dtype=torch.float64))
        t_r, t_c = torch.ones((n, K), device=other, dtype=torch.float64), torch.ones((m, K), device=DEV, dtype=torch.float64)
        score = C.c_double(-1.0)
        d = [_lib.DeviceMatrix(t.data_ptr(), _lib.DTYPE_F64, K, 1) for t in (t_r, t_c)]
        assert e._lib.resnmtf_bisil_device(e._h, 0, K, C.byref(d[0]), C.byref(d[1]), 0, None, None, C.byref(score), None) == 1
        assert "not device memory" in e._lib.resnmtf_last_error(e._h).decode()


# ---- the pipeline: post_on_device=True against the same call without it

def planted(seed, noise=0.1):
    """test-resnmtf.R:38-52: three 60 x 60 blocks of height 10 + noise |N(0, 1)| (as in test_gpu_spurious_pipeline.py)."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1))); cc = np.kron(np.eye(3), np.ones((60, 1)))
    return rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + noise * np.abs(rng.normal(size=(180, 180)))


def _same(a, b, path="result"):
    """Key for key, bit for bit: tensors by dtype, shape, device and values, arrays on bytes, numbers with ==."""
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), (path, list(a), list(b))
        for key in a:
            _same(a[key], b[key], f"{path}[{key!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and a.stride() == b.stride(), path
        assert _bytes(a) == _bytes(b), path
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path
    else:
        assert a == b or (a != a and b != b), (path, a, b)


@pytest.fixture
def no_downloads(monkeypatch):
    """Engine.finalise / get_factors / bisil / bisil_sparse raise while armed."""
    state = {"armed": False}
    for name in ("finalise", "get_factors", "bisil", "bisil_sparse"):
        real = getattr(Engine, name)

        def guarded(self, *args, _real=real, _name=name, **kw):
            assert not state["armed"], f"Engine.{_name} was called with post_on_device=True"
            return _real(self, *args, **kw)
        monkeypatch.setattr(Engine, name, guarded)
    return state


def _both(fn, state):
    state["armed"] = True
    try:
        got = fn(post_on_device=True)
    finally:
        state["armed"] = False
    return got, fn()


def _inner_args(data):
    rn, cn = naming.give_names(data, None, None, None, None)
    pre = naming.check_data(data)
    return pre, naming.shared_names(rn), naming.shared_names(cn), rn, cn


@pytest.mark.parametrize("remove", [False, "planted", "forced"])
def test_res_nmtf_inner_post_on_device_equals_the_host_steps(no_downloads, monkeypatch, remove):
    """Without the removal; with it on the planted problem under heavy noise (five biclusters asked of three, the real
    check: it may flag none); and with a check that flags one F column per view whatever the data (``forced``: the same
    stand-in scores for both calls), so that columns are zeroed on the device and the cleaned tensors are scored."""
    noise = 1.5 if remove == "planted" else 0.1
    pre, ri, ci, rn, cn = _inner_args([planted(1, noise), planted(2, noise)])
    ts = [torch.as_tensor(x, device=DEV) for x in pre]
    k = 5 if remove == "planted" else 3
    if remove == "forced":
        check = {"score": np.array([[0.0, 0.5, 0.6], [0.7, 0.05, 0.5]]), "avg_threshold": np.array([0.2, 0.2]),
                 "max_threshold": np.array([0.1, 0.1])}
        monkeypatch.setattr(spurious, "check_on_device", lambda eng, *args, **kw: {key: val.copy() for key, val in check.items()})
    kw = dict(k_vec=[k, k], row_names=rn, col_names=cn, seed=11, n_iters=40, score_bisil=True, output="torch",
              spurious=bool(remove), spurious_on_device=bool(remove), num_repeats=3)
    got, want = _both(lambda **more: api.res_nmtf_inner(ts, ri, ci, **kw, **more), no_downloads)
    _same(got, want)
    assert isinstance(got["row_clusters"][0], torch.Tensor) and isinstance(got["lambda"][0], np.ndarray)
    if remove:
        removed = got["spurious"]["removed"]
        print(remove, "removed:", removed.sum(axis=1).tolist(), "bisil", got["bisil"])
        for v in range(2):
            for key in ("row_clusters", "col_clusters"):
                assert not got[key][v][:, torch.as_tensor(np.flatnonzero(removed[v]), device=DEV)].any().item()
    if remove == "forced":
        assert removed.sum(axis=1).tolist() == [1, 1]
    if remove != "planted":
        assert got["bisil"] != 0.0


def test_k_sweep_post_on_device_equals_the_host_steps(no_downloads):
    ts = [torch.as_tensor(planted(s), device=DEV) for s in (1, 2)]
    kw = dict(k_sweep=True, k_min=3, k_max=4, stability=False, spurious=False, output="torch", seed=3, n_iters=40, return_sweep=True)
    got, want = _both(lambda **more: resnmtf_amd.apply_resnmtf(ts, **kw, **more), no_downloads)
    _same(got, want)
    assert len(got["k_sweep"]["k"]) >= 2 and all(s != 0.0 for s in got["k_sweep"]["bisil"])


def test_mixed_sparse_and_dense_views_post_on_device(no_downloads):
    x1 = planted(1); x1[x1 < 0.5] = 0.0                    # sparse view: the blocks only
    data = naming.check_data([sp.csc_matrix(x1), planted(2)])
    rn, cn = naming.give_names(data, None, None, None, None)
    kw = dict(k_vec=[3, 3], spurious=False, row_names=rn, col_names=cn, seed=5, n_iters=30, score_bisil=True,
              bisil_sparse=True, output="torch")
    got, want = _both(lambda **more: api.res_nmtf_inner(data, naming.shared_names(rn), naming.shared_names(cn), **kw, **more),
                      no_downloads)
    _same(got, want)
    assert got["bisil"] != 0.0


def test_post_on_device_needs_torch_output():
    x = planted(1)
    with pytest.raises(ValueError, match="post_on_device=True needs output='torch'"):
        resnmtf_amd.apply_resnmtf([x], k_val=3, stability=False, spurious=False, post_on_device=True)
    pre, ri, ci, rn, cn = _inner_args([x])
    with pytest.raises(ValueError, match="post_on_device=True needs output='torch'"):
        api.res_nmtf_inner(pre, ri, ci, k_vec=[3], spurious=False, row_names=rn, col_names=cn, post_on_device=True)
