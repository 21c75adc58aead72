"""Host side of sparse views in the device-wide fp64 path (no GPU): the two structs and
signatures, the opt-ins of batched.run_job_fp64 and api.res_nmtf_inner and what they hand the runner, the refusals that
stay, resnmtf_fp64_sparse_plan as a function of structure and k alone, and the C-level refusals of
resnmtf_fp64_run_sparse, which come before any device work."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from resnmtf_amd import _lib, api, batched, engine, naming
from resnmtf_amd.engine import fp64_sparse_plan


def _never(*args, **kwargs):
    raise AssertionError("must not be reached")


def _echo(seen):
    def runner(problem, tol, max_iters, device_id):
        seen.update(problem=problem, tol=tol, max_iters=max_iters, device_id=device_id)
        n_v, k = len(problem["data"]), problem["k"]
        return {"f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": [np.ones(k)] * n_v,
                "mu": [np.ones(k)] * n_v, "all_error": np.array([0.3, 0.2]), "iters": 2}
    return runner


def _sparse_view(n=30, m=20, density=0.3, seed=1):
    x = sp.random(n, m, density=density, format="coo", random_state=seed) + sp.eye(n, m, format="coo")
    return x.tocoo()


def _init(shapes, k):
    rng = np.random.default_rng(0)
    return ([rng.random((n, k)) + 0.1 for n, _ in shapes], [rng.random((k, k)) + 0.1 for _ in shapes],
            [rng.random((m, k)) + 0.1 for _, m in shapes])


def test_signatures_and_struct_sizes():
    for name in ("resnmtf_fp64_run_sparse", "resnmtf_fp64_sparse_plan"):
        assert name in _lib.SIGNATURES
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.Fp64SparseView) == 3 * ptr
    assert C.sizeof(_lib.Fp64Sparse) == ptr + _lib.GROUP_MAX_VIEWS * 3 * ptr      # the int, padded to a pointer
    assert _lib.FP64_SPARSE_PLAN_INTS == 8 and _lib.ABI_VERSION == 2
    res, args = _lib.SIGNATURES["resnmtf_fp64_run_sparse"]
    assert res is C.c_int and len(args) == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    header = open(os.path.join(root, "include", "resnmtf_hip.h")).read()
    assert "#define RESNMTF_FP64_SPARSE_PLAN_INTS 8" in header


@pytest.mark.parametrize("pre_processed", [False, True])
def test_run_job_fp64_hands_the_runner_canonical_csc(pre_processed):
    raw = _sparse_view()
    dense = np.random.default_rng(2).random((30, 20)) + 0.01
    job = batched.Job([raw, dense], 3, n_iters=2)
    seen = {}
    res = batched.run_job_fp64(job, pre_processed=pre_processed, init=_init([(30, 20), (30, 20)], 3), runner=_echo(seen),
                               sparse=True)
    got = seen["problem"]["data"]
    assert sp.isspmatrix_csc(got[0]) and got[0].has_sorted_indices and got[0].dtype == np.float64
    assert isinstance(got[1], np.ndarray)
    want = raw.toarray() if pre_processed else naming.check_data([raw.toarray()])[0]
    np.testing.assert_allclose(got[0].toarray(), want, rtol=1e-14)
    assert (got[0].data != 0).all()
    assert res["bisil"] is None and res["row_clusters"][0].shape == (30, 3)
    assert raw.format == "coo"                                           # the caller's matrix is not modified


def test_sparse_needs_the_opt_in_an_init_and_valid_data():
    job = batched.Job([_sparse_view()], 3)
    init = _init([(30, 20)], 3)
    with pytest.raises(NotImplementedError, match="fp64 path takes dense views only"):
        batched.run_job_fp64(job, init=init, runner=_never)
    with pytest.raises(NotImplementedError, match="not available for sparse"):
        batched.run_job_fp64(job, runner=_never, sparse=True)
    neg = _sparse_view().tocsc()
    neg.data[3] = -1.0
    with pytest.raises(ValueError, match="negative"):
        batched.run_job_fp64(batched.Job([neg], 3), init=init, runner=_never, sparse=True)
    with pytest.raises(ValueError, match="exceeds a dimension"):
        batched.run_job_fp64(batched.Job([_sparse_view(30, 2)], 3), init=_init([(30, 2)], 3), runner=_never, sparse=True)


def test_the_grouped_path_still_refuses_sparse_views():
    job = batched.Job([_sparse_view()], 3)
    with pytest.raises(NotImplementedError, match="grouped path takes dense views only"):
        batched.run_jobs_grouped([job], group_runner=_never)
    with pytest.raises(NotImplementedError, match="grouped path takes dense views only"):
        batched.prepare_grouped_job(job, init=_init([(30, 20)], 3))
    with pytest.raises(ValueError, match="fp64_run alone"):
        engine._fill_group_job(_lib.GroupJob(), {"data": [_sparse_view()], "k": 3}, 0, 10, [])


def _inner_args(sparse_view=True):
    rng = np.random.default_rng(1)
    data = naming.check_data([rng.random((12, 9)) + 0.01, rng.random((12, 9)) + 0.01])
    rn, cn = naming.give_names(data)
    f, s, g, _, _ = api.svd_init(data, [2, 2], 0)
    z = np.zeros((2, 2))
    views = [sp.coo_matrix(data[0]) if sparse_view else data[0], data[1]]
    return data, (views, naming.shared_names(rn), naming.shared_names(cn), f, s, g, [2, 2], z, z, z, 5)


def test_fp64_sparse_reaches_the_runner(monkeypatch):
    import torch
    monkeypatch.setattr(api, "Engine", _never)
    seen = {}
    monkeypatch.setattr(engine, "fp64_run", _echo(seen))
    data, args = _inner_args()
    res = api.res_nmtf_inner(*args, spurious=False, precision="fp64", fp64_sparse=True, return_init=True)
    got = seen["problem"]["data"]
    assert sp.isspmatrix_csc(got[0]) and isinstance(got[1], np.ndarray)
    np.testing.assert_array_equal(got[0].toarray(), data[0])
    assert list(res)[:3] == ["output_f", "output_s", "output_g"] and len(res["init"]) == 2
    # a CPU sparse tensor is taken as its SciPy matrix
    t = torch.from_numpy(data[0]).to_sparse_csc()
    seen.clear()
    api.res_nmtf_inner(*([[t, data[1]]] + list(args[1:])), spurious=False, precision="fp64", fp64_sparse=True)
    assert sp.isspmatrix_csc(seen["problem"]["data"][0])
    np.testing.assert_array_equal(seen["problem"]["data"][0].toarray(), data[0])


def test_without_the_opt_in_todays_texts_are_raised(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    _, args = _inner_args()
    with pytest.raises(NotImplementedError, match="sparse views"):
        api.res_nmtf_inner(*args, spurious=False, precision="fp64")
    with pytest.raises(NotImplementedError, match="sparse views"):
        api.res_nmtf_inner(*args, spurious=False, precision="fp64", fp64_sparse=False)
    with pytest.raises(TypeError):                                      # keyword-only
        api.res_nmtf_inner(*args, 5, False, "euclidean", False, True)


def test_host_init_and_invalid_views_are_refused(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    _, args = _inner_args()
    no_init = list(args[:3]) + [None, None, None] + list(args[6:])
    with pytest.raises(NotImplementedError, match="host_init=True"):
        api.res_nmtf_inner(*no_init, spurious=False, precision="fp64", fp64_sparse=True, host_init=True)
    bad = sp.csc_matrix(args[0][0]).copy()
    bad.data[0] = -bad.data[0]
    with pytest.raises(ValueError, match="negative"):
        api.res_nmtf_inner(*([[bad, args[0][1]]] + list(args[1:])), spurious=False, precision="fp64", fp64_sparse=True)


class _CallLog:
    """Stands in for engine.Engine: records what the device initialisation of the fp64 route does with it."""
    calls, kwargs = [], {}

    def __init__(self, n_rows, n_cols, k, device_id=0, **kw):
        self.n_views, self.k, self.n_rows, self.n_cols = len(n_rows), list(k), list(n_rows), list(n_cols)
        self.owned = [True] * self.n_views
        _CallLog.calls, _CallLog.kwargs = ["create"], kw

    def _log(name, result=None):
        def method(self, *args, **kwargs):
            _CallLog.calls.append(name)
            return result(self, *args) if result else None
        return method

    set_view = _log("set_view")
    set_view_sparse = _log("set_view_sparse")
    init_svd = _log("init_svd")
    set_restrictions = _log("set_restrictions")
    set_shared_rows = _log("set_shared_rows")
    set_shared_cols = _log("set_shared_cols")
    get_factors = _log("get_factors", lambda self, v: (np.ones((self.n_rows[v], self.k[v])), np.ones((self.k[v], self.k[v])),
                                                       np.ones((self.n_cols[v], self.k[v])), np.ones(self.k[v]), np.ones(self.k[v])))
    close = _log("close")


def test_device_initialisation_goes_through_a_short_lived_sparse_engine(monkeypatch):
    monkeypatch.setattr(api, "Engine", _CallLog)
    seen = {}
    monkeypatch.setattr(engine, "fp64_run", _echo(seen))
    data, args = _inner_args()
    no_init = list(args[:3]) + [None, None, None] + list(args[6:])
    api.res_nmtf_inner(*no_init, spurious=False, precision="fp64", fp64_sparse=True, seed=4)
    assert _CallLog.kwargs["nnz"] == [int((data[0] != 0).sum()), None]
    assert _CallLog.calls == (["create", "set_view_sparse", "init_svd", "set_view", "init_svd", "set_restrictions"] +
                              ["set_shared_rows", "set_shared_cols"] * 2 + ["get_factors"] * 2 + ["close"])
    assert sp.isspmatrix_csc(seen["problem"]["data"][0]) and seen["problem"]["init_lam"][0].shape == (2,)


def test_f32_accepts_the_flag_as_a_no_op(monkeypatch):
    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()
    monkeypatch.setattr(api, "Engine", stop)
    monkeypatch.setattr(engine, "fp64_run", _never)
    _, args = _inner_args(sparse_view=False)
    for kw in ({}, {"fp64_sparse": True}):                               # both reach the engine of the f32 route
        with pytest.raises(Stop):
            api.res_nmtf_inner(*args, spurious=False, **kw)


# ---- resnmtf_fp64_sparse_plan: structure and k alone ----
def _skewed(n=600, m=400, seed=0):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < 0.01
    mask[5, :] = True                      # one full row: 400 entries
    mask[:, 7] = True                      # one full column: 600 entries
    return sp.csc_matrix(mask.astype(np.float64))


def test_plan_is_a_function_of_structure_and_k():
    x = _skewed()
    a = fp64_sparse_plan(x, 16)
    assert a == fp64_sparse_plan(x, 16)
    y = x.copy()
    y.data = y.data * np.random.default_rng(1).random(y.nnz) + 0.5       # other values, the same structure
    assert fp64_sparse_plan(y, 16) == a
    assert fp64_sparse_plan(sp.coo_matrix(x), 16) == a                   # any format: its canonical CSC
    assert a["kp"] == 16 and a["lines_per_wave"] == 4
    assert a["xg"] == (2, 200, 400) and a["xtf"] == (3, 200, 600)        # ceil(longest / 256) pieces of equal length
    for k, kp, lpw in ((3, 16, 4), (17, 32, 2), (33, 48, 1), (64, 64, 1)):
        p = fp64_sparse_plan(x, k)
        assert (p["kp"], p["lines_per_wave"]) == (kp, lpw) and p["xg"] == a["xg"] and p["xtf"] == a["xtf"]
    thin = fp64_sparse_plan(sp.eye(50, 40, format="csc"), 4)
    assert thin["xg"] == (1, 1, 1) and thin["xtf"] == (1, 1, 1)
    full = fp64_sparse_plan(sp.csc_matrix(np.ones((10000, 20))), 4)
    assert full["xtf"] == (16, 625, 10000) and full["xg"] == (1, 20, 20)  # at most 16 pieces


def test_plan_refuses_bad_input():
    lib = _lib.load()
    out = (C.c_int * _lib.FP64_SPARSE_PLAN_INTS)()
    lp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_int)

    def plan(n, m, k, ptr, idx, o=out):
        ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int32)
        rc = lib.resnmtf_fp64_sparse_plan(n, m, k, ptr.ctypes.data_as(lp), idx.ctypes.data_as(ip), o)
        return rc, lib.resnmtf_last_error(None)

    assert plan(4, 3, 2, [0, 1, 2, 3], [0, 1, 2])[0] == _lib.OK
    for args, word in (((4, 3, 2, [1, 1, 2, 3], [0, 1, 2]), b"col_ptr[0]"),
                       ((4, 3, 2, [0, 2, 1, 3], [0, 1, 2]), b"monotone"),
                       ((4, 3, 2, [0, 1, 2, 3], [0, 4, 2]), b"out of range"),
                       ((4, 3, 2, [0, 1, 2, 3], [0, -1, 2]), b"out of range"),
                       ((4, 3, 2, [0, 2, 2, 3], [1, 1, 2]), b"strictly increasing"),
                       ((4, 3, 2, [0, 2, 2, 3], [2, 1, 2]), b"strictly increasing"),
                       ((4, 3, 0, [0, 1, 2, 3], [0, 1, 2]), b"k must be in [1, 64]"),
                       ((4, 3, 4, [0, 1, 2, 3], [0, 1, 2]), b"exceeds a view dimension"),
                       ((0, 3, 1, [0, 0, 0, 0], [0]), b"positive")):
        rc, text = plan(*args)
        assert rc == 1 and word in text, (args, text)
    assert plan(4, 3, 2, [0, 1, 2, 3], [0, 1, 2], None)[0] == 1
    assert lib.resnmtf_fp64_sparse_plan(4, 3, 2, None, None, out) == 1
    with pytest.raises(_lib.ResnmtfError):
        fp64_sparse_plan(sp.eye(5, 4, format="csc"), 5)


# ---- the C-level refusals of resnmtf_fp64_run_sparse: before any device work, so they need no device ----
def _c_job(n=10, m=8, k=2):
    rng = np.random.default_rng(0)
    j = _lib.GroupJob()
    j.struct_size = C.sizeof(_lib.GroupJob)
    j.n_views, j.k, j.n_iters = 1, k, 5
    dp = C.POINTER(C.c_double)
    arrs = [np.asfortranarray(rng.random(s) + 0.1) for s in ((n, k), (k, k), (m, k))]
    outs = [np.full(s, -7.0, order="F") for s in ((n, k), (k, k), (m, k), (k,), (k,))]
    j.n_rows[0], j.n_cols[0] = n, m
    j.f0[0], j.s0[0], j.g0[0] = (a.ctypes.data_as(dp) for a in arrs)
    j.f_out[0], j.s_out[0], j.g_out[0], j.lambda_out[0], j.mu_out[0] = (a.ctypes.data_as(dp) for a in outs)
    err, it = np.full(16, -7.0), np.full(1, -7, dtype=np.int32)
    j.all_error, j.err_capacity, j.iters_done = err.ctypes.data_as(dp), 16, it.ctypes.data_as(C.POINTER(C.c_int))
    return j, arrs, outs + [err, it]


def _c_sparse(x):
    c = sp.csc_matrix(x)
    arrs = [c.indptr.astype(np.int64), c.indices.astype(np.int32), c.data.astype(np.float64)]
    s = _lib.Fp64Sparse()
    s.struct_size = C.sizeof(_lib.Fp64Sparse)
    s.view[0].col_ptr = arrs[0].ctypes.data_as(C.POINTER(C.c_longlong))
    s.view[0].row_idx = arrs[1].ctypes.data_as(C.POINTER(C.c_int))
    s.view[0].values = arrs[2].ctypes.data_as(C.POINTER(C.c_double))
    return s, arrs


def test_c_level_refusals_need_no_device():
    lib = _lib.load()
    j, keep, outs = _c_job()
    x = np.random.default_rng(3).random((10, 8)) + 0.1

    def refused(job, s, word):
        assert lib.resnmtf_fp64_run_sparse(0, C.byref(job), C.byref(s), 1e-6, 100) == 1
        assert word in lib.resnmtf_last_error(None), lib.resnmtf_last_error(None)
        assert all(np.all(o == -7) for o in outs)                       # a refusal writes no output

    s, arrs = _c_sparse(x)
    arrs[1][[0, 1]] = arrs[1][[1, 0]]
    refused(j, s, b"strictly increasing")
    s, arrs = _c_sparse(x)
    arrs[1][5] = 10
    refused(j, s, b"out of range")
    s, arrs = _c_sparse(x)
    arrs[2][4] = -0.5
    refused(j, s, b"negative")
    s, arrs = _c_sparse(x)
    arrs[2][4] = np.nan
    refused(j, s, b"non-finite")
    s, arrs = _c_sparse(x)
    arrs[0][0] = 1
    refused(j, s, b"col_ptr[0]")
    s, arrs = _c_sparse(x)
    arrs[0][3] = arrs[0][2] - 1
    refused(j, s, b"monotone")
    s, arrs = _c_sparse(x)
    xf = np.asfortranarray(x)
    both = _lib.GroupJob.from_buffer_copy(j)
    both.x[0] = xf.ctypes.data_as(C.POINTER(C.c_double))
    refused(both, s, b"both dense")
    refused(j, _lib.Fp64Sparse(struct_size=C.sizeof(_lib.Fp64Sparse)), b"x / f0 / s0 / g0 is NULL")      # neither
    s.struct_size = 8
    refused(j, s, b"struct_size")
    s, arrs = _c_sparse(x)
    s.view[0].values = None
    refused(j, s, b"values is NULL")
    s, arrs = _c_sparse(x)
    s.view[3].col_ptr = arrs[0].ctypes.data_as(C.POINTER(C.c_longlong))
    refused(j, s, b"beyond n_views")
    s, arrs = _c_sparse(x)
    bad = _lib.GroupJob.from_buffer_copy(j)
    bad.k = 65
    refused(bad, s, b"k must be in [1, 64]")                            # the job's own refusals keep their texts
