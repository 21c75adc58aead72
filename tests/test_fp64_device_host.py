"""Host side of the fp64 path from device memory (resnmtf_fp64_run_device, engine.fp64_run(output=, return_state=),
api.res_nmtf_inner(precision="fp64", fp64_device=True); no GPU): the symbol and the struct are
bound, the flag is keyword-only and opt-in -- without it every refusal of tests/test_fp64_host.py still fires, with it
what still needs a live handle is still refused --, precision="f32" ignores it, and the C entry refuses a malformed
resnmtf_fp64_device before it touches a device, by text."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from resnmtf_amd import _lib, api, engine, naming


def _never(*args, **kwargs):
    raise AssertionError("the device runner must not be reached")


def _inner_args(n_views=1):
    rng = np.random.default_rng(1)
    data = naming.check_data([rng.random((12, 9)) + 0.01 for _ in range(n_views)])
    rn, cn = naming.give_names(data)
    f, s, g, _, _ = api.svd_init(data, [2] * n_views, 0)
    z = np.zeros((n_views, n_views))
    return (data, naming.shared_names(rn), naming.shared_names(cn), f, s, g, [2] * n_views, z, z, z, 5)


# ---- the binding ----
def test_symbol_and_struct_are_bound():
    assert "resnmtf_fp64_run_device" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["resnmtf_fp64_run_device"]
    assert restype is C.c_int
    assert argtypes == [C.c_int, C.POINTER(_lib.GroupJob), C.POINTER(_lib.Fp64Sparse), C.POINTER(_lib.Fp64Device), C.c_double, C.c_int]
    lib = _lib.load()
    assert lib.resnmtf_fp64_run_device.argtypes == argtypes
    names = [f[0] for f in _lib.Fp64Device._fields_]
    assert names == ["struct_size", "stream", "x", "f0", "s0", "g0", "lambda0", "mu0", "f_out", "s_out", "g_out", "lambda_out",
                     "mu_out", "state_f", "state_s", "state_g", "state_lambda", "state_mu"]
    # int + padding, a pointer, 6 x 8 descriptors of (pointer, int + padding, 2 long long), 10 x 8 pointers
    assert C.sizeof(_lib.Fp64Device) == 16 + 6 * 8 * C.sizeof(_lib.DeviceMatrix) + 10 * 8 * 8
    assert C.sizeof(_lib.DeviceMatrix) == 32


# ---- api.res_nmtf_inner: the flag ----
def test_the_flag_is_keyword_only(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    with pytest.raises(TypeError):
        api.res_nmtf_inner(*_inner_args(), 5, False, "euclidean", False, "fp64", False, True)


@pytest.mark.parametrize("flag,kwargs", [
    ("spurious_on_device", dict(spurious=True, spurious_on_device=True)),
    ("score_bisil", dict(spurious=False, score_bisil=True)),
    ("output=\"torch\"", dict(spurious=False, output="torch")),
    ("post_on_device", dict(spurious=False, output="torch", post_on_device=True)),
    ("return_state", dict(spurious=False, return_state=True)),
])
@pytest.mark.parametrize("spelled", [False, True])
def test_flag_off_keeps_the_live_handle_refusals(monkeypatch, flag, kwargs, spelled):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    more = {"fp64_device": False} if spelled else {}
    with pytest.raises(NotImplementedError, match=flag):
        api.res_nmtf_inner(*_inner_args(), precision="fp64", **kwargs, **more)


def test_flag_off_keeps_the_device_memory_refusals(monkeypatch):
    import torch
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = list(_inner_args())
    sparse_args = [[sp.csc_matrix(args[0][0])]] + args[1:]
    with pytest.raises(NotImplementedError, match="sparse views"):
        api.res_nmtf_inner(*sparse_args, spurious=False, precision="fp64", fp64_device=False)
    there = torch.empty((12, 9), dtype=torch.float64, device="meta")       # (not on the CPU: stands for device memory)
    with pytest.raises(NotImplementedError, match="views in device memory"):
        api.res_nmtf_inner(*([[there]] + args[1:]), spurious=False, precision="fp64", fp64_device=False)
    f_there = [torch.empty((12, 2), dtype=torch.float64, device="meta")]
    with pytest.raises(NotImplementedError, match="factors in device memory"):
        api.res_nmtf_inner(*(args[:3] + [f_there] + args[4:]), spurious=False, precision="fp64", fp64_device=False)
    lm_there = ([torch.empty(2, dtype=torch.float64, device="meta")], [np.ones(2)])
    with pytest.raises(NotImplementedError, match="factors in device memory"):
        api.res_nmtf_inner(*args, spurious=False, precision="fp64", init_lm=lm_there)


@pytest.mark.parametrize("flag,kwargs", [
    ("spurious_on_device", dict(spurious=True, spurious_on_device=True)),
    ("score_bisil", dict(spurious=False, score_bisil=True)),
    ("post_on_device", dict(spurious=False, output="torch", post_on_device=True)),
])
def test_flag_on_still_refuses_what_needs_a_live_handle(monkeypatch, flag, kwargs):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    with pytest.raises(NotImplementedError, match=flag):
        api.res_nmtf_inner(*_inner_args(), precision="fp64", fp64_device=True, **kwargs)


@pytest.mark.parametrize("fp64_sparse", [False, True])
def test_flag_on_still_refuses_sparse_tensors_in_device_memory(monkeypatch, fp64_sparse):
    import torch
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = list(_inner_args())
    there = torch.sparse_csc_tensor(torch.zeros(10, dtype=torch.int64, device="meta"), torch.zeros(0, dtype=torch.int64, device="meta"),
                                    torch.zeros(0, dtype=torch.float64, device="meta"), size=(12, 9), check_invariants=False)
    with pytest.raises(NotImplementedError, match="sparse views"):
        api.res_nmtf_inner(*([[there]] + args[1:]), spurious=False, precision="fp64", fp64_device=True, fp64_sparse=fp64_sparse)


def test_flag_on_return_state_needs_torch_output(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    with pytest.raises(ValueError, match="return_state"):
        api.res_nmtf_inner(*_inner_args(), spurious=False, precision="fp64", fp64_device=True, return_state=True)


def test_flag_on_hands_output_and_return_state_to_the_runner(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    seen = {}

    def runner(problem, tol, max_iters, device_id, **more):
        seen.update(problem=problem, more=more)
        n_v, k = len(problem["data"]), problem["k"]
        return {"f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": [np.ones(k)] * n_v,
                "mu": [np.ones(k)] * n_v, "all_error": np.array([0.3, 0.2]), "iters": 2}
    monkeypatch.setattr(engine, "fp64_run", runner)
    args = _inner_args(2)
    res = api.res_nmtf_inner(*args, spurious=False, precision="fp64", fp64_device=True)
    assert seen["more"] == {"output": "numpy", "return_state": False}
    for v in range(2):
        np.testing.assert_array_equal(seen["problem"]["data"][v], args[0][v])
        np.testing.assert_array_equal(seen["problem"]["init_f"][v], args[3][v])
    assert list(res) == ["output_f", "output_s", "output_g", "Error", "All_Error", "bisil", "row_clusters", "col_clusters",
                         "lambda", "mu"]
    # ... and without the flag the runner is called as it always was
    seen.clear()
    api.res_nmtf_inner(*args, spurious=False, precision="fp64")
    assert seen["more"] == {}


class _CallLog:
    """Stands in for engine.Engine inside api.res_nmtf_inner and records the order of the calls made on it."""
    calls = []

    def __init__(self, n_rows, n_cols, k, device_id=0, **kw):
        self.n_views, self.k, self.n_rows, self.n_cols = len(n_rows), list(k), list(n_rows), list(n_cols)
        self.owned = [True] * self.n_views
        _CallLog.calls = ["create"]

    def _log(name, result=None):
        def method(self, *args, **kwargs):
            _CallLog.calls.append(name)
            return result(self, *args) if result else None
        return method

    def _state(self, v):
        return (np.ones((self.n_rows[v], self.k[v])), np.ones((self.k[v], self.k[v])), np.ones((self.n_cols[v], self.k[v])),
                np.ones(self.k[v]), np.ones(self.k[v]))

    set_view = _log("set_view")
    init_svd = _log("init_svd")
    set_factors = _log("set_factors")
    set_restrictions = _log("set_restrictions")
    set_shared_rows = _log("set_shared_rows")
    set_shared_cols = _log("set_shared_cols")
    run = _log("run", lambda self, *a: np.array([0.5]))
    finalise = _log("finalise", lambda self, v: (np.ones((self.n_rows[v], self.k[v])), np.ones((self.k[v], self.k[v])),
                                                 np.ones((self.n_cols[v], self.k[v])), np.ones((self.n_rows[v], self.k[v])),
                                                 np.ones((self.n_cols[v], self.k[v]))))
    get_factors = _log("get_factors", _state)
    get_factors_device = _log("get_factors_device", _state)
    close = _log("close")


def test_f32_ignores_the_flag(monkeypatch):
    """The call sequence test_default_precision_leaves_the_call_sequence_as_it_is (tests/test_fp64_host.py) records."""
    monkeypatch.setattr(api, "Engine", _CallLog)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = _inner_args(2)
    want = (["create"] + ["set_view", "set_factors"] * 2 + ["set_restrictions"] + ["set_shared_rows", "set_shared_cols"] * 2 +
            ["run"] + ["finalise", "get_factors"] * 2 + ["close"])
    plain = api.res_nmtf_inner(*args, spurious=False)
    assert _CallLog.calls == want
    flagged = api.res_nmtf_inner(*args, spurious=False, precision="f32", fp64_device=True)
    assert _CallLog.calls == want and list(plain) == list(flagged)


def test_device_initialisation_is_read_on_the_device_under_the_flag(monkeypatch):
    monkeypatch.setattr(api, "Engine", _CallLog)
    seen = {}
    monkeypatch.setattr(engine, "fp64_run", lambda problem, **kw: seen.update(problem=problem) or {
        "f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": problem["init_lam"],
        "mu": problem["init_mu"], "all_error": np.array([0.3]), "iters": 1})
    args = _inner_args(2)
    load = ["create"] + ["set_view", "init_svd"] * 2 + ["set_restrictions"] + ["set_shared_rows", "set_shared_cols"] * 2
    api.res_nmtf_inner(*(args[:3] + (None, None, None) + args[6:]), spurious=False, precision="fp64", seed=4)
    assert _CallLog.calls == load + ["get_factors"] * 2 + ["close"]
    api.res_nmtf_inner(*(args[:3] + (None, None, None) + args[6:]), spurious=False, precision="fp64", seed=4, fp64_device=True)
    assert _CallLog.calls == load + ["get_factors_device"] * 2 + ["close"]
    assert seen["problem"]["init_lam"][0].shape == (2,)


# ---- engine.fp64_run ----
def _problem():
    rng = np.random.default_rng(2)
    return {"data": [rng.random((10, 8)) + 0.1], "k": 2, "init_f": [rng.random((10, 2))], "init_s": [rng.random((2, 2))],
            "init_g": [rng.random((8, 2))], "n_iters": 3}


def test_fp64_run_refuses_the_raw_state_without_torch_output():
    with pytest.raises(ValueError, match="return_state"):
        engine.fp64_run(_problem(), output="numpy", return_state=True)
    with pytest.raises(ValueError, match="output"):
        engine.fp64_run(_problem(), output="cupy")


def test_fp64_run_refuses_a_mix_and_another_device_before_the_library(monkeypatch):
    import torch
    monkeypatch.setattr(_lib, "load", lambda: None)                       # (a library call would fail on None)
    p = _problem()
    p["init_f"] = [torch.empty((10, 2), dtype=torch.float64, device="meta")]
    with pytest.raises(ValueError, match="mix device tensors and host arrays"):
        engine.fp64_run(p)
    p = _problem()
    p["data"] = [torch.empty((10, 8), dtype=torch.float64, device="meta")]
    with pytest.raises(ValueError, match="lives on meta"):
        engine.fp64_run(p)


# ---- the C entry: what it refuses before it touches a device ----
_DP = C.POINTER(C.c_double)
THERE = 0x7F0000001000          # stands for a device address: these refusals come before any pointer is looked at


def _c_job(n=10, m=8, k=2, V=1):
    rng = np.random.default_rng(0)
    keep, outs_all = [], []
    j = _lib.GroupJob()
    j.struct_size = C.sizeof(_lib.GroupJob)
    j.n_views, j.k, j.n_iters = V, k, 5
    for v in range(V):
        arrs = [np.asfortranarray(rng.random(s) + 0.1) for s in ((n, m), (n, k), (k, k), (m, k))]
        outs = [np.full(s, -7.0, order="F") for s in ((n, k), (k, k), (m, k), (k,), (k,))]
        keep += arrs + outs
        outs_all += outs
        j.n_rows[v], j.n_cols[v] = n, m
        j.x[v], j.f0[v], j.s0[v], j.g0[v] = (a.ctypes.data_as(_DP) for a in arrs)
        j.f_out[v], j.s_out[v], j.g_out[v], j.lambda_out[v], j.mu_out[v] = (a.ctypes.data_as(_DP) for a in outs)
    err, it = np.full(16, -7.0), np.full(1, -7, dtype=np.int32)
    keep += [err, it]
    outs_all += [err, it]
    j.all_error, j.err_capacity, j.iters_done = err.ctypes.data_as(_DP), 16, it.ctypes.data_as(C.POINTER(C.c_int))
    return j, keep, outs_all


def _dev():
    d = _lib.Fp64Device()
    d.struct_size = C.sizeof(_lib.Fp64Device)
    return d


def _mat(ptr=THERE, dtype=_lib.DTYPE_F64, rs=1, cs=10):
    return _lib.DeviceMatrix(ptr, dtype, rs, cs)


def _null(j, *fields, v=0):
    j = _lib.GroupJob.from_buffer_copy(j)
    for f in fields:
        getattr(j, f)[v] = _DP()
    return j


def _cases():
    """(name, edit of (job, dev) returning the job to pass, the text expected)."""
    def both(j, d):
        d.x[0] = _mat()
        return j

    def neither(j, d):
        return _null(j, "x")

    def partial_factors(j, d):
        d.f0[0], d.g0[0] = _mat(), _mat(cs=8)
        return _null(j, "f0", "s0", "g0")

    def factors_twice(j, d):
        d.f0[0], d.s0[0], d.g0[0] = _mat(), _mat(cs=2), _mat(cs=8)
        return j

    def lm_alone(j, d):
        d.lambda0[0] = _mat()
        return j

    def partial_outputs(j, d):
        d.f_out[0], d.s_out[0], d.lambda_out[0], d.mu_out[0] = THERE, THERE, THERE, THERE
        return j

    def partial_state(j, d):
        d.state_f[0] = THERE
        return j

    def negative_stride(j, d):
        d.x[0] = _mat(rs=-1)
        return _null(j, "x")

    def unknown_dtype(j, d):
        d.x[0] = _mat(dtype=4)
        return _null(j, "x")

    def bad_size(j, d):
        d.struct_size = C.sizeof(_lib.Fp64Device) - 8
        return j

    def beyond(j, d):
        d.x[1] = _mat()
        return j

    return [("both", both, b"view 0: x is given both in the job (job->x) and in device memory (dev->x)"),
            ("neither", neither, b"view 0: x is given neither in the job (job->x) nor in device memory (dev->x)"),
            ("partial factors", partial_factors, b"view 0: f0 / s0 / g0 are given partly in device memory (dev->s0 NULL)"),
            ("factors twice", factors_twice, b"view 0: f0 / s0 / g0 are given in device memory: job->f0 / s0 / g0 / lambda0 / mu0 must be NULL"),
            ("lambda0 alone", lm_alone, b"view 0: dev->lambda0 / dev->mu0 need f0 / s0 / g0 in device memory"),
            ("partial outputs", partial_outputs, b"view 0: dev->g_out is NULL while other device outputs are given"),
            ("partial state", partial_state, b"view 0: dev->state_s is NULL while other device state outputs are given"),
            ("negative stride", negative_stride, b"view 0: dev->x has a negative stride"),
            ("unknown dtype", unknown_dtype, b"view 0: dev->x has an unknown dtype (4)"),
            ("struct_size", bad_size, b"resnmtf_fp64_device struct_size mismatch"),
            ("beyond n_views", beyond, b"view 1: dev->x is given beyond n_views")]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_c_entry_refuses_a_malformed_device_struct(case):
    _, edit, text = case
    lib = _lib.load()
    invalid = {name: c for c, name in _lib.ERR_NAMES.items()}["INVALID"]
    j, keep, outs = _c_job()
    d = _dev()
    j = edit(j, d)
    assert lib.resnmtf_fp64_run_device(0, C.byref(j), None, C.byref(d), 1e-6, 100) == invalid
    assert text in lib.resnmtf_last_error(None), lib.resnmtf_last_error(None)
    assert all(np.all(o == -7) for o in outs)                             # a refusal writes no output


def test_c_entry_refuses_a_partial_set_over_two_views():
    """Every output of view 0 and none of view 1: the set is for every view of the job, or for none."""
    lib = _lib.load()
    j, keep, outs = _c_job(V=2)
    d = _dev()
    for name in ("f_out", "s_out", "g_out", "lambda_out", "mu_out"):
        getattr(d, name)[0] = THERE
    assert lib.resnmtf_fp64_run_device(0, C.byref(j), None, C.byref(d), 1e-6, 100) != _lib.OK
    assert b"view 1: dev->f_out is NULL while other device outputs are given" in lib.resnmtf_last_error(None)


def test_c_entry_refuses_host_memory_given_as_device_memory():
    """The pointers are looked at after the structure and before any allocation; host memory is not device memory
    (without a device the runtime knows no pointer at all, and the refusal is the same)."""
    lib = _lib.load()
    j, keep, outs = _c_job()
    x = np.asfortranarray(np.ones((10, 8)))
    d = _dev()
    d.x[0] = _mat(ptr=x.ctypes.data)
    j = _null(j, "x")
    assert lib.resnmtf_fp64_run_device(0, C.byref(j), None, C.byref(d), 1e-6, 100) != _lib.OK
    assert b"view 0: dev->x is not device memory of device 0" in lib.resnmtf_last_error(None)
    d = _dev()
    for name, a in zip(("f_out", "s_out", "g_out", "lambda_out", "mu_out"), outs):
        getattr(d, name)[0] = a.ctypes.data
    j, keep, outs = _c_job()
    assert lib.resnmtf_fp64_run_device(0, C.byref(j), None, C.byref(d), 1e-6, 100) != _lib.OK
    assert b"view 0: dev->f_out is not device memory of device 0" in lib.resnmtf_last_error(None)
    assert all(np.all(o == -7) for o in outs)
