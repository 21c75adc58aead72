"""GPU tests of the fp64 path from device memory (resnmtf_fp64_run_device): views, initial factors,
results and the raw state as ``torch`` tensors on the GPU.  Every comparison is bit for bit (the bytes of F, S, G, lambda,
mu and All_Error, and the sweep count) against ``fp64_run`` on ``t.double().cpu().numpy()`` of the same tensors: the tile
edges of the images kernel, source layouts and dtypes, factors from the device with and without lambda / mu, a job mixing
device, host and sparse views, a coupled job to convergence, tensors out, resuming from the raw state, dev == NULL, stream
ordering, the API route (with section 21's bars against the oracle: 1e-11 / 1e-13), repeatability and the refusals that need
device memory.  Runs are at most 5 fixed sweeps unless said otherwise."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import helpers
from oracle import resnmtf_oracle as O
from resnmtf_amd import _lib, api, batched, engine, naming, synth
from resnmtf_amd.engine import fp64_plan, fp64_run
from resnmtf_amd.problem import pair_table
from resnmtf_amd.synth import Problem

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SWEEPS = 4
KEYS = ("f", "s", "g", "lambda", "mu")
with open(os.path.join(helpers.ROOT, "resnmtf_amd", "csrc", "resnmtf_fp64_device.hip.inc")) as _src:
    T = int(re.search(r"constexpr int F64_DEV_TILE = (\d+);", _src.read()).group(1))      # the tile side of the images kernel


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _same_bits(a, b, what=""):
    """F, S, G, lambda, mu, All_Error and the sweep count: equal as arrays and byte for byte."""
    assert a["iters"] == b["iters"], (what, a["iters"], b["iters"])
    assert np.array_equal(a["all_error"], b["all_error"]) and a["all_error"].tobytes() == b["all_error"].tobytes(), (what, "all_error")
    for key in KEYS:
        assert len(a[key]) == len(b[key])
        for v, (x, y) in enumerate(zip(a[key], b[key])):
            x, y = _np(x), _np(y)
            assert x.shape == y.shape and x.dtype == y.dtype == np.float64, (what, key, v)
            assert np.array_equal(x, y, equal_nan=True) and np.asfortranarray(x).tobytes() == np.asfortranarray(y).tobytes(), (what, key, v)


def _single(n, m, k, seed):
    rng = np.random.default_rng(seed)
    kb = max(1, min(k, n, m))
    rb, cb = np.arange(n) * kb // n, np.arange(m) * kb // m
    x = 10.0 * (rb[:, None] == cb[None, :]) + 0.1 * np.abs(rng.standard_normal((n, m)))
    x = x / x.sum(axis=0)[None, :]
    f, s, g = synth.random_init(n, m, k, seed + 7)
    return Problem([x], [f], [s], [g], np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), k, "single",
                   row_names=[[f"r{i}" for i in range(n)]], col_names=[[f"c{j}" for j in range(m)]])


def _problem(prob, n_iters, **replace):
    p = {"data": list(prob.data), "k": prob.init_f[0].shape[1], "init_f": list(prob.init_f), "init_s": list(prob.init_s),
         "init_g": list(prob.init_g), "phi": prob.phi, "xi": prob.xi, "psi": prob.psi, "row_pairs": pair_table(prob.row_names),
         "col_pairs": pair_table(prob.col_names), "n_iters": n_iters}
    p.update(replace)
    return p


def _host_twin(problem):
    """The same problem with every tensor replaced by ``t.double().cpu().numpy()``."""
    def host(x):
        return x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else x
    return {key: [host(x) for x in val] if isinstance(val, list) else val for key, val in problem.items()}


def _row_major(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype).contiguous()


# ---- 1. the tile edges of the images kernel, fp64 row-major ----
EDGES = [(2, 2, 1), (T - 1, T + 1, 5), (T + 1, T - 1, 5), (T, T, 5), (129, 127, 16), (33, 257, 17), (257, 33, 16)]


@pytest.mark.parametrize("n,m,k", EDGES)
def test_tile_edges(n, m, k):
    plan = fp64_plan(n, m, k)
    if (n, m) == (33, 257):
        assert plan["xg"][1] == 5 and plan["xtf"][1] == 1 and plan["resid"][1] > 1      # the five-way split of section 21
    if (n, m) == (257, 33):
        assert plan["xtf"][1] == 5 and plan["xg"][1] == 1
    if (n, m) == (129, 127):
        assert plan["xg"][0] == 2 and plan["xtf"][0] == 1 and plan["resid"][0] == 3
    prob = _single(n, m, k, 100 + n + m + k)
    t = _row_major(prob.data[0])
    assert t.stride() == (m, 1)
    p = _problem(prob, SWEEPS, data=[t])
    _same_bits(fp64_run(p), fp64_run(_host_twin(p)), (n, m, k))


# ---- 2. layouts and dtypes at 129 x 127 ----
@pytest.fixture(scope="module")
def edge_problem():
    return _single(129, 127, 16, 372)


def _layout(x, layout):
    n, m = x.shape
    if layout == "column-major":
        t = torch.as_tensor(np.ascontiguousarray(x.T), device=DEV).T
        assert t.stride() == (1, n)
    elif layout == "slice":
        big = torch.zeros((2 * n + 1, m + 7), dtype=torch.float64, device=DEV)
        big[1::2, 3:3 + m] = torch.as_tensor(x, device=DEV)
        t = big[1::2, 3:3 + m]
        assert t.stride() == (2 * (m + 7), 1) and not t.is_contiguous()
    elif layout == "transposed":
        t = torch.as_tensor(np.ascontiguousarray(x.T), device=DEV).contiguous().T
        assert t.stride() == (1, n)
    else:                                   # every row is row 0: a row stride of 0
        t = torch.as_tensor(np.ascontiguousarray(x[:1]), device=DEV).expand(n, m)
        assert t.stride() == (0, 1)
    assert tuple(t.shape) == (n, m)
    return t


@pytest.mark.parametrize("layout", ["column-major", "slice", "transposed", "expanded"])
def test_layouts(edge_problem, layout):
    p = _problem(edge_problem, SWEEPS, data=[_layout(edge_problem.data[0], layout)])
    _same_bits(fp64_run(p), fp64_run(_host_twin(p)), layout)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_dtypes(edge_problem, dtype):
    t = _row_major(edge_problem.data[0] * 64.0, dtype)          # (scaled: fp16 keeps the small entries normal)
    assert t.dtype == dtype
    p = _problem(edge_problem, SWEEPS, data=[t])
    _same_bits(fp64_run(p), fp64_run(_host_twin(p)), dtype)


# ---- 3. initial factors from the device ----
def _factors(prob, dtype=torch.float64, strided=False):
    out = []
    for a in (prob.init_f[0], prob.init_s[0], prob.init_g[0]):
        if strided:                         # every second row and column of a larger tensor
            big = torch.zeros((2 * a.shape[0], 2 * a.shape[1] + 3), dtype=dtype, device=DEV)
            big[::2, 1:1 + 2 * a.shape[1]:2] = torch.as_tensor(a, device=DEV).to(dtype)
            out.append(big[::2, 1:1 + 2 * a.shape[1]:2])
        else:
            out.append(_row_major(a, dtype))
    return out


@pytest.mark.parametrize("dtype,strided,view_there", [(torch.float64, False, True), (torch.float32, False, False),
                                                      (torch.float16, False, True), (torch.bfloat16, False, False),
                                                      (torch.float64, True, True)])
def test_factors_from_the_device(edge_problem, dtype, strided, view_there):
    f, s, g = _factors(edge_problem, dtype, strided)
    data = [_row_major(edge_problem.data[0])] if view_there else list(edge_problem.data)
    p = _problem(edge_problem, SWEEPS, data=data, init_f=[f], init_s=[s], init_g=[g])
    _same_bits(fp64_run(p), fp64_run(_host_twin(p)), (dtype, strided))


@pytest.mark.parametrize("shape,k", [((129, 127), 16), ((257, 33), 33)])
@pytest.mark.parametrize("lm", ["given", "column sums", "lambda alone"])
def test_factors_with_and_without_lambda_mu(shape, k, lm):
    """Without them the sequential column sums on the device must give the host loop's bits; (257, 33) at k = 33 is
    the 48-wide padded class."""
    prob = _single(*shape, k, 41 + k)
    assert fp64_plan(*shape, k)["kp"] == (48 if k == 33 else 16)
    f, s, g = _factors(prob)
    rng = np.random.default_rng(5)
    lam = torch.as_tensor(rng.random(k) + 0.5, device=DEV)
    mu = torch.as_tensor(rng.random(2 * k) + 0.5, device=DEV)[::2]       # (a strided vector)
    more = {"given": dict(init_lam=[lam], init_mu=[mu]), "column sums": {}, "lambda alone": dict(init_lam=[lam], init_mu=[None])}[lm]
    p = _problem(prob, SWEEPS, data=[_row_major(prob.data[0])], init_f=[f], init_s=[s], init_g=[g], **more)
    _same_bits(fp64_run(p), fp64_run(_host_twin(p)), (shape, k, lm))


# ---- 4. a mixed job, and a coupled job to convergence ----
def test_mixed_job_device_host_and_sparse_views():
    g = helpers.load_golden("g3_three_views_phi_psi_xi")
    prob = helpers.golden_problem(g)
    data = [_row_major(prob.data[0]), prob.data[1], sp.csc_matrix(prob.data[2])]
    p = _problem(prob, 5, data=data)
    p["init_f"][1], p["init_s"][1], p["init_g"][1] = (_row_major(a) for a in (prob.init_f[1], prob.init_s[1], prob.init_g[1]))
    _same_bits(fp64_run(p), fp64_run(_host_twin(p)), "g3")


def test_coupled_job_to_convergence_from_the_device():
    prob = helpers.coupled_problem([(70, 50), (64, 44), (56, 50)], 4, 103, phi_w=1.0, psi_w=0.5, xi_w=0.3)
    p = _problem(prob, None, data=[_row_major(x) for x in prob.data], init_f=[_row_major(a) for a in prob.init_f],
                 init_s=[_row_major(a) for a in prob.init_s], init_g=[_row_major(a) for a in prob.init_g])
    there, host = fp64_run(p, max_iters=3000), fp64_run(_host_twin(p), max_iters=3000)
    assert 1 < host["iters"] < 3000
    _same_bits(there, host, "convergence")


# ---- 5. results left on the device ----
def test_torch_output_is_the_numpy_output(edge_problem):
    p = _problem(edge_problem, SWEEPS, data=[_row_major(edge_problem.data[0])])
    there, host = fp64_run(p, output="torch"), fp64_run(p)
    for key in KEYS:
        t = there[key][0]
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == DEV
        if t.ndim == 2:
            assert t.stride() == (1, t.shape[0])                         # column-major, as get_factors_device wraps its own
    assert isinstance(there["all_error"], np.ndarray) and isinstance(there["iters"], int)
    _same_bits(there, host, "torch")
    _same_bits(fp64_run(_host_twin(p), output="torch"), host, "torch from host arrays")
    rc, cc = api._binary_clusters_device(there["f"][0], there["g"][0], there["s"][0])
    want_rc, want_cc = batched._binary_clusters(host["f"][0], host["g"][0], host["s"][0])
    assert rc.device == DEV and rc.dtype == torch.float64
    assert np.array_equal(_np(rc), want_rc) and np.array_equal(_np(cc), want_cc) and want_rc.sum() > 0


# ---- 6. resuming from the raw state ----
def test_resume_from_the_raw_state():
    prob = _single(300, 200, 17, 8)
    start = dict(data=[_row_major(prob.data[0])], init_f=[_row_major(prob.init_f[0])], init_s=[_row_major(prob.init_s[0])],
                 init_g=[_row_major(prob.init_g[0])])
    whole = fp64_run(_problem(prob, 20, **start), output="torch", return_state=True)
    first = fp64_run(_problem(prob, 12, **start), output="torch", return_state=True)
    f, s, g, lam, mu = first["state"][0]
    assert all(isinstance(t, torch.Tensor) and t.device == DEV and t.dtype == torch.float64 for t in (f, s, g, lam, mu))
    second = fp64_run(_problem(prob, 8, data=start["data"], init_f=[f], init_s=[s], init_g=[g], init_lam=[lam], init_mu=[mu]),
                      output="torch", return_state=True)
    joined = np.concatenate([first["all_error"], second["all_error"]])
    assert first["iters"] == 12 and second["iters"] == 8 and whole["iters"] == 20
    assert np.array_equal(joined, whole["all_error"]) and joined.tobytes() == whole["all_error"].tobytes()
    _same_bits(dict(second, all_error=joined, iters=20), whole, "outputs")
    for a, b in zip(second["state"][0], whole["state"][0]):
        assert np.array_equal(_np(a), _np(b)) and _np(a).tobytes() == _np(b).tobytes()
    # the raw state is not the normalised output, and the host route resumes from its values alike
    assert not np.array_equal(_np(whole["state"][0][0]), _np(whole["f"][0]))
    again = fp64_run(_host_twin(_problem(prob, 8, data=start["data"], init_f=[f], init_s=[s], init_g=[g], init_lam=[lam], init_mu=[mu])))
    _same_bits(again, dict(second, state=None), "host resume")


# ---- 7. dev == NULL through the new entry ----
@pytest.mark.parametrize("sparse_view", [False, True])
def test_null_dev_is_the_sparse_entry(edge_problem, sparse_view):
    lib = _lib.load()
    data = [sp.csc_matrix(edge_problem.data[0] * (edge_problem.data[0] > 0.002))] if sparse_view else list(edge_problem.data)
    p = _problem(edge_problem, SWEEPS, data=data)
    outs = []
    for entry in ("sparse", "device"):
        job, keep = _lib.GroupJob(), []
        spv = _lib.Fp64Sparse()
        spv.struct_size = C.sizeof(_lib.Fp64Sparse)
        out = engine._fill_group_job(job, p, 0, 100, keep, sp=spv)
        if entry == "sparse":
            rc = lib.resnmtf_fp64_run_sparse(0, C.byref(job), C.byref(spv), 1e-6, 100)
        else:
            rc = lib.resnmtf_fp64_run_device(0, C.byref(job), C.byref(spv), None, 1e-6, 100)
        assert rc == _lib.OK, lib.resnmtf_last_error(None)
        outs.append(engine._group_result(out))
    _same_bits(outs[1], outs[0], "dev == NULL")
    _same_bits(fp64_run(p), outs[0], "fp64_run")


# ---- 8. ordering with the caller's stream ----
def test_the_run_waits_for_the_callers_stream(edge_problem):
    x = torch.as_tensor(edge_problem.data[0], device=DEV)
    ballast = torch.ones((4096, 4096), dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(200):                # keeps the side stream busy while the view is still to be written
            ballast = ballast * 1.0000001
        view = (x * 2.0 + ballast[:129, :127] * 0.0) * 0.5              # produced last, on the side stream
        p = _problem(edge_problem, SWEEPS, data=[view])
        there = fp64_run(p, output="torch")                             # (its outputs are ordered on that stream too)
    torch.cuda.synchronize(DEV)
    assert np.array_equal(_np(view), edge_problem.data[0])
    _same_bits(there, fp64_run(_problem(edge_problem, SWEEPS)), "side stream")


# ---- 9. the API route ----
def test_api_route_from_the_device_initialisation():
    prob = helpers.coupled_problem([(120, 90), (100, 90)], 4, 5, phi_w=1.0, psi_w=0.5)
    k_vec, rs, cs = [4, 4], naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)
    common = dict(spurious=False, row_names=prob.row_names, col_names=prob.col_names, precision="fp64", seed=3)
    data = [_row_major(prob.data[0]), _row_major(prob.data[1], torch.float64).T.contiguous().T]
    res = api.res_nmtf_inner(data, rs, cs, None, None, None, k_vec, prob.phi, prob.xi, prob.psi, 20, fp64_device=True,
                             return_init=True, return_state=True, output="torch", **common)
    for key in ("output_f", "output_s", "output_g", "row_clusters", "col_clusters"):
        assert all(isinstance(t, torch.Tensor) and t.device == DEV and t.dtype == torch.float64 for t in res[key]), key
    assert all(isinstance(t, torch.Tensor) and t.device == DEV for st in res["init"] + res["state"] for t in st)
    init = [tuple(_np(t) for t in st) for st in res["init"]]
    host = api.res_nmtf_inner(prob.data, rs, cs, [i[0] for i in init], [i[1] for i in init], [i[2] for i in init], k_vec,
                              prob.phi, prob.xi, prob.psi, 20, init_lm=([i[3] for i in init], [i[4] for i in init]), **common)
    for key in ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "lambda", "mu"):
        for v in range(2):
            a, b = _np(res[key][v]), _np(host[key][v])
            assert np.array_equal(a, b, equal_nan=True) and np.asfortranarray(a).tobytes() == np.asfortranarray(b).tobytes(), (key, v)
    assert np.array_equal(res["All_Error"], host["All_Error"]) and res["Error"] == host["Error"]
    ref = O.res_nmtf_inner(prob.data, [i[0] for i in init], [i[1] for i in init], [i[2] for i in init], prob.phi, prob.xi,
                           prob.psi, row_names=prob.row_names, col_names=prob.col_names, n_iters=20,
                           init_lam=[i[3] for i in init], init_mu=[i[4] for i in init])
    for key in ("output_f", "output_g", "output_s"):
        for v in range(2):
            d = helpers.rel_fro(_np(res[key][v]), ref[key][v])
            assert d <= 1e-11, (key, v, d)
    assert float(np.max(np.abs(res["All_Error"] - ref["All_Error"]))) <= 1e-13
    # explicit factors and init_lm from the device, NumPy out: the host route's result again
    there = api.res_nmtf_inner(data, rs, cs, [st[0] for st in res["init"]], [st[1] for st in res["init"]],
                               [st[2] for st in res["init"]], k_vec, prob.phi, prob.xi, prob.psi, 20, fp64_device=True,
                               init_lm=([st[3] for st in res["init"]], [st[4] for st in res["init"]]), **common)
    for key in ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "lambda", "mu"):
        for v in range(2):
            assert isinstance(there[key][v], np.ndarray) and np.array_equal(there[key][v], host[key][v], equal_nan=True), (key, v)


# ---- 10. repeatability ----
def test_two_device_runs_give_the_same_bits():
    prob = _single(33, 257, 17, 11)
    f, s, g = _factors(prob, torch.float32)
    p = _problem(prob, 5, data=[_row_major(prob.data[0], torch.float32)], init_f=[f], init_s=[s], init_g=[g])
    _same_bits(fp64_run(p, output="torch"), fp64_run(p, output="torch"), "repeat")


# ---- 11. the refusals that need device memory: a refusal, never a launch ----
def _c_call(n, m, k, edit):
    rng = np.random.default_rng(0)
    prob = {"data": [rng.random((n, m)) + 0.1], "k": k, "init_f": [rng.random((n, k))], "init_s": [rng.random((k, k))],
            "init_g": [rng.random((m, k))], "n_iters": 2}
    job, keep = _lib.GroupJob(), []
    out = engine._fill_group_job(job, prob, 0, 100, keep)
    for key in KEYS:
        out[key][0][...] = -7.0
    d = _lib.Fp64Device()
    d.struct_size = C.sizeof(_lib.Fp64Device)
    edit(job, d)
    lib = _lib.load()
    rc = lib.resnmtf_fp64_run_device(0, C.byref(job), None, C.byref(d), 1e-6, 100)
    assert all(np.all(out[key][0] == -7.0) for key in KEYS)              # nothing was written
    return rc, lib.resnmtf_last_error(None)


def test_refuses_host_memory_and_a_tensor_too_short_for_its_shape():
    invalid = {name: c for c, name in _lib.ERR_NAMES.items()}["INVALID"]
    on_cpu = torch.ones((10, 8), dtype=torch.float64)

    def cpu_view(job, d):
        job.x[0] = C.POINTER(C.c_double)()
        d.x[0] = _lib.DeviceMatrix(on_cpu.data_ptr(), _lib.DTYPE_F64, 8, 1)
    rc, text = _c_call(10, 8, 2, cpu_view)
    assert rc == invalid and b"view 0: dev->x is not device memory of device 0" in text
    short = torch.ones(16, dtype=torch.float64, device=DEV)               # 128 bytes described as 1024 x 1024 doubles

    def short_view(job, d):
        job.x[0] = C.POINTER(C.c_double)()
        d.x[0] = _lib.DeviceMatrix(short.data_ptr(), _lib.DTYPE_F64, 1024, 1)
    rc, text = _c_call(1024, 1024, 2, short_view)
    assert rc == invalid and b"view 0: dev->x reaches beyond its allocation" in text
    with pytest.raises(ValueError, match="lives on cpu"):                 # the Python layer says it before the library
        engine._device_matrix(on_cpu, (10, 8), 0, "view 0")
    wrong = _problem(_single(20, 16, 2, 3), 2)
    wrong["init_f"], wrong["init_s"], wrong["init_g"] = ([torch.ones((19, 2), device=DEV)], [torch.ones((2, 2), device=DEV)],
                                                         [torch.ones((16, 2), device=DEV)])
    with pytest.raises(ValueError, match="expected shape"):
        fp64_run(wrong)
