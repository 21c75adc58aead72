"""GPU tests of the device-wide fp64 path (resnmtf_fp64_run) against the fp64 oracle from the same
initial factors: the goldens, single views at every padded-k class and tile edge, coupled problems, jobs beyond the
grouped limits, the grouped path on the same jobs, bitwise repeatability, the f32 engine, the three initial states of
``api.res_nmtf_inner(precision="fp64")`` and the guards of the C entry.

Bars (the grouped path's own): F, G, S <= 1e-11 relative Frobenius, All_Error <= 1e-13 absolute, lambda / mu rtol 1e-11,
with fixed counts of at most 30 sweeps; convergence jobs F, G <= 1e-8 and the oracle's stop sweep."""
import ctypes as C

import numpy as np
import pytest

import helpers
from oracle import resnmtf_oracle as O
from resnmtf_amd import _lib, api, batched, naming, synth
from resnmtf_amd.engine import fp64_plan, fp64_run, group_run
from resnmtf_amd.problem import pair_table
from resnmtf_amd.synth import Problem

pytestmark = pytest.mark.gpu

FIX_F, FIX_ERR, CONV_F, LM_RTOL = 1e-11, 1e-13, 1e-8, 1e-11
CLUSTER_EPS = 1e-4      # check_clusters' rule: a binary entry may differ only within this relative distance of 1/n
MAX_ITERS = 3000


def _problem(prob, n_iters):
    return {"data": prob.data, "k": prob.init_f[0].shape[1], "init_f": prob.init_f, "init_s": prob.init_s,
            "init_g": prob.init_g, "phi": prob.phi, "xi": prob.xi, "psi": prob.psi, "row_pairs": pair_table(prob.row_names),
            "col_pairs": pair_table(prob.col_names), "n_iters": n_iters}


def _oracle(prob, n_iters, max_iters=None):
    return O.res_nmtf_inner(prob.data, prob.init_f, prob.init_s, prob.init_g, prob.phi, prob.xi, prob.psi,
                            row_names=prob.row_names, col_names=prob.col_names, n_iters=n_iters, max_iters=max_iters)


def _single(n, m, k, seed):
    rng = np.random.default_rng(seed)
    kb = max(1, min(k, n, m))
    rb, cb = np.arange(n) * kb // n, np.arange(m) * kb // m
    x = 10.0 * (rb[:, None] == cb[None, :]) + 0.1 * np.abs(rng.standard_normal((n, m)))
    x = x / x.sum(axis=0)[None, :]
    f, s, g = synth.random_init(n, m, k, seed + 7)
    return Problem([x], [f], [s], [g], np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), k, "single",
                   row_names=[[f"r{i}" for i in range(n)]], col_names=[[f"c{j}" for j in range(m)]])


def _check(out, ref, n_views, fixed, what):
    """The bars of the module docstring; ``ref``: the oracle's result.  Returns (worst factor distance, worst error)."""
    assert out["iters"] == len(ref["All_Error"]), (what, out["iters"], len(ref["All_Error"]))
    bar = FIX_F if fixed else CONV_F
    worst = 0.0
    for key, rk in (("f", "output_f"), ("g", "output_g"), ("s", "output_s")):
        if not fixed and key == "s":
            continue
        for v in range(n_views):
            d = helpers.rel_fro(out[key][v], ref[rk][v])          # (NaN positions must coincide)
            worst = max(worst, d)
            assert d <= bar, (what, key, v, d)
    e = float(np.max(np.abs(out["all_error"] - ref["All_Error"])))
    if fixed:
        assert e <= FIX_ERR, (what, e)
        for v in range(n_views):
            np.testing.assert_allclose(out["lambda"][v], ref["lambda"][v], rtol=LM_RTOL, err_msg=str(what))
            np.testing.assert_allclose(out["mu"][v], ref["mu"][v], rtol=LM_RTOL, err_msg=str(what))
    return worst, e


# ---- 1. the goldens ----
@pytest.mark.parametrize("name", helpers.GOLDEN_NAMES)
def test_golden(name):
    g = helpers.load_golden(name)
    out = fp64_run(_problem(helpers.golden_problem(g), g["n_iters"]))
    assert out["iters"] == g["n_iters"]
    for key, gk in (("f", "out_f"), ("g", "out_g"), ("s", "out_s")):
        for v in range(g["n_views"]):
            d = helpers.rel_fro(out[key][v], g[gk][v])              # (NaN positions must coincide: g4)
            assert d <= FIX_F, (name, key, v, d)
    assert float(np.max(np.abs(out["all_error"] - g["all_error"]))) <= FIX_ERR
    for v in range(g["n_views"]):
        np.testing.assert_allclose(out["lambda"][v], g["lam"][v], rtol=LM_RTOL)
        np.testing.assert_allclose(out["mu"][v], g["mu"][v], rtol=LM_RTOL)


# ---- 2. single views at the edges: every padded-k class on both sides of its edge, the tile edges, a split contraction ----
# (n, m, k, sweeps, padded k).  129 x 127: one above / one below a multiple of the 128-row product tile (and of the 64-row
# residual and update tiles).  33 x 257 and 257 x 33: a contraction of five LDS stages over one row tile, split five ways.
EDGES = [(2, 2, 1, 20, 16), (5, 4, 3, 30, 16), (16, 16, 15, 20, 16), (16, 16, 16, 20, 16), (17, 15, 15, 20, 16),
         (33, 257, 17, 25, 32), (33, 257, 32, 20, 32), (33, 257, 33, 20, 48), (257, 33, 16, 20, 16), (257, 33, 33, 20, 48),
         (64, 100, 48, 20, 48), (64, 100, 49, 20, 64), (64, 100, 64, 20, 64), (7, 300, 1, 30, 16), (7, 300, 7, 30, 16),
         (129, 127, 16, 20, 16), (129, 127, 64, 15, 64), (300, 200, 17, 25, 32)]


@pytest.mark.parametrize("n,m,k,sweeps,kp", EDGES)
def test_single_view_edges(n, m, k, sweeps, kp):
    plan = fp64_plan(n, m, k)
    assert plan["kp"] == kp                                             # the kernel instance this case reaches
    assert plan["xg"][0] == -(-n // 128) and plan["xtf"][0] == -(-m // 128) and plan["resid"][0] == -(-n // 64)
    if (n, m) == (33, 257):
        assert plan["xg"][1] == 5 and plan["xtf"][1] == 1 and plan["resid"][1] > 1      # slab partials summed in split order
    if (n, m) == (257, 33):
        assert plan["xtf"][1] == 5 and plan["xg"][1] == 1
    if (n, m) == (129, 127):
        assert plan["xg"][0] == 2 and plan["xtf"][0] == 1 and plan["resid"][0] == 3
    prob = _single(n, m, k, 100 + n + m + k)
    _check(fp64_run(_problem(prob, sweeps)), _oracle(prob, sweeps), 1, True, (n, m, k))


def test_plan_depends_on_the_shape_alone():
    assert fp64_plan(10000, 2000, 16) == fp64_plan(10000, 2000, 16)
    a, b = fp64_plan(10000, 2000, 3), fp64_plan(10000, 2000, 16)
    assert a["xg"] == b["xg"] and a["xtf"] == b["xtf"] and a["xg"][1] > 1 and a["xtf"][1] > 1
    with pytest.raises(_lib.ResnmtfError):
        fp64_plan(10, 10, 11)
    with pytest.raises(_lib.ResnmtfError):
        fp64_plan(100, 100, 65)


# ---- 3. coupled problems: phi, psi, xi apart and together, partial overlap, an NA pair, same-order views, 4 views,
# k = 20 with the whole-psi branch; each as a fixed count and to convergence ----
COUPLED = [
    ([(50, 40), (46, 40)], 3, dict(phi_w=1.0), 30),
    ([(60, 44), (60, 50)], 4, dict(psi_w=0.7), 30),
    ([(40, 30), (40, 30)], 2, dict(xi_w=0.5), 30),
    ([(70, 50), (64, 44), (56, 50)], 4, dict(phi_w=1.0, psi_w=0.5, xi_w=0.3), 25),
    ([(48, 40), (44, 40), (40, 24)], 20, dict(psi_w=1.0), 20),
    ([(80, 60), (70, 60), (90, 50), (60, 40)], 5, dict(phi_w=0.8, psi_w=0.8, na_pairs=[(0, 2)]), 25),
    ([(30, 20), (30, 20), (30, 20), (30, 20)], 3, dict(phi_w=1.0, xi_w=1.0, same_order_views=(0, 1, 2, 3)), 30),
    ([(200, 150), (180, 150)], 8, dict(phi_w=2.0, overlap=0.5), 25),
    ([(64, 48), (64, 48)], 10, dict(psi_w=2.0, xi_w=0.2), 25),
]


@pytest.fixture(scope="module")
def coupled():
    return [helpers.coupled_problem(shapes, k, 100 + i, **kw) for i, (shapes, k, kw, _) in enumerate(COUPLED)]


@pytest.mark.parametrize("idx", range(len(COUPLED)))
@pytest.mark.parametrize("mode", ["fixed", "convergence"])
def test_coupled(coupled, idx, mode):
    prob = coupled[idx]
    n_iters = COUPLED[idx][3] if mode == "fixed" else None
    out = fp64_run(_problem(prob, n_iters), max_iters=MAX_ITERS)
    _check(out, _oracle(prob, n_iters, MAX_ITERS), len(prob.data), n_iters is not None, (idx, mode))


def test_max_iters_stops_convergence_mode():
    prob = _single(60, 40, 3, 4)
    out = fp64_run(_problem(prob, None), max_iters=7)
    ref = _oracle(prob, None, 7)
    assert out["iters"] == 7 and len(ref["All_Error"]) == 7
    assert float(np.max(np.abs(out["all_error"] - ref["All_Error"]))) <= FIX_ERR
    assert fp64_run(_problem(prob, 50), max_iters=7)["iters"] == 7       # max_iters bounds the fixed count too


# ---- 4. beyond the grouped limits ----
def _beyond(which):
    if which == "k40":
        return _single(2304, 1900, 40, 41), 10
    if which == "k64":
        return _single(2304, 1900, 64, 42), 30
    return helpers.coupled_problem([(2304, 1000), (2304, 1000)], 33, 43, phi_w=1.0), 10


@pytest.mark.parametrize("which", ["k40", "k64", "pair_k33"])
def test_beyond_the_grouped_limits(which):
    prob, sweeps = _beyond(which)
    out = fp64_run(_problem(prob, sweeps))
    worst, e = _check(out, _oracle(prob, sweeps), len(prob.data), True, which)
    print(f"{which}: worst rel-Frobenius {worst:.2e}, max |d All_Error| {e:.2e}")
    job = batched.Job(prob.data, prob.init_f[0].shape[1], prob.phi, prob.xi, prob.psi, sweeps, row_names=prob.row_names,
                      col_names=prob.col_names)
    with pytest.raises(ValueError):
        batched.run_jobs_grouped([job], pre_processed=True, inits=[(prob.init_f, prob.init_s, prob.init_g)])


# ---- 5. against the grouped path: ten jobs inside its limits, both at the bars (their bits may differ) ----
def test_both_fp64_paths_meet_the_oracle(coupled):
    jobs = [(_single(60, 40, 3, 4), 30), (_single(1000, 400, 8, 6), 20), (_single(1000, 400, 32, 7), 15),
            (_single(300, 200, 16, 8), 25), (_single(100, 64, 32, 9), 20), (_single(33, 257, 17, 11), 25),
            (coupled[0], 30), (coupled[3], 25), (coupled[5], 25), (coupled[7], 25)]
    probs = [_problem(p, n) for p, n in jobs]
    grouped = group_run(probs)
    for i, ((prob, n), pd, g) in enumerate(zip(jobs, probs, grouped)):
        ref = _oracle(prob, n)
        _check(fp64_run(pd), ref, len(prob.data), True, ("fp64", i))
        _check(g, ref, len(prob.data), True, ("grouped", i))


# ---- 6. bitwise repeatability ----
def _same_bits(a, b):
    assert a["iters"] == b["iters"]
    assert a["all_error"].tobytes() == b["all_error"].tobytes()
    for key in ("f", "s", "g", "lambda", "mu"):
        for x, y in zip(a[key], b[key]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), key


def test_two_runs_give_the_same_bits(coupled):
    assert fp64_plan(33, 257, 17)["xg"][1] > 1
    split = _problem(_single(33, 257, 17, 11), 25)
    _same_bits(fp64_run(split), fp64_run(split))
    conv = _problem(coupled[3], None)
    _same_bits(fp64_run(conv, max_iters=MAX_ITERS), fp64_run(conv, max_iters=MAX_ITERS))


# ---- 7. against the f32 engine: 2000 x 500, k = 16, 100 fixed sweeps from one explicit start ----
def _api_call(prob, n_iters, **kw):
    k = prob.init_f[0].shape[1]
    return api.res_nmtf_inner(prob.data, naming.shared_names(prob.row_names), naming.shared_names(prob.col_names),
                              prob.init_f, prob.init_s, prob.init_g, [k] * len(prob.data), prob.phi, prob.xi, prob.psi,
                              n_iters, spurious=False, row_names=prob.row_names, col_names=prob.col_names, **kw)


def test_fp64_against_the_f32_engine():
    prob = _single(2000, 500, 16, 77)
    f32 = _api_call(prob, 100)
    f64 = _api_call(prob, 100, precision="fp64")
    ref = _oracle(prob, 100)
    assert list(f64.keys()) == list(f32.keys())
    for key in ("output_f", "output_g", "output_s"):
        d32 = helpers.rel_fro(f64[key][0], f32[key][0])
        d64 = helpers.rel_fro(f64[key][0], ref[key][0])
        print(f"{key}: fp64 vs f32 engine {d32:.2e}, fp64 vs oracle {d64:.2e}")
        assert d32 <= 2e-5 and d64 <= 1e-11, (key, d32, d64)
    e32 = float(np.max(np.abs(f64["All_Error"] - f32["All_Error"])))
    print(f"All_Error: fp64 vs f32 engine {e32:.2e}, fp64 vs oracle {float(np.max(np.abs(f64['All_Error'] - ref['All_Error']))):.2e}")
    assert e32 <= 2e-5 and len(f64["All_Error"]) == 100
    # the binary clusters: identical off the 1/n threshold (check_clusters' rule)
    rel = np.argmax(ref["output_s"][0], axis=0)
    assert np.array_equal(np.argmax(f64["output_s"][0], axis=0), rel) and np.array_equal(np.argmax(f32["output_s"][0], axis=0), rel)
    for key, fac in (("row_clusters", ref["output_f"][0][:, rel]), ("col_clusters", ref["output_g"][0])):
        on_threshold = np.abs(fac * fac.shape[0] - 1.0) < CLUSTER_EPS
        mism = np.asarray(f64[key][0]) != np.asarray(f32[key][0])
        assert not (mism & ~on_threshold).any(), key
        assert not ((np.asarray(f64[key][0]) != ref[key][0]) & ~on_threshold).any(), key


# ---- 8. api.res_nmtf_inner(precision="fp64"): the three initial states ----
def _oracle_from_init(prob, init, n_iters):
    return O.res_nmtf_inner(prob.data, [i[0] for i in init], [i[1] for i in init], [i[2] for i in init], prob.phi, prob.xi,
                            prob.psi, row_names=prob.row_names, col_names=prob.col_names, n_iters=n_iters,
                            init_lam=[i[3] for i in init], init_mu=[i[4] for i in init])


def _check_api(res, ref, n_views, what):
    out = {"f": res["output_f"], "g": res["output_g"], "s": res["output_s"], "lambda": res["lambda"], "mu": res["mu"],
           "all_error": res["All_Error"], "iters": len(res["All_Error"])}
    _check(out, ref, n_views, True, what)


@pytest.mark.parametrize("start", ["device", "host", "explicit"])
def test_api_initial_states(start):
    prob = helpers.coupled_problem([(120, 90), (100, 90)], 4, 5, phi_w=1.0, psi_w=0.5)
    k_vec, rs, cs = [4, 4], naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)
    common = dict(spurious=False, row_names=prob.row_names, col_names=prob.col_names, precision="fp64", return_init=True, seed=3)
    if start == "explicit":
        rng = np.random.default_rng(9)
        lm = ([rng.random(4) + 0.5 for _ in range(2)], [rng.random(4) + 0.5 for _ in range(2)])
        res = api.res_nmtf_inner(prob.data, rs, cs, prob.init_f, prob.init_s, prob.init_g, k_vec, prob.phi, prob.xi, prob.psi,
                                 20, init_lm=lm, **common)
        for v in range(2):
            assert np.array_equal(res["init"][v][3], lm[0][v]) and np.array_equal(res["init"][v][0], prob.init_f[v])
    else:
        res = api.res_nmtf_inner(prob.data, rs, cs, None, None, None, k_vec, prob.phi, prob.xi, prob.psi, 20,
                                 host_init=(start == "host"), **common)
    assert len(res["init"]) == 2 and len(res["init"][0]) == 5
    _check_api(res, _oracle_from_init(prob, res["init"], 20), 2, start)


# ---- 9. the guards through the C entry ----
def _c_job(n=10, m=8, k=2, V=1):
    rng = np.random.default_rng(0)
    keep = []
    j = _lib.GroupJob()
    j.struct_size = C.sizeof(_lib.GroupJob)
    j.n_views, j.k, j.n_iters = V, k, 5
    dp = C.POINTER(C.c_double)
    outs_all = []
    for v in range(V):
        arrs = [np.asfortranarray(rng.random(s) + 0.1) for s in ((n, m), (n, k), (k, k), (m, k))]
        outs = [np.full(s, -7.0, order="F") for s in ((n, k), (k, k), (m, k), (k,), (k,))]
        keep += arrs + outs
        outs_all += outs
        j.n_rows[v], j.n_cols[v] = n, m
        j.x[v], j.f0[v], j.s0[v], j.g0[v] = (a.ctypes.data_as(dp) for a in arrs)
        j.f_out[v], j.s_out[v], j.g_out[v], j.lambda_out[v], j.mu_out[v] = (a.ctypes.data_as(dp) for a in outs)
    err = np.full(16, -7.0); it = np.full(1, -7, dtype=np.int32)
    keep += [err, it]
    outs_all += [err, it]
    j.all_error, j.err_capacity, j.iters_done = err.ctypes.data_as(dp), 16, it.ctypes.data_as(C.POINTER(C.c_int))
    return j, keep, outs_all


def test_c_level_refusals():
    lib = _lib.load()
    code = {name: c for c, name in _lib.ERR_NAMES.items()}
    INVALID, ALLOC = code["INVALID"], code["ALLOC"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def run(j, tol=1e-6, max_iters=100):
        return lib.resnmtf_fp64_run(0, C.byref(j), tol, max_iters)

    def refused(bad, outs, word, want=INVALID):
        assert run(bad) == want
        assert word in lib.resnmtf_last_error(None), lib.resnmtf_last_error(None)
        assert all(np.all(o == -7) for o in outs)                       # a refusal writes no output

    j, keep, outs = _c_job()
    assert lib.resnmtf_fp64_run(0, None, 1e-6, 10) == INVALID
    assert run(j, max_iters=0) == INVALID and run(j, tol=float("inf")) == INVALID
    bad = _lib.GroupJob.from_buffer_copy(j); bad.struct_size = 8
    refused(bad, outs, b"struct_size")
    bad = _lib.GroupJob.from_buffer_copy(j); bad.k = 65
    refused(bad, outs, b"k must be in [1, 64]")
    bad = _lib.GroupJob.from_buffer_copy(j); bad.k = 9                  # above n_cols = 8
    refused(bad, outs, b"exceeds a view dimension")
    bad = _lib.GroupJob.from_buffer_copy(j); bad.n_views = 9
    refused(bad, outs, b"n_views")
    xbad = np.asfortranarray(np.ones((10, 8))); xbad[3, 3] = np.nan
    bad = _lib.GroupJob.from_buffer_copy(j); bad.x[0] = xbad.ctypes.data_as(dp)
    refused(bad, outs, b"non-finite")
    bad = _lib.GroupJob.from_buffer_copy(j); bad.err_capacity = 4
    refused(bad, outs, b"err_capacity")
    bad = _lib.GroupJob.from_buffer_copy(j); bad.n_iters = -1
    refused(bad, outs, b"n_iters")
    j2, keep2, outs2 = _c_job(V=2)
    phi = np.asfortranarray([[0.0, -1.0], [-1.0, 0.0]])
    bad = _lib.GroupJob.from_buffer_copy(j2); bad.phi = phi.ctypes.data_as(dp)
    refused(bad, outs2, b"non-negative")
    iv, iw = np.array([0, 10], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    bad = _lib.GroupJob.from_buffer_copy(j2)
    bad.row_count[0][1] = 2
    bad.row_idx_v[0][1] = iv.ctypes.data_as(ip); bad.row_idx_w[0][1] = iw.ctypes.data_as(ip)
    refused(bad, outs2, b"out of range")
    # an absurd shape: the descriptor only -- refused on its byte count, before the data behind it would be read
    bad = _lib.GroupJob.from_buffer_copy(j); bad.n_rows[0], bad.n_cols[0] = 1 << 30, 1 << 30
    refused(bad, outs, b"bytes asked for", want=ALLOC)
    assert run(j) == _lib.OK and run(j2) == _lib.OK
    assert not any(np.any(o == -7) for o in outs[:5]) and outs[-1][0] == 5
