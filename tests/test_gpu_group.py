"""GPU tests of the grouped path (resnmtf_group_run: one workgroup per job, fp64): the golden problems in one batch,
a mixed batch of 40+ jobs against the fp64 oracle, independence of a job's bits from the rest of the batch, a batch
larger than the device, the guards, agreement with the f32 engine, and the grouped spurious check."""
import ctypes as C

import numpy as np
import pytest

import helpers
from oracle import resnmtf_oracle as O
from resnmtf_amd import _lib, api, batched, naming, spurious
from resnmtf_amd.engine import group_run
from resnmtf_amd.problem import pair_table

pytestmark = pytest.mark.gpu

FIX_F, FIX_ERR, CONV_F = 1e-11, 1e-13, 1e-8


def _problem(prob, n_iters):
    rp, cp = pair_table(prob.row_names), pair_table(prob.col_names)
    return {"data": prob.data, "k": prob.init_f[0].shape[1], "init_f": prob.init_f, "init_s": prob.init_s,
            "init_g": prob.init_g, "phi": prob.phi, "xi": prob.xi, "psi": prob.psi, "row_pairs": rp, "col_pairs": cp,
            "n_iters": n_iters}


def _oracle(prob, n_iters, max_iters=None):
    return O.res_nmtf_inner(prob.data, prob.init_f, prob.init_s, prob.init_g, prob.phi, prob.xi, prob.psi,
                            row_names=prob.row_names, col_names=prob.col_names, n_iters=n_iters, max_iters=max_iters)


def _single(n, m, k, seed):
    from resnmtf_amd import synth
    from resnmtf_amd.synth import Problem
    rng = np.random.default_rng(seed)
    kb = max(1, min(k, n, m))
    rb, cb = np.arange(n) * kb // n, np.arange(m) * kb // m
    x = 10.0 * (rb[:, None] == cb[None, :]) + 0.1 * np.abs(rng.standard_normal((n, m)))
    x = x / x.sum(axis=0)[None, :]
    f, s, g = synth.random_init(n, m, k, seed + 7)
    return Problem([x], [f], [s], [g], np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), k, "single",
                   row_names=[[f"r{i}" for i in range(n)]], col_names=[[f"c{j}" for j in range(m)]])


def _mixed():
    """(problem, n_iters) pairs: 1-4 views, 2 x 2 up to 1000 x 400, k 1..32, phi / psi / xi couplings, partial and NA
    overlaps, fixed-count and convergence jobs."""
    cp = helpers.coupled_problem
    out = [
        (_single(2, 2, 1, 1), 20), (_single(2, 3, 2, 2), 20), (_single(5, 4, 3, 3), 30), (_single(60, 40, 3, 4), 30),
        (_single(180, 180, 3, 5), None), (_single(1000, 400, 8, 6), 20), (_single(1000, 400, 32, 7), 15),
        (_single(300, 200, 16, 8), 25), (_single(100, 64, 32, 9), 20), (_single(64, 100, 9, 10), None),
        (_single(33, 257, 17, 11), 25), (_single(257, 33, 5, 12), None), (_single(7, 300, 4, 13), 30),
        (_single(90, 60, 1, 14), None), (_single(40, 40, 20, 15), 20), (_single(120, 80, 12, 16), 25),
    ]
    specs = [
        ([(50, 40), (46, 40)], 3, dict(phi_w=1.0), 30), ([(50, 40), (46, 40)], 3, dict(phi_w=1.0), None),
        ([(60, 44), (60, 50)], 4, dict(psi_w=0.7), 30), ([(60, 44), (60, 50)], 4, dict(psi_w=0.7), None),
        ([(40, 30), (40, 30)], 2, dict(xi_w=0.5), 30), ([(40, 30), (40, 30)], 2, dict(xi_w=0.5), None),
        ([(70, 50), (64, 44), (56, 50)], 4, dict(phi_w=1.0, psi_w=0.5, xi_w=0.3), 25),
        ([(70, 50), (64, 44), (56, 50)], 4, dict(phi_w=1.0, psi_w=0.5, xi_w=0.3), None),
        ([(48, 40), (44, 40), (40, 24)], 20, dict(psi_w=1.0), 20),
        ([(80, 60), (70, 60), (90, 50), (60, 40)], 5, dict(phi_w=0.8, psi_w=0.8, na_pairs=[(0, 2)]), 25),
        ([(80, 60), (70, 60), (90, 50), (60, 40)], 5, dict(phi_w=0.8, psi_w=0.8, na_pairs=[(0, 2)]), None),
        ([(30, 20), (30, 20), (30, 20), (30, 20)], 3, dict(phi_w=1.0, xi_w=1.0, same_order_views=(0, 1, 2, 3)), 30),
        ([(200, 150), (180, 150)], 8, dict(phi_w=2.0, overlap=0.5), 25),
        ([(200, 150), (180, 150)], 8, dict(phi_w=2.0, overlap=0.5), None),
        ([(400, 300), (350, 300)], 16, dict(phi_w=1.0, psi_w=1.0), 15),
        ([(500, 400), (450, 380), (300, 200)], 32, dict(phi_w=0.5, psi_w=0.5, xi_w=0.5), 10),
        ([(12, 10), (10, 12)], 2, dict(phi_w=1.0, psi_w=1.0), 30),
        ([(12, 10), (10, 12)], 2, dict(phi_w=1.0, psi_w=1.0), None),
        ([(100, 80), (100, 80), (100, 80)], 6, dict(phi_w=1.0, na_pairs=[(1, 2)]), 25),
        ([(100, 80), (100, 80), (100, 80)], 6, dict(phi_w=1.0, na_pairs=[(1, 2)]), None),
        ([(64, 48), (64, 48)], 10, dict(psi_w=2.0, xi_w=0.2), 25),
        ([(64, 48), (64, 48)], 10, dict(psi_w=2.0, xi_w=0.2), None),
        ([(150, 90), (120, 90), (100, 70), (90, 60)], 7, dict(phi_w=0.5, psi_w=0.5, xi_w=0.5), 20),
        ([(150, 90), (120, 90), (100, 70), (90, 60)], 7, dict(phi_w=0.5, psi_w=0.5, xi_w=0.5), None),
        ([(25, 25), (25, 25)], 1, dict(phi_w=1.0), 30),
    ]
    for i, (shapes, k, kw, n_iters) in enumerate(specs):
        out.append((cp(shapes, k, 100 + i, **kw), n_iters))
    return out


MAX_ITERS = 3000


@pytest.fixture(scope="module")
def mixed():
    jobs = _mixed()
    assert len(jobs) >= 40
    probs = [_problem(p, n) for p, n in jobs]
    first = group_run(probs, max_iters=MAX_ITERS)
    again = group_run(probs, max_iters=MAX_ITERS)
    rev = group_run(probs[::-1], max_iters=MAX_ITERS)[::-1]
    refs = [_oracle(p, n, MAX_ITERS) for p, n in jobs]
    return jobs, probs, first, again, rev, refs


def _same_bits(a, b):
    assert a["iters"] == b["iters"]
    assert a["all_error"].tobytes() == b["all_error"].tobytes()
    for key in ("f", "s", "g", "lambda", "mu"):
        for x, y in zip(a[key], b[key]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), key


def test_goldens_in_one_batch():
    gs = [helpers.load_golden(name) for name in helpers.GOLDEN_NAMES]
    probs = [_problem(helpers.golden_problem(g), g["n_iters"]) for g in gs]
    outs = group_run(probs)
    for name, g, out in zip(helpers.GOLDEN_NAMES, gs, outs):
        assert out["iters"] == g["n_iters"], name
        for key, gk in (("f", "out_f"), ("g", "out_g"), ("s", "out_s")):
            for v in range(g["n_views"]):
                d = helpers.rel_fro(out[key][v], g[gk][v])          # (NaN positions must coincide: g4)
                assert d <= FIX_F, (name, key, v, d)
        assert float(np.max(np.abs(out["all_error"] - g["all_error"]))) <= FIX_ERR, name
        for v in range(g["n_views"]):
            np.testing.assert_allclose(out["lambda"][v], g["lam"][v], rtol=1e-11)
            np.testing.assert_allclose(out["mu"][v], g["mu"][v], rtol=1e-11)


def _cluster_agree(res_rc, ref_rc, f_ref):
    """Binary clusters identical except at rows where |F n - 1| < 1e-9 (a threshold tie)."""
    n = f_ref.shape[0]
    tie = np.abs(f_ref * n - 1.0) < 1e-9
    diff = res_rc != ref_rc
    return not diff.any() or bool(np.all(tie.any(axis=1)[diff.any(axis=1)]))


def test_mixed_batch_matches_oracle(mixed):
    jobs, probs, first, _, _, refs = mixed
    worst_fix, worst_conv, worst_err = 0.0, 0.0, 0.0
    for i, ((prob, n_iters), out, ref) in enumerate(zip(jobs, first, refs)):
        assert out["iters"] == len(ref["All_Error"]), (i, out["iters"], len(ref["All_Error"]))
        bar = FIX_F if n_iters is not None else CONV_F
        for key, rk in (("f", "output_f"), ("g", "output_g"), ("s", "output_s")):
            for v in range(len(prob.data)):
                d = helpers.rel_fro(out[key][v], ref[rk][v])
                assert d <= bar, (i, key, v, d)
                if n_iters is None:
                    worst_conv = max(worst_conv, d)
                else:
                    worst_fix = max(worst_fix, d)
        if n_iters is not None:
            e = float(np.max(np.abs(out["all_error"] - ref["All_Error"])))
            worst_err = max(worst_err, e)
            assert e <= FIX_ERR, (i, e)
        res = batched._binary_clusters
        for v in range(len(prob.data)):
            rc, cc = res(out["f"][v], out["g"][v], out["s"][v])
            assert _cluster_agree(rc, ref["row_clusters"][v], ref["output_f"][v][:, np.argmax(ref["output_s"][v], axis=0)]), (i, v)
            assert _cluster_agree(cc, ref["col_clusters"][v], ref["output_g"][v]), (i, v)
    print(f"worst rel-Frobenius: fixed {worst_fix:.2e}, convergence {worst_conv:.2e}; worst |d All_Error| {worst_err:.2e}")


@pytest.mark.parametrize("idx", [0, 21, 39])
def test_job_bits_do_not_depend_on_the_batch(mixed, idx):
    _, probs, first, again, rev, _ = mixed
    alone = group_run([probs[idx]], max_iters=MAX_ITERS)[0]
    for other in (first[idx], again[idx], rev[idx]):
        _same_bits(alone, other)


def test_batch_larger_than_the_device():
    rng = np.random.default_rng(5)
    probs = []
    for q in range(600):
        n, m, k = int(rng.integers(8, 60)), int(rng.integers(8, 60)), int(rng.integers(1, 8))
        probs.append(_problem(_single(n, m, k, 1000 + q), 40 if q % 2 else None))
    outs = group_run(probs, max_iters=500)
    assert len(outs) == 600 and all(o["iters"] >= 1 for o in outs)
    for q in rng.choice(600, 8, replace=False):
        _same_bits(group_run([probs[q]], max_iters=500)[0], outs[q])


def test_max_iters_stops_convergence_mode():
    prob = _single(60, 40, 3, 4)
    out = group_run([_problem(prob, None)], max_iters=7)[0]
    ref = _oracle(prob, None, 7)
    assert out["iters"] == 7 and len(ref["All_Error"]) == 7
    assert float(np.max(np.abs(out["all_error"] - ref["All_Error"]))) <= FIX_ERR
    fixed = group_run([_problem(prob, 50)], max_iters=7)[0]          # max_iters bounds the fixed count too
    assert fixed["iters"] == 7


def _c_job(n=10, m=8, k=2, V=1):
    rng = np.random.default_rng(0)
    keep = []
    j = _lib.GroupJob()
    j.struct_size = C.sizeof(_lib.GroupJob)
    j.n_views, j.k, j.n_iters = V, k, 5
    dp = C.POINTER(C.c_double)
    for v in range(V):
        arrs = [np.asfortranarray(rng.random(s) + 0.1) for s in ((n, m), (n, k), (k, k), (m, k))]
        outs = [np.zeros(s, order="F") for s in ((n, k), (k, k), (m, k), (k,), (k,))]
        keep += arrs + outs
        j.n_rows[v], j.n_cols[v] = n, m
        j.x[v], j.f0[v], j.s0[v], j.g0[v] = (a.ctypes.data_as(dp) for a in arrs)
        j.f_out[v], j.s_out[v], j.g_out[v], j.lambda_out[v], j.mu_out[v] = (a.ctypes.data_as(dp) for a in outs)
    err = np.zeros(16); it = np.zeros(1, dtype=np.int32)
    keep += [err, it]
    j.all_error, j.err_capacity, j.iters_done = err.ctypes.data_as(dp), 16, it.ctypes.data_as(C.POINTER(C.c_int))
    return j, keep


def test_c_level_refusals():
    lib = _lib.load()
    INVALID = next(c for c, name in _lib.ERR_NAMES.items() if name == "INVALID")     # RESNMTF_ERR_INVALID

    def run(j, tol=1e-6, max_iters=100, n=1):
        arr = (_lib.GroupJob * 1)(j)
        return lib.resnmtf_group_run(0, n, arr, tol, max_iters)

    j, keep = _c_job()
    assert run(j) == _lib.OK
    assert lib.resnmtf_group_run(0, 0, None, 1e-6, 10) == _lib.OK
    assert lib.resnmtf_group_run(0, -1, None, 1e-6, 10) == INVALID
    assert lib.resnmtf_group_run(0, 1, None, 1e-6, 10) == INVALID
    assert run(j, max_iters=0) == INVALID
    assert run(j, tol=float("nan")) == INVALID
    bad = _lib.GroupJob.from_buffer_copy(j); bad.struct_size = 8
    assert run(bad) == INVALID and b"struct_size" in lib.resnmtf_last_error(None)
    bad = _lib.GroupJob.from_buffer_copy(j); bad.n_views = 9
    assert run(bad) == INVALID and b"n_views" in lib.resnmtf_last_error(None)
    for k in (0, 33):
        bad = _lib.GroupJob.from_buffer_copy(j); bad.k = k
        assert run(bad) == INVALID and b"k must be" in lib.resnmtf_last_error(None)
    bad = _lib.GroupJob.from_buffer_copy(j); bad.n_rows[0], bad.n_cols[0] = 4096, 1025     # no data needed: refused first
    assert run(bad) == INVALID and b"2^22" in lib.resnmtf_last_error(None)
    bad = _lib.GroupJob.from_buffer_copy(j); bad.err_capacity = 4
    assert run(bad) == INVALID and b"err_capacity" in lib.resnmtf_last_error(None)
    bad = _lib.GroupJob.from_buffer_copy(j); bad.n_iters = -1
    assert run(bad) == INVALID
    bad = _lib.GroupJob.from_buffer_copy(j); bad.g0[0] = None
    assert run(bad) == INVALID and b"NULL" in lib.resnmtf_last_error(None)
    xbad = np.asfortranarray(np.ones((10, 8))); xbad[3, 3] = np.nan
    bad = _lib.GroupJob.from_buffer_copy(j); bad.x[0] = xbad.ctypes.data_as(C.POINTER(C.c_double))
    assert run(bad) == INVALID and b"non-finite" in lib.resnmtf_last_error(None)
    j2, keep2 = _c_job(V=2)
    phi = np.asfortranarray([[0.0, -1.0], [-1.0, 0.0]])
    bad = _lib.GroupJob.from_buffer_copy(j2); bad.phi = phi.ctypes.data_as(C.POINTER(C.c_double))
    assert run(bad) == INVALID and b"non-negative" in lib.resnmtf_last_error(None)
    diag = np.asfortranarray([[1.0, 0.0], [0.0, 0.0]])
    bad = _lib.GroupJob.from_buffer_copy(j2); bad.psi = diag.ctypes.data_as(C.POINTER(C.c_double))
    assert run(bad) == INVALID and b"diagonal" in lib.resnmtf_last_error(None)
    iv, iw = np.array([0, 10], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    bad = _lib.GroupJob.from_buffer_copy(j2)
    bad.row_count[0][1] = 2
    bad.row_idx_v[0][1] = iv.ctypes.data_as(C.POINTER(C.c_int)); bad.row_idx_w[0][1] = iw.ctypes.data_as(C.POINTER(C.c_int))
    assert run(bad) == INVALID and b"out of range" in lib.resnmtf_last_error(None)
    assert run(j2) == _lib.OK
    with pytest.raises(_lib.ResnmtfError):
        group_run([{"data": [np.ones((10, 8))], "k": 40, "init_f": [np.ones((10, 40))], "init_s": [np.ones((40, 40))],
                    "init_g": [np.ones((8, 40))], "n_iters": 3}])


def _planted(seed):
    rng = np.random.default_rng(seed)
    rc = np.zeros((180, 3)); cc = np.zeros((180, 3))
    for i in range(3):
        rc[i * 60:(i + 1) * 60, i] = 1
        cc[i * 60:(i + 1) * 60, i] = 1
    return rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + 0.1 * np.abs(rng.normal(size=(180, 180))), rc, cc


def test_reference_planted_test_through_grouped_path():
    """test-resnmtf.R:98-118 ("resnmtf runs with no stability and no spurious removal") through run_jobs_grouped."""
    x1, rc, cc = _planted(1)
    x2, _, _ = _planted(2)
    res = batched.run_jobs_grouped([batched.Job([x1, x2], 3, seed=3)])[0]
    np.testing.assert_allclose(res["output_f"][0].sum(0), np.ones(3), atol=1e-12)
    np.testing.assert_allclose(res["output_g"][0].sum(0), np.ones(3), atol=1e-12)
    recon = res["output_f"][0] @ res["output_s"][0] @ res["output_g"][0].T
    assert np.mean(recon.sum(0) - 1.0) < 1e-3
    assert len(res["output_f"]) == 2 and res["output_f"][0].shape == (180, 3)
    for v in range(2):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))
    assert res["bisil"] is None and np.isfinite(res["Error"]) and len(res["All_Error"]) > 1


def test_k_sweep_agrees_with_f32_engine():
    x1, _, _ = _planted(1)
    x2, _, _ = _planted(2)
    jobs = batched.k_sweep_jobs([x1, x2], 3, 8, n_iters=200, seed=0)
    data = naming.check_data([x1, x2])
    inits = [api.svd_init(data, [j.k_val] * 2, j.seed) for j in jobs]
    grouped = batched.run_jobs_grouped(jobs, inits=inits)
    rn, cn = naming.give_names(data)
    worst = 0.0
    for job, init, res in zip(jobs, inits, grouped):
        ref = api.res_nmtf_inner(data, naming.shared_names(rn), naming.shared_names(cn), init[0], init[1], init[2],
                                 [job.k_val] * 2, np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2)), 200,
                                 spurious=False, row_names=rn, col_names=cn)
        for key in ("output_f", "output_g"):
            for v in range(2):
                d = helpers.rel_fro(res[key][v], ref[key][v])
                worst = max(worst, d)
                assert d <= 1e-4, (job.tag, key, v, d)
    print(f"k sweep 3..8 at 200 sweeps: worst rel-Frobenius grouped fp64 vs f32 engine {worst:.2e}")


def test_grouped_spurious_check_equals_feeding_the_grouped_shuffles():
    x1, _, _ = _planted(1)
    x2, _, _ = _planted(2)
    data = naming.check_data([x1, x2])
    res = batched.run_jobs_grouped([batched.Job(data, 3, seed=3)], pre_processed=True)[0]
    got = spurious.check_biclusters(data, res["output_f"], 3, seed=11, grouped=True)
    reps = batched.run_jobs_grouped(batched.shuffled_jobs(data, 3, 3, seed=11))
    want = spurious.check_biclusters(data, res["output_f"], 3, shuffled_f=[r["output_f"] for r in reps])
    for key in ("score", "avg_threshold", "max_threshold"):
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
    removed = api.remove_spurious(data, res, 3, seed=11, grouped=True)
    assert removed["spurious"]["score"].tobytes() == np.asarray(got["score"]).tobytes()
