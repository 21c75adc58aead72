"""GPU tests of sparse views in the device-wide fp64 path (resnmtf_fp64_run_sparse).  Two yardsticks
from the same initial factors: the fp64 oracle on the DENSIFIED matrix and ``fp64_run`` on the densified matrix.  Bars
are test_gpu_fp64.py's own: F, G, S <= 1e-11 relative Frobenius, All_Error <= 1e-13 absolute, lambda / mu rtol 1e-11 at
fixed counts of at most 30 sweeps; to convergence F, G <= 1e-8 and the oracle's stop sweep.  Cases are built as
test_gpu_sparse.py builds them: a planted view, a mask, one entry per column, columns re-normalised."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from oracle import resnmtf_oracle as O
from resnmtf_amd import _lib, api, naming, synth
from resnmtf_amd.engine import fp64_run, fp64_sparse_plan
from resnmtf_amd.problem import pair_table
from test_gpu_fp64 import CLUSTER_EPS, COUPLED, FIX_ERR, FIX_F, MAX_ITERS, _check, _check_api, _oracle, _oracle_from_init, _same_bits

pytestmark = pytest.mark.gpu


def sparsify(x, density, seed, keep=None):
    """x with a random `density` of its entries kept (plus `keep`, a mask, and one entry per column), columns
    re-normalised: a pre-processed view, dense fp64 (for the oracle)."""
    rng = np.random.default_rng(seed)
    mask = rng.random(x.shape) < density
    if keep is not None:
        mask |= keep
    mask[rng.integers(0, x.shape[0], x.shape[1]), np.arange(x.shape[1])] = True
    y = np.where(mask, x, 0.0)
    return y / y.sum(axis=0)[None, :]


def single(x, k, seed, name="sparse"):
    n, m = x.shape
    f, s, g = synth.random_init(n, m, k, seed)
    z = np.zeros((1, 1))
    return synth.Problem([x], [f], [s], [g], z, z, z, k, name, row_names=[[f"row_{i}" for i in range(n)]],
                         col_names=[[f"col_{j}" for j in range(m)]])


def one_view(n, m, k, density, seed):
    return single(sparsify(synth.planted_view(n, m, max(k // 2, 2), seed), density, seed + 1), k, seed + 2)


def problem(prob, n_iters, dense=()):
    """The problem dict of ``fp64_run``: every view a ``scipy.sparse`` matrix, except those in ``dense``."""
    data = [x if v in dense else sp.csc_matrix(x) for v, x in enumerate(prob.data)]
    return {"data": data, "k": prob.init_f[0].shape[1], "init_f": prob.init_f, "init_s": prob.init_s, "init_g": prob.init_g,
            "phi": prob.phi, "xi": prob.xi, "psi": prob.psi, "row_pairs": pair_table(prob.row_names),
            "col_pairs": pair_table(prob.col_names), "n_iters": n_iters}


def as_ref(out):
    """A result of ``fp64_run`` in the oracle's keys (the second yardstick of ``_check``)."""
    return {"output_f": out["f"], "output_g": out["g"], "output_s": out["s"], "lambda": out["lambda"], "mu": out["mu"],
            "All_Error": out["all_error"]}


def check_both(prob, n_iters, what, dense=(), oracle=True, max_iters=MAX_ITERS):
    """The sparse run against the oracle on the densified views and against ``fp64_run`` on them."""
    n_v, fixed = len(prob.data), n_iters is not None
    out = fp64_run(problem(prob, n_iters, dense), max_iters=max_iters)
    dense_out = fp64_run(problem(prob, n_iters, range(n_v)), max_iters=max_iters)
    worst_d, err_d = _check(out, as_ref(dense_out), n_v, fixed, (what, "dense fp64 path"))
    print(f"{what}: vs the dense fp64 path {worst_d:.2e}, All_Error {err_d:.2e}")
    if oracle:
        ref = _oracle(prob, n_iters, max_iters)
        worst_o, err_o = _check(out, ref, n_v, fixed, (what, "oracle"))
        print(f"{what}: vs the oracle {worst_o:.2e}, All_Error {err_o:.2e}")
    return out


# ---- 1. one view across the padded-k classes ----
@pytest.mark.parametrize("k", [3, 16, 17, 32, 33, 48, 49, 64])
def test_one_view_across_k(k):
    prob = one_view(400, 300, k, 0.05, 10 + k)
    plan = fp64_sparse_plan(sp.csc_matrix(prob.data[0]), k)
    assert plan["kp"] == -(-k // 16) * 16 and plan["lines_per_wave"] == (4 if k <= 16 else 2 if k <= 32 else 1)
    check_both(prob, 20, f"k={k}")


# ---- 2. densities ----
@pytest.mark.parametrize("density", [0.001, 0.05, 0.5])
def test_densities(density):
    prob = one_view(3000, 700, 8, density, 40)
    plan = fp64_sparse_plan(sp.csc_matrix(prob.data[0]), 8)
    assert (plan["xtf"][0] > 1) == (density == 0.5)                     # columns of ~1500 entries are cut, the others whole
    check_both(prob, 20, f"density={density}")


# ---- 3. edge shapes ----
def _edge(which):
    rng = np.random.default_rng(5)
    if which == "2x2":
        return single(np.array([[0.25, 0.6], [0.75, 0.4]]), 1, 3), 20
    if which in ("129x127", "33x257", "257x33"):
        n, m = (int(s) for s in which.split("x"))
        k = 16 if n == 129 else 5
        return one_view(n, m, k, 0.10, 21 + n), 20
    n, m, k = 200, 150, 4
    x = sparsify(synth.planted_view(n, m, 2, 8), 0.2, 9)
    if which == "empty_rows":                                            # 40 rows without a stored entry: the stale-slab case
        x[rng.choice(n, 40, replace=False), :] = 0.0
    elif which == "one_entry_row":
        x[17, :] = 0.0
        x[17, 23] = 0.5
    elif which == "last_row_empty_last_col_full":
        x[:, m - 1] = 0.1 + rng.random(n)
        x[n - 1, :] = 0.0
    elif which == "last_row_full_last_col_empty":
        x[n - 1, :] = 0.1 + rng.random(m)
        x[:, m - 1] = 0.0
    sums = x.sum(axis=0)
    x = x / np.where(sums > 0, sums, 1.0)[None, :]
    return single(x, k, 12), 20


EDGES = ["2x2", "129x127", "33x257", "257x33", "empty_rows", "one_entry_row", "last_row_empty_last_col_full",
         "last_row_full_last_col_empty"]


@pytest.mark.parametrize("which", EDGES)
def test_edge_shapes(which):
    prob, sweeps = _edge(which)
    x = prob.data[0]
    if which == "2x2":
        assert np.count_nonzero(x) == 4                                  # every entry stored
    if which == "empty_rows":
        assert (np.count_nonzero(x, axis=1) == 0).sum() >= 40
    if which == "one_entry_row":
        assert np.count_nonzero(x[17]) == 1
    if which.startswith("last_row_empty"):
        assert not x[-1].any() and x[:-1, -1].all()
    if which.startswith("last_row_full"):
        assert x[-1, :-1].all() and not x[:, -1].any()
    check_both(prob, sweeps, which)


# ---- 4. skew: one row and one column at 60 % among 0.2 %, with empty rows ----
def _skewed():
    n, m, k = 2500, 900, 6
    rng = np.random.default_rng(3)
    x = synth.planted_view(n, m, 3, 4)
    keep = np.zeros((n, m), dtype=bool)
    keep[7, rng.random(m) < 0.6] = True
    keep[rng.random(n) < 0.6, 11] = True
    y = sparsify(x, 0.002, 5, keep)
    empty = rng.choice(np.setdiff1d(np.arange(n), [7]), 40, replace=False)
    y[empty, :] = 0.0
    y = np.where(y.sum(axis=0)[None, :] > 0, y, x)          # (no column left empty)
    y /= y.sum(axis=0)[None, :]
    return single(y, k, 6, "skewed")


def test_skewed_view():
    prob = _skewed()
    x = prob.data[0]
    plan = fp64_sparse_plan(sp.csc_matrix(x), 6)
    longest_row, longest_col = int(np.count_nonzero(x, axis=1).max()), int(np.count_nonzero(x, axis=0).max())
    assert plan["xg"][2] == longest_row > 256 and plan["xtf"][2] == longest_col > 256
    assert plan["xg"][0] == -(-longest_row // 256) > 1 and plan["xtf"][0] == -(-longest_col // 256) > 1      # both products cut their lines
    assert (np.count_nonzero(x, axis=1) == 0).sum() >= 40
    check_both(prob, 20, "skewed")                                       # (one form: every line piece is a lane group's)


# ---- 5. coupled problems: g2 and g3 sparsified at 30 % (g3 keeps a dense view: both error forms in one job), and
# two of test_gpu_fp64.COUPLED's problems sparsified, as a fixed count and to convergence ----
@pytest.mark.parametrize("name,dense", [("g2_two_views_phi_partial", ()), ("g3_three_views_phi_psi_xi", (1,))])
def test_goldens_sparsified(name, dense):
    prob = helpers.golden_problem(helpers.load_golden(name))
    prob.data = [sparsify(x, 0.3, 70 + v) for v, x in enumerate(prob.data)]
    check_both(prob, 30, name, dense=dense)


@pytest.fixture(scope="module")
def coupled_sparse():
    out = {}
    for idx in (3, 5):
        shapes, k, kw, _ = COUPLED[idx]
        prob = helpers.coupled_problem(shapes, k, 100 + idx, **kw)
        prob.data = [sparsify(x, 0.3, 80 + v) for v, x in enumerate(prob.data)]
        out[idx] = prob
    return out


@pytest.mark.parametrize("idx", [3, 5])
@pytest.mark.parametrize("mode", ["fixed", "convergence"])
def test_coupled_sparsified(coupled_sparse, idx, mode):
    n_iters = COUPLED[idx][3] if mode == "fixed" else None
    check_both(coupled_sparse[idx], n_iters, (idx, mode), dense=(1,) if idx == 5 else ())


# ---- 6. convergence: the oracle's stop sweep, on a trace that keeps clear of the tolerance ----
CONV_SEED = 90


def test_convergence_stops_on_the_oracles_sweep():
    prob = one_view(800, 500, 5, 0.05, CONV_SEED)
    ref = _oracle(prob, None, MAX_ITERS)
    trace = np.asarray(ref["All_Error"])
    delta = np.abs(np.diff(np.concatenate([[0.0], trace])))
    assert np.min(np.abs(delta - 1e-6)) >= 1e-10, np.min(np.abs(delta - 1e-6))      # no sweep sits on the stop rule
    assert len(trace) < MAX_ITERS
    out = fp64_run(problem(prob, None), max_iters=MAX_ITERS)
    assert out["iters"] == len(trace)
    worst, e = _check(out, ref, 1, False, "convergence")
    print(f"convergence: {out['iters']} sweeps, worst F / G distance {worst:.2e}, All_Error {e:.2e}")


# ---- 7. beyond the oracle's comfort: against fp64_run on the densified matrix ----
@pytest.mark.parametrize("k", [40, 64])
def test_beyond_the_oracles_comfort(k):
    check_both(one_view(2304, 1900, k, 0.02, 60 + k), 10, f"2304x1900 k={k}", oracle=False)


# ---- 8. bitwise repeatability ----
def test_two_runs_give_the_same_bits(coupled_sparse):
    skew = problem(_skewed(), 15)
    _same_bits(fp64_run(skew), fp64_run(skew))
    conv = problem(coupled_sparse[5], None, dense=(1,))
    _same_bits(fp64_run(conv, max_iters=MAX_ITERS), fp64_run(conv, max_iters=MAX_ITERS))


def _c_job(prob, n_iters, sparse_views=()):
    """A resnmtf_group_job (and the resnmtf_fp64_sparse beside it) filled by hand from a problem with no coupling."""
    keep, outs = [], []
    dp = C.POINTER(C.c_double)
    j = _lib.GroupJob()
    j.struct_size = C.sizeof(_lib.GroupJob)
    V, k = len(prob.data), prob.init_f[0].shape[1]
    j.n_views, j.k, j.n_iters = V, k, n_iters
    s = _lib.Fp64Sparse()
    s.struct_size = C.sizeof(_lib.Fp64Sparse)
    for v, x in enumerate(prob.data):
        n, m = x.shape
        arrs = [np.asfortranarray(a, dtype=np.float64) for a in (x, prob.init_f[v], prob.init_s[v], prob.init_g[v])]
        res = [np.full(shape, -7.0, order="F") for shape in ((n, k), (k, k), (m, k), (k,), (k,))]
        j.n_rows[v], j.n_cols[v] = n, m
        j.f0[v], j.s0[v], j.g0[v] = (a.ctypes.data_as(dp) for a in arrs[1:])
        if v in sparse_views:
            c = sp.csc_matrix(x)
            csc = [c.indptr.astype(np.int64), c.indices.astype(np.int32), c.data.astype(np.float64)]
            s.view[v].col_ptr = csc[0].ctypes.data_as(C.POINTER(C.c_longlong))
            s.view[v].row_idx = csc[1].ctypes.data_as(C.POINTER(C.c_int))
            s.view[v].values = csc[2].ctypes.data_as(dp)
            keep += csc
        else:
            j.x[v] = arrs[0].ctypes.data_as(dp)
        j.f_out[v], j.s_out[v], j.g_out[v], j.lambda_out[v], j.mu_out[v] = (a.ctypes.data_as(dp) for a in res)
        keep += arrs
        outs += res
    for a in range(V):
        for b in range(V):
            j.row_count[a][b] = j.col_count[a][b] = -1
    err, it = np.full(max(n_iters, 1), -7.0), np.full(1, -7, dtype=np.int32)
    j.all_error, j.err_capacity, j.iters_done = err.ctypes.data_as(dp), len(err), it.ctypes.data_as(C.POINTER(C.c_int))
    return j, s, keep, outs + [err, it]


def test_a_job_without_sparse_views_is_bitwise_fp64_run():
    lib = _lib.load()
    prob = one_view(300, 257, 17, 0.3, 31)
    ja, _, keep_a, outs_a = _c_job(prob, 12)
    jb, sb, keep_b, outs_b = _c_job(prob, 12)
    jc, _, keep_c, outs_c = _c_job(prob, 12)
    assert lib.resnmtf_fp64_run(0, C.byref(ja), 1e-6, 100) == _lib.OK
    assert lib.resnmtf_fp64_run_sparse(0, C.byref(jb), C.byref(sb), 1e-6, 100) == _lib.OK       # no view marked sparse
    assert lib.resnmtf_fp64_run_sparse(0, C.byref(jc), None, 1e-6, 100) == _lib.OK              # no struct at all
    for a, b, c in zip(outs_a, outs_b, outs_c):
        assert not np.any(a == -7) and a.tobytes() == b.tobytes() == c.tobytes()


# ---- 9. against the f32 sparse engine: 2000 x 500, k = 16, 5 %, 100 sweeps from one explicit start ----
def _api_call(prob, n_iters, data, **kw):
    k = prob.init_f[0].shape[1]
    return api.res_nmtf_inner(data, naming.shared_names(prob.row_names), naming.shared_names(prob.col_names),
                              prob.init_f, prob.init_s, prob.init_g, [k] * len(data), prob.phi, prob.xi, prob.psi,
                              n_iters, spurious=False, row_names=prob.row_names, col_names=prob.col_names, **kw)


def test_against_the_f32_sparse_engine():
    prob = one_view(2000, 500, 16, 0.05, 77)
    data = [sp.csr_matrix(prob.data[0])]
    f32 = _api_call(prob, 100, data)
    f64 = _api_call(prob, 100, data, precision="fp64", fp64_sparse=True)
    assert list(f64.keys()) == list(f32.keys()) and len(f64["All_Error"]) == 100
    for key in ("output_f", "output_g"):
        d = helpers.rel_fro(f64[key][0], f32[key][0])
        print(f"{key}: fp64 sparse path vs f32 sparse engine {d:.2e}")
        assert d <= 2e-5, (key, d)
    rel = np.argmax(f64["output_s"][0], axis=0)
    assert np.array_equal(np.argmax(f32["output_s"][0], axis=0), rel)
    for key, fac in (("row_clusters", f64["output_f"][0][:, rel]), ("col_clusters", f64["output_g"][0])):
        on_threshold = np.abs(fac * fac.shape[0] - 1.0) < CLUSTER_EPS     # identical off the 1/n threshold
        assert not ((np.asarray(f64[key][0]) != np.asarray(f32[key][0])) & ~on_threshold).any(), key


# ---- 10. api.res_nmtf_inner(precision="fp64", fp64_sparse=True) ----
@pytest.fixture(scope="module")
def api_problem():
    prob = helpers.coupled_problem([(120, 90), (100, 90)], 4, 5, phi_w=1.0, psi_w=0.5)
    prob.data = [sparsify(x, 0.3, 50 + v) for v, x in enumerate(prob.data)]
    return prob


@pytest.mark.parametrize("start,dense", [("device", ()), ("explicit", ()), ("explicit", (1,))])
def test_api_route(api_problem, start, dense):
    prob = api_problem
    data = [x if v in dense else sp.coo_matrix(x) for v, x in enumerate(prob.data)]
    k_vec, rs, cs = [4, 4], naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)
    common = dict(spurious=False, row_names=prob.row_names, col_names=prob.col_names, precision="fp64", fp64_sparse=True,
                  return_init=True, seed=3)
    if start == "explicit":
        rng = np.random.default_rng(9)
        lm = ([rng.random(4) + 0.5 for _ in range(2)], [rng.random(4) + 0.5 for _ in range(2)])
        res = api.res_nmtf_inner(data, rs, cs, prob.init_f, prob.init_s, prob.init_g, k_vec, prob.phi, prob.xi, prob.psi, 20,
                                 init_lm=lm, **common)
        assert np.array_equal(res["init"][1][3], lm[0][1]) and np.array_equal(res["init"][0][0], prob.init_f[0])
    else:
        res = api.res_nmtf_inner(data, rs, cs, None, None, None, k_vec, prob.phi, prob.xi, prob.psi, 20, **common)
    assert len(res["init"]) == 2 and len(res["init"][0]) == 5
    _check_api(res, _oracle_from_init(prob, res["init"], 20), 2, (start, dense))


# ---- 11. the refusals through the C entry, each leaving the outputs untouched ----
def test_c_level_refusals_then_a_run():
    lib = _lib.load()
    prob = one_view(40, 30, 3, 0.3, 15)
    j, s, keep, outs = _c_job(prob, 5, sparse_views=(0,))
    csc = keep[:3]

    def refused(job, sparse, word):
        assert lib.resnmtf_fp64_run_sparse(0, C.byref(job), C.byref(sparse), 1e-6, 100) == 1
        assert word in lib.resnmtf_last_error(None), lib.resnmtf_last_error(None)
        assert all(np.all(o == -7) for o in outs)

    def broken(which, edit):
        saved = csc[which].copy()
        edit(csc[which])
        return saved

    def restore(which, saved):
        csc[which][:] = saved

    e0 = int(csc[0][1])                                                  # column 1's first entry; column 0 holds >= 2 entries
    assert e0 >= 2
    saved = broken(1, lambda a: a.__setitem__([0, 1], a[[1, 0]])); refused(j, s, b"strictly increasing"); restore(1, saved)
    saved = broken(1, lambda a: a.__setitem__(e0, 40)); refused(j, s, b"out of range"); restore(1, saved)
    saved = broken(2, lambda a: a.__setitem__(3, -1.0)); refused(j, s, b"negative"); restore(2, saved)
    saved = broken(2, lambda a: a.__setitem__(3, np.nan)); refused(j, s, b"non-finite"); restore(2, saved)
    xf = np.asfortranarray(prob.data[0])
    both = _lib.GroupJob.from_buffer_copy(j)
    both.x[0] = xf.ctypes.data_as(C.POINTER(C.c_double))
    refused(both, s, b"both dense")
    refused(j, _lib.Fp64Sparse(struct_size=C.sizeof(_lib.Fp64Sparse)), b"x / f0 / s0 / g0 is NULL")      # neither
    wrong = _lib.Fp64Sparse.from_buffer_copy(s)
    wrong.struct_size = 8
    refused(j, wrong, b"struct_size")
    assert lib.resnmtf_fp64_run_sparse(0, C.byref(j), C.byref(s), 1e-6, 100) == _lib.OK
    assert not any(np.any(o == -7) for o in outs[:5]) and outs[-1][0] == 5
    ref = _oracle(prob, 5)
    assert helpers.rel_fro(outs[0], ref["output_f"][0]) <= FIX_F and np.max(np.abs(outs[-2] - ref["All_Error"])) <= FIX_ERR
