"""The SVD initialisation in double precision (resnmtf_fp64_init_svd) checked STAGE BY STAGE against
fp64 (host side: tests/init_ref.py, which describes this algorithm unchanged), then its routes and its wiring.

Every case reads the signed basis (``engine.fp64_init_svd(return_basis=True)``) with sigma = 0 and checks one stage per
test against the fp64 values the call was GIVEN -- there is no f32 image on this route, so no widening and no f32 bar:

* ``test_basis_is_orthonormal``: max |U^T U - I| <= orth_bar(len, L) of test_gpu_init_svd.py (the same derivation);
* ``test_last_product_entry_by_entry``: |X^T U - V diag(d)|[i, j] <= BAR sqrt(L) ||X[:, i]|| with BAR = 2.0e-13, the
  project's bar for "fp64 throughout", for EVERY class (the f32 route's bars are 1.5e-7 ... 3.5e-7);
* ``test_triplets_converged``: residual and singular values <= max(BAR, 4 x the init_ref.sketch_svd yardstick over five
  Omega seeds); where the yardstick is exact the f32 route measured 2.5e-8 ... 7.4e-8 and this one must meet BAR;
* ``test_finish``: F0, S0, G0, lambda0, mu0 are init_ref.finish(U, V, d, k) within FINISH_BAR elementwise.

Worst product statistic measured on the MI355X per class (the device is run-to-run deterministic): see MEASURED below.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import init_ref as R
import test_gpu_init_svd as T
from resnmtf_amd import api, batched, engine, naming, synth
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine
from sweep_ref import rel_stat
from test_gpu_sparse import sparsify
from test_gpu_sweep_elementwise import sparse_one

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

BAR = T.BARS["thin"]               # 2.0e-13: "fp64 throughout"
FINISH_BAR = T.FINISH_BAR          # 1e-13
N_POWER = T.N_POWER
REF_SEEDS = T.REF_SEEDS
POOR = T.POOR
assert BAR == 2.0e-13 and FINISH_BAR == 1e-13

# Worst |X^T U - V diag(d)| / (sqrt(L) ||X[:, i]||) measured per class on the MI355X, with the case (bar 2.0e-13):
MEASURED = {
    "L16": "5.9e-16 (sketch_1000x700_k8)", "L32": "6.0e-16 (splits_1500x1100_k16)", "L48": "3.2e-16 (sketch_257x200_k40)",
    "L64": "3.9e-16 (sketch_513x320_k56)", "sparse": "2.6e-16 (sparse_long_lines_k8)", "thin": "3.0e-15 (thin_4100x12_k12)",
}

# Where the algorithm itself is poor in fp64 (test_gpu_init_svd.FINDINGS, same rule): the cases shared with that file
# keep its bounds; the bound of a case of this file alone is twice the larger yardstick statistic over the five seeds.
FINDINGS = dict({cid: T.FINDINGS[cid] for cid in ("sketch_513x320_k64", "sparse_1500x900_k8", "sparse_1500x900_k20",
                                                   "sparse_1500x900_k40", "sparse_1500x900_k64", "sparse_skew_empty_k12")},
                **{"sparse_long_lines_k8": 6e-2})   # [3.0e-2 on the host: a flat spectrum below the two dense lines]

RUNS, PASSED = {}, {}


def long_lines(n, m, seed):
    """A sparse view with one row and one column stored whole (more than 256 entries each: the SpMM cuts them)."""
    y = sparsify(T.dense_data(n, m, 8, seed), 0.05, seed + 1)
    rng = np.random.default_rng(seed + 2)
    y[n // 3, :] = rng.uniform(0.1, 1.0, m)
    y[:, m // 4] = rng.uniform(0.1, 1.0, n)
    return y / y.sum(axis=0)[None, :]


def with_zero_lines(n, m, k, seed):
    """dense_data with an all-zero column and an all-zero row (a pre-processed view may hold them)."""
    x = T.dense_data(n, m, k, seed)
    x[:, m // 2] = 0.0
    x[n // 2, :] = 0.0
    return x


def _cases():
    C = []

    def add(cid, n, m, k, make=None, sparse=False, rank=None, exact=False):
        C.append(dict(id=cid, n=n, m=m, k=k, make=make or (lambda: T.dense_data(n, m, k, 100 + n + k)), sparse=sparse, rank=rank,
                      exact=exact))
    add("sketch_1000x700_k8", 1000, 700, 8)                                  # L16
    add("splits_1500x1100_k16", 1500, 1100, 16)                              # L32, both products split
    add("sketch_257x200_k40", 257, 200, 40)                                  # L48
    add("sketch_513x320_k56", 513, 320, 56)                                  # L64
    add("sketch_513x320_k64", 513, 320, 64)                                  # L64, no oversampling
    add("sketch_64x200_k48", 64, 200, 48, exact=True)                        # min(n, m) = L: the sketch spans the row space
    add("edge_129x127_k8", 129, 127, 8, make=lambda: with_zero_lines(129, 127, 8, 364))      # one above / below the 128-row tile
    add("edge_33x257_k8", 33, 257, 8)                                        # the contraction of X G split five ways
    add("edge_257x33_k8", 257, 33, 8)                                        # ... of X^T F
    add("thin_63x200_k48", 63, 200, 48, exact=True)
    add("thin_5x4_k2", 5, 4, 2, exact=True)
    add("thin_4100x12_k12", 4100, 12, 12, exact=True)
    add("thin_sparse_500x12_k4", 500, 12, 4, make=lambda: T.thin_sparse(500, 12, 31), sparse=True, exact=True)
    add("thin_sparse_12x500_k4", 12, 500, 4, make=lambda: T.thin_sparse(12, 500, 32), sparse=True, exact=True)
    for k, dens in ((8, 0.05), (20, 0.1), (40, 0.02), (64, 0.3)):
        add(f"sparse_1500x900_k{k}", 1500, 900, k, make=lambda k=k, dens=dens: sparse_one(1500, 900, k, dens, 70 + k).data[0],
            sparse=True)
    add("sparse_skew_empty_k12", 1500, 900, 12, make=lambda: sparse_one(1500, 900, 12, 0.01, 82, skew=True, empty=True).data[0],
        sparse=True)
    add("sparse_long_lines_k8", 600, 400, 8, make=lambda: long_lines(600, 400, 51), sparse=True)
    add("lowrank_ten_rows_sparse_k8", 400, 300, 8, make=lambda: T.ten_rows(400, 300, 42), sparse=True, rank=10, exact=True)
    add("lowrank_three_blocks_k3", 180, 180, 3, make=T.three_blocks, rank=3, exact=True)
    add("lowrank_rank10_k12", 300, 200, 12, make=lambda: T.rank10(300, 200, 43), rank=10, exact=True)
    return C


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def view_of(c, x):
    return sp.csc_matrix(x) if c["sparse"] else x


def run_case(cid):
    """Everything the stage tests read, once per case: the device's basis and start, and the fp64 yardstick on X."""
    if cid in RUNS:
        if isinstance(RUNS[cid], Exception):
            raise RUNS[cid]
        return RUNS[cid]
    c = case(cid)
    n, m, k = c["n"], c["m"], c["k"]
    x = np.asarray(c["make"](), dtype=np.float64)
    assert x.shape == (n, m)
    try:
        f0, s0, g0, lam, mu, d, U, V, d_all = engine.fp64_init_svd([view_of(c, x)], k, seed=1, sigma=0.0, return_basis=True)[0]
    except Exception as exc:
        RUNS[cid] = exc
        raise
    plan = engine.fp64_sparse_plan(sp.csc_matrix(x), k) if c["sparse"] else engine.fp64_plan(n, m, k)
    sketch = R.takes_sketch(n, m, k)
    L = R.sketch_width(k) if sketch else min(n, m)
    sigma = np.linalg.svd(x, compute_uv=False)
    cols = k if c["rank"] is None else min(k, c["rank"])
    refs = [R.sketch_svd(x, L, N_POWER, np.random.default_rng(s)) for s in REF_SEEDS] if sketch else [R.thin_svd(x)]
    reach = {"residual": max(R.residual_stat(x, ru, rv, rd, cols) for ru, rv, rd in refs),
             "sv": max(R.sv_stat(rd, sigma, cols) for ru, rv, rd in refs)}
    klass = "thin" if not sketch else ("sparse" if c["sparse"] else f"L{L}")
    RUNS[cid] = dict(c=c, x=x, d=d, U=U, V=V, d_all=d_all, factors=(f0, s0, g0, lam, mu), plan=plan, sketch=sketch, L=L,
                     sigma=sigma, cols=cols, reach=reach, klass=klass)
    return RUNS[cid]


def record(cid, stage=None, **figures):
    for key, val in figures.items():
        print(f"MEASURED {cid} {key}: {val:.3e}")
    if stage:
        PASSED.setdefault(cid, set()).add(stage)


def same_bits(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_same_start(got, ref, what):
    assert len(got) == len(ref), what
    for v, (a, b) in enumerate(zip(got, ref)):
        assert len(a) == len(b), what
        for name, p, q in zip(("F0", "S0", "G0", "lambda0", "mu0", "d", "U", "V", "d_all"), a, b):
            assert same_bits(p, q), f"{what}: view {v}, {name} differs"


# ---------------------------------------------------------------------------------------------------------------------
# one test per stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_basis_is_orthonormal(cid):
    r = run_case(cid)
    n, m, cols, L, k = r["c"]["n"], r["c"]["m"], r["cols"], r["L"], r["c"]["k"]
    assert np.isfinite(r["U"]).all() and np.isfinite(r["V"]).all() and np.isfinite(r["d_all"]).all()
    assert len(r["d_all"]) == min(L, n, m) and np.all(np.diff(r["d_all"]) <= 0) and np.all(r["d_all"] >= 0)
    assert np.array_equal(r["d"], r["d_all"][:k]) and r["U"].shape == (n, k) and r["V"].shape == (m, k)
    if r["sketch"]:
        stat, bar = R.orth_stat(r["U"], cols), T.orth_bar(n, L)
        record(cid, orth_U=stat, orth_U_over_bar=stat / bar)
        assert stat <= bar, f"max |U^T U - I| = {stat:.3e} (bar {bar:.3e})"
    else:                                          # (the thin route: test_gpu_init_svd.test_basis_is_orthonormal's rule)
        short_is_v = m <= n
        short, long_ = (r["V"], r["U"]) if short_is_v else (r["U"], r["V"])
        strong = int(np.count_nonzero(r["d"][:cols] > 1e-3 * r["d"][0]))
        s_short, s_long = R.orth_stat(short, cols), R.orth_stat(long_, strong)
        bar = T.orth_bar(max(n, m), L)
        bar_long = bar * (r["d"][0] / r["d"][strong - 1]) ** 2
        record(cid, orth_short=s_short, orth_long=s_long, orth_long_over_bar=s_long / bar_long)
        assert s_short <= bar, f"short side: max |W^T W - I| = {s_short:.3e} (bar {bar:.3e})"
        assert s_long <= bar_long, f"long side: {s_long:.3e} over {strong} triplets (bar {bar_long:.3e})"
    PASSED.setdefault(cid, set()).add("orth")


@pytest.mark.parametrize("cid", CASE_IDS)
def test_last_product_entry_by_entry(cid):
    r = run_case(cid)
    k, cols = r["c"]["k"], r["cols"]
    live = int(np.count_nonzero(r["d"] > BAR * r["d"][0]))
    if r["c"]["rank"] is None:
        assert live == k, f"only {live} of {k} singular values above {BAR:.1e} d_1"
    else:                                          # past the rank of the view every d is exactly 0 (the rank cut)
        assert live == cols, f"{live} singular values above {BAR:.1e} d_1 for a view of rank {r['c']['rank']}: {r['d']}"
        assert not r["d_all"][r["c"]["rank"]:].any(), f"d past the rank: {r['d_all'][r['c']['rank']:]}"
    stat, nz = R.product_stat(r["x"], r["U"], r["V"], r["d"], r["L"], cols)
    record(cid, product=stat)
    assert nz == 0, f"{nz} entries of V non-zero where the column of X is all zero"
    assert stat <= BAR, f"max |X^T U - V d|[i, j] / (sqrt(L) ||X[:, i]||) = {stat:.3e} (bar {BAR:.1e}, class {r['klass']})"
    PASSED.setdefault(cid, set()).add("product")


@pytest.mark.parametrize("cid", CASE_IDS)
def test_triplets_converged(cid):
    r = run_case(cid)
    cols = r["cols"]
    res = R.residual_stat(r["x"], r["U"], r["V"], r["d"], cols)
    sv = R.sv_stat(r["d"], r["sigma"], cols)
    record(cid, residual=res, residual_fp64=r["reach"]["residual"], sv=sv, sv_fp64=r["reach"]["sv"])
    bar_res, bar_sv = max(BAR, 4.0 * r["reach"]["residual"]), max(BAR, 4.0 * r["reach"]["sv"])
    assert res <= bar_res, f"max ||X v - d u|| / d_1 = {res:.3e} (bar {bar_res:.3e}; fp64 reaches {r['reach']['residual']:.3e})"
    assert sv <= bar_sv, f"max |d - sigma| / sigma_1 = {sv:.3e} (bar {bar_sv:.3e}; fp64 reaches {r['reach']['sv']:.3e})"
    yard = max(r["reach"].values())
    if r["c"]["exact"]:                            # the improvement the route exists for: the f32 route is at 2.5e-8 ... 7.4e-8
        assert yard <= BAR / 4, f"the yardstick of an exact case reaches only {yard:.3e}"
        assert res <= BAR and sv <= BAR, (res, sv)
    elif cid in FINDINGS:
        assert yard <= FINDINGS[cid], f"the fp64 yardstick reaches only {yard:.3e} (bound {FINDINGS[cid]:.1e})"
        assert max(res, sv) > BAR, f"the finding no longer shows ({res:.3e}, {sv:.3e}): move {cid} out of FINDINGS"
    else:
        assert yard <= POOR, f"the fp64 yardstick itself reaches only {yard:.3e}: record the case in FINDINGS"
    PASSED.setdefault(cid, set()).add("converged")


def test_the_f32_route_does_not_meet_the_fp64_bar():
    """lowrank_rank10_k12, where the algorithm is exact: this route meets 2.0e-13, Engine.init_svd's basis does not -- so
    the bar above cannot be met by a start that went through the f32 image."""
    r = run_case("lowrank_rank10_k12")
    c = r["c"]
    mine = R.residual_stat(r["x"], r["U"], r["V"], r["d"], r["cols"])
    with Engine([c["n"]], [c["m"]], [c["k"]]) as e:
        e.set_view(0, r["x"])
        d, U, V, _ = e.init_svd(0, seed=1, sigma=0.0, return_basis=True)
    theirs = R.residual_stat(r["x"], U, V, d, r["cols"])
    record("lowrank_rank10_k12", residual_fp64_route=mine, residual_f32_route=theirs)
    assert mine <= BAR < theirs, (mine, theirs)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_finish(cid):
    r = run_case(cid)
    k = r["c"]["k"]
    ref = R.finish(r["U"], r["V"], r["d"], k)
    worst = 0.0
    for name, got, want in zip(("F0", "S0", "G0", "lambda", "mu"), r["factors"], ref):
        assert np.isfinite(got).all(), f"{name} is not finite"
        assert (got >= 0).all(), f"{name} has negative entries"
        stat, nz = rel_stat(got, want)
        worst = max(worst, stat)
        assert nz == 0, f"{name}: {nz} entries non-zero where the reference is zero"
        assert stat <= FINISH_BAR, f"{name}: max |got / ref - 1| = {stat:.3e} (bar {FINISH_BAR:.0e})"
    record(cid, finish=worst)
    PASSED.setdefault(cid, set()).add("finish")


def test_s0_noise_is_half_normal():
    """k = 64: 4096 draws; (S0(sigma) - S0(0)) / (cF cG) is |N(0, sigma)|, the existing test's z limit of 5."""
    c = case("sketch_513x320_k64")
    x, sig = c["make"](), 0.05
    clean = engine.fp64_init_svd([x], 64, seed=7, sigma=0.0, return_basis=True)[0]
    noisy = engine.fp64_init_svd([x], 64, seed=7, sigma=sig, return_basis=True)[0]
    assert same_bits(clean[6], noisy[6]) and same_bits(clean[7], noisy[7])
    scale = np.abs(clean[6]).sum(axis=0) * np.abs(clean[7]).sum(axis=0)
    noise = (noisy[1] - clean[1]) / scale[None, :]
    assert noise.shape == (64, 64) and (noise >= -1e-12).all()
    z_mean, z_m2 = R.half_normal_z(noise, sig)
    print(f"MEASURED S0 noise z scores: mean {z_mean:.2f}, second moment {z_m2:.2f}")
    assert abs(z_mean) <= 5 and abs(z_m2) <= 5, (z_mean, z_m2)
    z_wrong = R.half_normal_z(noise, sig * sig)
    assert min(abs(z_wrong[0]), abs(z_wrong[1])) > 5


@pytest.mark.parametrize("cid", ["sketch_257x200_k40", "sparse_1500x900_k8", "thin_63x200_k48"])
def test_seeds(cid):
    """The same seed twice: the same bits.  Another seed: another basis (on the sketch route), d within the bar."""
    r = run_case(cid)
    c = r["c"]
    view = view_of(c, r["x"])
    again = engine.fp64_init_svd([view], c["k"], seed=1, sigma=0.0, return_basis=True)
    assert_same_start(again, [r["factors"] + (r["d"], r["U"], r["V"], r["d_all"])], cid)
    other = engine.fp64_init_svd([view], c["k"], seed=2, sigma=0.0, return_basis=True)[0]
    assert R.sv_stat(other[5], r["sigma"], r["cols"]) <= max(BAR, 4.0 * r["reach"]["sv"])
    if r["sketch"]:
        assert not np.array_equal(other[6], r["U"])


def test_the_same_seed_is_the_same_sketch_on_both_routes():
    """The f32 engine and this route draw Omega alike.  After ONE round (n_power = 1) the L singular values still depend
    on the sketch: from one seed the two routes agree within the f32 route's own ceiling (2e-5 d_1), from two seeds they
    do not."""
    c = case("sketch_257x200_k40")
    x = c["make"]()
    mine = engine.fp64_init_svd([x], c["k"], seed=1, sigma=0.0, n_power=1, return_basis=True)[0][8]
    with Engine([c["n"]], [c["m"]], [c["k"]]) as e:
        e.set_view(0, x)
        same_seed = e.init_svd(0, seed=1, sigma=0.0, n_power=1, return_basis=True)[3]
        other_seed = e.init_svd(0, seed=2, sigma=0.0, n_power=1, return_basis=True)[3]
    same = np.abs(same_seed - mine).max() / mine[0]
    other = np.abs(other_seed - mine).max() / mine[0]
    record(c["id"], same_seed_d_gap=same, other_seed_d_gap=other)
    assert same <= T.CEILING < other, (same, other)


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
def _passed(cid):
    stages = {"orth": test_basis_is_orthonormal, "product": test_last_product_entry_by_entry,
              "converged": test_triplets_converged, "finish": test_finish}
    for stage, fn in stages.items():
        if stage not in PASSED.get(cid, ()):
            try:
                fn(cid)
            except Exception:
                return False
    return True


def test_cases_covered():
    """The cases that passed reach every sketch width, both routes, both storages and every edge of the run's geometry,
    read from resnmtf_fp64_plan / resnmtf_fp64_sparse_plan."""
    reached = set()
    for c in CASES:
        cid = c["id"]
        if not _passed(cid):
            continue
        r = RUNS[cid]
        n, m, plan = c["n"], c["m"], r["plan"]
        kind = "sparse" if c["sparse"] else "dense"
        if r["sketch"]:
            reached.add(("sketch", kind))
            reached.add(("L", r["L"]))
            if min(n, m) == r["L"]:
                reached.add("min(n, m) = L")
            if c["rank"] is not None:
                reached.add(("low rank", kind))
            if c["sparse"]:
                if plan["xg"][0] > 1 and plan["xtf"][0] > 1 and plan["xg"][2] > 256 and plan["xtf"][2] > 256:
                    reached.add("rows and columns longer than 256 entries, cut into pieces")
            else:
                if plan["xg"][1] > 1 and plan["xtf"][1] > 1:
                    reached.add("both products split")
                if plan["xg"][0] == 2 and n == 129 and plan["xtf"][0] == 1 and m == 127:
                    reached.add("one row above / one below the 128-row tile")
                if plan["xg"][1] == 5 and plan["xg"][0] == 1:
                    reached.add("X G contraction split five ways")
                if plan["xtf"][1] == 5 and plan["xtf"][0] == 1:
                    reached.add("X^T F contraction split five ways")
        else:
            reached.add(("thin", kind, "tall" if m <= n else "wide"))
            if min(n, m) == R.sketch_width(c["k"]) - 1:
                reached.add("min(n, m) = L - 1")
    want = {("sketch", "dense"), ("sketch", "sparse"), ("L", 16), ("L", 32), ("L", 48), ("L", 64),
            ("thin", "dense", "tall"), ("thin", "dense", "wide"), ("thin", "sparse", "tall"), ("thin", "sparse", "wide"),
            "min(n, m) = L", "min(n, m) = L - 1", ("low rank", "dense"), ("low rank", "sparse"), "both products split",
            "one row above / one below the 128-row tile", "X G contraction split five ways",
            "X^T F contraction split five ways", "rows and columns longer than 256 entries, cut into pieces"}
    missing = sorted(str(w) for w in want - reached)
    assert not missing, "no passing case reaches: " + ", ".join(missing)


# ---------------------------------------------------------------------------------------------------------------------
# routes: bit for bit
# ---------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def start(view, k, **kw):
    return engine.fp64_init_svd([view], k, seed=3, sigma=0.05, return_basis=True, **kw)


def test_dense_routes_give_the_same_bits():
    x = T.dense_data(300, 129, 30, 7)
    ref = start(x, 30)
    t = torch.as_tensor(x, device=DEV)
    assert_same_start(start(t, 30), ref, "a device fp64 tensor")
    tt = torch.as_tensor(np.ascontiguousarray(x.T), device=DEV).T
    assert tt.stride() == (1, 300)
    assert_same_start(start(tt, 30), ref, "a transposed-stride tensor")
    assert_same_start(start(x, 30), ref, "two calls")
    row = torch.as_tensor(np.random.default_rng(5).uniform(0.1, 1.0, (1, 90)), device=DEV)
    wide = row.expand(70, 90)
    assert wide.stride()[0] == 0
    assert_same_start(start(wide, 3), start(wide.cpu().numpy().copy(), 3), "an expanded tensor")
    for dtype in (torch.float32, torch.bfloat16):
        low = torch.as_tensor(x, device=DEV).to(dtype)
        assert_same_start(start(low, 30), start(low.double().cpu().numpy(), 30), str(dtype))


@pytest.mark.parametrize("layout, index", [("csc", torch.int32), ("csc_perm", torch.int64), ("csr", torch.int32),
                                           ("coo", torch.int64)])
def test_sparse_routes_give_the_same_bits(layout, index):
    from test_gpu_fp64_sparse_device import device_view, entries, host_view
    n, m, k = 700, 450, 12
    rows, cols, vals = entries(n, m, 0.06, 11)
    ref = start(host_view(rows, cols, vals, (n, m)), k)
    got = start(device_view(layout, rows, cols, vals, (n, m), index_dtype=index), k)
    assert_same_start(got, ref, f"{layout} with {index}")


def test_host_and_device_outputs_give_the_same_bits():
    x0, x1 = T.dense_data(257, 200, 9, 3), sp.csc_matrix(sparsify(T.dense_data(300, 180, 9, 4), 0.2, 5))
    host = engine.fp64_init_svd([x0, x1], 9, seed=4)
    dev = engine.fp64_init_svd([x0, x1], 9, seed=4, output="torch")
    assert all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 for five in dev for t in five)
    assert dev[0][0].stride() == (1, 257)          # column-major, as fp64_run's device outputs
    assert_same_start(dev, host, "output='torch'")
    alone = engine.fp64_init_svd([x1], 9, seed=[5])          # view 1 draws from seed + 1
    assert_same_start(alone, host[1:], "the seed of view v is seed + v")


@pytest.mark.parametrize("cid", ["lowrank_ten_rows_sparse_k8", "lowrank_rank10_k12"])
def test_dense_and_sparse_storage_of_one_matrix_agree(cid):
    """Not bitwise (the SpMM and the MFMA product sum in different orders): sigma = 0, |U|, |V| and d of the leading
    triplets within 2.0e-13.  The cases: the yardstick is exact (rank 10 below the sketch width) and the ten singular
    values are planted apart (factors 1 ... 10), because a singular vector moves by the rounding over the relative gap
    to its neighbours -- at gaps of 1e-2 and more the rounding of a few u stays far below the bar."""
    c = case(cid)
    x = np.asarray(c["make"](), dtype=np.float64)
    cols = c["k"] if c["rank"] is None else min(c["k"], c["rank"])
    a = engine.fp64_init_svd([x], c["k"], seed=1, sigma=0.0, return_basis=True)[0]
    b = engine.fp64_init_svd([sp.csc_matrix(x)], c["k"], seed=1, sigma=0.0, return_basis=True)[0]
    gap_d = np.abs(a[5][:cols] - b[5][:cols]).max() / a[5][0]
    sep = np.min(np.abs(np.diff(a[8][:cols + 1]))) / a[5][0]
    gap_u = np.abs(np.abs(a[6][:, :cols]) - np.abs(b[6][:, :cols])).max()
    gap_v = np.abs(np.abs(a[7][:, :cols]) - np.abs(b[7][:, :cols])).max()
    record(cid, storage_gap_d=gap_d, storage_gap_u=gap_u, storage_gap_v=gap_v, separation=sep)
    assert gap_d <= BAR and gap_u <= BAR and gap_v <= BAR, (gap_d, gap_u, gap_v, sep)


# ---------------------------------------------------------------------------------------------------------------------
# wiring
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coupled():
    return synth.make_problem([(300, 200), (300, 160)], 5, phi=2.0)


def _inner(data, prob, n_iters, idx=(0,), **more):
    """res_nmtf_inner(precision="fp64") on the views ``idx`` of the coupled problem (``data``: those views as given)."""
    idx = list(idx)
    names = dict(row_names=[prob.row_names[i] for i in idx], col_names=[prob.col_names[i] for i in idx])
    rs, cs = naming.shared_names(names["row_names"]), naming.shared_names(names["col_names"])
    mats = [np.asarray(mm, dtype=np.float64)[np.ix_(idx, idx)] for mm in (prob.phi, prob.xi, prob.psi)]
    V = len(idx)
    res = api.res_nmtf_inner(data, rs, cs, None, None, None, [5] * V, *mats, n_iters=n_iters, spurious=False, seed=6,
                             max_iters=300, precision="fp64", **names, **more)
    return res, names, rs, cs, mats


@pytest.mark.parametrize("kind", ["dense", "sparse", "mixed"])
@pytest.mark.parametrize("n_iters", [10, None])
def test_res_nmtf_inner_reports_and_runs_from_this_start(kind, n_iters):
    prob = coupled()
    thin_out = sp.csc_matrix(sparsify(np.asarray(prob.data[1]), 0.3, 9))
    data = {"dense": [prob.data[0]], "sparse": [thin_out], "mixed": [prob.data[0], thin_out]}[kind]
    idx = {"dense": (0,), "sparse": (1,), "mixed": (0, 1)}[kind]
    flags = {} if kind == "dense" else {"fp64_sparse": True}
    res, names, rs, cs, mats = _inner(data, prob, n_iters, idx, fp64_init=True, return_init=True, **flags)
    want = engine.fp64_init_svd(data, 5, seed=6)
    assert_same_start(res["init"], want, kind)
    problem = {"data": data, "k": 5, "init_f": [w[0] for w in want], "init_s": [w[1] for w in want], "init_g": [w[2] for w in want],
               "init_lam": [w[3] for w in want], "init_mu": [w[4] for w in want], "phi": mats[0], "xi": mats[1], "psi": mats[2],
               "row_pairs": batched.pair_table(names["row_names"], rs), "col_pairs": batched.pair_table(names["col_names"], cs),
               "n_iters": n_iters}
    ref = engine.fp64_run(problem, tol=1.0e-6, max_iters=300)
    for key, out in (("output_f", "f"), ("output_s", "s"), ("output_g", "g")):
        for v in range(len(data)):
            assert same_bits(res[key][v], ref[out][v]), (kind, key, v)
    assert np.asarray(res["All_Error"]).tobytes() == np.asarray(ref["all_error"]).tobytes()
    if n_iters is None:
        assert 1 < ref["iters"] < 300


def test_the_start_stays_on_the_device_under_fp64_device():
    prob = coupled()
    t = torch.as_tensor(np.asarray(prob.data[0]), device=DEV)
    res, *_ = _inner([t], prob, 5, fp64_init=True, return_init=True, fp64_device=True, output="torch")
    want = engine.fp64_init_svd([t], 5, seed=6, output="torch")
    assert all(torch.is_tensor(a) and a.is_cuda for a in res["init"][0])
    assert_same_start(res["init"], want, "fp64_device")


def test_flag_on_and_off_agree_to_the_f32_routes_bar():
    """dense_data(1000, 700, 8, .), 30 sweeps: the two starts differ by the f32 rounding of the image alone, and F, G, S
    after the sweeps agree within the f32 route's own bar of 2e-5 (relative Frobenius norm per factor)."""
    x = T.dense_data(1000, 700, 8, 1108)
    runs = [api.res_nmtf_inner([x], None, None, None, None, None, [8], None, None, None, n_iters=30, spurious=False, seed=2,
                               precision="fp64", **flag) for flag in ({}, {"fp64_init": True})]
    for key in ("output_f", "output_g", "output_s"):
        a, b = runs[0][key][0], runs[1][key][0]
        gap = np.linalg.norm(a - b) / np.linalg.norm(a)
        record("flag_on_off", **{key: gap})
        assert gap <= T.CEILING, (key, gap)
    assert not same_bits(runs[0]["output_f"][0], runs[1]["output_f"][0])


def test_fp64_default_pipeline_with_fp64_init_picks_the_planted_k():
    """test_gpu_fp64_stability.test_fp64_default_pipeline_picks_the_planted_k with every start from this route."""
    from test_gpu_bisil import planted as planted_blocks
    x1, rc, cc = planted_blocks(1)
    x2, _, _ = planted_blocks(2)
    res = api.apply_resnmtf([x1, x2], k_max=5, k_sweep=True, return_sweep=True, seed=3, precision="fp64", num_repeats=2,
                            n_stability=2, max_iters=300, spurious=True, spurious_on_device=True, fp64_spurious=True,
                            fp64_stability=True, fp64_init=True)
    sweep = res["k_sweep"]
    assert sweep["k"][:3] == [3, 4, 5] and sweep["k"][int(np.argmax(sweep["bisil"]))] == 3
    assert res["output_f"][0].shape == (180, 3)
    for v in range(2):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# refusals that reach the device checks
# ---------------------------------------------------------------------------------------------------------------------
def test_an_all_zero_view_and_a_non_finite_device_view_are_refused_and_write_nothing():
    with pytest.raises(ResnmtfError, match="view 0 is all zero"):
        engine.fp64_init_svd([np.zeros((40, 30))], 3)
    bad = torch.ones((40, 30), dtype=torch.float64, device=DEV)
    bad[3, 4] = float("nan")
    with pytest.raises(ResnmtfError, match="view 1 holds entries that are not finite"):
        engine.fp64_init_svd([T.dense_data(40, 30, 3, 1), bad], 3)
    with pytest.raises(ResnmtfError, match="k exceeds a view dimension"):
        engine.fp64_init_svd([T.dense_data(40, 30, 3, 1)], 31)
    ok = engine.fp64_init_svd([T.dense_data(40, 30, 3, 1)], 3)      # the next call runs
    assert np.isfinite(ok[0][0]).all()
