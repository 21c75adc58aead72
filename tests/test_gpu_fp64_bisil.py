"""The bisilhouette in double precision (resnmtf_fp64_bisil): engine.fp64_bisil against the fp64
restatement (bisil_ref) on data that fp32 does NOT hold, what fp32 cannot see, bit for bit the existing scorer where both
see the same numbers, every route X takes in, the API (score, device route, fp64 k sweep) and the guards of the C entry.

Data of section 1: ``rng.random`` doubles times planted block structure (``planted``: the blocks, backgrounds and
defectors of test_gpu_bisil_forms.structured, every entry multiplied by a uniform double in [0.75, 1.25)), so no entry is
fp32-representable and the reference silhouettes spread over negative and positive values (asserted per case).

Cases of section 1 (the launch forms are those of test_gpu_bisil_forms.py; ``test_forms_covered`` asserts them):
* shapes     150 x 90 and 40 x 30 at K = 1, 3, 5 (one empty, one singleton bicluster), 17 and 64, overlapping.
* edges      150 x 90, K = 3: member counts 63 / 64 / 65 on a union of exactly 128 rows, 31 / 32 / 33 on a union of
             exactly 64 columns (the column side has members and features swapped; both unions end on a 64 boundary).
* chunks     2950 x 60 (test_gpu_bisil_forms.chunk2_ragged's clusters): chunk_tiles 2, 24 chunks, the last of one tile.
* kq         150 x 90 at K = 4, 5, 8, 9, 16, 17, 32, 33, 64: both sides of every switch of the kq table.

References: ``bisil_ref.silhouettes`` everywhere but the chunk case (``silhouettes_allpairs``).

Bars (absolute, per metric): the worst |engine.fp64_bisil - reference| over all of these cases and both sides measured on
the MI355X, times four, rounded up to one significant digit; none may exceed 1e-9, the bar of test_gpu_bisil.py.  The
margin covers another draw of the same size (the device is deterministic; the reference sums in NumPy's order).

    metric      worst measured   case and side          bar
    euclidean   6.453e-16        s150_K8 columns        3e-15
    manhattan   8.119e-16        s150_K4 rows           4e-15
    cosine      1.976e-14        s150_K64 columns       8e-14   (1 - cos cancels for near-parallel lines)

The chunk case measured 4.4e-16 / 5.1e-16 / 7.8e-16, the sub-fp32 case of section 2 2.2e-16 (euclidean) and exactly 0
(manhattan).  The same values stand in MEASURED_WORST / BARS below.

Every test prints ``MEASURED <case> <metric> <side>: <value>`` before it asserts.

Mutants (no GPU, ``test_mutants_clear_the_bars``; the machinery is test_gpu_bisil_forms._side_with_bug): a dropped last
tile of U, a dropped ragged feature stage, the member left in its own count and an empty set taken as b = 0 each lie at
least 4 x the bar from the reference on these cases (the weakest is 1.1e-3 away).

Section 2 asserts euclidean and manhattan; cosine is left out there: 1 - cos of rows that agree to 2^-24 is rounding
noise in the reference itself (bisil_ref returns silhouettes of -24 on that matrix).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bisil_ref as B
import helpers
import test_gpu_bisil_forms as F
from resnmtf_amd import _lib, api, bisil, engine, naming
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

gpu = pytest.mark.gpu

METRICS = ("euclidean", "manhattan", "cosine")
CEILING = 1e-9
# worst |device - reference| measured on the MI355X over every case of section 1 and both sides, and where
MEASURED_WORST = {"euclidean": (6.453e-16, "s150_K8 cols"), "manhattan": (8.119e-16, "s150_K4 rows"),
                  "cosine": (1.976e-14, "s150_K64 cols")}
BARS = {"euclidean": 3e-15, "manhattan": 4e-15, "cosine": 8e-14}       # four times the worst, rounded up to one digit
assert all(BARS[m] >= 4.0 * MEASURED_WORST[m][0] for m in BARS)
assert max(BARS.values()) <= CEILING
MUTANT_MARGIN = 4.0


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def planted(rc, cc, seed, **kw):
    """test_gpu_bisil_forms.structured's planted blocks times uniform doubles: nothing here is fp32-representable."""
    rng = np.random.default_rng(seed + 7)
    x = F.structured(rc, cc, seed, **kw) * (0.75 + 0.5 * rng.random((rc.shape[0], cc.shape[0])))
    assert (x.astype(np.float32).astype(np.float64) != x).mean() > 0.99
    return x


def members(rng, n_pts, K, size, empty=(), singleton=()):
    """n_pts x K, ``size`` members per bicluster at random positions (overlapping); for K >= 8 bicluster K - 1 shares
    members with bicluster 0 (bits K - 1 and 0 in one mask)."""
    mem = np.zeros((n_pts, K))
    for l in range(K):
        mem[rng.choice(n_pts, size, replace=False), l] = 1.0
    if K >= 8:
        mem[rng.choice(np.flatnonzero(mem[:, 0]), 3, replace=False), K - 1] = 1.0
    for l in empty:
        mem[:, l] = 0.0
    for l in singleton:
        mem[:, l] = 0.0
        mem[rng.choice(np.flatnonzero(mem[:, 0]), 1), l] = 1.0        # (a member of bicluster 0 too)
    return mem


def shape_case(n, m, K, seed):
    rng = np.random.default_rng(seed)
    rsize, csize = max(4, min(n // 3, 2 * n // max(K, 1))), max(3, min(m // 3, 2 * m // max(K, 1)))
    if K == 5:                                  # one bicluster without rows, one with a single row
        rc, cc = members(rng, n, K, rsize, empty=(3,), singleton=(1,)), members(rng, m, K, csize)
    else:
        rc, cc = members(rng, n, K, rsize), members(rng, m, K, csize)
    return dict(x=planted(rc, cc, seed + 1), rc=rc, cc=cc)


def edges_case():
    """150 x 90, K = 3: 63 / 64 / 65 rows on a union of exactly 128, 31 / 32 / 33 columns on a union of exactly 64."""
    rng = np.random.default_rng(41)
    rp, cp = np.sort(rng.choice(150, 128, replace=False)), np.sort(rng.choice(90, 64, replace=False))
    rc, cc = F.exact_members(rng, 150, [63, 64, 65], rp), F.exact_members(rng, 90, [31, 32, 33], cp)
    return dict(x=planted(rc, cc, 42), rc=rc, cc=cc)


def chunk_case():
    c = F.case("chunk2_ragged")
    rng = np.random.default_rng(73)
    x = c["x"] * (0.75 + 0.5 * rng.random(c["x"].shape))
    return dict(x=x, rc=c["rc"], cc=c["cc"])


KQ_KS = (4, 5, 8, 9, 16, 17, 32, 33, 64)
BUILDERS = {f"s150_K{K}": functools.partial(shape_case, 150, 90, K, 1000 + K) for K in (1, 3) + KQ_KS}
BUILDERS.update({f"s40_K{K}": functools.partial(shape_case, 40, 30, K, 2000 + K) for K in (1, 3, 5, 17, 64)})
BUILDERS.update({"edges": edges_case, "chunk": chunk_case})
ALLPAIRS = ("chunk",)
CASES = tuple(BUILDERS)
SPREAD = tuple(c for c in CASES if not c.endswith("_K1"))       # (K = 1: no other bicluster, every silhouette is 0)


@functools.lru_cache(maxsize=None)
def case(cid):
    return BUILDERS[cid]()


@functools.lru_cache(maxsize=None)
def reference(cid, metric):
    c = case(cid)
    fn = B.silhouettes_allpairs if cid in ALLPAIRS else B.silhouettes
    wr, wc = fn(c["x"], c["rc"], c["cc"], metric)
    wr.setflags(write=False); wc.setflags(write=False)
    return wr, wc


@functools.lru_cache(maxsize=None)
def device(cid):
    """{metric: (row_sil, col_sil)} from the host route (X a NumPy array), "again" a second call of every metric."""
    c = case(cid)
    out = {"again": {}}
    for metric in METRICS:
        out[metric] = engine.fp64_bisil(c["x"], c["rc"], c["cc"], metric)
        out["again"][metric] = engine.fp64_bisil(c["x"], c["rc"], c["cc"], metric)
    return out


def check_against(cid, metric, got, want, mems, bar):
    worst = []
    for side, g, w, mem in zip(("rows", "cols"), got, want, mems):
        assert np.isfinite(g).all()
        assert (g[mem == 0] == 0).all()
        worst.append(float(np.abs(g - w).max()))
        print(f"MEASURED {cid} {metric} {side}: {worst[-1]:.3e}")
    assert max(worst) <= bar, f"{cid} {metric}: |device - reference| = {max(worst):.3e} above {bar:.1e}"


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: the forms these cases reach, the spread of the references, the mutants
# ---------------------------------------------------------------------------------------------------------------------
def test_forms_covered():
    forms = {cid: F.side_forms(case(cid)["rc"], case(cid)["cc"]) for cid in CASES}
    flat = [f for fs in forms.values() for f in fs]
    assert {f["kq"] for f in flat} == {1, 2, 4, 8, 16}
    assert {1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64} <= {f["K"] for f in flat}
    e = forms["edges"]
    assert {f["n_mem"] for f in e if f["side"] == 0} == {63, 64, 65} and {f["nf"] for f in e if f["side"] == 0} == {31, 32, 33}
    assert {f["n_u"] for f in e if f["side"] == 0} == {128} and {f["n_u"] for f in e if f["side"] == 1} == {64}
    c = [f for f in forms["chunk"] if f["side"] == 0 and f["k"] == 0][0]
    assert (c["tiles_u"], c["chunk_tiles"], c["n_chunks"]) == (47, 2, 24) and c["tiles_u"] % c["chunk_tiles"] == 1
    k5 = case("s40_K5")
    assert k5["rc"][:, 3].sum() == 0 and k5["rc"][:, 1].sum() == 1
    for cid in CASES:                          # the library's own plan says the same (no device work)
        for f in forms[cid]:
            p = engine.fp64_bisil_plan(f["n_u"], f["n_mem"], f["K"])
            assert (p["kq"], p["chunk_tiles"], p["chunks"]) == (f["kq"], f["chunk_tiles"], f["n_chunks"])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", SPREAD)
def test_reference_silhouettes_are_spread(cid, metric):
    c = case(cid)
    wr, wc = reference(cid, metric)
    s = np.concatenate([wr[c["rc"] == 1], wc[c["cc"] == 1]])
    assert s.min() < -0.05 and s.max() > 0.3, f"{cid} {metric}: reference silhouettes span only [{s.min():.3f}, {s.max():.3f}]"


MUTANTS = {          # case -> the bugs its launch forms can show
    "edges": ("last_tile_of_u_dropped", "ragged_stage_dropped", "own_bit_left_in_the_count"),
    "chunk": ("last_tile_of_u_dropped", "ragged_stage_dropped", "own_bit_left_in_the_count"),
    "s40_K5": ("own_bit_left_in_the_count", "empty_taken_as_zero"),
}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", sorted(MUTANTS))
def test_mutants_clear_the_bars(cid, metric):
    c = case(cid)
    rows, cols = B.index_sets(c["rc"], c["cc"])
    sides = ((c["x"], rows, cols), (c["x"].T, cols, rows))
    want = reference(cid, metric)
    caches = ({}, {})
    for bug in (None,) + MUTANTS[cid]:
        got = [F._side_with_bug(x, mem, feat, metric, bug, cache) for (x, mem, feat), cache in zip(sides, caches)]
        dist = max(np.abs(g[0] - w).max() for g, w in zip(got, want))
        if bug is None:
            assert dist <= 1e-13
            continue
        print(f"MUTANT {cid} {metric} {bug}: {dist:.3e} ({dist / BARS[metric]:.1e} x the bar)")
        assert any(g[1] for g in got), f"{cid}: '{bug}' changes nothing in this case's forms"
        assert dist >= MUTANT_MARGIN * BARS[metric]


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the definition
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", CASES)
def test_every_member_matches_the_reference(cid, metric):
    c = case(cid)
    check_against(cid, metric, device(cid)[metric], reference(cid, metric), (c["rc"], c["cc"]), BARS[metric])


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", ("chunk", "s150_K17", "s40_K5"))
def test_two_calls_give_equal_bits(cid, metric):
    d = device(cid)
    assert d[metric][0].any() and d[metric][1].any()
    assert np.array_equal(d[metric][0], d["again"][metric][0]) and np.array_equal(d[metric][1], d["again"][metric][1])


@gpu
def test_no_active_bicluster_gives_zeros():
    rc, cc = np.zeros((40, 3)), np.zeros((30, 3))
    rc[:5, 0] = 1.0                             # rows without columns, columns without rows
    cc[:4, 1] = 1.0
    rs, cs = engine.fp64_bisil(np.random.default_rng(0).random((40, 30)), rc, cc)
    assert rs.shape == (40, 3) and cs.shape == (30, 3) and not rs.any() and not cs.any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. what fp32 cannot see
# ---------------------------------------------------------------------------------------------------------------------
def below_fp32():
    """X = 1 + 2^-30 P, P a planted integer matrix: three blocks of height 40 plus integer noise below 16.  Every entry
    is exact in fp64 and rounds to 1.0 in fp32: the entries of P stay below 2^6, since 2^-30 P must stay below half of
    fp32's step at 1, 2^-24 (an entry of 2^10 would survive in the fp32 image as 1 + 2^-20)."""
    rng = np.random.default_rng(5)
    n, m, K = 90, 60, 3
    rb, cb = np.repeat(np.arange(K), 30), np.repeat(np.arange(K), 20)
    rc, cc = np.eye(K)[rb], np.eye(K)[cb]
    rc[rng.choice(n, 6, replace=False), 0] = 1.0            # a few rows in two biclusters: misplaced in bicluster 0
    p = (40 * (rb[:, None] == cb[None, :]) + rng.integers(0, 16, (n, m))).astype(np.float64)
    assert p.max() < 64 <= 2 ** 10 and (p == np.round(p)).all()
    x = 1.0 + 2.0 ** -30 * p
    assert ((x - 1.0) * 2.0 ** 30 == p).all() and (x.astype(np.float32) == 1.0).all()
    return x, p, rc, cc


@gpu
@pytest.mark.parametrize("metric", ("euclidean", "manhattan"))
def test_differences_below_fp32_decide_the_score(metric):
    """Expected: the silhouettes of X are those of the integer matrix P itself, bit for bit in the reference -- the
    differences x - y = 2^-30 (p - q) are exact, and a power-of-two scale passes exactly through squares, sums, square
    roots and the quotient (b - a) / max(a, b) -- so the planted blocks score as they do on P (members above 0.5,
    the misplaced rows below 0), while the fp32 image is all ones and scores 0 everywhere."""
    x, p, rc, cc = below_fp32()
    want = B.silhouettes(x, rc, cc, metric)
    of_p = B.silhouettes(p, rc, cc, metric)
    assert np.array_equal(want[0], of_p[0]) and np.array_equal(want[1], of_p[1])
    assert (want[0][60:90, 2] > 0.5).all() and want[0].min() < 0.0 and np.abs(want[1]).max() > 0.1
    got = engine.fp64_bisil(x, rc, cc, metric)
    check_against("below_fp32", metric, got, want, (rc, cc), BARS[metric])
    assert np.abs(got[0]).max() > 0.1 and np.abs(got[1]).max() > 0.1
    with Engine([90], [60], [2]) as e:          # the workaround: a handle holds X as fp32, i.e. as ones
        e.set_view(0, x)
        assert (e.get_view(0) == 1.0).all()
        rs32, cs32 = e.bisil(0, rc, cc, metric)
    assert not rs32.any() and not cs32.any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. bit for bit the existing scorer where both see the same numbers
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", ("chunk2_ragged", "K17", "edges_K12"))       # K = 3 with 24 chunks, K = 17, K = 12
def test_bitwise_the_fp32_image_scorer_on_fp32_valued_data(cid):
    c = F.case(cid)                             # float32-valued entries
    n, m = c["x"].shape
    assert np.array_equal(F.f32(c["x"]), c["x"])
    with Engine([n], [m], [2]) as e:
        e.set_view(0, c["x"])                   # loaded pre-processed: the image holds these values
        assert np.array_equal(e.get_view(0), c["x"])
        for metric in METRICS:
            a = e.bisil(0, c["rc"], c["cc"], metric)
            b = engine.fp64_bisil(c["x"], c["rc"], c["cc"], metric)
            assert a[0].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), metric


# ---------------------------------------------------------------------------------------------------------------------
# 4. every route in
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("row_major", "col_major", "strided", "expanded")
DTYPES = ("float64", "float32", "float16", "bfloat16")


def _tensor(x, layout, dtype):
    import torch
    dev, dt = torch.device("cuda", 0), getattr(torch, dtype)
    n, m = x.shape
    if layout == "row_major":
        return torch.as_tensor(x, device=dev).to(dt).contiguous()
    if layout == "col_major":
        return torch.as_tensor(x, device=dev).to(dt).t().contiguous().t()
    if layout == "strided":
        big = torch.zeros((2 * n, 3 * m + 1), dtype=dt, device=dev)
        big[::2, 1::3] = torch.as_tensor(x, device=dev).to(dt)
        return big[::2, 1::3]
    return torch.as_tensor(x[:1], device=dev).to(dt).expand(n, m)           # stride 0 along the rows


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_device_routes_are_bitwise_the_host_route(layout, dtype):
    c = case("s150_K5") if layout != "expanded" else case("s150_K3")
    t = _tensor(c["x"], layout, dtype)
    assert tuple(t.shape) == c["x"].shape
    rs, cs = int(t.stride(0)), int(t.stride(1))
    want_forms = {"row_major": ("lds", "points"), "col_major": ("points", "lds"), "strided": ("lds", "points"),
                  "expanded": ("points", "lds")}[layout]
    assert engine.fp64_bisil_plan(64, 64, 5, rs, cs)["gather"] == want_forms
    host = t.double().cpu().numpy()
    for metric in METRICS:
        a = engine.fp64_bisil(t, c["rc"], c["cc"], metric)
        b = engine.fp64_bisil(host, c["rc"], c["cc"], metric)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), metric
        again = engine.fp64_bisil(t, c["rc"], c["cc"], metric)
        assert np.array_equal(a[0], again[0]) and np.array_equal(a[1], again[1])
        if layout != "expanded":
            assert a[0].any() and a[1].any()
        if dtype == "float64" and layout != "expanded":
            check_against(f"{layout}", metric, a, reference("s150_K5", metric), (c["rc"], c["cc"]), BARS[metric])


@gpu
def test_both_gather_forms_on_both_sides():
    """Row-major puts the LDS transpose on the row side and lanes along the points on the column side; column-major the
    reverse: together both forms run on both sides (from the host-only plan), and both give the host route's bits."""
    forms = {lay: engine.fp64_bisil_plan(128, 64, 3, *s)["gather"] for lay, s in (("row_major", (90, 1)), ("col_major", (1, 150)))}
    assert forms == {"row_major": ("lds", "points"), "col_major": ("points", "lds")}
    assert {f[0] for f in forms.values()} == {"lds", "points"} and {f[1] for f in forms.values()} == {"lds", "points"}
    c = case("edges")
    host = engine.fp64_bisil(c["x"], c["rc"], c["cc"], "euclidean")
    for lay in forms:
        got = engine.fp64_bisil(_tensor(c["x"], lay, "float64"), c["rc"], c["cc"], "euclidean")
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])


@gpu
def test_cluster_tensors_and_cpu_tensors_are_brought_to_the_host():
    import torch
    c = case("s40_K5")
    want = engine.fp64_bisil(c["x"], c["rc"], c["cc"], "manhattan")
    dev = torch.device("cuda", 0)
    got = engine.fp64_bisil(torch.as_tensor(c["x"]), torch.as_tensor(c["rc"], device=dev), torch.as_tensor(c["cc"]), "manhattan")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="floating dtype"):
        engine.fp64_bisil(torch.ones((40, 30), dtype=torch.int32, device=dev), c["rc"], c["cc"])
    with pytest.raises(ValueError, match="row clusters must be 40 x k"):
        engine.fp64_bisil(c["x"], c["rc"][:39], c["cc"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the API
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coupled():
    prob = helpers.coupled_problem([(120, 90), (100, 90)], 4, 5, phi_w=1.0)
    rs, cs = naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)
    common = dict(spurious=False, row_names=prob.row_names, col_names=prob.col_names, precision="fp64", seed=3,
                  score_bisil=True, fp64_bisil=True)
    res = api.res_nmtf_inner(prob.data, rs, cs, None, None, None, [4, 4], prob.phi, prob.xi, prob.psi, 40, **common)
    return prob, rs, cs, common, res


@gpu
def test_api_score_is_the_combination_of_fp64_bisil():
    prob, _, _, _, res = coupled()
    views = []
    for v in range(2):
        sil = engine.fp64_bisil(prob.data[v], res["row_clusters"][v], res["col_clusters"][v], "euclidean")
        views.append(bisil.view_score(res["row_clusters"][v], res["col_clusters"][v], *sil))
    assert res["bisil"] == bisil.overall(views) and res["bisil"] != 0.0
    want = B.bisil(prob.data, res["row_clusters"], res["col_clusters"], "euclidean")
    print(f"MEASURED api bisil euclidean: {abs(res['bisil'] - want):.3e}")
    assert abs(res["bisil"] - want) <= BARS["euclidean"]


@gpu
def test_api_device_route_gives_the_same_bits():
    import torch
    prob, rs, cs, common, res = coupled()
    dev = torch.device("cuda", 0)
    data = [torch.as_tensor(prob.data[0], device=dev), torch.as_tensor(prob.data[1], device=dev).t().contiguous().t()]
    there = api.res_nmtf_inner(data, rs, cs, None, None, None, [4, 4], prob.phi, prob.xi, prob.psi, 40, fp64_device=True,
                               output="torch", **common)
    assert isinstance(there["row_clusters"][0], torch.Tensor) and there["row_clusters"][0].device == dev
    assert there["bisil"] == res["bisil"]
    for key in ("output_f", "row_clusters", "col_clusters"):
        for v in range(2):
            assert np.array_equal(there[key][v].cpu().numpy(), res[key][v]), (key, v)


@gpu
def test_fp64_k_sweep_picks_the_planted_k():
    """test-resnmtf.R:123-135 ("resnmtf runs with k not specified") as tests/test_gpu_bisil.py builds it, in fp64."""
    from test_gpu_bisil import planted as planted_blocks
    x1, rc, cc = planted_blocks(1)
    x2, _, _ = planted_blocks(2)
    data = [x1, x2]
    res = api.apply_resnmtf(data, k_max=5, spurious=False, stability=False, k_sweep=True, return_sweep=True, seed=3,
                            precision="fp64")
    sweep = res["k_sweep"]
    assert sweep["k"][:3] == [3, 4, 5] and sweep["k"][int(np.argmax(sweep["bisil"]))] == 3
    assert res["output_f"][0].shape == (180, 3) and res["bisil"] == max(sweep["bisil"])
    for v in range(2):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))
    p = api.prepare(data, None, None, None, None, None, normalise=True, symmetrise=True)
    one = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, k_vec=[3, 3], phi=p.phi, xi=p.xi, psi=p.psi, spurious=False,
                             row_names=p.row_names, col_names=p.col_names, seed=3 + 3, precision="fp64", score_bisil=True,
                             fp64_bisil=True)
    assert one["bisil"] == res["bisil"]
    for key in ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "lambda", "mu"):
        for v in range(2):
            assert np.array_equal(one[key][v], res[key][v]), (key, v)
    assert np.array_equal(one["All_Error"], res["All_Error"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the guards of the C entry: each refusal returns its code and leaves the outputs untouched
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _call(n=40, m=30, k=3, metric=0, x="host", rc=None, cc=None, struct_size=None, x_dev=None, device_id=0, null=()):
    """resnmtf_fp64_bisil through ctypes; returns (code, text, row_sil, col_sil), the outputs pre-filled with SENTINEL."""
    lib = _lib.load()
    rng = np.random.default_rng(0)
    shape = (max(n, 1), max(m, 1), max(min(k, 64), 1))
    xh = np.asfortranarray(rng.random(shape[:2]))
    rc = np.asfortranarray((rng.random((shape[0], shape[2])) < 0.5).astype(np.float64) if rc is None else rc)
    cc = np.asfortranarray((rng.random((shape[1], shape[2])) < 0.5).astype(np.float64) if cc is None else cc)
    rs, cs = np.full((shape[0], 65), SENTINEL, order="F"), np.full((shape[1], 65), SENTINEL, order="F")
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                  # noqa: E731
    job = _lib.Fp64BisilJob()
    job.struct_size = C.sizeof(job) if struct_size is None else struct_size
    job.n, job.m, job.k, job.metric = n, m, k, metric
    if x in ("host", "both"):
        job.x = dp(xh)
    if x_dev is not None:
        job.x_dev = x_dev
    job.row_clusters, job.col_clusters, job.row_sil, job.col_sil = dp(rc), dp(cc), dp(rs), dp(cs)
    for name in null:
        setattr(job, name, None)
    code = lib.resnmtf_fp64_bisil(device_id, C.byref(job))
    return code, (lib.resnmtf_last_error(None) or b"").decode(), rs, cs


def _refused(code, want_code, text, match, rs, cs):
    assert code == want_code and match in text, (code, text)
    assert (rs == SENTINEL).all() and (cs == SENTINEL).all()


@gpu
def test_guards_of_the_c_entry():
    import torch
    dev = torch.device("cuda", 0)
    t = torch.rand((40, 30), dtype=torch.float64, device=dev)
    dm = lambda ptr, dtype=0, rs=30, cs=1: _lib.DeviceMatrix(ptr, dtype, rs, cs)      # noqa: E731
    for kw, match in ((dict(struct_size=8), "struct_size mismatch"), (dict(k=0), "k must be in [1, 64]"), (dict(k=65), "k must be in [1, 64]"),
                      (dict(n=0), "view dimensions must be positive"), (dict(m=-1), "view dimensions must be positive"),
                      (dict(metric=3), "metric must be 0"), (dict(metric=-1), "metric must be 0"),
                      (dict(x="both", x_dev=dm(t.data_ptr())), "X is given in two places"),
                      (dict(x="none"), "X is given in no place"),
                      (dict(null=("row_sil",)), "are NULL"), (dict(null=("col_clusters",)), "are NULL"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), dtype=4)), "unknown dtype"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), dtype=-1)), "unknown dtype"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), rs=-30)), "strides must be >= 0"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), cs=-1)), "strides must be >= 0"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), rs=1 << 40)), "reaches beyond its allocation")):
        code, text, rs, cs = _call(**kw)
        _refused(code, 1, text, match, rs, cs)
    host = np.zeros((40, 30))
    code, text, rs, cs = _call(x="none", x_dev=dm(host.ctypes.data))
    _refused(code, 1, text, "x_dev is not device memory of device 0", rs, cs)
    # a cluster entry other than 0 or 1: resnmtf_bisil's messages, the rows first
    rng = np.random.default_rng(1)
    rc, cc = (rng.random((40, 3)) < 0.5).astype(np.float64), (rng.random((30, 3)) < 0.5).astype(np.float64)
    bad_r, bad_c = rc.copy(), cc.copy()
    bad_r[5, 0], bad_c[2, 0] = 0.5, np.nan
    for kw, match in ((dict(rc=bad_r, cc=bad_c), "row_clusters entries must be 0 or 1"), (dict(rc=bad_r), "row_clusters entries must be 0 or 1"),
                      (dict(cc=bad_c), "col_clusters entries must be 0 or 1")):
        for route in (dict(), dict(x="none", x_dev=dm(t.data_ptr()))):
            code, text, rs, cs = _call(**kw, **route)
            _refused(code, 1, text, match, rs, cs)
    code, text, rs, cs = _call(device_id=99)
    _refused(code, 1, text, "device_id out of range", rs, cs)
    # the job itself is fine: the same call without a fault runs, on both routes, and gives the same bits
    code, _, rs, cs = _call(rc=rc, cc=cc)
    assert code == 0 and (rs[:, :3] != SENTINEL).all() and (rs[:, 3:] == SENTINEL).all() and (cs[:, 3:] == SENTINEL).all()
    assert lib_null_job() == 1


def lib_null_job():
    return _lib.load().resnmtf_fp64_bisil(0, None)


@gpu
def test_workspace_above_the_free_memory_is_refused_with_its_byte_count():
    """200000 x 200000 through an expanded two-byte tensor (one element of device memory), one bicluster holding every
    row and column: G alone is 200000 x 200000 doubles = 320 GB, more than the device has.  Nothing is allocated."""
    import torch
    n = 200000
    t = torch.ones((1, 1), dtype=torch.float16, device=torch.device("cuda", 0)).expand(n, n)
    ones = np.ones((n, 1))
    with pytest.raises(ResnmtfError, match=r"fp64_bisil workspace: \d+ bytes asked for \(320000000000 of them the restricted block") as e:
        engine.fp64_bisil(t, ones, ones)
    assert e.value.code == 4
