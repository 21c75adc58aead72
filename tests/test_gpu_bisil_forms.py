"""The bisilhouette kernels checked member by member against fp64, for every launch form of resnmtf_bisil.

``bisil_impl`` (csrc/resnmtf_hip.hip) picks, per side and active bicluster, a ``bisil_dist_kernel`` instantiation from K
and a chunking of U's 64-wide tiles from the sizes; the kernel stages 32 features at a time and 64 members per workgroup.
The cases below are chosen from those forms, not drawn at random:

* K forms    150 x 97 at K = 4, 5, 8, 9, 12, 16, 17, 32, 33, 64: both sides of every switch of the kq table, K = 12 and
             16 inside the kq = 4 range; for K >= 8 bicluster K - 1 shares members with bicluster 0 (bits K - 1 and 0 in
             one mask, bit 63 at K = 64).
* edges      330 x 150, K = 12, exact member counts at random positions: n_mem = 1, 2, 63, 64, 65, 128, 129 and
             nf = 1, 31, 32, 33, 64, 65 on the row side (the column side has them swapped); a variant whose unions are
             exactly 192 rows / 128 columns (n_u == upad: no padding behind the last point) and one with 129 / 129.
* chunks     chunk2_ragged 2950 x 60 (tiles_u = tiles_m = 47: chunk_tiles 2, 24 chunks, the last of one tile, the last
             tile 6 wide; two smaller biclusters at chunk_tiles 1 in the same call) and chunk3 5000 x 40 (tiles_u 79,
             tiles_m 63: chunk_tiles 3, 27 chunks, the last of one tile).
* crafted    the epilogue's rules, each asserted on the device's own output: c = cnt[l] - own bit, c == 0 skipped, the
             first minimum, max(a, b) == 0, a singleton, biclusters with rows or columns only, zero rows under cosine.
* sparse     edges_K12, K = 16 and chunk2_ragged thinned to about 30 % stored with a dense and an empty line, through
             resnmtf_bisil_sparse and through resnmtf_bisil on a dense handle with the same fp32 values (bitwise equal).

Data: planted rank-one blocks with per-bicluster profiles plus background and noise (``structured``); a share of every
bicluster's stated members carries no block ("defectors"), so every data case holds members with a > b.  The spread of
the reference silhouettes is asserted per case and metric: some member below -0.2, some above +0.5.  The crafted cases
assert their rule instead.  The data are rounded to fp32 on the host, the device's copy is asserted equal to it, so the
references are computed once and shared with the host tests.

References: ``bisil_ref.silhouettes`` (the literal loops) everywhere but the two chunk cases, which use
``bisil_ref.silhouettes_allpairs`` (2 to 5 s per metric and case on the host; the device takes under a second);
``test_allpairs_agrees_with_the_literal_loops`` (no GPU) holds the two statements together at 1e-13.

Bars (absolute, per metric; ceiling 1e-9, the bar of test_gpu_bisil.py).  Each is the worst |device - reference| over
all cases and both sides measured on the MI355X, times a margin of at least 4 (the device is deterministic, the
reference's summation order is not the device's and may change with the NumPy build; margins of 11 to 13 x chosen):

    metric      worst measured   case and side          bar       margin
    euclidean   1.193e-15        chunk3 rows            1.5e-14   12.6 x
    manhattan   2.220e-16        chunk2_ragged rows     2.5e-15   11.3 x   (exactly 0 in all but the two chunk cases)
    cosine      2.098e-14        edges_K12_u129 rows    2.5e-13   11.9 x   (1 - cos cancels for near-parallel rows)

The same values stand in MEASURED_WORST / BARS below; every test prints ``MEASURED <case> <metric> <side>: <value>``.
The weakest mutant is 9.3e-4 away (chunk2_ragged, manhattan, the last tile of U dropped): 3.7e11 x its bar.

Mutants (no GPU, ``test_mutants_clear_the_bars``): for one representative per family, host references of the bugs this
suite exists to catch must be at least 4 x the bar away from the true reference.  ``test_forms_covered`` (no GPU)
restates the chunk rule and the kq table and asserts that the case list reaches every form named above.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import bisil_ref as B
from resnmtf_amd.engine import Engine

gpu = pytest.mark.gpu

METRICS = ("euclidean", "manhattan", "cosine")
CEILING = 1e-9
# worst |device - reference| measured on the MI355X over every case and side, and the case that produced it
MEASURED_WORST = {
    "euclidean": (1.193e-15, "chunk3 rows"),             # (next: 7.6e-16 edges_K12_u192_u128 rows)
    "manhattan": (2.220e-16, "chunk2_ragged rows"),      # (chunk3 rows 1.7e-16; every other case and side exactly 0)
    "cosine": (2.098e-14, "edges_K12_u129 rows"),        # (1.9e-14 its columns; 1.4e-14 edges_K12 columns)
}
BARS = {"euclidean": 1.5e-14, "manhattan": 2.5e-15, "cosine": 2.5e-13}       # margins 12.6 x, 11.3 x, 11.9 x
assert all(BARS[m] >= 4.0 * MEASURED_WORST[m][0] for m in BARS)
assert max(BARS.values()) <= CEILING
MUTANT_MARGIN = 4.0


# ---------------------------------------------------------------------------------------------------------------------
# the launch forms: a restatement of bisil_impl's rules (csrc/resnmtf_hip.hip names this module at the rule)
# ---------------------------------------------------------------------------------------------------------------------
def kq_of(K):
    return 1 if K <= 4 else 2 if K <= 8 else 4 if K <= 16 else 8 if K <= 32 else 16


def chunk_plan(n_u, n_mem):
    """(tiles_u, chunk_tiles, n_chunks) of one side of one bicluster."""
    tiles_u, tiles_m = -(-n_u // 64), -(-n_mem // 64)
    chunk_tiles = -(-tiles_u // max(1, min(tiles_u, -(-2048 // tiles_m))))
    return tiles_u, chunk_tiles, -(-tiles_u // chunk_tiles)


def side_forms(rc, cc):
    """Per side (0 rows, 1 columns) and active bicluster: the sizes bisil_impl launches with."""
    K = rc.shape[1]
    active = [k for k in range(K) if rc[:, k].any() and cc[:, k].any()]
    out = []
    for sd, (mine, other) in enumerate(((rc, cc), (cc, rc))):
        n_u = int(mine[:, active].any(axis=1).sum()) if active else 0
        for k in active:
            n_mem, nf = int(mine[:, k].sum()), int(other[:, k].sum())
            tiles_u, chunk_tiles, n_chunks = chunk_plan(n_u, n_mem)
            out.append(dict(side=sd, k=k, K=K, kq=kq_of(K), n_u=n_u, n_mem=n_mem, nf=nf, tiles_u=tiles_u,
                            chunk_tiles=chunk_tiles, n_chunks=n_chunks))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def structured(rc, cc, seed, true_rc=None, true_cc=None, defect=0.12, noise=0.05):
    """Planted blocks plus noise for the stated clusters ``rc`` / ``cc``: block l is the rank-one profile
    h_l r_l[i] p_l[j] on its TRUE rows and columns, every true member also carries a background profile of its bicluster
    over the whole line, and uniform noise covers the view.  The true sets are the stated ones without a share
    ``defect`` of the members of every bicluster with at least 8 (at least one each): those are stated members that look
    like non-members, so their a exceeds their b."""
    rng = np.random.default_rng(seed)
    (n, K), m = rc.shape, cc.shape[0]

    def true_sets(stated, given):
        if given is not None:
            return given.copy()
        t = stated.copy()
        for l in range(K):
            mem = np.flatnonzero(t[:, l])
            if mem.size >= 8:
                t[rng.choice(mem, max(1, int(defect * mem.size)), replace=False), l] = 0.0
        return t

    trc, tcc = true_sets(rc, true_rc), true_sets(cc, true_cc)
    h = np.exp(rng.uniform(np.log(1.0), np.log(60.0), K))
    r, p = 0.85 + 0.3 * rng.random((n, K)), 0.85 + 0.3 * rng.random((K, m))
    q, t = rng.random((K, m)) ** 3, rng.random((n, K)) ** 3
    x = (trc * r * h[None, :]) @ (tcc.T * p) + 0.3 * (trc @ q + t @ tcc.T) + noise * rng.random((n, m))
    return f32(x)


def exact_members(rng, n_pts, sizes, pool=None):
    """n_pts x K 0 / 1 with exactly sizes[l] members of bicluster l at random positions of ``pool`` (default: every
    point), every pool point in some bicluster: the biclusters overlap and are non-contiguous."""
    pool = np.arange(n_pts) if pool is None else np.asarray(pool)
    assert sum(sizes) >= pool.size and max(sizes) <= pool.size
    out = np.zeros((n_pts, len(sizes)))
    fresh = list(rng.permutation(pool))
    for l in rng.permutation(len(sizes)):
        take = [fresh.pop() for _ in range(min(sizes[l], len(fresh)))]
        rest = np.setdiff1d(pool, take)
        take += list(rng.choice(rest, sizes[l] - len(take), replace=False))
        out[take, l] = 1.0
    assert not fresh and (out.sum(0) == np.asarray(sizes)).all()
    return out


def k_form(K):
    """150 x 97, 20 members per bicluster and side; for K >= 8 bicluster K - 1 holds five members of bicluster 0."""
    rng = np.random.default_rng(500 + K)
    sides = []
    for n_pts in (150, 97):
        mem = np.zeros((n_pts, K))
        for l in range(K):
            mem[rng.choice(n_pts, 20, replace=False), l] = 1.0
        if K >= 8:
            mem[:, K - 1] = 0.0
            shared = rng.choice(np.flatnonzero(mem[:, 0]), 5, replace=False)
            mem[shared, K - 1] = 1.0
            mem[rng.choice(np.flatnonzero(mem[:, 0] == 0), 15, replace=False), K - 1] = 1.0
        sides.append(mem)
    rc, cc = sides
    return dict(x=structured(rc, cc, 600 + K), rc=rc, cc=cc)


EDGE_ROWS = [129, 128, 65, 64, 63, 2, 1, 64, 63, 65, 2, 129]      # n_mem of the row side, nf of the column side
EDGE_COLS = [65, 64, 33, 32, 31, 1, 33, 1, 65, 31, 64, 32]        # nf of the row side, n_mem of the column side


def edges(seed, row_pool=None, col_pool=None):
    """330 x 150, K = 12 with the member counts above; the unions are the pools (every row / column by default).  The
    one-row bicluster's row is also a member of bicluster 0 (for that row the one-row bicluster is skipped)."""
    rng = np.random.default_rng(seed)
    n, m = 330, 150
    rp = None if row_pool is None else np.sort(rng.choice(n, row_pool, replace=False))
    cp = None if col_pool is None else np.sort(rng.choice(m, col_pool, replace=False))
    rc, cc = exact_members(rng, n, EDGE_ROWS, rp), exact_members(rng, m, EDGE_COLS, cp)
    sole = int(np.flatnonzero(rc[:, 6])[0])
    if rc[sole, 0] == 0:                                   # (swap it in: the count stays 129)
        out = np.flatnonzero((rc[:, 0] == 1) & (rc.sum(1) > 1))[0]
        rc[out, 0] = 0.0
        rc[sole, 0] = 1.0
    return dict(x=structured(rc, cc, seed + 1), rc=rc, cc=cc)


def chunk2_ragged():
    """2950 x 60: bicluster 0 holds 2945 rows (47 member tiles over U's 47 tiles), biclusters 1 and 2 hold 200 and 70."""
    rng = np.random.default_rng(71)
    n, m = 2950, 60
    rc, cc = np.zeros((n, 3)), np.zeros((m, 3))
    rc[rng.choice(n, 200, replace=False), 1] = 1.0
    rc[rng.choice(n, 70, replace=False), 2] = 1.0
    rc[:, 0] = 1.0
    rc[rng.choice(np.flatnonzero(rc[:, 1]), 5, replace=False), 0] = 0.0
    for l, nc in enumerate((40, 33, 17)):
        cc[rng.choice(m, nc, replace=False), l] = 1.0
    true_rc = rc.copy()
    true_rc[(rc[:, 1] + rc[:, 2]) > 0, 0] = 0.0            # the small biclusters' rows carry no block of bicluster 0
    for l in (1, 2):
        mem = np.flatnonzero(rc[:, l])
        true_rc[rng.choice(mem, mem.size // 8, replace=False), l] = 0.0
    return dict(x=structured(rc, cc, 72, true_rc=true_rc), rc=rc, cc=cc)


def chunk3():
    """5000 x 40: bicluster 0 holds 4000 rows on 24 columns, bicluster 1 the other 1000 and 150 of those, bicluster 2
    90 rows."""
    rng = np.random.default_rng(81)
    n, m = 5000, 40
    rc, cc = np.zeros((n, 3)), np.zeros((m, 3))
    big = rng.choice(n, 4000, replace=False)
    rc[big, 0] = 1.0
    rc[rc[:, 0] == 0, 1] = 1.0
    rc[rng.choice(big, 150, replace=False), 1] = 1.0
    rc[rng.choice(n, 90, replace=False), 2] = 1.0
    for l, nc in enumerate((24, 16, 9)):
        cc[rng.choice(m, nc, replace=False), l] = 1.0
    return dict(x=structured(rc, cc, 82), rc=rc, cc=cc)


def thinned(case):
    """The largest 30 % of the entries stored (the blocks stay, most of the background goes); row ``dense`` keeps
    every entry, row and column ``empty`` none.  The three lines are members / features of bicluster 0."""
    x, rc, cc = case["x"], case["rc"], case["cc"]
    rows0, cols0 = np.flatnonzero(rc[:, 0]), np.flatnonzero(cc[:, 0])
    dense_row, empty_row, empty_col = int(rows0[1]), int(rows0[2]), int(cols0[1])
    y = np.where(x > np.quantile(x, 0.7), x, 0.0)
    y[dense_row] = x[dense_row] + 0.01
    y[empty_row] = 0.0
    y[:, empty_col] = 0.0
    return dict(x=f32(y), rc=rc, cc=cc, lines=(dense_row, empty_row, empty_col))


# ---- crafted epilogue cases: 40 x 30, K = 4 ... 6; ``rows`` / ``cols`` list each bicluster's members ----------------
def _crafted(seed, rows, cols, n=40, m=30, vary=1.0):
    rng = np.random.default_rng(seed)
    K = len(rows)
    rc, cc = np.zeros((n, K)), np.zeros((m, K))
    for l in range(K):
        rc[list(rows[l]), l] = 1.0
        cc[list(cols[l]), l] = 1.0
    x = 0.1 + 0.3 * rng.random((n, m))
    for l in range(K):
        x += 2.0 * np.outer(rc[:, l] * (0.5 + vary * rng.random(n)), cc[:, l] * (0.5 + vary * rng.random(m)))
    return dict(x=x, rc=rc, cc=cc)


def sole_member_shared():
    """Row 3 is the only row of bicluster 1 and a member of bicluster 0: for row 3 bicluster 1 is skipped (c = 1 - 1),
    for every other row it counts, and it is their nearest.  Bicluster 3 has columns but no rows, bicluster 4 rows but no
    columns."""
    c = _crafted(901, [range(10), [3], range(20, 30), [], range(30, 35)],
                 [range(12), range(5, 17), range(15, 26), [26, 27], []])
    c["x"] = f32(c["x"])
    return c


def two_active_other_is_sole():
    """Biclusters 0 (ten rows) and 1 (row 3 of them alone) are the only active ones: row 3 has no l left, s = 0."""
    c = _crafted(902, [range(10), [3], range(30, 35), []], [range(12), range(5, 17), [], [26, 27]])
    c["x"] = f32(c["x"])
    return c


def identical_sets():
    """Biclusters 1 and 2 hold the same rows on different columns: a tie in b for bicluster 0's rows, and b = a (s = 0)
    for their own."""
    c = _crafted(903, [range(20, 30), range(5, 15), range(5, 15), []], [range(20, 30), range(10), range(10, 20), []],
                 vary=0.1)
    c["x"] = f32(c["x"])
    return c


def identical_members():
    """Every row of U is the same vector on bicluster 0's columns: every distance 0, max(a, b) = 0, s = 0 (not NaN).
    The vector's entries are multiples of 1 / 8, so its norm and dot products are exact in any order of summation and
    the cosine distance is the same power of two (or 0) in every statement of the definition."""
    c = _crafted(904, [range(8), range(10, 18), [], []], [range(10), range(10, 20), [], []])
    c["x"][np.ix_(list(range(8)) + list(range(10, 18)), range(10))] = np.round(8.0 * c["x"][0, :10]) / 8.0
    c["x"] = f32(c["x"])
    return c


def cosine_zero_rows():
    """Rows 0 and 1 are zero on bicluster 0's columns and non-zero elsewhere, row 2 is zero everywhere; rows 3, 4, 5
    complete bicluster 0.  Under cosine the three are at distance 0 from each other and 1 from every other row."""
    c = _crafted(905, [range(6), range(10, 18), [], [], []], [range(10), range(10, 20), [], [], []])
    c["x"][0:2, :10] = 0.0
    c["x"][2, :] = 0.0
    c["x"] = f32(c["x"])
    return c


K_FORMS = (4, 5, 8, 9, 12, 16, 17, 32, 33, 64)
BUILDERS = {f"K{K}": functools.partial(k_form, K) for K in K_FORMS}
BUILDERS.update({
    "edges_K12": functools.partial(edges, 31),
    "edges_K12_u192_u128": functools.partial(edges, 33, 192, 128),
    "edges_K12_u129": functools.partial(edges, 35, 129, 129),
    "chunk2_ragged": chunk2_ragged,
    "chunk3": chunk3,
    "sole_member_shared": sole_member_shared,
    "two_active_other_is_sole": two_active_other_is_sole,
    "identical_sets": identical_sets,
    "identical_members": identical_members,
    "cosine_zero_rows": cosine_zero_rows,
})
SPARSE_OF = {"sparse_edges_K12": "edges_K12", "sparse_K16": "K16", "sparse_chunk2_ragged": "chunk2_ragged"}
CRAFTED = ("sole_member_shared", "two_active_other_is_sole", "identical_sets", "identical_members", "cosine_zero_rows")
ALLPAIRS = ("chunk2_ragged", "chunk3", "sparse_chunk2_ragged")       # too large for the literal loops
DENSE_CASES = tuple(BUILDERS)
DATA_CASES = tuple(c for c in DENSE_CASES if c not in CRAFTED)
FAMILY = {c: "k_forms" for c in BUILDERS if c[0] == "K"}
FAMILY.update({c: "edges" for c in BUILDERS if c.startswith("edges")})
FAMILY.update({"chunk2_ragged": "chunks", "chunk3": "chunks"})
FAMILY.update({c: "crafted" for c in CRAFTED})
FAMILY.update({c: "sparse" for c in SPARSE_OF})


@functools.lru_cache(maxsize=None)
def case(cid):
    if cid in SPARSE_OF:
        return thinned(case(SPARSE_OF[cid]))
    return BUILDERS[cid]()


@functools.lru_cache(maxsize=None)
def reference(cid, metric):
    """(row_sil, col_sil) of the case in fp64, computed once and never written to."""
    c = case(cid)
    fn = B.silhouettes_allpairs if cid in ALLPAIRS else B.silhouettes
    wr, wc = fn(c["x"], c["rc"], c["cc"], metric)
    wr.setflags(write=False); wc.setflags(write=False)
    return wr, wc


def assert_spread(cid, metric):
    c = case(cid)
    wr, wc = reference(cid, metric)
    s = np.concatenate([wr[c["rc"] == 1], wc[c["cc"] == 1]])
    assert s.min() < -0.2 and s.max() > 0.5 and np.abs(s).max() >= 0.5, \
        f"{cid} {metric}: reference silhouettes span only [{s.min():.3f}, {s.max():.3f}]"


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: the two statements of the definition, the coverage of the forms, the mutants
# ---------------------------------------------------------------------------------------------------------------------
def _small_configs():
    """Overlap, a singleton, an empty side; for cosine a zero row (sole_member_shared has the singleton and both kinds
    of empty side, cosine_zero_rows the zero rows, K5 and edges_K12 heavy overlap)."""
    return ("sole_member_shared", "two_active_other_is_sole", "identical_sets", "identical_members", "cosine_zero_rows",
            "K5", "edges_K12")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", _small_configs())
def test_allpairs_agrees_with_the_literal_loops(cid, metric):
    c = case(cid)
    x = c["x"].copy()
    if metric == "cosine":
        x[int(np.flatnonzero(c["rc"][:, 0])[-1]), :] = 0.0            # a zero row among bicluster 0's members
    lr, lc = B.silhouettes(x, c["rc"], c["cc"], metric)
    ar, ac = B.silhouettes_allpairs(x, c["rc"], c["cc"], metric)
    worst = max(np.abs(lr - ar).max(), np.abs(lc - ac).max())
    print(f"{cid} {metric}: literal against all-pairs {worst:.3e}")
    assert np.isfinite(ar).all() and np.isfinite(ac).all()
    assert worst <= 1e-13


def test_forms_covered():
    forms = {cid: side_forms(case(cid)["rc"], case(cid)["cc"]) for cid in list(DENSE_CASES) + list(SPARSE_OF)}
    flat = [f for fs in forms.values() for f in fs]
    Ks = {f["K"] for f in flat}
    missing = []

    def need(name, ok):
        if not ok:
            missing.append(name)

    for lo, hi in ((4, 5), (8, 9), (16, 17), (32, 33)):
        need(f"both sides of the kq switch {lo}|{hi}", lo in Ks and hi in Ks and kq_of(lo) != kq_of(hi))
    need("every kq", {f["kq"] for f in flat} == {1, 2, 4, 8, 16})
    need("a K inside 9...16 besides 16", 12 in Ks and kq_of(12) == 4)
    need("K = 64", 64 in Ks)
    need("chunk_tiles 1, 2 and >= 3", {min(f["chunk_tiles"], 3) for f in flat} == {1, 2, 3})
    need("both chunkings in one call", {f["chunk_tiles"] for f in forms["chunk2_ragged"] if f["side"] == 0} == {1, 2})
    multi = [f for f in flat if f["chunk_tiles"] > 1]
    need("a last chunk shorter than the rest", any(f["tiles_u"] % f["chunk_tiles"] for f in multi))
    need("a ragged last tile behind a multi-tile chunk", any(f["n_u"] % 64 for f in multi))
    need("a full last tile behind a multi-tile chunk or n_u == upad", any(f["n_u"] % 64 == 0 for f in flat))
    need("n_u == upad with several tiles", any(f["n_u"] % 64 == 0 and f["tiles_u"] >= 2 for f in flat))
    need("n_u == upad + 1", any(f["n_u"] % 64 == 1 and f["tiles_u"] >= 2 for f in flat))
    need("n_mem % 64 in {0, 1, 63}", {0, 1, 63} <= {f["n_mem"] % 64 for f in flat if f["n_mem"] >= 63})
    need("nf % 32 in {0, 1, 31}", {0, 1, 31} <= {f["nf"] % 32 for f in flat if f["nf"] >= 31})
    need("nf = 1 and n_mem = 1", any(f["nf"] == 1 for f in flat) and any(f["n_mem"] == 1 for f in flat))
    need("n_mem 63, 64, 65, 128, 129", {63, 64, 65, 128, 129} <= {f["n_mem"] for f in flat})
    need("nf 1, 31, 32, 33, 64, 65", {1, 31, 32, 33, 64, 65} <= {f["nf"] for f in flat})
    c2 = [f for f in forms["chunk2_ragged"] if f["side"] == 0 and f["k"] == 0][0]
    need("chunk2_ragged's plan", (c2["tiles_u"], -(-c2["n_mem"] // 64), c2["chunk_tiles"], c2["n_chunks"]) == (47, 47, 2, 24))
    c3 = [f for f in forms["chunk3"] if f["side"] == 0 and f["k"] == 0][0]
    need("chunk3's plan", (c3["tiles_u"], -(-c3["n_mem"] // 64), c3["chunk_tiles"], c3["n_chunks"]) == (79, 63, 3, 27))
    need("chunk3 has at most 24 features", max(f["nf"] for f in forms["chunk3"] if f["side"] == 0) <= 24)
    for K in K_FORMS:
        if K >= 8:
            c = case(f"K{K}")
            need(f"K{K}: bicluster K - 1 active and overlapping bicluster 0",
                 (c["rc"][:, 0] * c["rc"][:, K - 1]).sum() >= 1 and (c["cc"][:, 0] * c["cc"][:, K - 1]).sum() >= 1)
    for cid in SPARSE_OF:
        c = case(cid)
        d, e, ec = c["lines"]
        need(f"{cid}: a dense line, an empty row and column, about 30 % stored",
             np.count_nonzero(c["x"][d]) == c["x"].shape[1] - 1 and not c["x"][e].any() and not c["x"][:, ec].any()
             and 0.25 < np.count_nonzero(c["x"]) / c["x"].size < 0.35)
    assert not missing, f"forms not reached by the case list: {missing}"


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", DATA_CASES + tuple(SPARSE_OF))
def test_reference_silhouettes_are_spread(cid, metric):
    assert_spread(cid, metric)


# ---- mutants: the side's silhouettes restated with switches for the bugs this suite exists to catch ----------------
def _side_with_bug(x, members, features, metric, bug, cache):
    """One side's silhouettes with ``bug`` (None: the definition).  The launch sizes come from ``chunk_plan``; ``cache``
    keeps the side's distance matrices from one bug to the next."""
    K = len(members)
    out = np.zeros((x.shape[0], K))
    act = [l for l in range(K) if len(members[l]) > 0 and len(features[l]) > 0]
    union = np.array(sorted(set().union(*[set(int(p) for p in members[l]) for l in act])), dtype=np.int64)
    pos = {int(p): u for u, p in enumerate(union)}
    memb = np.zeros((union.size, K))
    for l in act:
        memb[[pos[int(p)] for p in members[l]], l] = 1.0
    read = memb.copy()                                   # the bits the contraction reads
    if bug == "top_bit_read_as_the_one_below" and K >= 2:
        read[:, K - 1] = memb[:, K - 2]
    last_tile = 64 * (-(-union.size // 64) - 1)
    applied = False
    for k in act:
        feats = np.asarray(features[k], dtype=np.int64)
        if bug == "ragged_stage_dropped" and feats.size > 32 and feats.size % 32:
            feats = feats[:feats.size // 32 * 32]
            applied = True
        sub = x[np.ix_(union, feats)]
        me = np.array([pos[int(p)] for p in members[k]], dtype=np.int64)
        if (k, feats.size) not in cache:
            cache[k, feats.size] = B.pairwise(sub[me], sub, metric)
            cache[k, feats.size][np.arange(me.size), me] = 0.0
        d = cache[k, feats.size]
        _, chunk_tiles, n_chunks = chunk_plan(union.size, me.size)
        if last_tile > 0 and (bug == "last_tile_of_u_dropped" or           # (the last chunk ends with U's last tile)
                              (bug == "last_tile_of_last_chunk_dropped" and chunk_tiles > 1)):
            d = d.copy()
            d[:, last_tile:] = 0.0
            applied = True
        count = memb.sum(0)[None, :] - (0.0 if bug == "own_bit_left_in_the_count" else memb[me])
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(count > 0, (d @ read) / count, 0.0 if bug == "empty_taken_as_zero" else np.inf)
        applied = applied or bug in ("own_bit_left_in_the_count", "top_bit_read_as_the_one_below") or \
            (bug == "empty_taken_as_zero" and (count[:, act] == 0).any())
        others = [l for l in act if l != k]
        a = mean[:, k]
        b = mean[:, others].min(axis=1) if others else np.full(me.size, np.inf)
        mx = np.maximum(a, b)
        ok = (memb[:, k].sum() > 1) & np.isfinite(a) & np.isfinite(b) & (mx != 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[union[me], k] = np.where(ok, (b - a) / mx, 0.0)
    return out, applied


BUGS = ("last_tile_of_u_dropped", "last_tile_of_last_chunk_dropped", "ragged_stage_dropped",
        "top_bit_read_as_the_one_below", "own_bit_left_in_the_count", "empty_taken_as_zero")
REPRESENTATIVES = {          # family -> (case, the bugs that its launch forms can show)
    "k_forms": ("K16", ("last_tile_of_u_dropped", "top_bit_read_as_the_one_below", "own_bit_left_in_the_count")),
    "edges": ("edges_K12", ("last_tile_of_u_dropped", "ragged_stage_dropped", "top_bit_read_as_the_one_below",
                            "own_bit_left_in_the_count", "empty_taken_as_zero")),
    "chunks": ("chunk2_ragged", ("last_tile_of_u_dropped", "last_tile_of_last_chunk_dropped", "ragged_stage_dropped",
                                 "top_bit_read_as_the_one_below", "own_bit_left_in_the_count")),
    "crafted": ("sole_member_shared", ("own_bit_left_in_the_count", "empty_taken_as_zero")),
    "sparse": ("sparse_edges_K12", ("last_tile_of_u_dropped", "ragged_stage_dropped", "top_bit_read_as_the_one_below",
                                    "own_bit_left_in_the_count", "empty_taken_as_zero")),
}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family", sorted(REPRESENTATIVES))
def test_mutants_clear_the_bars(family, metric):
    """Every bug moves some member's silhouette at least MUTANT_MARGIN x the metric's bar away from the reference, on
    the planted data of the family's representative; the unmutated restatement is the reference to 1e-13."""
    cid, bugs = REPRESENTATIVES[family]
    c = case(cid)
    rows, cols = B.index_sets(c["rc"], c["cc"])
    sides = ((c["x"], rows, cols), (c["x"].T, cols, rows))
    want = reference(cid, metric)
    caches = ({}, {})
    for bug in (None,) + bugs:
        got = [_side_with_bug(x, mem, feat, metric, bug, cache) for (x, mem, feat), cache in zip(sides, caches)]
        dist = max(np.abs(g[0] - w).max() for g, w in zip(got, want))
        if bug is None:
            assert dist <= 1e-13, f"{cid} {metric}: the mutant machinery restates the reference only to {dist:.3e}"
            continue
        print(f"MUTANT {cid} {metric} {bug}: {dist:.3e} ({dist / BARS[metric]:.1e} x the bar)")
        assert any(g[1] for g in got), f"{cid}: '{bug}' changes nothing in this case's forms"
        assert dist >= MUTANT_MARGIN * BARS[metric], \
            f"{cid} {metric}: mutant '{bug}' is only {dist:.3e} from the reference against the bar {BARS[metric]:.1e}"


def test_every_bug_has_a_representative():
    assert {b for _, bugs in REPRESENTATIVES.values() for b in bugs} == set(BUGS)
    assert set(REPRESENTATIVES) == set(FAMILY.values())


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
TWICE = ("chunk2_ragged", "K16")           # the determinism cases: every metric is called a second time


@functools.lru_cache(maxsize=None)
def device(cid):
    """{metric: (row_sil, col_sil)} of a dense case from one handle; "again" the second calls of the TWICE cases."""
    c = case(cid)
    n, m = c["x"].shape
    out = {"again": {}}
    with Engine([n], [m], [2]) as e:
        e.set_view(0, c["x"])
        assert np.array_equal(e.get_view(0), c["x"])          # the device scores the image the references were fed
        for metric in METRICS:
            out[metric] = e.bisil(0, c["rc"], c["cc"], metric)
            if cid in TWICE:
                out["again"][metric] = e.bisil(0, c["rc"], c["cc"], metric)
    return out


@functools.lru_cache(maxsize=None)
def device_sparse(cid):
    """{metric: (row_sil, col_sil)} through resnmtf_bisil_sparse, "dense": the same through resnmtf_bisil on a dense
    handle with the same fp32 values."""
    c = case(cid)
    n, m = c["x"].shape
    xs = sp.csc_matrix(c["x"])
    out = {"dense": {}}
    with Engine([n], [m], [2], nnz=[xs.nnz]) as es, Engine([n], [m], [2]) as ed:
        es.set_view_sparse(0, xs, pre_processed=True)
        ed.set_view(0, c["x"])
        assert np.array_equal(ed.get_view(0), c["x"])
        assert np.array_equal(es.get_view_sparse(0).toarray(), c["x"])
        for metric in METRICS:
            out[metric] = es.bisil_sparse(0, c["rc"], c["cc"], metric)
            out["dense"][metric] = ed.bisil(0, c["rc"], c["cc"], metric)
    return out


def _check_against_reference(cid, metric, got):
    c = case(cid)
    worst = []
    for side, g, w, mem in zip(("rows", "cols"), got, reference(cid, metric), (c["rc"], c["cc"])):
        assert np.isfinite(g).all()
        assert (g[mem == 0] == 0).all()
        worst.append(float(np.abs(g - w).max()))
        print(f"MEASURED {cid} {metric} {side}: {worst[-1]:.3e}")
    assert max(worst) <= BARS[metric], f"{cid} {metric}: |device - reference| = {max(worst):.3e} above {BARS[metric]:.1e}"


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", DENSE_CASES)
def test_every_member_matches_the_reference(cid, metric):
    if cid not in CRAFTED:
        assert_spread(cid, metric)
    _check_against_reference(cid, metric, device(cid)[metric])


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", tuple(SPARSE_OF))
def test_sparse_route(cid, metric):
    assert_spread(cid, metric)
    d = device_sparse(cid)
    assert np.array_equal(d[metric][0], d["dense"][metric][0])
    assert np.array_equal(d[metric][1], d["dense"][metric][1])
    _check_against_reference(cid, metric, d[metric])
    _check_against_reference(cid, metric, d["dense"][metric])


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cid", TWICE)
def test_two_calls_are_bitwise_equal(cid, metric):
    d = device(cid)
    assert d[metric][0].any() and d[metric][1].any()
    assert np.array_equal(d[metric][0], d["again"][metric][0])
    assert np.array_equal(d[metric][1], d["again"][metric][1])


# ---- the crafted cases: each rule on the device's own output --------------------------------------------------------
def _mean_dist(x, i, others, feats, metric):
    return float(np.mean([B.dist(x[i, feats], x[j, feats], metric) for j in others]))


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_rule_sole_member_shared(metric):
    """c = cnt[l] - own bit: bicluster 1 = {row 3} is skipped for row 3 (a member of bicluster 0) and counts, as the
    nearest, for bicluster 0's other rows; a singleton scores 0; biclusters with one empty side score 0 and are no l."""
    c = case("sole_member_shared")
    x, bar = c["x"], BARS[metric]
    rs, cs = device("sole_member_shared")[metric]
    j0, i0, i2 = list(range(12)), list(range(10)), list(range(20, 30))
    assert rs[3, 1] == 0.0                                                   # |I_1| = 1
    a = _mean_dist(x, 3, [i for i in i0 if i != 3], j0, metric)
    b = _mean_dist(x, 3, i2, j0, metric)                                     # bicluster 1 is skipped: only 2 is left
    assert abs(rs[3, 0] - (b - a) / max(a, b)) <= bar
    for i in (0, 9):
        a = _mean_dist(x, i, [p for p in i0 if p != i], j0, metric)
        b1, b2 = _mean_dist(x, i, [3], j0, metric), _mean_dist(x, i, i2, j0, metric)
        assert b1 < b2                                                       # the one-row bicluster is the nearest
        assert abs(rs[i, 0] - (b1 - a) / max(a, b1)) <= bar
        assert abs(rs[i, 0] - (b2 - a) / max(a, b2)) > 1e3 * bar             # (and taking bicluster 2 would show)
    assert not rs[:, 3:].any() and not cs[:, 3:].any() and not rs[30:35].any() and not cs[26:28].any()
    assert rs[:, 0].any() and rs[:, 2].any() and cs[:, 0].any() and cs[:, 2].any()
    assert cs[:, 1].any() or metric == "cosine"          # (one feature, row 3: every cosine distance is 0, s = 0)


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_rule_two_active_other_is_sole(metric):
    """Row 3 of bicluster 0 is all of bicluster 1, the only other active one: no l is left for it, s = 0 exactly; the
    other rows of bicluster 0 take b from row 3 alone."""
    c = case("two_active_other_is_sole")
    x, bar = c["x"], BARS[metric]
    rs, cs = device("two_active_other_is_sole")[metric]
    assert rs[3, 0] == 0.0 and rs[3, 1] == 0.0
    j0, i0 = list(range(12)), list(range(10))
    for i in (0, 4, 9):
        a = _mean_dist(x, i, [p for p in i0 if p != i], j0, metric)
        b = _mean_dist(x, i, [3], j0, metric)
        assert rs[i, 0] != 0.0 and abs(rs[i, 0] - (b - a) / max(a, b)) <= bar
    assert not rs[:, 2:].any() and not cs[:, 2:].any() and not rs[30:35].any() and not cs[26:28].any()
    assert cs[:12, 0].all() and (cs[5:17, 1].all() or metric == "cosine")    # (cosine on the one feature row 3: all 0)


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_rule_identical_sets(metric):
    """Biclusters 1 and 2 hold the same rows: for those rows the other one's mean is their own a, bit for bit (the
    same distances in the same order), and it is the minimum: s = 0 exactly.  For bicluster 0's rows the two tie."""
    c = case("identical_sets")
    x, bar = c["x"], BARS[metric]
    rs, _ = device("identical_sets")[metric]
    for k, feats in ((1, list(range(10))), (2, list(range(10, 20)))):
        for i in range(5, 15):
            a = _mean_dist(x, i, [p for p in range(5, 15) if p != i], feats, metric)
            assert a < _mean_dist(x, i, range(20, 30), feats, metric)        # the twin is the nearest
            assert rs[i, k] == 0.0
    j0 = list(range(20, 30))
    for i in (20, 29):
        a = _mean_dist(x, i, [p for p in range(20, 30) if p != i], j0, metric)
        b = _mean_dist(x, i, range(5, 15), j0, metric)
        assert rs[i, 0] != 0.0 and abs(rs[i, 0] - (b - a) / max(a, b)) <= bar


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_rule_identical_members(metric):
    """Every row of U is one vector on bicluster 0's columns: a = b = 0, max(a, b) = 0, s = 0 and not NaN."""
    rs, cs = device("identical_members")[metric]
    assert np.isfinite(rs).all() and np.isfinite(cs).all()
    assert (rs[:, 0] == 0.0).all()
    assert rs[10:18, 1].all() and cs[:20].any(axis=1).all()                  # (the rest of the call is not degenerate)


@gpu
def test_rule_cosine_zero_rows():
    """Cosine with zero norms: rows 0, 1 (zero on bicluster 0's columns only) and 2 (zero everywhere) are at distance 0
    from each other and 1 from every other row: a = 3 / 5, b = 1, s = 2 / 5; a non-zero row has three neighbours at 1."""
    c = case("cosine_zero_rows")
    x = c["x"]
    assert x[0, 10:].all() and x[1, 10:].all() and not x[2].any() and not x[:2, :10].any()
    rs, _ = device("cosine_zero_rows")["cosine"]
    for i in (0, 1, 2):
        assert abs(rs[i, 0] - 0.4) <= 1e-15
    j0 = list(range(10))
    a = (3.0 + B.dist(x[3, j0], x[4, j0], "cosine") + B.dist(x[3, j0], x[5, j0], "cosine")) / 5.0
    b = _mean_dist(x, 3, range(10, 18), j0, "cosine")
    assert abs(rs[3, 0] - (b - a) / max(a, b)) <= BARS["cosine"]
