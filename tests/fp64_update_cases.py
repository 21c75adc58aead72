"""The cases of the fp64 paths' entry-by-entry update tests, their bars and their mutants (host only: NumPy and the
oracle; ``tests/test_fp64_update_cases_host.py`` runs all of it without a GPU, ``tests/test_gpu_fp64_update_forms.py``
runs the cases on the device through every route of ``engine.fp64_run`` and through ``engine.group_run``).

The f32 engine has this coverage in ``tests/update_cases.py``; its problems, its statement of the coupling rule
(``expected_plan`` / ``coupled_views``), its one-sweep reference (``oracle_sweep`` from ``initial_state``) and its mutants
are used here as they stand.  What differs for the fp64 paths: one k per job, at most 8 views, and the shape constants
of ``csrc/resnmtf_fp64_job.h`` (``CONSTANTS``, read from the header) in place of the f32 row groups.  Every 8-view
problem is built on ``SHAPES8``: extents distinct per view, none a multiple of the 32-row leading-dimension rounding (a
wrong map offset or a wrong ``nw`` cannot cancel), every row count above the 128-row product tile and ending inside a
64-row update workgroup, one view above the 256-row Gram workgroup, every column count between 65 and 127.

The bars
--------
All data, factors and weights are non-negative: every compared entry is a quotient of sums of non-negative products and
nothing cancels.  With u = 2^-53, a sum of N such terms in ANY order is within (N - 1) u of the exact one, a product or
a quotient adds the errors of its operands plus u, and a sum is no worse than its worst term plus u per addition.  Per
side (the device and the oracle, each in its own order), for a view of n x m at k among V views:

    F   p (num + np) / (den + rsum p + lambda / 2)
          num = (X G) S^T: m + k;  np = sum_w r_w F_w n_w / n: V + 2;  the sum: + 1          max(m + k, V + 2) + 1
          den = (F S)((G^T G) S^T): k + (m + k) + k;  rsum p: V;  two additions              max(m + 3 k, V) + 2
          the quotient and the product                                                        + 2
    G   the same with n for m (the contraction runs over the rows)
    S   s (num + acc) / (den + xsum s)
          num = (F^T X) G: n + m;  acc = sum_w xi_w S_w: V + 1;  the sum                      max(n + m, V + 1) + 1
          den = ((F^T F) S)(G^T G): n + k + m + k;  xsum s: V;  one addition, one for den     max(n + m + 2 k, V) + 2
          the quotient and the product                                                        + 2
    lambda, mu   a column sum of n (m) terms and one product                                 n + 1, m + 1

``local_counts`` returns these; twice a count (both sides) times u is the LOCAL bar of a quantity -- the bound on
``|got / ref - 1|`` when the step reads the same inputs on both sides.  The reference is ONE oracle sweep from the
device's start, so within the sweep a step reads quantities the two sides have already computed apart: F_v enters G_v's
numerator once and its denominator twice (F^T F), F_v and G_v enter S_v the same way, lambda and mu read the new F and G,
and the coupled sums read this sweep's factors of the earlier views (a weighted mean of them: at most the worst).
``case_bars`` adds these at their local bars, with those multiplicities:

    bar F_v      = local F_v + max over coupled w < v of local F_w
    bar G_v      = local G_v + max(local F_v, max over coupled w < v of local G_w) + 2 local F_v
    bar S_v      = local S_v + max(local F_v + local G_v, max over xi-coupled w < v of local S_w) + 2 local F_v + 2 local G_v
    bar lambda_v = 2 (n + 1) u + local F_v          bar mu_v = 2 (m + 1) u + local G_v

The chain is cut after this one level: the inputs are taken at their local bars, not at their full ones.  Carried to
the end the recursion multiplies the count by about twelve from F_v to S_v and again from view to view; it passes
1e-11, the bar of whole trajectories, at V = 8, and is no test of one sweep.  What the cut leaves out enters through the
same weights (quotients of non-negative sums, each at most 1) and is as far below the first level as the measured
errors are below the counts: ``test_fp64_update_cases_host.py`` runs the same sweep in ``np.longdouble`` and requires
the fp64 oracle -- whose roundings go through the whole chain -- to stay within a quarter of every bar (it stays within
a hundredth), and the measured device values are recorded in ``tests/test_gpu_fp64_update_forms.py``.

``group_run`` returns normalised factors (``normalisation_check``): F / cF adds a column sum of n terms and a quotient
per side and reads the new F again, S cF cG the two sums and two products (``norm_bars``).

Every bar must come out below ``BAR_LIMIT`` = 1e-12, a tenth of the trajectory bar; the host test asserts it.

The mutants
-----------
``update_cases.update_mutants`` (a slot dropped, a view read twice, a map shifted by a row, the wrong ``n_other``, last
sweep's factor, sigma w missing, an xi term dropped) and two that the fp64 layout invites (``layout_mutants``): the map
of (w, v) used for (v, w), and view w read through the map of the next pair.  Each is the oracle called on altered
names, so the reference of a bug is computed by the code that computes the true one.
"""
from __future__ import annotations

import os
import re

import numpy as np

import update_cases as U
from helpers import ROOT, coupled_problem
from oracle import resnmtf_oracle as O

U53 = 2.0 ** -53
BAR_LIMIT = 1e-12
KEYS = ("f", "s", "g", "lam", "mu")                # the order of a state tuple (update_cases.initial_state)
PADDED = {8: 16, 20: 32, 40: 48, 64: 64}           # one k per padded class


def _constants():
    """The shape constants of the fp64 kernels, from csrc/resnmtf_fp64_job.h itself."""
    text = open(os.path.join(ROOT, "resnmtf_amd", "csrc", "resnmtf_fp64_job.h")).read()
    out = {name: int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1))
           for name in ("F64_ROWS", "F64_UPD_ROWS", "F64_RES_ROWS", "F64_GRAM_ROWS", "F64_JC")}
    out["LD"] = int(re.search(r"ld = \(rows \+ (\d+)\) / (\d+) \* \2;", text).group(2))       # f64_ld's rounding
    return out


CONSTANTS = _constants()

# rows: above the product tile (two tiles), 3 to 5 update workgroups with a ragged last one, view 2 above the Gram
# workgroup; columns: 65 .. 127 (two LDS stages, one product tile on the G side); all distinct, none a multiple of 32
SHAPES8 = [(131, 67), (139, 71), (261, 69), (150, 75), (157, 79), (163, 83), (171, 87), (178, 91)]
IDENTITY_SHAPE = (261, 71)


# ---------------------------------------------------------------------------------------------------------------------
# problems (those of update_cases where they fit)
# ---------------------------------------------------------------------------------------------------------------------
def bucket8_problem(k, seed, **kw):
    """``update_cases.bucket_problem`` on SHAPES8: eight views, every pair coupled through phi, psi and xi but (0, 7)."""
    return coupled_problem(SHAPES8, k, seed, phi_w=1.5, psi_w=1.0, xi_w=0.4, **kw)


def bucket(n_v, k, seed):
    return bucket8_problem(k, seed) if n_v == 8 else U.bucket_problem(n_v, k, seed)


def thinned(prob, views, seed):
    """The views ``views`` of ``prob`` thinned to a density of about 0.2, as ``update_cases.sparse_problem`` thins them."""
    from test_gpu_sparse import sparsify
    for v in views:
        prob.data[v] = sparsify(prob.data[v], 0.2, seed + v)
    return prob


def identity8_problem(k, seed):
    """The eight-view twin of ``update_cases.identity_problem``: one shape, the pool's first names in pool order."""
    return coupled_problem([IDENTITY_SHAPE] * 8, k, seed, phi_w=1.5, psi_w=1.0, xi_w=0.4, same_order_views=range(8), overlap=1.0)


NA_ZERO_PAIRS = [(1, 2)] + [(6, w) for w in (0, 1, 4, 5, 7)]


def na_zero_problem(k, seed):
    """Eight views; view 4 has row names of its own (NA towards every view, its weights kept), the pairs NA_ZERO_PAIRS
    have weight zero in phi, psi and xi: the G side couples 5, 5, 6, 7, 6, 6, 2, 5 views, the F side 4, 4, 5, 6, 0, 5, 2, 4."""
    prob = bucket8_problem(k, seed, na_pairs=((0, 4),))
    for a, b in NA_ZERO_PAIRS:
        for mat in (prob.phi, prob.psi, prob.xi):
            mat[a, b] = mat[b, a] = 0.0
    return prob


def isolated_problem(k, seed):
    """Five views of one k, 0 and 1 coupled, 2 .. 4 with zero rows and columns in phi, psi and xi: their F goes
    unrestricted, their G and S through the coupled formula with sigma = 0 and no coupled view."""
    return U.mixed_k_problem([k] * 5, seed, coupled_01=True)


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
SOURCES = ("host dense", "scipy.sparse", "torch dense", "torch sparse")        # F64Source, in the order of the header
DENSE_ROUTES = ("host_dense", "torch_dense", "group")
SPARSE_ROUTES = ("scipy_sparse", "torch_sparse")


class Case:
    def __init__(self, cid, make, before=0, sparse=(), routes=DENSE_ROUTES, nan_view=None, sources=None):
        self.id, self.make, self.before, self.sparse, self.routes, self.nan_view = cid, make, before, tuple(sparse), routes, nan_view
        self.sources = sources          # the mixed-source case: per view an index into SOURCES

    def used_sources(self):
        if self.sources is not None:
            return {SOURCES[s] for s in self.sources}
        return {"host dense", "torch dense"} if not self.sparse else {"scipy.sparse", "torch sparse"}


MIXED_SOURCES = [v % 4 for v in range(8)]


def _cases():
    C = []
    ten_before = {(8, 8), (20, 6), (40, 7), (64, 5)}            # one per padded class also runs after ten sweeps
    for k in PADDED:
        for n_v in (5, 6, 7, 8):
            C.append(Case(f"k{k}_v{n_v}", lambda k=k, n_v=n_v: bucket(n_v, k, 100 * n_v + k)))
            if (k, n_v) in ten_before:
                C.append(Case(f"k{k}_v{n_v}_after10", lambda k=k, n_v=n_v: bucket(n_v, k, 100 * n_v + k), before=10))
    C.append(Case("identity_k8_v8", lambda: identity8_problem(8, 800)))
    C.append(Case("mixed_maps_k8_v6", lambda: U.mixed_maps_problem(8, 810)))
    C.append(Case("na_zero_k8_v8", lambda: na_zero_problem(8, 815)))
    C.append(Case("isolated_k8_v5", lambda: isolated_problem(8, 870)))
    C.append(Case("edge_psi_elsewhere_nan", lambda: U.psi_edge_problem(820), nan_view=2))
    C.append(Case("edge_all_pairs_na", lambda: U.na_edge_problem(830)))
    C.append(Case("edge_xi_only", lambda: U.xi_edge_problem(840)))
    for k in PADDED:
        C.append(Case(f"sparse_k{k}_v6", lambda k=k: U.sparse_problem(6, k, 700 + k), sparse=range(6), routes=SPARSE_ROUTES))
        C.append(Case(f"sparse_k{k}_v8", lambda k=k: thinned(bucket8_problem(k, 900 + k), range(8), 900 + k), sparse=range(8),
                      routes=SPARSE_ROUTES))
    sparse_views = [v for v in range(8) if MIXED_SOURCES[v] in (1, 3)]
    C.append(Case("mixed_sources_k20_v8", lambda: thinned(bucket8_problem(20, 950), sparse_views, 950), sparse=sparse_views,
                  routes=("mixed",), sources=MIXED_SOURCES))
    return C


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
ROUTE_PARAMS = [(c.id, r) for c in CASES for r in c.routes]


def case(cid) -> Case:
    return CASES[CASE_IDS.index(cid)]


def in_grouped_limits(prob, limits) -> bool:
    """Whether ``group_run`` takes the problem, asked of the limits themselves (``batched.GROUPED_LIMITS``)."""
    k = U.ks_of(prob)[0]
    return (len(prob.data) <= limits.max_views and 1 <= k <= limits.max_k
            and all(x.shape[0] * x.shape[1] <= limits.max_view_entries for x in prob.data))


# ---------------------------------------------------------------------------------------------------------------------
# the reference: one oracle sweep, in fp64 or in long double
# ---------------------------------------------------------------------------------------------------------------------
def oracle_sweep_as(prob, x, before, dtype):
    """``update_cases.oracle_sweep`` with every input cast to ``dtype`` (the oracle's arithmetic follows its inputs)."""
    cast = lambda a: np.asarray(a, dtype=dtype)                      # noqa: E731
    sh_r, sh_c = U.shared(prob)
    f, s, g, lam, mu = O.update_matrices([cast(d) for d in x], *([cast(b[i]) for b in before] for i in range(5)), cast(prob.phi),
                                         cast(prob.xi), cast(prob.psi), sh_r, sh_c, prob.row_names, prob.col_names)
    return [(f[v], s[v], g[v], lam[v], mu[v]) for v in range(len(x))]


def sweep_error(x, after):
    """The sweep's mean error (calculate_error, R/utils.r:157-166) of the state ``after``."""
    norms = np.array([np.linalg.norm(d, "fro") ** 2 for d in x])
    return float(np.mean(O.calculate_error(x, [a[0] for a in after], [a[1] for a in after], [a[2] for a in after], norms)))


# ---------------------------------------------------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------------------------------------------------
def local_counts(n: int, m: int, k: int, n_v: int) -> dict:
    """Roundings per side along the worst path of one entry of each quantity (the table of the module docstring)."""
    return {"f": max(m + k, n_v + 2) + 1 + max(m + 3 * k, n_v) + 2 + 2,
            "g": max(n + k, n_v + 2) + 1 + max(n + 3 * k, n_v) + 2 + 2,
            "s": max(n + m, n_v + 1) + 1 + max(n + m + 2 * k, n_v) + 2 + 2,
            "lam": n + 1, "mu": m + 1}


def case_bars(prob) -> list:
    """Per view ``{quantity: bar}`` on ``max |got / ref - 1|`` of the raw state after one sweep (module docstring)."""
    n_v, k = len(prob.data), U.ks_of(prob)[0]
    sh = U.shared(prob)
    loc = [{q: 2 * c * U53 for q, c in local_counts(*prob.data[v].shape, k, n_v).items()} for v in range(n_v)]
    out = []
    for v in range(n_v):
        earlier = []
        for side, coup in ((0, prob.phi), (1, prob.psi)):
            _, cl = U.coupled_views(coup, sh[side][v], v, whole_matrix=side == 1)
            earlier.append(max([loc[w]["fg"[side]] for w in cl if w < v], default=0.0))
        s_earlier = max([loc[w]["s"] for w in range(v) if np.sum(prob.xi) != 0 and prob.xi[w, v] != 0], default=0.0)
        lf, lg = loc[v]["f"], loc[v]["g"]
        out.append({"f": lf + earlier[0],
                    "g": lg + max(lf, earlier[1]) + 2 * lf,
                    "s": loc[v]["s"] + max(lf + lg, s_earlier) + 2 * lf + 2 * lg,
                    "lam": loc[v]["lam"] + lf, "mu": loc[v]["mu"] + lg})
    return out


def norm_bars(prob) -> list:
    """The bars of ``group_run``'s outputs: F, G and S normalised (a column sum and a quotient, or two sums and two
    products, per side, reading the new factors once more), lambda and mu raw."""
    n_v, k = len(prob.data), U.ks_of(prob)[0]
    out = []
    for v, b in enumerate(case_bars(prob)):
        n, m = prob.data[v].shape
        loc = {q: 2 * c * U53 for q, c in local_counts(n, m, k, n_v).items()}
        out.append({"f": b["f"] + 2 * n * U53 + loc["f"], "g": b["g"] + 2 * m * U53 + loc["g"],
                    "s": b["s"] + 2 * (n + m) * U53 + loc["f"] + loc["g"], "lam": b["lam"], "mu": b["mu"]})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the mutants the fp64 layout invites
# ---------------------------------------------------------------------------------------------------------------------
def _pairs(names_v, names_w, shared_vw):
    """[(row of v, row of w)] of the names views v and w share: the device's map of (v, w), entry by entry."""
    if shared_vw is None:
        return []
    return list(zip(O._positions(names_v, shared_vw).tolist(), O._positions(names_w, shared_vw).tolist()))


def _read_through(names, sh_v, v, w, reads):
    """(names, shared names of v) under which the oracle reads row b of view w for row a of view v, for (a, b) in
    ``reads``: view w is renamed -- row b gets the name of v's row a, every other row a name nobody has."""
    fake = [f"nobody{w}_{t}" for t in range(len(names[w]))]
    for a, b in reads:
        fake[b] = names[v][a]
    out = list(names); out[w] = fake
    return out, {**sh_v, w: [names[v][a] for a, _ in reads]}


def layout_mutants(x, before, after, prob, v) -> dict:
    """``{name: statistic}`` of the two bugs of ``fp64_layout``'s map offsets, in the manner of
    ``update_cases.update_mutants``: (1) the map of (w, v) used for (v, w) -- row b of v reads row a of w where the true
    map sends a to b; (2) view w's map read at the offset of the next pair -- view w read through the map of (v, w'), w'
    the next coupled view.  Rows the wrong map sends beyond view w are left unmatched (they keep the view's own row).
    A mutant whose map sends every row where the true one does computes the true step and is not a bug: none is emitted
    for it (the identity case, where all maps coincide, has none)."""
    sh = U.shared(prob)
    F0, S0, G0, lam0, mu0 = before[v]
    F1 = after[v][0]
    out = {}
    for side, tag, coup, names in ((0, "F", prob.phi, prob.row_names), (1, "G", prob.psi, prob.col_names)):
        i = 0 if side == 0 else 2
        ws = [a[i] for a in after[:v]] + [b[i] for b in before[v:]]

        def step(names_, sh_, side=side, ws=ws, coup=coup):
            if side == 0:
                return O.update_f(x[v], ws, S0, G0, lam0, coup, v, sh_, names_[v], names_)
            return O.update_g(x[v], F1, S0, ws, mu0, coup, v, sh_, names_[v], names_)
        restricted, cl = U.coupled_views(coup, sh[side][v], v, whole_matrix=side == 1)
        if not restricted or not cl:
            continue
        true = step(names, sh[side][v])
        len_v = len(names[v])
        for pos, w in enumerate(cl):
            true_map = _pairs(names[v], names[w], sh[side][v][w])
            len_w = len(names[w])
            swapped = [(b, a) for a, b in true_map if b < len_v and a < len_w]
            if sorted(swapped) != sorted(true_map):
                out[f"{tag}: the map of ({w}, {v}) used for ({v}, {w})"] = U._stat(step(*_read_through(names, sh[side][v], v, w, swapped)), true)
            nxt = cl[(pos + 1) % len(cl)]
            if nxt != w:
                other = [(a, b) for a, b in _pairs(names[v], names[nxt], sh[side][v][nxt]) if b < len_w]
                if sorted(other) != sorted(true_map):
                    out[f"{tag}: view {w} read through the map of ({v}, {nxt})"] = U._stat(step(*_read_through(names, sh[side][v], v, w, other)), true)
    return out


def all_mutants(x, before, after, prob, v) -> dict:
    return {**U.update_mutants(x, before, after, prob, v), **layout_mutants(x, before, after, prob, v)}


def covered(cases=None) -> set:
    """What the case table reaches, from ``expected_plan`` / ``coupled_views`` alone (tags; the host test lists the
    ones it demands, the GPU test counts only the cases that passed)."""
    out = set()
    for c in (CASES if cases is None else cases):
        prob = c.make()
        n_v, k = len(prob.data), U.ks_of(prob)[0]
        out |= {("V", n_v), ("kp", 16 * ((k + 15) // 16))} | {("source", s) for s in c.used_sources()}
        sh = U.shared(prob)
        for v, p in enumerate(U.expected_plan(prob)):
            for s in (0, 1):
                if p["restricted"][s]:
                    out.add(("n_couple", "FG"[s], p["n_couple"][s]))
                    if p["n_couple"][s]:
                        out.add(("maps", "identity" if not p["n_index_maps"][s] else "index" if not p["n_identity_maps"][s] else "mixed"))
                    coup = (prob.phi, prob.psi)[s]
                    if any(coup[w, v] != 0 and sh[s][v][w] is None for w in range(n_v) if w != v):
                        out.add(("NA pair inside a restricted view", "FG"[s]))
                    if p["n_couple"][s] and any(coup[w, v] == 0 for w in range(n_v) if w != v):
                        out.add(("zero weight inside a restricted view", "FG"[s]))
            out.add(("s_n_couple", p["s_n_couple"]))
            if not p["restricted"][0] and p["restricted"][1]:
                out.add(("unrestricted F beside a restricted G",))
                if p["sigma_is_zero"][1] and not p["n_couple"][1]:
                    out.add(("restricted G with sigma = 0 and no coupled view",))
    return out


DEMANDED = ({("V", n) for n in (5, 6, 7, 8)} | {("kp", kp) for kp in (16, 32, 48, 64)} | {("source", s) for s in SOURCES}
            | {("n_couple", side, n) for side in "FG" for n in range(8)} | {("s_n_couple", n) for n in range(8)}
            | {("maps", kind) for kind in ("identity", "index", "mixed")}
            | {("NA pair inside a restricted view", "F"), ("zero weight inside a restricted view", "F"),
               ("zero weight inside a restricted view", "G"), ("unrestricted F beside a restricted G",),
               ("restricted G with sigma = 0 and no coupled view",)})
