"""The cases of the update-side elementwise tests, their expected coupling tables and their mutants (host only: NumPy and
the oracle; ``tests/test_update_forms_host.py`` runs all of it without a GPU, ``tests/test_gpu_update_forms.py`` runs the
cases on the device).

``factor_update_kernel<KP, IS_G, NCB, EMIT>`` exists in 4 x 2 x 4 x 2 forms (KP 16 / 32 / 48 / 64, the F or the G side,
coupling-count bucket 0 / 4 / 8 / 16, with or without its own fp64 Gram partials) and each form switches at run time
between three slab-prefetch depths (4 / 8 / 16).  A case is a problem plus engine options chosen so that its views land
in given forms; ``expected_plan`` restates ``fill_update``'s rule on the host (weight != 0, not the view itself, pair not
NA) and says which coupling counts each view and side must get, and ``update_mutants`` builds, from oracle calls only,
the references of the bugs per-slot register indexing invites (a slot dropped, read twice, read from the wrong view).
"""
from __future__ import annotations

import numpy as np

from data_ref import nan_stat
from helpers import coupled_problem
from oracle import resnmtf_oracle as O
from resnmtf_amd import naming, synth

UPDATE_BLOCKS = 3           # workgroups per update launch: several, with a ragged last one
ROWS_PER_GROUP = {16: 32, 32: 16, 48: 21, 64: 16}      # update_threads(KP) / KP


def kp_of(k: int) -> int:
    return 16 * ((k + 15) // 16)


def ks_of(prob):
    return [int(f.shape[1]) for f in prob.init_f]


def sizes(start: int, step: int, count: int):
    """``count`` distinct extents from ``start`` on, none a multiple of a row group (16, 32 or 21 rows): the last
    update workgroup of every view then ends inside a row group."""
    out, x = [], start
    while len(out) < count:
        if x % 16 and x % 21:
            out.append(x)
        x += step
    return out


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def bucket_problem(n_v, k, seed, **kw):
    """n_v views of about 150 x 90 with distinct extents, names shared in part at different positions, every pair
    coupled through phi, psi and xi but (0, n_v - 1): the views get n_v - 1 or n_v - 2 coupled terms."""
    w = 0.3 if n_v >= 17 else 1.0           # (many views: weights scaled down so that the iteration stays tame)
    shapes = list(zip(sizes(150, 7, n_v), sizes(90, 3, n_v)))
    return coupled_problem(shapes, k, seed, phi_w=1.5 * w, psi_w=1.0 * w, xi_w=0.4 * w, **kw)


def sparse_problem(n_v, k, seed, dense_views=()):
    """bucket_problem with every view but ``dense_views`` thinned to a density of about 0.2 (columns re-normalised)."""
    from test_gpu_sparse import sparsify
    prob = bucket_problem(n_v, k, seed)
    for v in range(n_v):
        if v not in dense_views:
            prob.data[v] = sparsify(prob.data[v], 0.2, seed + v)
    return prob


def identity_problem(k, seed):
    """Nine views of one shape whose names are the pool's first, in pool order: every map is the identity."""
    return coupled_problem([(150, 93)] * 9, k, seed, phi_w=1.5, psi_w=1.0, xi_w=0.4, same_order_views=range(9), overlap=1.0)


def mixed_maps_problem(k, seed):
    """Six views; 0, 1 and 2 have one shape and the pool's first names in pool order (identity maps among them), the
    others distinct extents and permuted names (index maps)."""
    shapes = [(150, 93)] * 3 + list(zip(sizes(157, 7, 3), sizes(99, 3, 3)))
    return coupled_problem(shapes, k, seed, phi_w=1.5, psi_w=1.0, xi_w=0.4, same_order_views=(0, 1, 2))


def slab_problem(k, seed):
    """Two coupled views whose contraction extents all pad to 1024: 16 splits of 64 rows exist."""
    return coupled_problem([(1010, 1000), (1001, 1015)], k, seed, phi_w=1.5, psi_w=1.0, xi_w=0.4)


def psi_edge_problem(seed):
    """Three views, psi between 0 and 1 only.  update_g branches on the WHOLE matrix, so view 2 takes the coupled formula
    with no coupled view and sigma = 0 -- the form without the NaN -> 1 guard.  Column 5 of X_2 is zero, row 5 of G_2
    starts at zero and mu_2 is zero: numerator and denominator of that row are 0 and the row becomes NaN."""
    prob = coupled_problem(list(zip(sizes(150, 7, 3), sizes(90, 3, 3))), 8, seed, psi_w=1.0)
    prob.psi[2, :] = 0.0; prob.psi[:, 2] = 0.0
    x = prob.data[2].copy()
    x[:, 5] = 0.0
    with np.errstate(invalid="ignore"):
        x = x / x.sum(axis=0)[None, :]
    x[:, 5] = 0.0
    prob.data[2] = x
    prob.init_g[2][5, :] = 0.0
    prob.init_mu = {2: np.zeros(8)}
    return prob


def na_edge_problem(seed):
    """Two views, phi weight, disjoint row names: the numerator is empty and sigma w stays in the denominator."""
    return coupled_problem(list(zip(sizes(150, 7, 2), sizes(90, 3, 2))), 8, seed, phi_w=1.5, na_pairs=((0, 1),))


def xi_edge_problem(seed):
    """Two views coupled through xi only: F and G stay unrestricted while S takes the coupled formula."""
    return coupled_problem(list(zip(sizes(150, 7, 2), sizes(90, 3, 2))), 8, seed, xi_w=0.4)


def mixed_k_problem(ks, seed, coupled_01=False):
    """Views of different k on one handle: uncoupled, or views 0 and 1 (equal k) coupled through phi / psi / xi with
    zero weights to the rest."""
    n_v = len(ks)
    w = dict(phi_w=1.5, psi_w=1.0, xi_w=0.4) if coupled_01 else {}
    prob = coupled_problem(list(zip(sizes(150, 7, n_v), sizes(90, 3, n_v))), ks[0], seed, **w)
    for v in range(n_v):
        n, m = prob.data[v].shape
        prob.init_f[v], prob.init_s[v], prob.init_g[v] = synth.random_init(n, m, ks[v], seed * 100 + 70 + v)
        if coupled_01 and v >= 2:
            for mat in (prob.phi, prob.psi, prob.xi):
                mat[v, :] = 0.0; mat[:, v] = 0.0
    return prob


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cid, make, opts=None, before=0, sparse=None, want=None, slab=False, nan_view=None):
        self.id, self.make, self.before, self.sparse, self.slab, self.nan_view = cid, make, before, sparse, slab, nan_view
        self.opts = dict(update_blocks=UPDATE_BLOCKS, **(opts or {}))
        self.want = dict(want or {})      # what the case is there for: {"n_couple": {...}, "s_n_couple": {...}, "maps": {...}}

    def sparse_flags(self, n_v):
        return [False] * n_v if self.sparse is None else [v in self.sparse for v in range(n_v)]

    def form(self, v, k):
        """The pass form whose bar the view is judged by (tests/test_gpu_sweep_elementwise.py BARS): the update is fp64,
        its error is that of the f32 slabs it sums."""
        if self.sparse is not None and v in self.sparse:
            return "sparse"
        return "f32" if k <= 16 else "wide"


WANT_BY_VIEWS = {5: {3, 4}, 6: {4, 5}, 9: {7, 8}, 10: {8, 9}, 17: {15, 16}}      # n_v - 2 (views 0 and n_v - 1) and n_v - 1


def _cases():
    C = []
    ten_before = {(8, 6), (20, 9), (40, 10), (64, 5)}          # one case per KP runs ten sweeps first
    for k in (8, 20, 40, 64):
        for n_v in (5, 6, 9, 10, 17):
            C.append(Case(f"k{k}_v{n_v}", lambda k=k, n_v=n_v: bucket_problem(n_v, k, 100 * n_v + k),
                          before=10 if (k, n_v) in ten_before else 0,
                          want={"n_couple": WANT_BY_VIEWS[n_v], "s_n_couple": WANT_BY_VIEWS[n_v], "maps": {"index"}}))
        for n_v in (6, 10):                                      # the other hand-off mode
            C.append(Case(f"k{k}_v{n_v}_flipped", lambda k=k, n_v=n_v: bucket_problem(n_v, k, 100 * n_v + k + 1),
                          {"kk_mode": 2 if k <= 16 else 1}, want={"n_couple": WANT_BY_VIEWS[n_v], "emit": {0 if k <= 16 else 1}}))
    for k in (20, 40, 64):                                       # sparse, coupled, k > 16: EMIT at KP 32 / 48 / 64
        C.append(Case(f"sparse_k{k}_v6", lambda k=k: sparse_problem(6, k, 700 + k), sparse=range(6),
                      want={"n_couple": {4, 5}, "emit": {1}}))
    C.append(Case("sparse_k40_v6_one_dense", lambda: sparse_problem(6, 40, 760, dense_views=(2,)), sparse=(0, 1, 3, 4, 5),
                  want={"n_couple": {4, 5}, "emit": {0, 1}}))
    C.append(Case("identity_k8_v9", lambda: identity_problem(8, 800), want={"n_couple": {7, 8}, "maps": {"identity"}}))
    C.append(Case("mixed_maps_k8_v6", lambda: mixed_maps_problem(8, 810), want={"n_couple": {4, 5}, "maps": {"mixed"}}))
    for k in (8, 20, 40, 64):
        for xg, xtf in ((16, 7), (6, 16)):
            C.append(Case(f"slabs_k{k}_{xg}_{xtf}", lambda k=k: slab_problem(k, 900 + k),
                          {"pass_splits_xg": xg, "pass_splits_xtf": xtf}, want={"n_couple": {1}}, slab=True))
    C.append(Case("edge_psi_elsewhere_nan", lambda: psi_edge_problem(820), want={"n_couple": {0, 1}}, nan_view=2))
    C.append(Case("edge_all_pairs_na", lambda: na_edge_problem(830), want={"n_couple": {0}}))
    C.append(Case("edge_xi_only", lambda: xi_edge_problem(840), want={"s_n_couple": {1}}))
    C.append(Case("mixed_k_5_20_64", lambda: mixed_k_problem([5, 20, 64], 850)))
    C.append(Case("mixed_k_8_8_40_coupled", lambda: mixed_k_problem([8, 8, 40], 860, coupled_01=True),
                  want={"n_couple": {0, 1}, "s_n_couple": {0, 1}}))
    return C


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def case(cid) -> Case:
    return CASES[CASE_IDS.index(cid)]


# ---------------------------------------------------------------------------------------------------------------------
# the host's own statement of fill_update / build_args: who is coupled to whom
# ---------------------------------------------------------------------------------------------------------------------
def shared(prob):
    """(rows, columns): per view {other view: shared names or None (NA)} -- exactly the names present in both."""
    return naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)


def coupled_views(coup, sh_v, v, whole_matrix):
    """The views whose factor enters view v's numerator (R/utils.r:63-78): weight != 0, not v itself, pair not NA --
    in view order.  ``(restricted, list)``; F restricts on its own column of phi, G on the whole of psi."""
    restricted = bool((np.sum(coup) if whole_matrix else np.sum(coup[:, v])) != 0)
    if not restricted:
        return False, []
    return True, [i for i in range(coup.shape[0]) if coup[i, v] != 0 and i != v and sh_v[i] is not None]


def _is_identity(names_v, names_w):
    return len(names_w) >= len(names_v) and all(a == b for a, b in zip(names_v, names_w))


def expected_plan(prob):
    """Per view: the coupling fields Engine.update_plan must report, side-wise (F, G)."""
    sh = shared(prob)
    out = []
    for v in range(len(prob.data)):
        e = {"restricted": [], "n_couple": [], "couple_bucket": [], "n_identity_maps": [], "n_index_maps": [], "sigma_is_zero": []}
        for side, (coup, names) in enumerate(((prob.phi, prob.row_names), (prob.psi, prob.col_names))):
            restricted, cl = coupled_views(coup, sh[side][v], v, whole_matrix=side == 1)
            ident = sum(_is_identity(names[v], names[c]) for c in cl)
            e["restricted"].append(int(restricted)); e["n_couple"].append(len(cl))
            e["couple_bucket"].append(0 if not restricted else 4 if len(cl) <= 4 else 8 if len(cl) <= 8 else 16)
            e["n_identity_maps"].append(ident); e["n_index_maps"].append(len(cl) - ident)
            e["sigma_is_zero"].append(int(np.sum(coup[:, v]) == 0))       # (the view's own column, restricted or not)
        e = {key: tuple(val) for key, val in e.items()}
        e["s_restricted"] = int(np.sum(prob.xi) != 0)
        e["s_n_couple"] = sum(1 for i in range(len(prob.data)) if prob.xi[i, v] != 0 and i != v) if e["s_restricted"] else 0
        out.append(e)
    return out


def check_wants(c: Case, plans):
    """The coupling counts, map kinds and hand-off modes the case is in the table for are there (``plans``: per view,
    expected_plan's keys; the device's plans also carry ``emit``)."""
    got = {p["n_couple"][s] for p in plans for s in (0, 1) if p["restricted"][s]}
    assert c.want.get("n_couple", set()) <= got, f"{c.id}: coupling counts {sorted(got)}, wanted {sorted(c.want['n_couple'])}"
    got_s = {p["s_n_couple"] for p in plans}
    assert c.want.get("s_n_couple", set()) <= got_s, f"{c.id}: S coupling counts {sorted(got_s)}"
    kinds = set()
    for p in plans:
        for s in (0, 1):
            if p["n_couple"][s]:
                kinds.add("identity" if not p["n_index_maps"][s] else "index" if not p["n_identity_maps"][s] else "mixed")
    assert c.want.get("maps", set()) <= kinds, f"{c.id}: map lists {sorted(kinds)}"
    if "emit" in c.want and "emit" in plans[0]:
        assert {p["emit"] for p in plans} == c.want["emit"], f"{c.id}: emit {[p['emit'] for p in plans]}"


# ---------------------------------------------------------------------------------------------------------------------
# host state of a case: the initial factors and one oracle sweep
# ---------------------------------------------------------------------------------------------------------------------
def initial_state(prob):
    """``before`` as Engine.get_factors returns it ahead of the first sweep: (F, S, G, lambda, mu), lambda and mu the
    column sums (R/update_steps.r:49-56) unless the problem sets them (``init_lam`` / ``init_mu``: {view: values})."""
    lam, mu = O.explicit_init_lm(prob.init_f, prob.init_g)
    for v, val in getattr(prob, "init_lam", {}).items():
        lam[v] = np.asarray(val, dtype=np.float64)
    for v, val in getattr(prob, "init_mu", {}).items():
        mu[v] = np.asarray(val, dtype=np.float64)
    return [(prob.init_f[v], prob.init_s[v], prob.init_g[v], lam[v], mu[v]) for v in range(len(prob.data))]


def oracle_sweep(prob, x, before):
    sh_r, sh_c = shared(prob)
    f, s, g, lam, mu = O.update_matrices(x, [b[0] for b in before], [b[1] for b in before], [b[2] for b in before],
                                         [b[3] for b in before], [b[4] for b in before], prob.phi, prob.xi, prob.psi,
                                         sh_r, sh_c, prob.row_names, prob.col_names)
    return [(f[v], s[v], g[v], lam[v], mu[v]) for v in range(len(x))]


def host_slab_start(extent: int) -> int:
    """First contraction row of the last slab at its SHORTEST: every split is a whole number of 32-row steps of the
    extent padded to 64, so the last one holds the padded extent's last 32 rows at least (the device tests take the
    true start from Engine.view_plan and assert that it is not later than this one)."""
    return 64 * ((extent + 63) // 64) - 32


# ---------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------
def _stat(mutant, true):
    worst, nz, nans = nan_stat(mutant, true)
    return np.inf if (nz or nans) else worst


def update_mutants(x, before, after, prob, v, slab_start=None):
    """``{name: statistic}`` between the step references of view v and references with one bug each; every reference is
    a call of the oracle's update_f / update_g / update_s on altered inputs (or, for the two bugs that no input can
    express, a combination of such calls: the update is |W (num + sum_i t_i) / den| with non-negative terms, so a term is
    the difference of two calls and a denominator the ratio of two).  ``x``: the streamed images; ``before`` / ``after``:
    the state around the sweep (Gauss-Seidel: this sweep's factors of the views before v).  ``slab_start``: (first
    column of the last X.G slab, first row of the last Xt.F slab) of view v, or None."""
    n_v = len(x)
    sh = shared(prob)
    F0, S0, G0, lam0, mu0 = before[v]
    F1, G1 = after[v][0], after[v][2]
    out = {}
    for side, tag, coup, names in ((0, "F", prob.phi, prob.row_names), (1, "G", prob.psi, prob.col_names)):
        i = 0 if side == 0 else 2
        ws = [a[i] for a in after[:v]] + [b[i] for b in before[v:]]

        def step(ws_=ws, names_=names, sh_=sh[side][v], coup_=coup, xm=x[v]):
            if side == 0:
                return O.update_f(xm, ws_, S0, G0, lam0, coup_, v, sh_, names_[v], names_)
            return O.update_g(xm, F1, S0, ws_, mu0, coup_, v, sh_, names_[v], names_)
        true = step()
        restricted, cl = coupled_views(coup, sh[side][v], v, whole_matrix=side == 1)
        if slab_start is not None:
            xm = x[v].copy()
            if side == 0:
                xm[:, slab_start[0]:] = 0.0
            else:
                xm[slab_start[1]:, :] = 0.0
            out[f"{tag}: the last slab left out of the sum"] = _stat(step(xm=xm), true)
        if not restricted:
            continue
        na = lambda *views: {**sh[side][v], **{c: None for c in views}}      # noqa: E731  (NA: out of the numerator only)
        if cl:
            out[f"{tag}: the last coupled view's term dropped"] = _stat(step(sh_=na(cl[-1])), true)
            c = cl[len(cl) // 2]
            moved = list(names); moved[c] = list(names[c][1:]) + list(names[c][:1])
            out[f"{tag}: view {c}'s name map shifted by one row"] = _stat(step(names_=moved), true)
            # n_other of the view itself: term c scaled by len_v / len_c (the term is the difference of two calls)
            c = max(cl, key=lambda t: abs(len(names[v]) / len(names[t]) - 1.0))
            if len(names[c]) != len(names[v]):
                term = true - step(sh_=na(c))
                out[f"{tag}: n_other of the view itself for view {c}"] = _stat(true + (len(names[v]) / len(names[c]) - 1.0) * term, true)
        if len(cl) >= 2:
            ws2 = list(ws); ws2[cl[1]] = ws[cl[0]]
            nm2 = list(names); nm2[cl[1]] = names[cl[0]]
            sh2 = dict(sh[side][v]); sh2[cl[1]] = sh[side][v][cl[0]]
            out[f"{tag}: view {cl[0]}'s rows read twice, in place of view {cl[1]}'s"] = _stat(step(ws_=ws2, names_=nm2, sh_=sh2), true)
        earlier = [c for c in cl if c < v]
        if earlier:
            ws2 = list(ws); ws2[earlier[-1]] = before[earlier[-1]][i]
            out[f"{tag}: the previous sweep's factor of view {earlier[-1]}"] = _stat(step(ws_=ws2), true)
        if np.sum(coup[:, v]) != 0:
            # sigma w left out of the denominator: the denominators with and without it are the ratio of the call with every
            # pair NA to the unrestricted call (both have the bare numerator)
            all_na = step(sh_=na(*range(n_v)))
            bare = step(coup_=np.zeros_like(coup))
            ok = np.isfinite(all_na) & (all_na > 0) & np.isfinite(bare)
            mut = np.where(ok, true * np.divide(bare, all_na, out=np.ones_like(bare), where=ok), true)
            out[f"{tag}: sigma w left out of the denominator"] = _stat(mut, true)
    ss = [a[1] for a in after[:v]] + [b[1] for b in before[v:]]
    cs = [c for c in range(n_v) if prob.xi[c, v] != 0 and c != v]
    if np.sum(prob.xi) != 0 and cs:
        true = O.update_s(x[v], F1, ss, G1, prob.xi, v)
        ss2 = list(ss); ss2[cs[-1]] = np.zeros_like(ss[cs[-1]])
        out[f"S: the xi term of view {cs[-1]} dropped"] = _stat(O.update_s(x[v], F1, ss2, G1, prob.xi, v), true)
    return out
