"""The factor updates of one device sweep checked ENTRY BY ENTRY against fp64, at every coupling bucket, hand-off mode
and slab bucket of ``factor_update_kernel<KP, IS_G, NCB, EMIT>``.

The machinery is that of tests/test_gpu_sweep_elementwise.py (0 or 10 sweeps, raw state, ONE sweep, raw state; every
step against ``sweep_ref.step_reference``; the same per-form BARS, ERR_BAR and MUTANT_MARGIN); the cases, their expected
coupling tables and their mutants are in tests/update_cases.py, which tests/test_update_forms_host.py checks without a
GPU.  What is new here:

* the problems couple 5 to 17 views through partial, non-identity name maps (``helpers.coupled_problem``), so that the
  updates run with 3 .. 16 coupled terms -- both sides of the bucket edges 4|5 and 8|9, and 16 -- at KP 16, 32, 48 and 64,
  in both hand-off modes (EMIT on and off), on dense and on sparse views, with 6, 7 and 16 slabs, with identity, index
  and mixed map lists, on handles that mix k, and at the branch edges of ``fill_update``;
* ``update_blocks = 3`` and extents that are no multiple of a row group: every update launch has several workgroups and
  a last one that ends inside a row group;
* ``Engine.update_plan`` of every view is compared with the host's own statement of the coupling rule
  (``update_cases.expected_plan``) and recorded; ``test_update_forms_covered`` asserts from the recorded plans that the
  cases -- with those of the elementwise suite -- reach all 64 instantiations and every slab bucket of every (KP, side);
* the statistic is ``data_ref.nan_stat``: ``rel_stat`` plus "NaN exactly where the reference is NaN" (the coupled form has
  no NaN -> 1 guard, and one case makes it produce a NaN row).  Nothing is excused: no band, no skipped entry.

Bars: the update is fp64, so its error is that of the f32 slabs it sums and every view is judged by the bar of its pass
form, ``BARS[form_of(view_plan)]``.  Worst ``max |got / ref - 1|`` measured on the MI355X over the cases of this file
(each test prints its own as ``MEASURED ...``):

    form     bar      worst measured
    f32      1.0e-6   1.19e-7  (k8_v6_flipped)
    wide     1.5e-6   2.25e-7  (mixed_k_5_20_64)
    sparse   1.0e-6   8.71e-8  (sparse_k20_v6)
    error    5e-7     2.23e-9  (mixed_k_5_20_64; absolute)
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_sweep_elementwise as EW
import update_cases as U
from data_ref import nan_stat
from sweep_ref import step_reference, stream_image

pytestmark = pytest.mark.gpu

RESULTS = {}               # case id -> Engine.update_plan of every view, of the cases that passed
ATTEMPTED = set()          # cases run in this session (a failed one covers nothing)
KEYS = ("f", "s", "g", "lam", "mu")
ERR_INVALID = 1            # RESNMTF_ERR_INVALID


def _run(c, prob):
    n_v = len(prob.data)
    e = EW._engine(prob, c.sparse_flags(n_v) if c.sparse is not None else False, c.opts)
    try:
        if c.before:
            e.run(c.before)
        before = [e.get_factors(v) for v in range(n_v)]
        err = e.run(1)
        after = [e.get_factors(v) for v in range(n_v)]
        vplans = [e.view_plan(v) for v in range(n_v)]
        uplans = [e.update_plan(v) for v in range(n_v)]
        images = [stream_image(e, v, prob.data[v], vplans[v]) for v in range(n_v)]
    finally:
        e.close()
    return before, after, err, vplans, uplans, images


def _rows_off(got, ref, bar):
    """The rows of a factor that hold an entry off its bar, a NaN out of place or a non-zero where the reference is zero."""
    got = np.atleast_2d(np.asarray(got, dtype=np.float64)); ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(ref > 0, np.abs(got / ref - 1.0), np.where(np.isnan(ref), 0.0, np.where(got != 0, np.inf, 0.0)))
    bad = ~(dev <= bar) | (np.isnan(got) != np.isnan(ref))
    rows = np.flatnonzero(bad.any(axis=1))
    return f"{rows.size} rows, first {rows[:8].tolist()}"


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_update_forms_elementwise(cid):
    c = U.case(cid)
    prob = c.make()
    n_v, ks = len(prob.data), U.ks_of(prob)
    before, after, err, vplans, uplans, images = _run(c, prob)
    ATTEMPTED.add(cid)
    # --- the plan: the coupling table is the host's, the geometry what the case is built for
    expected = U.expected_plan(prob)
    for v in range(n_v):
        up = uplans[v]
        assert up["prepared"] and (up["k"], up["kp"]) == (ks[v], U.kp_of(ks[v]))
        assert up["rows_per_group"] == U.ROWS_PER_GROUP[up["kp"]] == up["threads"] // up["kp"]
        for key, val in expected[v].items():
            assert up[key] == val, f"view {v}: update_plan {key} = {up[key]}, the coupling rule gives {val}"
        for s in (0, 1):
            assert up["couple_bucket"][s] == (0 if not up["restricted"][s] else 4 if up["n_couple"][s] <= 4 else 8 if up["n_couple"][s] <= 8 else 16)
            assert up["split_bucket"][s] == (4 if up["nsplit"][s] <= 4 else 8 if up["nsplit"][s] <= 8 else 16) and up["nsplit"][s] <= 16
            assert up["nsplit"][s] == vplans[v]["nsplit"][s]
            assert up["route"][s] == "kernel", f"view {v}: the update does not run as factor_update_kernel ({up['route']})"
            assert up["nblk"][s] >= 2 and up["last_block_rows"][s] % up["rows_per_group"], f"view {v} side {s}: {up}"
            assert up["last_block_rows"][s] == prob.data[v].shape[s] - (up["nblk"][s] - 1) * up["rows_per_block"][s]
        assert EW.form_of(vplans[v]) == c.form(v, ks[v])
        assert up["emit"] == (1 if vplans[v]["kk_mode"] == 0 else 0)
    U.check_wants(c, uplans)
    # --- every step of the sweep against its fp64 reference
    data = [np.asarray(d, dtype=np.float64) for d in prob.data]
    sh_r, sh_c = U.shared(prob)
    ref = step_reference(images, before, after, prob.phi, prob.xi, prob.psi, prob.row_names, prob.col_names, data=data,
                         row_indices=sh_r, col_indices=sh_c)
    failures, worst = [], {}
    for v in range(n_v):
        form = c.form(v, ks[v])
        bar = EW.BARS[form]
        for i, key in enumerate(KEYS):
            st, nz, nans = nan_stat(after[v][i], ref[key][v])
            worst[form] = max(worst.get(form, 0.0), st)
            if st > bar or nz or nans:
                side = {"f": 0, "g": 1}.get(key)
                what = "" if side is None else (f", update form (KP {uplans[v]['kp']}, {'FG'[side]}, NCB {uplans[v]['couple_bucket'][side]}, "
                                                f"EMIT {uplans[v]['emit']}, PF {uplans[v]['split_bucket'][side]}, n_couple {uplans[v]['n_couple'][side]})")
                failures.append(f"view {v} ({form}) step {key}: max |got/ref - 1| = {st:.3e} (bar {bar:.1e}), {nz} non-zero where the "
                                f"reference is zero, {nans} NaN mismatches; {_rows_off(after[v][i], ref[key][v], bar)}{what}")
        slab = None
        if c.slab:
            vp = vplans[v]
            slab = tuple((vp["nsplit"][s] - 1) * vp["rows_per_split"][s] for s in (0, 1))
            for s in (0, 1):      # (the host test drops a last slab that is no longer than the device's)
                assert U.host_slab_start(prob.data[v].shape[1 - s]) >= slab[s] and slab[s] < prob.data[v].shape[1 - s]
        for name, val in U.update_mutants(images, before, after, prob, v, slab_start=slab).items():
            assert val >= EW.MUTANT_MARGIN * bar, f"view {v}: mutant '{name}' gives only {val:.3e} against the bar {bar:.1e}"
    ref_err = float(np.mean(ref["err"]))
    d_err = abs(float(err[-1]) - ref_err)
    print(f"MEASURED {cid} " + " ".join(f"{form}={val:.3e}" for form, val in sorted(worst.items())) + f" err={d_err:.3e}")
    assert not failures, "\n".join(failures)
    if np.isnan(ref_err):
        assert c.nan_view is not None and np.isnan(err[-1]), f"error {err[-1]!r} where the reference is NaN"
    else:
        assert d_err < EW.ERR_BAR, f"error {err[-1]!r} against {ref_err!r}"
    if c.nan_view is not None:
        g = after[c.nan_view][2]
        assert np.isnan(g[5, :]).all() and np.isnan(g).sum() == g.shape[1], "the NaN row of the unguarded coupled form"
    RESULTS[cid] = uplans


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
def _fresh_plans(prob, sparse_views, opts):
    e = EW._engine(prob, sparse_views, opts)
    try:
        e.prepare()
        return [e.update_plan(v) for v in range(len(prob.data))]
    finally:
        e.close()


def _all_plans():
    """[(case id, update plans)] of the cases of this file and of the elementwise suite: as the tests that passed recorded
    them, or -- a case was not run in this session -- from a fresh engine after prepare.  A case that ran and failed covers
    nothing; the elementwise suite's FINDINGS cases do not count."""
    out = []
    for c in U.CASES:
        if c.id not in RESULTS and c.id not in ATTEMPTED:
            prob = c.make()
            RESULTS[c.id] = _fresh_plans(prob, c.sparse_flags(len(prob.data)) if c.sparse is not None else False, c.opts)
        if c.id in RESULTS:
            out.append((c.id, RESULTS[c.id]))
    for cid, make, opts, _, sparse_views in EW.CASES:
        if cid in EW.FINDINGS:
            continue
        if cid in EW.RESULTS and cid in EW.UPDATE_PLANS:
            out.append((cid, EW.UPDATE_PLANS[cid]))
        elif cid not in EW.ATTEMPTED:
            out.append((cid, _fresh_plans(make(), sparse_views, opts)))
    return out


def test_update_forms_covered():
    """The cases together reach every instantiation of factor_update_kernel and every slab bucket of every (KP, side), read
    from Engine.update_plan.  Only updates that run as a factor_update_kernel launch count (route "kernel": not the ones
    the hoisted F chain or a fused pass launch runs instead).

    The product of the two tables is NOT demanded: in factor_update_body the ``request`` loops over the NC coupling slots
    and over the PF slab slots share no index -- ``cval[c]`` is filled from ``a.couple[c]`` and ``praw[q]`` from slab q
    independently -- so a slab bucket is exercised the same whatever the coupling bucket, and the other way round."""
    reached = set()
    for cid, plans in _all_plans():
        kps = set()
        for p in plans:
            kps.add(p["kp"])
            for s in (0, 1):
                if p["route"][s] != "kernel":
                    continue
                reached.add(("form", p["kp"], "FG"[s], p["couple_bucket"][s], p["emit"]))
                reached.add(("slabs", p["kp"], "FG"[s], p["split_bucket"][s]))
                if p["restricted"][s]:
                    reached.add(("n_couple", "FG"[s], p["n_couple"][s]))
                    if p["n_couple"][s]:
                        reached.add(("maps", "identity" if not p["n_index_maps"][s] else "index" if not p["n_identity_maps"][s] else "mixed"))
                    reached.add(("restricted, sigma", "zero" if p["sigma_is_zero"][s] else "non-zero", "no coupled view" if not p["n_couple"][s] else "coupled"))
                if p["nblk"][s] >= 2 and p["last_block_rows"][s] % p["rows_per_group"]:
                    reached.add(("ragged last block", p["kp"], "FG"[s]))
            reached.add(("mm64", p["kp"], p["mm64"])); reached.add(("packk", p["kp"], p["emit"], p["packk"]))
            if p["s_n_couple"] == 16:
                reached.add(("s_n_couple", "16"))
            elif p["s_n_couple"] >= 5:
                reached.add(("s_n_couple", ">= 5"))
            if p["s_restricted"] and not p["restricted"][0] and not p["restricted"][1]:
                reached.add(("S coupled, F and G unrestricted",))
        if len(kps) > 1:
            reached.add(("mixed KP on one handle", tuple(sorted(kps))))
    want = {("form", kp, side, ncb, emit) for kp in (16, 32, 48, 64) for side in "FG" for ncb in (0, 4, 8, 16) for emit in (0, 1)}
    assert len(want) == 64
    want |= {("slabs", kp, side, pf) for kp in (16, 32, 48, 64) for side in "FG" for pf in (4, 8, 16)}
    want |= {("ragged last block", kp, side) for kp in (16, 32, 48, 64) for side in "FG"}
    want |= {("n_couple", side, n) for side in "FG" for n in (0, 1, 4, 5, 8, 9, 16)}
    want |= {("maps", kind) for kind in ("identity", "index", "mixed")}
    want |= {("restricted, sigma", "zero", "no coupled view"), ("restricted, sigma", "non-zero", "no coupled view"), ("restricted, sigma", "non-zero", "coupled")}
    want |= {("mm64", 16, 1), ("mm64", 32, 1), ("mm64", 48, 0), ("mm64", 64, 1)}
    want |= {("packk", 32, 0, 1), ("packk", 64, 0, 1), ("packk", 32, 1, 0), ("packk", 64, 1, 0), ("packk", 16, 0, 0), ("packk", 48, 0, 0)}
    want |= {("s_n_couple", ">= 5"), ("s_n_couple", "16"), ("S coupled, F and G unrestricted",)}
    want |= {("mixed KP on one handle", (16, 32, 64)), ("mixed KP on one handle", (16, 48))}
    want |= {("body", "EMIT slice reduction (KK < UT)"), ("body", "strided tail (nsplit > PF)")}
    # branches of factor_update_body that cannot be reached from resnmtf_run on one handle, with what rules them out
    unreachable = {
        ("body", "EMIT slice reduction (KK < UT)"): "KK = KP * KP is below the workgroup's threads at KP 16 only (256 < 512), and KP 16 with "
                                                   "EMIT always takes the MFMA Gram chain (MFMA64 = EMIT && KP == 16)",
        ("body", "strided tail (nsplit > PF)"): "PF is 16 for any nsplit above 8 and size_pass / plan_wide / the sparse planner cap the "
                                                "splits at 16, the depth of this prefetch",
    }
    missing = sorted(str(w) for w in want - reached - set(unreachable))
    assert not missing, "update forms no case reaches: " + ", ".join(missing)


# ---------------------------------------------------------------------------------------------------------------------
# the query itself
# ---------------------------------------------------------------------------------------------------------------------
def test_update_plan_refuses_bad_arguments_and_changes_nothing():
    """resnmtf_update_plan: NULL handle / out, a bad view and a struct_size mismatch are RESNMTF_ERR_INVALID; before the
    first prepare the coupling fields read 0; the sweeps after a query are bitwise the sweeps without it."""
    from resnmtf_amd import _lib
    lib = _lib.load()
    c = U.case("k8_v5")
    prob = c.make()
    runs = []
    for query in (False, True):
        e = EW._engine(prob, False, c.opts)
        try:
            if query:
                p = _lib.UpdatePlan()
                p.struct_size = C.sizeof(_lib.UpdatePlan)
                assert lib.resnmtf_update_plan(None, 0, C.byref(p)) == ERR_INVALID
                assert lib.resnmtf_update_plan(e._h, 0, None) == ERR_INVALID
                assert lib.resnmtf_update_plan(e._h, 5, C.byref(p)) == ERR_INVALID
                assert lib.resnmtf_update_plan(e._h, -1, C.byref(p)) == ERR_INVALID
                p.struct_size -= 4
                assert lib.resnmtf_update_plan(e._h, 0, C.byref(p)) == ERR_INVALID
                with pytest.raises(_lib.ResnmtfError, match="struct_size"):
                    e._check(ERR_INVALID)
                p.struct_size += 4
                assert lib.resnmtf_update_plan(e._h, 0, C.byref(p)) == _lib.OK
                early = e.update_plan(1)
                assert not early["prepared"] and (early["kp"], early["threads"], early["rows_per_group"], early["emit"]) == (16, 512, 32, 1)
                assert early["nblk"] == (3, 3) and early["split_bucket"] == (4, 4)
                for key in ("restricted", "n_couple", "couple_bucket", "n_identity_maps", "n_index_maps", "sigma_is_zero"):
                    assert early[key] == (0, 0), key
                assert (early["s_restricted"], early["s_n_couple"]) == (0, 0)
            errs = e.run(2)
            if query:
                late = e.update_plan(1)
                assert late["prepared"] and late["n_couple"] == (4, 4) and late["couple_bucket"] == (4, 4) and late["s_n_couple"] == 4
                assert {key: late[key] for key in ("nsplit", "split_bucket", "rows_per_block", "nblk", "last_block_rows")} == \
                       {key: early[key] for key in ("nsplit", "split_bucket", "rows_per_block", "nblk", "last_block_rows")}
            errs = np.concatenate([errs, e.run(1)])
            runs.append((errs, [e.get_factors(v) for v in range(len(prob.data))]))
        finally:
            e.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
