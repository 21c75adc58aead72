"""The fp64 update cases (tests/fp64_update_cases.py) on the host, with the oracle only: what
``tests/test_gpu_fp64_update_forms.py`` relies on can be checked without a GPU.

* the table reaches what it is there for (V = 5 .. 8, coupled counts 0 .. 7 on either side and for S, the three kinds of
  map list, an NA pair and a zero weight inside a restricted view, an unrestricted F beside a restricted G, every padded
  k class, all four sources) and its extents straddle the shape constants of csrc/resnmtf_fp64_job.h;
* every bar is below 1e-12, and the reference alone stays well inside: the same sweep in ``np.longdouble`` is within a
  quarter of every bar of the fp64 oracle (worst seen: 13.2 units of 2^-53, k64_v7; the smallest bar is 342 units);
* every mutant -- those of ``update_cases.update_mutants`` and the two of the fp64 layout -- is at least MUTANT_MARGIN x
  the case's bar away from the true step;
* the restriction matrices of an 8-view case have column sums that numpy's pairwise order and the sequential one round
  differently, so the cases reach the V = 8 branch of the short sums with data that tells the two apart.
"""
import re

import numpy as np
import pytest

import fp64_update_cases as F
import update_cases as U
from data_ref import nan_stat
from test_gpu_sweep_elementwise import MUTANT_MARGIN

_STATE = {}


def _state(cid):
    """(case, problem, before, after) of one oracle sweep from the initial factors, or from ``case.before`` oracle sweeps
    after them -- computed once, left unchanged."""
    if cid not in _STATE:
        c = F.case(cid)
        prob = c.make()
        before = U.initial_state(prob)
        for _ in range(c.before):
            before = U.oracle_sweep(prob, prob.data, before)
        _STATE[cid] = (c, prob, before, U.oracle_sweep(prob, prob.data, before))
    return _STATE[cid]


def test_the_table_reaches_what_it_is_there_for():
    missing = sorted(str(t) for t in F.DEMANDED - F.covered())
    assert not missing, "no case reaches: " + ", ".join(missing)
    assert len(set(F.CASE_IDS)) == len(F.CASE_IDS)
    after10 = [c for c in F.CASES if c.before]
    assert sorted(16 * ((U.ks_of(c.make())[0] + 15) // 16) for c in after10) == [16, 32, 48, 64] and all(c.before == 10 for c in after10)
    mixed = F.case("mixed_sources_k20_v8")
    assert mixed.used_sources() == set(F.SOURCES) and [v for v in range(8) if mixed.sources[v] in (1, 3)] == list(mixed.sparse)


def test_extents_straddle_the_shape_constants():
    K = F.CONSTANTS
    assert (K["F64_ROWS"], K["F64_UPD_ROWS"], K["F64_RES_ROWS"], K["F64_GRAM_ROWS"], K["F64_JC"], K["LD"]) == (128, 64, 64, 256, 64, 32)
    for c in F.CASES:
        prob = c.make()
        shapes = [x.shape for x in prob.data]
        assert all(min(s) >= U.ks_of(prob)[0] for s in shapes)
        assert all(n % K["LD"] and m % K["LD"] for n, m in shapes), (c.id, shapes)       # no extent on the rounding
        assert all(n > K["F64_ROWS"] and n % K["F64_UPD_ROWS"] for n, _ in shapes), (c.id, shapes)      # two product tiles, a ragged last update workgroup
        assert all(K["F64_JC"] < m < K["F64_ROWS"] for _, m in shapes), (c.id, shapes)    # two LDS stages, one G-side tile
        if len(shapes) == 8:
            assert any(n > K["F64_GRAM_ROWS"] for n, _ in shapes), c.id                    # two Gram workgroups
            if c.id != "identity_k8_v8":                                                   # (identity maps need one shape)
                assert len({n for n, _ in shapes}) == 8 and len({m for _, m in shapes}) == 8
        elif "identity" not in c.id and "mixed_maps" not in c.id:
            assert len(set(shapes)) == len(shapes)


def test_edges_and_special_cases_are_what_they_claim():
    p = U.expected_plan(F.case("edge_psi_elsewhere_nan").make())[2]
    assert (p["restricted"][1], p["n_couple"][1], p["sigma_is_zero"][1], p["restricted"][0]) == (1, 0, 1, 0)
    for p in U.expected_plan(F.case("identity_k8_v8").make()):
        assert p["n_index_maps"] == (0, 0) and p["n_identity_maps"] == p["n_couple"]
    plans = U.expected_plan(F.case("na_zero_k8_v8").make())
    assert [p["n_couple"][1] for p in plans] == [5, 5, 6, 7, 6, 6, 2, 5] and [p["n_couple"][0] for p in plans] == [4, 4, 5, 6, 0, 5, 2, 4]
    assert plans[4]["restricted"][0] == 1 and [p["s_n_couple"] for p in plans] == [5, 5, 6, 7, 6, 6, 2, 5]
    plans = U.expected_plan(F.case("isolated_k8_v5").make())
    assert [p["n_couple"] for p in plans] == [(1, 1), (1, 1), (0, 0), (0, 0), (0, 0)]
    assert all(p["restricted"] == (0, 1) and p["s_restricted"] == 1 and p["s_n_couple"] == 0 for p in plans[2:])
    c, prob, before, after = _state("edge_psi_elsewhere_nan")
    g = after[c.nan_view][2]
    assert np.isnan(g[5, :]).all() and np.isnan(g).sum() == g.shape[1], "row 5 of G_2, and nothing else, is NaN"


def test_eight_view_restrictions_tell_the_pairwise_sum_from_the_sequential_one():
    prob = F.case("k8_v8").make()
    for name, mat in (("phi", prob.phi), ("psi", prob.psi), ("xi", prob.xi)):
        cols = [v for v in range(8) if float(np.sum(mat[:, v])) != sum(float(t) for t in mat[:, v])]
        assert cols, f"{name}: every column of the k8_v8 problem sums to the same bits in either order"


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_bars_hold_for_the_reference_itself(cid):
    """Every bar below 1e-12; the fp64 oracle within a quarter of it of the same sweep in long double (whose own
    roundings are 2^-11 of fp64's)."""
    c, prob, before, after = _state(cid)
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble must be wider than fp64 for this check to say anything"
    wide = F.oracle_sweep_as(prob, prob.data, before, np.longdouble)
    bars, nbars = F.case_bars(prob), F.norm_bars(prob)
    worst = 0.0
    for v in range(len(prob.data)):
        for i, key in enumerate(F.KEYS):
            assert bars[v][key] < F.BAR_LIMIT, (cid, v, key, bars[v][key])
            if "group" in c.routes and U.ks_of(prob)[0] <= 32:
                assert nbars[v][key] < F.BAR_LIMIT, (cid, v, key, nbars[v][key])
            assert wide[v][i].dtype == np.longdouble
            ref = np.asarray(wide[v][i])
            got = np.asarray(after[v][i], dtype=np.longdouble)
            pos = ref > 0
            st = float(np.max(np.abs(got[pos] / ref[pos] - 1))) if pos.any() else 0.0
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and not np.any(got[~pos & ~np.isnan(ref)] != 0), (cid, v, key)
            worst = max(worst, st / F.U53)
            assert st <= 0.25 * bars[v][key], f"{cid} view {v} {key}: the fp64 oracle is {st:.3e} from long double, bar {bars[v][key]:.3e}"
    print(f"MEASURED {cid} oracle against long double: {worst:.1f} units of 2^-53")


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_mutants_clear_the_margin(cid):
    c, prob, before, after = _state(cid)
    bars = F.case_bars(prob)
    plans = U.expected_plan(prob)
    names = set()
    for v in range(len(prob.data)):
        bar = max(bars[v][key] for key in ("f", "g", "s"))
        muts = F.all_mutants(prob.data, before, after, prob, v)
        for name, val in muts.items():
            assert val >= MUTANT_MARGIN * bar, f"{cid} view {v}: mutant '{name}' gives only {val:.3e} against the bar {bar:.1e}"
        names |= {re.sub(r"\d+", "#", n) for n in muts}
    if any(p["n_couple"][s] >= 2 for p in plans for s in (0, 1)):
        for tag in "FG":
            kinds = {n for n in names if n.startswith(tag + ":")}
            assert len(kinds) >= (5 if cid.startswith("identity") else 7), sorted(kinds)      # (identity maps: no layout mutant, no n_other)
        assert any(n.startswith("S:") for n in names)
    if not cid.startswith("identity") and any(p["n_couple"][s] >= 2 and p["n_index_maps"][s] for p in plans for s in (0, 1)):
        assert any("used for" in n for n in names) and any("read through the map" in n for n in names), sorted(names)


def test_statistic_sees_one_wrong_row():
    """What a Frobenius norm over the factor misses: one row of F reading the neighbouring row of the coupled view."""
    c, prob, before, after = _state("k8_v8")
    f = after[3][0]
    wrong = f.copy(); wrong[17, :] = f[18, :]
    assert nan_stat(wrong, f)[0] > 1e-3
    assert np.linalg.norm(wrong - f) / np.linalg.norm(f) < 0.2
