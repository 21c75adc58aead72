"""The update-side elementwise cases (tests/update_cases.py) on the host, with the oracle only: what
``tests/test_gpu_update_forms.py`` relies on can be checked without a GPU.

* the case table yields the coupling counts and bucket edges it is there for (``fill_update``'s rule restated:
  weight != 0, not the view itself, pair not NA) -- this table is what the device test compares ``Engine.update_plan`` with;
* for every case, ``before`` = the initial factors and ``after`` = one oracle sweep: every mutant (a coupled term dropped,
  read twice or through a shifted map, the wrong n_other, last sweep's factor, sigma w missing, an xi term dropped, the
  last slab missing) is at least MUTANT_MARGIN x the case's bar away from the true step reference;
* the NaN edge case produces its NaN row in the oracle.
"""
import re

import numpy as np
import pytest

import update_cases as U
from data_ref import nan_stat
from sweep_ref import step_reference
from test_gpu_sweep_elementwise import BARS, MUTANT_MARGIN

_STATE = {}


def _state(cid):
    """(case, problem, images, before, after) -- computed once per case and left unchanged."""
    if cid not in _STATE:
        c = U.case(cid)
        prob = c.make()
        x = [np.asarray(d, dtype=np.float64).astype(np.float32).astype(np.float64) for d in prob.data]      # the f32 image
        before = U.initial_state(prob)
        _STATE[cid] = (c, prob, x, before, U.oracle_sweep(prob, x, before))
    return _STATE[cid]


def test_case_table_covers_every_coupling_count_and_edge():
    n_couple, s_n_couple, kinds, buckets = {0: set(), 1: set()}, set(), set(), set()
    for c in U.CASES:
        prob = c.make()
        ks = U.ks_of(prob)
        plans = U.expected_plan(prob)
        U.check_wants(c, plans)
        for v, p in enumerate(plans):
            assert min(prob.data[v].shape) >= ks[v], f"{c.id}: view {v} is smaller than its k"
            for s in (0, 1):
                length = prob.data[v].shape[s]
                assert length % U.ROWS_PER_GROUP[U.kp_of(ks[v])], f"{c.id}: view {v} side {s} ends on a row-group boundary"
                if p["restricted"][s]:
                    n_couple[s].add(p["n_couple"][s])
                    buckets.add((U.kp_of(ks[v]), s, p["couple_bucket"][s]))
                    if p["n_couple"][s]:
                        kinds.add("identity" if not p["n_index_maps"][s] else "index" if not p["n_identity_maps"][s] else "mixed")
            s_n_couple.add(p["s_n_couple"])
        if len(set(ks)) > 1:
            kinds.add("mixed k")
    for s in (0, 1):
        assert {0, 1, 4, 5, 8, 9, 16} <= n_couple[s], (s, sorted(n_couple[s]))      # both sides of every bucket edge, and 16
    assert {(kp, s, b) for kp in (16, 32, 48, 64) for s in (0, 1) for b in (4, 8, 16)} <= buckets
    assert 16 in s_n_couple and any(5 <= n < 16 for n in s_n_couple)
    assert {"identity", "index", "mixed", "mixed k"} <= kinds


def test_branch_edges_are_what_they_claim():
    p = U.expected_plan(U.case("edge_psi_elsewhere_nan").make())[2]
    assert (p["restricted"][1], p["n_couple"][1], p["sigma_is_zero"][1], p["restricted"][0]) == (1, 0, 1, 0)
    for p in U.expected_plan(U.case("edge_all_pairs_na").make()):
        assert (p["restricted"][0], p["n_couple"][0], p["sigma_is_zero"][0]) == (1, 0, 0)
    for p in U.expected_plan(U.case("edge_xi_only").make()):
        assert p["restricted"] == (0, 0) and (p["s_restricted"], p["s_n_couple"]) == (1, 1)
    plans = U.expected_plan(U.case("mixed_k_8_8_40_coupled").make())
    assert [p["n_couple"] for p in plans] == [(1, 1), (1, 1), (0, 0)] and plans[2]["restricted"] == (0, 1)
    for p in U.expected_plan(U.case("identity_k8_v9").make()):
        assert p["n_index_maps"] == (0, 0) and p["n_identity_maps"] == p["n_couple"]


def test_nan_edge_case_has_its_nan_row_in_the_oracle():
    c, prob, x, before, after = _state("edge_psi_elsewhere_nan")
    g = after[c.nan_view][2]
    assert np.isnan(g[5, :]).all() and np.isnan(g).sum() == g.shape[1], "row 5 of G_2, and nothing else, is NaN"
    assert not any(np.isnan(a[0]).any() for a in after), "no F is touched"
    assert not any(np.isnan(after[v][2]).any() for v in (0, 1))
    # rel_stat would count the NaN of a correct device as "non-zero where the reference is zero"; nan_stat does not
    assert nan_stat(g, g) == (0.0, 0, 0)
    wrong = g.copy(); wrong[5, 0] = 0.0
    assert nan_stat(wrong, g)[2] == 1


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_mutants_clear_the_margin(cid):
    c, prob, x, before, after = _state(cid)
    ks = U.ks_of(prob)
    ref = step_reference(x, before, after, prob.phi, prob.xi, prob.psi, prob.row_names, prob.col_names,
                         row_indices=U.shared(prob)[0], col_indices=U.shared(prob)[1])
    names = set()
    for v in range(len(x)):
        for i, key in enumerate(("f", "s", "g", "lam", "mu")):        # (the step references of an oracle sweep are that sweep)
            assert nan_stat(after[v][i], ref[key][v]) == (0.0, 0, 0), (v, key)
        bar = BARS[c.form(v, ks[v])]
        slab = (U.host_slab_start(x[v].shape[1]), U.host_slab_start(x[v].shape[0])) if c.slab else None
        muts = U.update_mutants(x, before, after, prob, v, slab_start=slab)
        for name, val in muts.items():
            assert val >= MUTANT_MARGIN * bar, f"{cid} view {v}: mutant '{name}' gives only {val:.3e} against the bar {bar:.1e}"
        names |= {re.sub(r"\d+", "#", n) for n in muts}               # (the kinds of mutant, whichever views they name)
    plans = U.expected_plan(prob)
    if any(p["n_couple"][s] >= 2 for p in plans for s in (0, 1)):
        assert sum(1 for n in names if n.startswith("F:")) >= 5 and sum(1 for n in names if n.startswith("G:")) >= 5, sorted(names)
    if c.slab:
        assert any("last slab" in n for n in names)


def test_update_plan_is_exported_and_the_binding_follows_the_header():
    """An added entry point under ABI version 2; the ctypes structure has the header's fields in the header's order."""
    import ctypes as C
    import os
    from helpers import ROOT
    from resnmtf_amd import _lib
    lib = _lib.load()
    assert "resnmtf_update_plan" in _lib.SIGNATURES and hasattr(lib, "resnmtf_update_plan")
    assert lib.resnmtf_update_plan.argtypes == [C.c_void_p, C.c_int, C.POINTER(_lib.UpdatePlan)] and lib.resnmtf_update_plan.restype is C.c_int
    header = open(os.path.join(ROOT, "include", "resnmtf_hip.h")).read()
    assert re.search(r"#define\s+RESNMTF_ABI_VERSION\s+2\b", header) and lib.resnmtf_abi_version() == _lib.ABI_VERSION == 2      # additions only
    body = re.search(r"typedef struct resnmtf_update_plan_info \{(.*?)\} resnmtf_update_plan_info;", header, re.S).group(1)
    fields = []
    for decl in re.findall(r"^\s*int\s+([^;]+);", body, re.M):
        for name in decl.split(","):
            m = re.fullmatch(r"(\w+)(\[2\])?", name.strip())
            fields.append((m.group(1), C.c_int * 2 if m.group(2) else C.c_int))
    assert [(n, t) for n, t in _lib.UpdatePlan._fields_] == fields
    assert lib.resnmtf_update_plan(None, 0, None) == 1                 # RESNMTF_ERR_INVALID without a handle: no device needed
