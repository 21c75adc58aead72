"""loop_ref (the stop rule of R/main.r:50-81 on a vector of mean errors) against the oracle's own convergence loop, and
against mutants of the rule.  CPU only.

Three small problems: a plain 60 x 40 view (k = 3), two psi-coupled views, three partly name-coupled views.  For each, a
40-sweep fixed trace of the oracle; then the oracle's convergence loop at four tolerances -- the equality tolerance
``pick_stop`` chooses, 2.0 (errors lie in [0, 1]: the first sweep stops), 1e-6 and 0.0 under ``max_iters = 37`` -- must run
exactly ``stop_sweep(fixed trace, tol, max_iters)`` sweeps.  The same inputs separate every mutant of the rule from it.
"""
import numpy as np
import pytest

import loop_ref
from helpers import coupled_problem, run_oracle
from resnmtf_amd import synth

PROBLEMS = {
    "plain_60x40_k3": lambda: synth.make_problem([(60, 40)], 3),
    "two_views_psi": lambda: synth.make_problem([(50, 36), (44, 36)], 3, psi=0.8, seed_base=3),
    "three_views_names": lambda: coupled_problem([(48, 30), (44, 34), (40, 28)], 3, 1, phi_w=0.2, psi_w=0.1),
}
N_FIXED = 40
_TRACES = {}


def fixed_trace(name):
    if name not in _TRACES:
        prob = PROBLEMS[name]()
        _TRACES[name] = (prob, [float(x) for x in run_oracle(prob, n_iters=N_FIXED)["All_Error"]])
    return _TRACES[name]


def tolerances(trace):
    """(tol, max_iters) of the four convergence runs."""
    return [(loop_ref.pick_stop(trace)[1], None), (2.0, None), (1e-6, None), (0.0, 37)]


# ---------------------------------------------------------------------------------------------------------------------
# mutants of the rule: same signature as loop_ref.stop_sweep
# ---------------------------------------------------------------------------------------------------------------------
def _mutant(first_sweep_skipped=False, equality_continues=False, prev_not_updated=False, prev_is_diff=False):
    def rule(means, tol, max_iters=None):
        prev = None if first_sweep_skipped else 0.0
        for t, m in enumerate(means, start=1):
            m = float(m)
            if prev is None:
                diff, stop = None, False
            else:
                diff = abs(m - prev)
                stop = not (diff >= tol) if equality_continues else not (diff > tol)
            if prev_is_diff:
                prev = diff
            elif not prev_not_updated:
                prev = m
            if stop:
                return t
            if max_iters is not None and t >= max_iters:
                return int(max_iters)
        raise ValueError("trace too short")
    return rule


MUTANTS = {
    "the first sweep is skipped (prev = None)": _mutant(first_sweep_skipped=True),
    "diff >= tol continues (equality does not stop)": _mutant(equality_continues=True),
    "prev is not updated": _mutant(prev_not_updated=True),
    "prev is the previous diff": _mutant(prev_is_diff=True),
}


def test_record_lows_of_the_plain_trace():
    """The condition pick_stop places on a case holds for the plain problem with room to spare: record lows at sweeps 2, 3
    and every sweep from 11 to 33 of the 40-sweep trace."""
    _, trace = fixed_trace("plain_60x40_k3")
    lows = loop_ref.record_low_sweeps(trace)
    assert [t for t in lows if t <= 33] == [2, 3] + list(range(11, 34)), lows
    t, tol = loop_ref.pick_stop(trace)
    assert t == 11 and tol == loop_ref.diffs(trace)[10]


def test_rule_on_hand_made_traces():
    assert loop_ref.stop_sweep([0.9, 0.5, 0.4, 0.39], 0.05) == 4
    assert loop_ref.stop_sweep([0.9, 0.5, 0.4, 0.39], 0.9) == 1                 # equality on the first sweep: |0.9 - 0| = 0.9
    assert loop_ref.stop_sweep([0.9, 0.5, 0.4, 0.39], 0.0, max_iters=3) == 3
    assert loop_ref.stop_sweep([0.9, 0.5, 0.5], 0.0) == 3                       # a zero diff stops at tol 0
    assert loop_ref.stop_sweep([0.9, float("nan"), 0.1], 0.0) == 2              # NaN: `diff > tol` is false
    with pytest.raises(ValueError):
        loop_ref.stop_sweep([0.9, 0.5], 0.0)
    with pytest.raises(ValueError):
        loop_ref.stop_sweep([0.9, 0.5], 0.0, max_iters=3)
    assert loop_ref.record_low_sweeps([0.9, 0.5, 0.2, 0.1, 0.0]) == [2, 3, 4]   # diffs 0.9, 0.4, 0.3, 0.1, 0.1
    with pytest.raises(AssertionError):
        loop_ref.pick_stop([0.9, 0.5, 0.2, 0.1, 0.0])


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_oracle_loop_runs_stop_sweep_sweeps(name):
    prob, trace = fixed_trace(name)
    assert all(0.0 <= e <= 1.0 for e in trace)
    for tol, cap in tolerances(trace):
        want = loop_ref.stop_sweep(trace, tol, cap)
        got = run_oracle(prob, max_iters=cap, tol=tol)["All_Error"]
        assert len(got) == want, f"tol {tol!r}, max_iters {cap}: the oracle ran {len(got)} sweeps, stop_sweep says {want}"
        assert np.array_equal(got, trace[:want])
    t_star, tol = loop_ref.pick_stop(trace)
    assert 6 <= t_star <= 30 and loop_ref.stop_sweep(trace, tol) == t_star
    assert loop_ref.stop_sweep(trace, 2.0) == 1 and loop_ref.stop_sweep(trace, 0.0, 37) == 37
    assert all(d != 0.0 for d in loop_ref.diffs(trace)[:37])


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_is_separated(mutant):
    rule = MUTANTS[mutant]
    differs = []
    for name in PROBLEMS:
        _, trace = fixed_trace(name)
        for tol, cap in tolerances(trace):
            try:
                got = rule(trace, tol, cap)
            except ValueError:                  # the mutant never stops within the trace
                got = None
            if got != loop_ref.stop_sweep(trace, tol, cap):
                differs.append((name, tol))
    assert differs, f"mutant '{mutant}' gives the rule's count on every input"
    if mutant.startswith("the first sweep"):
        assert all(any(n == name and tol == 2.0 for n, tol in differs) for name in PROBLEMS)
    if mutant.startswith("diff >= tol"):
        assert all(any(n == name and tol not in (2.0, 1e-6, 0.0) for n, tol in differs) for name in PROBLEMS)
