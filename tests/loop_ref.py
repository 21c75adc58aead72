"""The stop rule of the convergence loop (``R/main.r:50-81``), stated once, on a vector of per-sweep mean errors.

The reference keeps ``err_temp`` (0 before the first sweep, ``:54``); after every sweep it takes ``err_diff = |mean error -
err_temp|`` (``:79``), stores the mean in ``err_temp`` (``:80``) and goes on while ``err_diff > tol`` (``:55``).  The first
sweep is therefore tested too (against 0), and equality stops.  Everything here is plain Python floats: the device forms the
same differences of the same fp64 means, so the stop sweep is an exact function of the trace a run returns.
"""
from __future__ import annotations


def diffs(means):
    """``err_diff`` after every sweep of the trace (entry t - 1 belongs to sweep t)."""
    out, prev = [], 0.0
    for m in means:
        m = float(m)
        out.append(abs(m - prev))
        prev = m
    return out


def stop_sweep(means, tol, max_iters=None) -> int:
    """The number of sweeps the reference's loop runs on this trace: the first sweep t (1-based) with ``not (diff > tol)``,
    else ``max_iters``; raises when the trace ends before either."""
    prev = 0.0
    for t, m in enumerate(means, start=1):
        m = float(m)
        diff = abs(m - prev)
        prev = m
        if not (diff > tol):
            return t
        if max_iters is not None and t >= max_iters:
            return int(max_iters)
    raise ValueError(f"the trace of {len(means)} sweeps ends before the rule stops (tol {tol!r}, max_iters {max_iters!r})")


def record_low_sweeps(means):
    """The sweeps t >= 2 whose ``diff`` is strictly below every earlier one.  With ``tol`` set to exactly that ``diff`` the
    rule stops at t (on equality: the ``>`` edge) and nowhere earlier."""
    d = diffs(means)
    out, low = [], d[0] if d else 0.0
    for t in range(2, len(d) + 1):
        if d[t - 1] < low:
            out.append(t)
            low = d[t - 1]
    return out


def pick_stop(means, lo=6, hi=30):
    """``(t, tol)``: the smallest record-low sweep in ``[lo, hi]`` and its ``diff``.  A trace without one is a condition the
    inputs failed, not a reason to skip: the AssertionError carries the trace, and the case gets another seed."""
    d = diffs(means)
    for t in record_low_sweeps(means):
        if lo <= t <= hi:
            assert stop_sweep(means, d[t - 1]) == t
            return t, d[t - 1]
    raise AssertionError(f"no record-low sweep in [{lo}, {hi}]: diffs {d!r}")
