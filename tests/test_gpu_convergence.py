"""Convergence mode of resnmtf_run pinned exactly: the stop sweep, the frozen state, every launch form.

The stop test of ``resnmtf_run(n_iters = 0, tol, max_iters)`` (R/main.r:50-81) runs on the device, in the k x k job of the
last view; the host looks at the flag only between batches of ``check_every`` sweeps, and every kernel of the sweeps already
enqueued behind the stop must leave at once.  The error trace is fp64 and the host's mean is the device's sum in the
device's order, so nothing here needs a tolerance -- every comparison is ``np.array_equal``:

* the stop sweep is ``loop_ref.stop_sweep`` of the trace the run returns;
* the state after a converged run is, bit for bit, the state after that many FIXED sweeps -- the factors, and (through five
  more sweeps on the same handle) the hidden state the resume path trusts: X.G slabs, F coefficients, Gram partials;
* a second convergence run on the same handle restarts the rule from ``prev = 0`` and continues the trace.

Protocol per (case, variant): engine A runs 40 fixed sweeps and ``loop_ref.pick_stop`` chooses a sweep t* in [6, 30] whose
``diff`` is a strict record low, and ``tol`` = exactly that diff (the run stops at t* on EQUALITY and nowhere earlier);
engine B runs t* fixed sweeps, then 5 more; engine C runs the variant.  The variants place the stop on a chosen sweep of a
batch (sweep 1 goes out eagerly, then batches of ``check_every``): inside one graph launch (``mid``), with plain launches
(``eager``), on the last sweep of a batch, on the first of the next, with a host check after every sweep, on the eager first
sweep (``tol = 2``: errors lie in [0, 1]) and never (``tol = 0`` under ``max_iters = 37`` = 1 + 32 + 4: the ladder remainder).

The cases are those of test_gpu_sweep_elementwise (same shapes and options, hence the same launch plans) plus three with
``fuse_updates``.  WARM: ``pick_stop`` is a condition on the inputs, and ten cases do not meet it from their random start --
their traces have a plateau at sweeps 2 - 4 (diff down to 1e-7, or 3e-11 for chain4_one_slab) before the descent begins, a
record low that nothing within 40 sweeps beats.  Those cases start instead from the raw state (F, S, G, lambda, mu) the
device reaches after WARM[case] fixed sweeps, uploaded through set_factors like any initial factors; the number comes from
the fp64 oracle's trace of the case (the smallest start with at least six record lows in [6, 30]), not from the device.
"""
import numpy as np
import pytest

import loop_ref
from resnmtf_amd import synth
from test_gpu_sweep_elementwise import CASES, CASE_IDS, _engine, dense, form_of

pytestmark = pytest.mark.gpu

N_FIXED = 40               # sweeps of engine A that pick_stop looks at
N_TRACE = 80               # ... and of its whole trace (the second convergence run is predicted from it)
MORE = 5
CAP = 37                   # 1 eager sweep + one batch of 32 + 4 off the ladder

BASE_CASES = ["k3_plain", "k16_modeB", "k8_pingpong", "tiny_13x63",
              "k17_wide", "k32_wide", "k64_wide", "k40_f32mfma", "k32_modeA",
              "half1_default", "half2_u3", "half3_guard_fail",
              "sparse_k8", "sparse_k40", "sparse_counts_129x64",
              "chain2_slabs", "chain4_one_slab", "chain3_no_f_chain",
              "coupled_partial_na", "coupled_k40_restricted", "zero_rows_coupled"]
FUSED_CASES = {      # id -> (problem factory, engine options, sweeps before, sparse upload), as a row of CASES
    "fuse1_700x300_k7": (lambda: dense(700, 300, 7, 0), {"fuse_updates": 1}, 0, False),
    "fuse2_700x300_k7": (lambda: dense(700, 300, 7, 0), {"fuse_updates": 2}, 0, False),
    "fuse1_phi_pair_k6": (lambda: synth.make_problem([(300, 200), (300, 170)], 6, phi=1.0), {"fuse_updates": 1}, 0, False),
}
ALL_SEVEN = ["k3_plain", "k32_wide", "sparse_k8", "chain2_slabs"]
BASE_VARIANTS = ["mid", "eager", "first_sweep", "cap"]
EXTRA_VARIANTS = ["last_of_batch", "first_of_next", "every"]
WARM = {"k32_wide": 12, "k64_wide": 19, "k32_modeA": 11, "k40_f32mfma": 8, "chain2_slabs": 5, "chain4_one_slab": 16,
        "chain3_no_f_chain": 7, "coupled_partial_na": 8, "coupled_k40_restricted": 11, "zero_rows_coupled": 4}

PARAMS = [(c, v) for c in BASE_CASES + list(FUSED_CASES) for v in BASE_VARIANTS] + \
         [(c, v) for c in ALL_SEVEN for v in EXTRA_VARIANTS]
PASSED, FAILED = {}, set()         # case id -> variants that passed / cases with a failed variant
PICKED = {}                        # case id -> (t*, tol): printed by test_cases_cover_every_form (pytest -s)


def _case(cid):
    if cid in FUSED_CASES:
        return FUSED_CASES[cid]
    return CASES[CASE_IDS.index(cid)][1:]


def state_of(e):
    return [e.get_factors(v) for v in range(e.n_views)]


def same_state(a, b):
    return all(np.array_equal(x, y) for va, vb in zip(a, b) for x, y in zip(va, vb))


class Reference:
    """Everything the variants of one case share: the problem, engine A's trace and the states of the fixed runs."""

    def __init__(self, cid):
        make, self.opts, _, self.sparse = _case(cid)
        self.prob = make()
        self.n_v = len(self.prob.data)
        self.warm = None
        if cid in WARM:
            e = _engine(self.prob, self.sparse, self.opts)
            try:
                e.run(WARM[cid])
                self.warm = state_of(e)
            finally:
                e.close()
        a = self.engine()
        try:
            first = a.run(N_FIXED)
            self.view_errs = [a.view_errors(v, 0, N_FIXED) for v in range(self.n_v)]
            self.errs = np.concatenate([first, a.run(N_TRACE - N_FIXED)])
            self.plans = [a.view_plan(v) for v in range(self.n_v)]
        finally:
            a.close()
        self.t, self.tol = loop_ref.pick_stop(self.errs[:N_FIXED])
        PICKED[cid] = (self.t, self.tol)
        self.fixed = {}

    def engine(self, **extra):
        e = _engine(self.prob, self.sparse, {**self.opts, **extra})
        if self.warm is not None:
            for v, (f, s, g, lam, mu) in enumerate(self.warm):
                e.set_factors(v, f, s, g, lam, mu)
        return e

    def after(self, n, more=0):
        """(state after a fresh run(n), state after run(more) on the same handle), default options, computed once."""
        if (n, more) not in self.fixed:
            b = self.engine()
            try:
                errs = b.run(n)
                assert np.array_equal(errs, self.errs[:n])
                first = state_of(b)
                second = None
                if more:
                    assert np.array_equal(b.run(more), self.errs[n:n + more])
                    second = state_of(b)
            finally:
                b.close()
            self.fixed[(n, more)] = (first, second)
        return self.fixed[(n, more)]


_REFS = {}


def reference(cid):
    if cid not in _REFS:
        _REFS.clear()                  # (one case's states at a time: the parameters come case by case)
        _REFS[cid] = Reference(cid)
    return _REFS[cid]


def variant_options(variant, t):
    return {"mid": dict(check_every=32), "eager": dict(use_graph=False), "last_of_batch": dict(check_every=t - 1),
            "first_of_next": dict(check_every=t - 2), "every": dict(check_every=1), "first_sweep": {}, "cap": {}}[variant]


def check_converged(ref, c, errs, t, tol):
    """Protocol step 3 up to the factors: a converged run of engine c that must have stopped at sweep t."""
    assert len(errs) == t == loop_ref.stop_sweep(errs, tol), (len(errs), t)
    assert np.array_equal(errs, ref.errs[:t])
    assert c.loop_state() == (t, True, t)
    for v in range(ref.n_v):
        assert np.array_equal(c.view_errors(v, 0, t), ref.view_errs[v][:t]), f"per-view errors of view {v}"


def run_variant(cid, variant):
    ref = reference(cid)
    t, tol = ref.t, ref.tol
    if variant == "first_sweep":
        # the stop is on the eager sweep: the whole first batch does nothing; a second convergence run stops at once again
        at1, at5 = ref.after(1, 4)
        c = ref.engine()
        try:
            errs = c.run(None, tol=2.0, max_iters=N_FIXED)
            check_converged(ref, c, errs, 1, 2.0)
            assert same_state(state_of(c), at1)
            assert np.array_equal(c.run(4), ref.errs[1:5])
            assert same_state(state_of(c), at5) and same_state(at5, ref.after(5)[0])
            assert np.array_equal(c.run(None, tol=2.0, max_iters=N_FIXED), ref.errs[5:6])
            assert c.loop_state() == (1, True, 1)
            assert same_state(state_of(c), ref.after(6)[0])
        finally:
            c.close()
        return
    if variant == "cap":
        assert all(d != 0.0 for d in loop_ref.diffs(ref.errs[:CAP]))
        c = ref.engine()
        try:
            errs = c.run(None, tol=0.0, max_iters=CAP)
            assert len(errs) == CAP == loop_ref.stop_sweep(errs, 0.0, CAP)
            assert np.array_equal(errs, ref.errs[:CAP])
            assert c.loop_state() == (CAP, False, 0)
            assert same_state(state_of(c), ref.after(CAP)[0])
        finally:
            c.close()
        return
    opts = variant_options(variant, t)
    at_t, at_t5 = ref.after(t, MORE)
    c = ref.engine(**opts)
    try:
        errs = c.run(None, tol=tol, max_iters=N_FIXED)
        check_converged(ref, c, errs, t, tol)
        assert same_state(state_of(c), at_t), "factors after the converged run"
        assert np.array_equal(c.run(MORE), ref.errs[t:t + MORE]), "five more sweeps on the converged handle"
        assert same_state(state_of(c), at_t5), "state after five more sweeps"
    finally:
        c.close()
    # a second convergence run on the same handle: the rule restarts from prev = 0, the trace continues
    n2 = loop_ref.stop_sweep(ref.errs[t:t + N_FIXED], tol, N_FIXED)
    c = ref.engine(**opts)
    try:
        assert len(c.run(None, tol=tol, max_iters=N_FIXED)) == t
        errs2 = c.run(None, tol=tol, max_iters=N_FIXED)
        assert len(errs2) == n2 == loop_ref.stop_sweep(errs2, tol, N_FIXED), (len(errs2), n2)
        assert np.array_equal(errs2, ref.errs[t:t + n2])
        assert c.loop_state() == ((n2, True, n2) if not (loop_ref.diffs(errs2)[-1] > tol) else (n2, False, 0))
        assert same_state(state_of(c), ref.after(t + n2)[0]), "factors after the second converged run"
    finally:
        c.close()


@pytest.mark.parametrize("cid,variant", PARAMS, ids=[f"{c}-{v}" for c, v in PARAMS])
def test_converged_run_is_the_fixed_run(cid, variant):
    try:
        run_variant(cid, variant)
    except BaseException:
        FAILED.add(cid)
        raise
    ref = reference(cid)
    PASSED.setdefault(cid, {"plans": ref.plans, "opts": ref.opts, "coupled": _is_coupled(ref.prob), "variants": []})
    PASSED[cid]["variants"].append(variant)


def _is_coupled(prob):
    return bool(np.any(prob.phi != 0) or np.any(prob.psi != 0) or np.any(prob.xi != 0))


def test_cases_cover_every_form():
    """The cases that passed reach every launch form whose kernels carry the early exit (read from Engine.view_plan).  A case
    with a failed variant covers nothing; a case not run in this session is read from a fresh engine after one sweep."""
    reached = set()
    for cid in BASE_CASES + list(FUSED_CASES):
        if cid in FAILED:
            continue
        if cid in PASSED:
            info = PASSED[cid]
        else:
            make, opts, _, sparse = _case(cid)
            prob = make()
            e = _engine(prob, sparse, opts)
            try:
                e.run(1)
                info = {"plans": [e.view_plan(v) for v in range(len(prob.data))], "opts": opts, "coupled": _is_coupled(prob)}
            finally:
                e.close()
        plans = info["plans"]
        hoisted = any(p["f_chain_hoisted"] for p in plans)
        for p in plans:
            reached.add(("form", form_of(p)))
            if p["image"] == "f32":
                reached.add(("nt", p["nt"]))
            if p["image"] == "f32" and p["nt"] == 1:
                reached.add(("kk_mode at k <= 16", p["kk_mode"]))
            if p["f_chain_hoisted"]:
                reached.add(("hoisted F chain, views", p["f_chain_views"]))
            if p["nt"] >= 2 and info["coupled"]:
                reached.add(("coupled, k > 16",))
            if info["opts"].get("fuse_updates") and p["image"] == "f32" and p["nt"] == 1 and p["kk_mode"] == 0 and p["waves"] == (8, 8):
                reached.add(("fused updates",))
        if len(plans) > 1 and not hoisted:
            reached.add(("several views, no hoisted chain",))
    want = {("form", f) for f in ("f32", "wide", "f32_mfma", "fp16", "u16", "sparse")}
    want |= {("nt", nt) for nt in (1, 2, 3, 4)}
    want |= {("kk_mode at k <= 16", 0), ("kk_mode at k <= 16", 1)}
    want |= {("hoisted F chain, views", 2), ("hoisted F chain, views", 4)}
    want |= {("several views, no hoisted chain",), ("coupled, k > 16",), ("fused updates",)}
    for cid in sorted(PICKED):
        print(f"{cid}: t* = {PICKED[cid][0]}, tol = {PICKED[cid][1]!r}")
    missing = sorted(str(w) for w in want - reached)
    assert not missing, "forms no passing case reaches: " + ", ".join(missing) + (f"; failed cases: {sorted(FAILED)}" if FAILED else "")


# ---------------------------------------------------------------------------------------------------------------------
# the error ring: 1024 rows of V = 2 per-view errors, indexed (base + t) % capacity by the device and by the host
# ---------------------------------------------------------------------------------------------------------------------
def _ring_problem():
    return synth.make_problem([(60, 40), (50, 40)], 3)


def _fresh(prob, n):
    e = _engine(prob, False, {})
    try:
        errs = e.run(n)
        return errs, state_of(e), [e.view_errors(v, 0, n) for v in range(2)]
    finally:
        e.close()


def test_ring_is_crossed_by_a_resumed_run():
    prob = _ring_problem()
    want, state, per_view = _fresh(prob, 1100)
    e = _engine(prob, False, {})
    try:
        got = np.concatenate([e.run(1000), e.run(100)])
        assert np.array_equal(got, want)
        for v in range(2):
            assert np.array_equal(e.view_errors(v, 0, 100), per_view[v][1000:])
        assert same_state(state_of(e), state)
    finally:
        e.close()


def test_ring_grows_between_two_resumed_runs():
    prob = _ring_problem()
    want, state, _ = _fresh(prob, 1510)
    e = _engine(prob, False, {})
    try:
        got = np.concatenate([e.run(10), e.run(1500)])          # 1500 > 1024: the ring is reallocated, the run resumes
        assert np.array_equal(got, want)
        assert same_state(state_of(e), state)
    finally:
        e.close()


def test_ring_reserved_between_two_resumed_runs():
    prob = _ring_problem()
    want, state, _ = _fresh(prob, 30)
    e = _engine(prob, False, {})
    try:
        first = e.run(10)
        e.reserve_sweeps(3000)
        got = np.concatenate([first, e.run(20)])
        assert np.array_equal(got, want)
        assert same_state(state_of(e), state)
    finally:
        e.close()


def test_convergence_run_behind_a_run_near_the_ring_end():
    prob = _ring_problem()
    n0 = 1020
    want, _, per_view = _fresh(prob, n0 + N_FIXED)
    tail = want[n0:]
    t, tol = loop_ref.pick_stop(tail)
    _, at_t, _ = _fresh(prob, n0 + t)
    _, at_t5, _ = _fresh(prob, n0 + t + MORE)
    e = _engine(prob, False, {})
    try:
        assert np.array_equal(e.run(n0), want[:n0])
        errs = e.run(None, tol=tol, max_iters=N_FIXED)
        assert len(errs) == t == loop_ref.stop_sweep(errs, tol), (len(errs), t)
        assert np.array_equal(errs, tail[:t])
        assert e.loop_state() == (t, True, t)
        for v in range(2):
            assert np.array_equal(e.view_errors(v, 0, t), per_view[v][n0:n0 + t])
        assert same_state(state_of(e), at_t)
        assert np.array_equal(e.run(MORE), want[n0 + t:n0 + t + MORE])
        assert same_state(state_of(e), at_t5)
    finally:
        e.close()
