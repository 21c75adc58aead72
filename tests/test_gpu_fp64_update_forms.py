"""The coupled updates of the fp64 paths checked ENTRY BY ENTRY at 5 to 8 views, on every route a job takes onto the
device.

The cases, their bars and their mutants are in tests/fp64_update_cases.py, which tests/test_fp64_update_cases_host.py
checks without a GPU.  For every case and route: the raw state before the step (the initial factors, or the ``state`` of
ten sweeps of ``fp64_run`` on the host-dense route), exactly ONE sweep from it on the route under test
(``init_f / s / g / lam / mu`` taken from that state, ``output="torch", return_state=True``), the raw state after it.
The reference is one ``update_cases.oracle_sweep`` on the dense views from the same state.  F, G, S, lambda and mu of
every view are compared with ``data_ref.nan_stat``: ``max |got / ref - 1|`` over ``ref > 0`` within the case's bar,
zero where the reference is zero, NaN on both sides or on neither; the sweep's error absolutely at ``FIX_ERR``.

Routes
------
``host_dense``    NumPy views.  The raw state needs ``output="torch"``, which is ``resnmtf_fp64_run_device`` with the data in
                  host memory; the same job through ``resnmtf_fp64_run`` itself (``output="numpy"``) must give the same
                  normalised results bit for bit, which ties that entry to the state compared.
``scipy_sparse``  every view a ``scipy.sparse`` matrix; likewise ``resnmtf_fp64_run_sparse`` against its ``output="torch"``.
``torch_dense``   every view an fp64 tensor on the device; at 8 views bit for bit the host-dense route.
``torch_sparse``  every view a sparse tensor on the device, CSC, CSR and COO in turn, no explicit zero stored; at 8 views
                  bit for bit the ``scipy.sparse`` route.
``mixed``         view v from source v mod 4 of: host dense, scipy.sparse, torch dense, torch sparse -- all four
                  ``F64Source`` values and both error forms (residual and trace) in one job.
``group``         ``group_run`` returns no raw state: the normalised outputs of ``n_iters=1`` against
                  ``oracle.res_nmtf_inner(n_iters=1, init_lam=, init_mu=)`` from the same start, under
                  ``fp64_update_cases.norm_bars``.  Cases beyond ``batched.GROUPED_LIMITS`` (k = 40, 64) are left out by
                  asking the limits.

No entry refuses an input of a case: the NaN-row case (a zero column in X, a zero row in G, mu = 0) runs on all of its
routes and the row is NaN on the device.

Measured on the MI355X (each test prints ``MEASURED case route quantity: value (bar)``); the worst ``max |got / ref - 1|``
per route over all cases, with the bar of that entry:

    route                        F          G          S          lambda     mu         error (absolute, bar 1e-13)
    host_dense, torch_dense      6.7e-16    1.0e-15    1.0e-15    1.1e-15    8.9e-16    3.3e-16
      (bar of that entry)        3.8e-14    2.2e-13    5.0e-13    7.8e-14    1.0e-13
    scipy_sparse, torch_sparse   4.4e-16    4.4e-16    7.8e-16    1.1e-15    6.7e-16    1.1e-16
      (bar of that entry)        3.8e-14    1.8e-13    4.8e-13    8.1e-14    9.9e-14
    mixed                        6.7e-16    6.7e-16    6.7e-16    1.1e-15    6.7e-16    0
      (bar of that entry)        4.9e-14    2.6e-13    5.0e-13    8.1e-14    1.1e-13
    group (normalised outputs)   1.1e-15    1.1e-15    2.0e-15    1.2e-15    8.9e-16    3.3e-16
      (bar of that entry)        1.1e-13    2.6e-13    6.6e-13    8.7e-14    9.9e-14

("worst" is the largest value relative to its bar.)  Nothing is above 2 % of its bar: on every entry of every case the
device is within ten units of 2^-53 of the oracle.  The torch routes gave the bits of their host twins at 8 views and the
entries without device memory the bits of their ``output="torch"`` twins.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import fp64_update_cases as F
import update_cases as U
from data_ref import nan_stat
from oracle import resnmtf_oracle as O
from resnmtf_amd import batched
from resnmtf_amd.engine import fp64_plan, fp64_run, fp64_sparse_plan, group_run
from resnmtf_amd.problem import pair_table
from test_gpu_fp64 import FIX_ERR
from test_gpu_sweep_elementwise import MUTANT_MARGIN

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT_KEYS = ("f", "s", "g", "lambda", "mu")          # the keys of a result, in the order of a state tuple
RESULTS = set()            # (case id, route) that passed
ATTEMPTED = set()          # (case id, route) run in this session (a failed one covers nothing)
_PROBS, _STARTS, _REFS, _RUNS = {}, {}, {}, {}


def _prob(cid):
    if cid not in _PROBS:
        _PROBS[cid] = F.case(cid).make()
    return _PROBS[cid]


def _grouped(cid):
    return F.in_grouped_limits(_prob(cid), batched.GROUPED_LIMITS)


PARAMS = [(cid, route) for cid, route in F.ROUTE_PARAMS if route != "group" or _grouped(cid)]


def _problem(prob, data, start, n_iters):
    return {"data": data, "k": U.ks_of(prob)[0], "init_f": [s[0] for s in start], "init_s": [s[1] for s in start],
            "init_g": [s[2] for s in start], "init_lam": [s[3] for s in start], "init_mu": [s[4] for s in start],
            "phi": prob.phi, "xi": prob.xi, "psi": prob.psi, "row_pairs": pair_table(prob.row_names),
            "col_pairs": pair_table(prob.col_names), "n_iters": n_iters}


def _numpy_state(state):
    return [tuple(np.asarray(t.cpu().numpy(), dtype=np.float64) for t in view) for view in state]


def _start(cid):
    """The raw state the step starts from, the same on every route: the initial factors, or the state after
    ``case.before`` sweeps on the host-dense route."""
    if cid not in _STARTS:
        c, prob = F.case(cid), _prob(cid)
        start = U.initial_state(prob)
        if c.before:
            out = fp64_run(_problem(prob, prob.data, start, c.before), output="torch", return_state=True)
            assert out["iters"] == c.before
            start = _numpy_state(out["state"])
        _STARTS[cid] = start
    return _STARTS[cid]


def _reference(cid):
    """(state after one oracle sweep from the device's start, the sweep's error) -- computed once per case and shared."""
    if cid not in _REFS:
        prob = _prob(cid)
        after = U.oracle_sweep(prob, prob.data, _start(cid))
        _REFS[cid] = (after, F.sweep_error(prob.data, after))
    return _REFS[cid]


# ---- a view as each source hands it over ----
def _torch_sparse(x, turn):
    """The non-zeros of x as a sparse tensor on the device: CSC, CSR, COO by ``turn``; no explicit zero is stored."""
    layout = ("csc", "csr", "coo")[turn % 3]
    there = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)      # noqa: E731
    if layout == "csc":
        m = sp.csc_matrix(x); m.eliminate_zeros(); m.sort_indices()
        return torch.sparse_csc_tensor(there(m.indptr, torch.int64), there(m.indices, torch.int64), there(m.data, torch.float64), x.shape)
    if layout == "csr":
        m = sp.csr_matrix(x); m.eliminate_zeros(); m.sort_indices()
        return torch.sparse_csr_tensor(there(m.indptr, torch.int64), there(m.indices, torch.int64), there(m.data, torch.float64), x.shape)
    m = sp.coo_matrix(x); m.eliminate_zeros()
    return torch.sparse_coo_tensor(there(np.stack([m.row, m.col]), torch.int64), there(m.data, torch.float64), x.shape).coalesce()


def _views(c, prob, route):
    data = [np.asarray(x, dtype=np.float64) for x in prob.data]
    source = {"host_dense": [0] * len(data), "scipy_sparse": [1] * len(data), "torch_dense": [2] * len(data),
              "torch_sparse": [3] * len(data), "mixed": c.sources}[route]
    out, turn = [], 0
    for v, x in enumerate(data):
        if source[v] == 0:
            out.append(x)
        elif source[v] == 1:
            out.append(sp.csc_matrix(x))
        elif source[v] == 2:
            out.append(torch.as_tensor(x, dtype=torch.float64, device=DEV))
        else:
            out.append(_torch_sparse(x, turn)); turn += 1
    return out


def _run(cid, route):
    """One sweep of the case on ``route`` from its start: ``{"state", "err", "out"}`` (kept: the bit-for-bit checks read
    the run of the twin route)."""
    if (cid, route) not in _RUNS:
        c, prob = F.case(cid), _prob(cid)
        pd = _problem(prob, _views(c, prob, route), _start(cid), 1)
        out = fp64_run(pd, output="torch", return_state=True)
        assert out["iters"] == 1 and len(out["all_error"]) == 1
        res = {"state": _numpy_state(out["state"]), "err": float(out["all_error"][0]),
               "out": {key: [t.cpu().numpy() for t in out[key]] for key in OUT_KEYS}, "all_error": out["all_error"]}
        if route in ("host_dense", "scipy_sparse"):         # the entry without device memory, on the same job
            res["plain"] = fp64_run(pd)
        _RUNS[cid, route] = res
    return _RUNS[cid, route]


def _same_bits(a, b, what):
    assert np.asarray(a["all_error"]).tobytes() == np.asarray(b["all_error"]).tobytes(), what
    for key in OUT_KEYS:
        for v, (x, y) in enumerate(zip(a["out"][key] if "out" in a else a[key], b["out"][key] if "out" in b else b[key])):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, key, v)
    if "state" in a and "state" in b:
        for v, (x, y) in enumerate(zip(a["state"], b["state"])):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), (what, "state", v)


def _rows_off(got, ref, bar):
    """The rows of a factor that hold an entry off its bar, a NaN out of place or a non-zero where the reference is zero."""
    got = np.atleast_2d(np.asarray(got, dtype=np.float64)); ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(ref > 0, np.abs(got / ref - 1.0), np.where(np.isnan(ref), 0.0, np.where(got != 0, np.inf, 0.0)))
    bad = ~(dev <= bar) | (np.isnan(got) != np.isnan(ref))
    rows = np.flatnonzero(bad.any(axis=1))
    return f"{rows.size} rows, first {rows[:8].tolist()}"


def _compare(cid, route, got, ref, bars, got_err, ref_err):
    """The statistic of the module docstring over every view and quantity; prints the figures, then asserts."""
    failures, worst = [], {}
    for v in range(len(got)):
        for i, key in enumerate(F.KEYS):
            st, nz, nans = nan_stat(got[v][i], ref[v][i])
            bar = bars[v][key]
            if key not in worst or st / bar > worst[key][0] / worst[key][1]:
                worst[key] = (st, bar)
            if st > bar or nz or nans:
                failures.append(f"view {v} {key}: max |got/ref - 1| = {st:.3e} (bar {bar:.3e}), {nz} non-zero where the reference "
                                f"is zero, {nans} NaN mismatches; {_rows_off(got[v][i], ref[v][i], bar)}")
    for key in F.KEYS:
        print(f"MEASURED {cid} {route} {key}: {worst[key][0]:.3e} ({worst[key][1]:.3e})")
    d_err = 0.0 if (np.isnan(got_err) and np.isnan(ref_err)) else abs(got_err - ref_err)
    print(f"MEASURED {cid} {route} err: {d_err:.3e} ({FIX_ERR:.1e})")
    assert not failures, "\n".join(failures)
    assert np.isnan(got_err) == np.isnan(ref_err) and d_err <= FIX_ERR, f"error {got_err!r} against {ref_err!r}"


@pytest.mark.parametrize("cid,route", PARAMS)
def test_one_sweep_elementwise(cid, route):
    c, prob = F.case(cid), _prob(cid)
    ATTEMPTED.add((cid, route))
    n_v = len(prob.data)
    if route == "group":
        start = _start(cid)
        got = group_run([_problem(prob, prob.data, start, 1)])[0]
        ref = O.res_nmtf_inner(prob.data, [s[0] for s in start], [s[1] for s in start], [s[2] for s in start], prob.phi, prob.xi,
                               prob.psi, row_names=prob.row_names, col_names=prob.col_names, n_iters=1,
                               init_lam=[s[3] for s in start], init_mu=[s[4] for s in start])
        assert got["iters"] == 1
        got_state = [tuple(got[key][v] for key in OUT_KEYS) for v in range(n_v)]
        ref_state = [(ref["output_f"][v], ref["output_s"][v], ref["output_g"][v], ref["lambda"][v], ref["mu"][v]) for v in range(n_v)]
        _compare(cid, route, got_state, ref_state, F.norm_bars(prob), float(got["all_error"][0]), float(ref["All_Error"][0]))
        if c.nan_view is not None:
            assert np.isnan(got["g"][c.nan_view]).all() and not np.isnan(got["f"][c.nan_view]).any()
        RESULTS.add((cid, route))
        return
    run = _run(cid, route)
    after, ref_err = _reference(cid)
    bars = F.case_bars(prob)
    _compare(cid, route, run["state"], after, bars, run["err"], ref_err)
    if c.nan_view is not None:
        g = run["state"][c.nan_view][2]
        assert np.isnan(g[5, :]).all() and np.isnan(g).sum() == g.shape[1], "the NaN row of the unguarded coupled form"
    # a start the host test has not seen (the device's own state after ten sweeps): the mutants of the reference the
    # device was held to are at least MUTANT_MARGIN bars away from it here too
    if c.before and route == "host_dense":
        for v in range(n_v):
            bar = max(bars[v][key] for key in ("f", "g", "s"))
            for name, val in F.all_mutants(prob.data, _start(cid), after, prob, v).items():
                assert val >= MUTANT_MARGIN * bar, f"view {v}: mutant '{name}' gives only {val:.3e} against the bar {bar:.1e}"
    # the documented identities between routes
    if "plain" in run:
        _same_bits(run["plain"], run, (cid, route, "the entry without device memory"))
    if n_v == 8 and route in ("torch_dense", "torch_sparse"):
        twin = "host_dense" if route == "torch_dense" else "scipy_sparse"
        _same_bits(run, _run(cid, twin), (cid, route, "bit for bit the route " + twin))
    RESULTS.add((cid, route))


def test_fp64_update_forms_covered():
    """The cases that count -- every route of theirs that ran has passed; a case not run in this session counts from the
    table -- reach V = 5 .. 8, every coupled count, map kind, source and padded k class, and in a coupled 8-view problem
    more than one product tile, Gram workgroup and slab split (``fp64_plan``)."""
    failed = {cid for cid, route in ATTEMPTED - RESULTS}
    counting = [c for c in F.CASES if c.id not in failed]
    missing = sorted(str(t) for t in F.DEMANDED - F.covered(counting))
    assert not missing, "no passing case reaches: " + ", ".join(missing) + f" (failed: {sorted(failed)})"
    geometry = set()
    for c in counting:
        prob = _prob(c.id)
        if len(prob.data) != 8:
            continue
        k = U.ks_of(prob)[0]
        for v, x in enumerate(prob.data):
            n, m = x.shape
            if v in c.sparse:
                plan = fp64_sparse_plan(sp.csc_matrix(x), k)
                assert plan["kp"] == F.PADDED[k] and plan["xg"][0] >= 1 and plan["xtf"][0] >= 1
                geometry.add(("sparse view", plan["kp"]))
                continue
            plan = fp64_plan(n, m, k)
            assert plan["kp"] == F.PADDED[k]
            assert plan["xg"][0] >= 2 and plan["resid"][0] >= 3, (c.id, v, plan)           # product tiles, 64-row tiles
            if plan["xg"][1] > 1 and plan["xtf"][1] > 1:
                geometry.add(("slab splits on both sides", plan["kp"]))
            if -(-n // F.CONSTANTS["F64_GRAM_ROWS"]) >= 2:
                geometry.add(("two Gram workgroups", plan["kp"]))
            if -(-n // F.CONSTANTS["F64_UPD_ROWS"]) >= 3 and n % F.CONSTANTS["F64_UPD_ROWS"]:
                geometry.add(("three update workgroups, the last ragged", plan["kp"]))
    want = {(what, kp) for kp in (16, 32, 48, 64) for what in ("slab splits on both sides", "two Gram workgroups",
                                                               "three update workgroups, the last ragged", "sparse view")}
    assert want <= geometry, sorted(str(t) for t in want - geometry)
