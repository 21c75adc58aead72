"""Timings of the fp64 sub-sample (resnmtf_fp64_subsample), the fp64 relevance (resnmtf_fp64_relevance) and of stability
selection in double precision, on one GPU.

    python tools/time_fp64_stability.py [--part subsample|once|relevance|pipeline] [--quick] [--big] [--out profiles/time_fp64_stability.jsonl]

subsample: 10000 x 2000 (--quick: 2000 x 500; --big: 50000 x 8000 as well), sample_rate 0.9.  Per shape the median of 5
           blocking calls after a warm-up, all in this session, of engine.fp64_subsample from an fp64 column-major device
           tensor, a row-major one and a host array, beside
             a device-to-device copy of the destination's n_sub m_sub doubles (torch's copy_, a hipMemcpyDtoD), synchronised,
             the f32 route: Engine.subsample_view_from into a probe handle + Engine.empty_lines.
           GB/s are destination bytes (8 n_sub m_sub) over the median.
once:      three sub-samples from the column-major tensor, three from the row-major one, and three
           engine.fp64_shuffle(normalise=False) of an array of the sub-sample's size: the run to put under a kernel trace,
           whose per-kernel sums give the split into gather, row sums and column sums, and the column sums beside
           fp64_shuffle_lines_kernel on the same extent (section 27's open item)
             rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_fp64_stability.py --part once
           (a run of its own: tracing slows the host, so no call time is taken from it).
relevance: engine.fp64_relevance against Engine.relevance at c2's sub-sample size (9000 x 1800 of 10000 x 2000, k = 16).
pipeline:  stability_check at c2 (one view 10000 x 2000, k = 16, n_stability = 5, n_iters = 200; --quick: 2000 x 500)
           under precision="fp64" against the f32 route, one timed call each after a warm-up call of both.
           The fp64 call's time is split by wrapping its four blocking steps with wall-clock timers for that one call: the
           one copy of the host view to the device, the sub-samples (probes), the fits and the scorings.
Prints one JSON line per measurement and writes them to --out, where they replace the earlier records of the same part
(the records of the other parts stay)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd import api, batched, engine, naming  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def median_ms(fn, reps=5):
    fn()                                                           # warm-up (code objects, allocator)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                       # blocking
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3), round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)


def raw(n, m, seed=3):
    rng = np.random.default_rng(seed)
    return rng.random((n, m)) * rng.uniform(0.5, 50.0, size=(1, m)) + 0.01


def draw(n, m, rate=0.9, seed=1):
    rng = np.random.default_rng(seed)
    return rng.choice(n, int(n * rate), replace=False), rng.choice(m, int(m * rate), replace=False)


def subsample_part(quick, big):
    import torch
    dev = torch.device("cuda", 0)
    shapes = [(2000, 500)] if quick else [(10000, 2000)] + ([(50000, 8000)] if big else [])
    for n, m in shapes:
        x = raw(n, m)
        rows, cols = draw(n, m)
        ns, ms = len(rows), len(cols)
        col = torch.as_tensor(x, device=dev).t().contiguous().t()
        row = torch.as_tensor(x, device=dev).contiguous()
        src = torch.empty((ms, ns), dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        gb = 8.0 * ns * ms / 1e9

        def dtod():
            dst.copy_(src)
            torch.cuda.synchronize()
        rec = {"part": "subsample", "n": n, "m": m, "n_sub": ns, "m_sub": ms, "destination_gb": round(gb, 4),
               "columns": "median, min, max ms of 5 blocking calls after a warm-up",
               "forms": [engine.fp64_subsample_plan(*t.stride())["gather"] for t in (col, row)],
               "fp64_col_major_ms": median_ms(lambda: engine.fp64_subsample(col, rows, cols)),
               "fp64_row_major_ms": median_ms(lambda: engine.fp64_subsample(row, rows, cols)),
               "fp64_host_ms": median_ms(lambda: engine.fp64_subsample(x, rows, cols), reps=3 if n * m > 10 ** 8 else 5),
               "dtod_copy_ms": median_ms(dtod)}
        with Engine([n], [m], [2]) as base:
            base.set_view(0, x)

            def f32_route():
                with Engine([ns], [ms], [2]) as probe:
                    probe.subsample_view_from(0, base, 0, rows, cols)
                    return probe.empty_lines(0)

            def f32_gather_only(live):
                live.subsample_view_from(0, base, 0, rows, cols)
                return live.empty_lines(0)
            rec["f32_probe_engine_ms"] = median_ms(f32_route)
            with Engine([ns], [ms], [2]) as live:
                rec["f32_gather_and_lines_ms"] = median_ms(lambda: f32_gather_only(live))
        for key in [k for k in rec if k.endswith("_ms")]:
            rec[key.replace("_ms", "_gb_per_s")] = round(gb / (rec[key][0] / 1e3), 2)
        emit(rec)


def once_part(quick):
    import torch
    dev = torch.device("cuda", 0)
    n, m = (2000, 500) if quick else (10000, 2000)
    x = raw(n, m)
    rows, cols = draw(n, m)
    col = torch.as_tensor(x, device=dev).t().contiguous().t()
    row = torch.as_tensor(x, device=dev).contiguous()
    same = torch.as_tensor(x[:len(rows), :len(cols)], device=dev).t().contiguous().t()
    for _ in range(3):                                             # (the trace holds three calls of each: divide its sums)
        engine.fp64_subsample(col, rows, cols)
    for _ in range(3):
        engine.fp64_subsample(row, rows, cols)
    for _ in range(3):
        engine.fp64_shuffle(same, 7, normalise=False)
    emit({"part": "once", "n": n, "m": m, "n_sub": len(rows), "m_sub": len(cols), "calls_of_each": 3})


def relevance_part(quick):
    import torch
    dev = torch.device("cuda", 0)
    n, m = (2000, 500) if quick else (10000, 2000)
    k = 16
    rows, cols = draw(n, m)
    ns, ms = len(rows), len(cols)
    rng = np.random.default_rng(5)
    rc_ref, cc_ref = (rng.random((n, k)) < 0.1).astype(np.float64), (rng.random((m, k)) < 0.1).astype(np.float64)
    f, g, s = rng.random((ns, k)) ** 3 + 1e-3, rng.random((ms, k)) ** 3 + 1e-3, rng.random((k, k)) + np.eye(k)
    with Engine([n], [m], [2]) as ref, Engine([ns], [ms], [k]) as eng:
        ref.set_reference_clusters(0, rc_ref, cc_ref)
        eng.set_factors(0, f, s, g)
        _, _, _, rc, cc = eng.finalise(0)
        t_rc, t_cc = torch.as_tensor(rc, device=dev), torch.as_tensor(cc, device=dev)
        t_rr, t_cr = torch.as_tensor(rc_ref, device=dev), torch.as_tensor(cc_ref, device=dev)
        a = eng.relevance(0, ref, 0, rows, cols)
        b = engine.fp64_relevance(t_rc, t_cc, t_rr, t_cr, rows, cols)
        emit({"part": "relevance", "n": n, "m": m, "n_sub": ns, "m_sub": ms, "k": k, "equal_bits": a.tobytes() == b.tobytes(),
              "columns": "median, min, max ms of 5 blocking calls after a warm-up",
              "f32_handle_relevance_ms": median_ms(lambda: eng.relevance(0, ref, 0, rows, cols)),
              "fp64_relevance_device_reference_ms": median_ms(lambda: engine.fp64_relevance(t_rc, t_cc, t_rr, t_cr, rows, cols)),
              "fp64_relevance_host_reference_ms": median_ms(lambda: engine.fp64_relevance(t_rc, t_cc, rc_ref, cc_ref, rows, cols))})


def pipeline_part(quick, n_iters):
    n, m = (2000, 500) if quick else (10000, 2000)
    k, seed = 16, 3
    data = naming.check_data([raw(n, m, 1)])
    p = api.prepare(data, None, None, None, None, None, normalise=False, symmetrise=True)
    common = dict(k_vec=[k], phi=p.phi, xi=p.xi, psi=p.psi, spurious=False, row_names=p.row_names, col_names=p.col_names, seed=seed)
    res64 = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, n_iters=n_iters, precision="fp64", **common)
    res32 = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, n_iters=n_iters, **common)

    def check(res, n_it, **more):
        return api.stability_check(p.data, res, k, p.phi, p.xi, p.psi, n_it, False, 5, False, "euclidean", 0.9, 5, 0.4, False,
                                   row_names=p.row_names, col_names=p.col_names, seed=seed, **more)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return round((time.perf_counter() - t0) * 1e3, 1), out
    check(res64, 2, precision="fp64"); check(res32, 2)                                       # warm-up of both routes
    spent = {}

    def clocked(owner, name, key):                 # (every wrapped step blocks until its device work is done)
        inner = getattr(owner, name)

        def wrapper(*args, **kw):
            t0 = time.perf_counter()
            try:
                return inner(*args, **kw)
            finally:
                spent[key] = spent.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
        setattr(owner, name, wrapper)
        return lambda: setattr(owner, name, inner)
    undo = [clocked(engine, "fp64_device_view", "source_copy_ms"), clocked(engine, "fp64_subsample", "subsamples_ms"),
            clocked(batched, "fit_fp64_on_device", "fits_ms"), clocked(engine, "fp64_relevance", "scorings_ms")]
    t64, out64 = timed(lambda: check(res64, n_iters, precision="fp64"))
    for put_back in undo:
        put_back()
    t32, out32 = timed(lambda: check(res32, n_iters))
    emit({"part": "pipeline", "n": n, "m": m, "views": 1, "k": k, "n_stability": 5, "n_iters": n_iters, "stability_check_fp64_ms": t64,
          "fp64_split_ms": {key: round(val, 1) for key, val in spent.items()}, "stability_check_f32_ms": t32, "mean_relevance_fp64": round(float(out64["relevance"].mean()), 4),
          "mean_relevance_f32": round(float(out32["relevance"].mean()), 4), "columns": "one call each, after a warm-up of both routes"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="subsample", choices=["subsample", "once", "relevance", "pipeline"])
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--n-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_stability.jsonl"))
    a = ap.parse_args()
    if a.part == "subsample":
        subsample_part(a.quick, a.big)
    elif a.part == "once":
        once_part(a.quick)
    elif a.part == "relevance":
        relevance_part(a.quick)
    else:
        pipeline_part(a.quick, a.n_iters)
    if a.part != "once":                        # the records of this part replace the file's earlier ones of the same part
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        kept = []
        if os.path.exists(a.out):
            kept = [ln for ln in open(a.out).read().splitlines() if ln.strip() and json.loads(ln).get("part") != a.part]
        with open(a.out, "w") as fh:
            fh.write("\n".join(kept + LINES) + "\n")


if __name__ == "__main__":
    main()
