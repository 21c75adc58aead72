"""Timings of the fp64 shuffle (resnmtf_fp64_shuffle) and of spurious-bicluster removal in double
precision, on one GPU.

    python tools/time_fp64_spurious.py [--part shuffle|once|pipeline] [--quick] [--big] [--out profiles/time_fp64_spurious.jsonl]

shuffle:   10000 x 2000 (--quick: 2000 x 500; --big: 50000 x 8000 as well).  Per shape the median of 5 blocking calls after
           a warm-up, all in this session, of engine.fp64_shuffle(normalise=True) from an fp64 column-major device tensor,
           a row-major one and a host array, beside
             a device-to-device copy of n m doubles (torch's copy_, a hipMemcpyDtoD), synchronised,
             Engine.shuffle_view_from into a handle (the f32 route: gather of the fp32 image, statistics, both images),
             the host route: a NumPy permutation of the entries + naming.check_data + the upload of n m doubles.
           GB/s are destination bytes (8 n m) over the median.
once:      one warm-up and two calls from the column-major tensor: the run to put under a kernel trace, whose per-kernel
           sums give the split into gather, lines, statistics and division
             rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_fp64_spurious.py --part once
           (a run of its own: tracing slows the host, so no call time is taken from it).
pipeline:  remove_spurious at c2's shape (two views of 10000 x 2000; --quick: 2000 x 500), k = 16, R = 5, every fit
           guarded by --max-iters sweeps: precision="fp64" against the f32 route, one timed call each after the result
           they start from, and the share of the fp64 call spent in the shuffled fits (problem.shuffled_fits_fp64 alone).
Prints one JSON line per measurement and writes them to --out (appending with --append)."""
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
from resnmtf_amd import api, engine, naming, problem  # noqa: E402
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
    return rng.random((n, m)) * rng.uniform(0.5, 50.0, size=(1, m)) - 0.1      # a few negative entries in every column


def shuffle_part(quick, big):
    import torch
    dev = torch.device("cuda", 0)
    shapes = [(2000, 500)] if quick else [(10000, 2000)] + ([(50000, 8000)] if big else [])
    for n, m in shapes:
        x = raw(n, m)
        col = torch.as_tensor(x, device=dev).t().contiguous().t()
        row = torch.as_tensor(x, device=dev).contiguous()
        dst = torch.empty_like(col)
        gb = 8.0 * n * m / 1e9

        def dtod():
            dst.copy_(col)
            torch.cuda.synchronize()

        def host_route():
            perm = np.random.default_rng(1).permutation(n * m)
            y = naming.check_data([x.reshape(-1)[perm].reshape((n, m), order="F")])[0]
            t = torch.as_tensor(np.asfortranarray(y), device=dev)
            torch.cuda.synchronize()
            return t
        rec = {"part": "shuffle", "n": n, "m": m, "destination_gb": round(gb, 4),
               "columns": "median, min, max ms of 5 blocking calls after a warm-up",
               "fp64_col_major_ms": median_ms(lambda: engine.fp64_shuffle(col, 7)),
               "fp64_row_major_ms": median_ms(lambda: engine.fp64_shuffle(row, 7)),
               "fp64_host_ms": median_ms(lambda: engine.fp64_shuffle(x, 7)),
               "fp64_col_major_draw_only_ms": median_ms(lambda: engine.fp64_shuffle(col, 7, normalise=False)),
               "dtod_copy_ms": median_ms(dtod)}
        with Engine([n], [m], [2]) as base, Engine([n], [m], [2]) as e:
            base.set_view(0, x)
            rec["f32_engine_ms"] = median_ms(lambda: e.shuffle_view_from(0, base, 0, seed=7, normalise=True))
        rec["host_numpy_ms"] = median_ms(host_route, reps=3 if n * m > 10 ** 8 else 5)
        for key in [k for k in rec if k.endswith("_ms")]:
            rec[key.replace("_ms", "_gb_per_s")] = round(gb / (rec[key][0] / 1e3), 2)
        emit(rec)


def once_part(quick):
    import torch
    n, m = (2000, 500) if quick else (10000, 2000)
    col = torch.as_tensor(raw(n, m), device=torch.device("cuda", 0)).t().contiguous().t()
    for _ in range(3):                                             # (the trace holds three calls: divide its sums)
        engine.fp64_shuffle(col, 7)
    emit({"part": "once", "n": n, "m": m, "calls": 3})


def pipeline_part(quick, max_iters):
    n, m = (2000, 500) if quick else (10000, 2000)
    k, R, seed = 16, 5, 3
    data = naming.check_data([np.abs(raw(n, m, 1)), np.abs(raw(n, m, 2))])
    p = api.prepare(data, None, None, None, None, None, normalise=False, symmetrise=True)
    common = dict(k_vec=[k, k], phi=p.phi, xi=p.xi, psi=p.psi, spurious=False, row_names=p.row_names, col_names=p.col_names,
                  seed=seed, max_iters=max_iters)
    res64 = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, precision="fp64", **common)
    res32 = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, **common)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return round((time.perf_counter() - t0) * 1e3, 1)
    problem.shuffled_fits_fp64(p.data, k, 2, seed, max_iters=2)                              # warm-up of both routes
    api.remove_spurious(p.data, res32, 2, seed=seed, max_iters=2)
    t64 = timed(lambda: api.remove_spurious(p.data, res64, R, seed=seed, max_iters=max_iters, precision="fp64"))
    fits = timed(lambda: problem.shuffled_fits_fp64(p.data, k, R, seed, max_iters=max_iters))
    t32 = timed(lambda: api.remove_spurious(p.data, res32, R, seed=seed, max_iters=max_iters))
    emit({"part": "pipeline", "n": n, "m": m, "views": 2, "k": k, "R": R, "max_iters": max_iters, "remove_spurious_fp64_ms": t64,
          "shuffled_fits_fp64_ms": fits, "share_of_the_shuffled_fits": round(fits / t64, 3), "remove_spurious_f32_ms": t32,
          "columns": "one call each, after a warm-up of both routes"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="shuffle", choices=["shuffle", "once", "pipeline"])
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--max-iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_spurious.jsonl"))
    a = ap.parse_args()
    if a.part == "shuffle":
        shuffle_part(a.quick, a.big)
    elif a.part == "once":
        once_part(a.quick)
    else:
        pipeline_part(a.quick, a.max_iters)
    if a.part != "once":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
