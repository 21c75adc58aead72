"""Timings of the fp64 bisilhouette (resnmtf_fp64_bisil) beside the fp32-image scorer, on one GPU.

    python tools/time_fp64_bisil.py [--part calls|once] [--quick] [--out profiles/time_fp64_bisil.jsonl]

calls:  c2's shape (10000 x 2000; --quick: 2000 x 500), k = 3 and k = 8 planted blocks with some rows in two biclusters,
        euclidean and cosine.  Per case the median of 5 blocking calls after a warm-up, all in this session, of
          engine.fp64_bisil from a device tensor (fp64, row-major) -- no copy of X,
          engine.fp64_bisil from a host array -- X uploaded once per call as n x m doubles,
          Engine.bisil on a handle that holds the view (the fp32 images are there already) on the same clusters,
        the largest |difference| between the fp64 and the fp32-image silhouettes, and the workspace of the fp64 call.
once:   one warm-up and ONE call of engine.fp64_bisil from a device tensor and one of Engine.bisil (k = 3, euclidean):
        the run to put under a kernel trace, whose per-kernel sums give the split into gather, distance and epilogue
          rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_fp64_bisil.py --part once
        (a run of its own: tracing slows the host, so no call time is taken from it).
Prints one JSON line per measurement and writes them to --out."""
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
from resnmtf_amd import engine  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def planted(n, m, k, seed=11):
    """test_gpu_bisil.py's c2 case at any k: planted blocks of height 2 on noise, 5 % of the rows also in bicluster 0."""
    rng = np.random.default_rng(seed)
    rl, cl = rng.integers(0, k, n), rng.integers(0, k, m)
    rc, cc = np.eye(k)[rl], np.eye(k)[cl]
    rc[rng.random(n) < 0.05, 0] = 1.0
    x = 0.2 * rng.random((n, m)) + 2.0 * (np.eye(k)[rl] @ np.eye(k)[cl].T)
    return x, rc, cc


def median_ms(fn, reps=5):
    fn()                                                           # warm-up (code objects, allocator)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                       # blocking: returns after the device-to-host copy
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3), round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)


def workspace_bytes(n, m, k, rc, cc, host_x):
    """The fp64 call's one buffer, restated from resnmtf_bisil_plan.h (G, norms, partials, silhouettes, lists, host X)."""
    active = [l for l in range(k) if rc[:, l].any() and cc[:, l].any()]
    g = part = 1
    upad_max, ints = 64, 0
    for mine, other in ((rc, cc), (cc, rc)):
        n_u = int(mine[:, active].any(axis=1).sum())
        upad = -(-n_u // 64) * 64
        upad_max = max(upad_max, upad)
        ints += n_u + k
        for l in active:
            p = engine.fp64_bisil_plan(n_u, int(mine[:, l].sum()), k)
            g = max(g, int(other[:, l].sum()) * upad)
            part = max(part, p["chunks"] * int(mine[:, l].sum()) * k)
            ints += int(mine[:, l].sum()) + int(other[:, l].sum())
    n_mask = sum(int(mine[:, active].any(axis=1).sum()) for mine in (rc, cc))
    return 8 * (g + upad_max + part + (n + m) * k + n_mask + -(-ints // 2) + (n * m if host_x else 0))


def calls_part(quick):
    import torch
    dev = torch.device("cuda", 0)
    n, m = (2000, 500) if quick else (10000, 2000)
    for k in (3, 8):
        x, rc, cc = planted(n, m, k)
        xt = torch.as_tensor(x, device=dev)
        with Engine([n], [m], [2]) as e:
            e.set_view(0, x)
            for metric in ("euclidean", "cosine"):
                a = engine.fp64_bisil(xt, rc, cc, metric)
                b = e.bisil(0, rc, cc, metric)
                rec = {"part": "calls", "n": n, "m": m, "k": k, "metric": metric,
                       "fp64_device_ms": median_ms(lambda: engine.fp64_bisil(xt, rc, cc, metric)),
                       "fp64_host_ms": median_ms(lambda: engine.fp64_bisil(x, rc, cc, metric)),
                       "f32_image_ms": median_ms(lambda: e.bisil(0, rc, cc, metric)),
                       "columns": "median, min, max of 5 blocking calls after a warm-up",
                       "max_abs_fp64_minus_f32_image": float(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())),
                       "fp64_workspace_bytes_device_x": workspace_bytes(n, m, k, rc, cc, False),
                       "fp64_workspace_bytes_host_x": workspace_bytes(n, m, k, rc, cc, True)}
                emit(rec)


def once_part(quick):
    import torch
    n, m = (2000, 500) if quick else (10000, 2000)
    x, rc, cc = planted(n, m, 3)
    xt = torch.as_tensor(x, device=torch.device("cuda", 0))
    with Engine([n], [m], [2]) as e:
        e.set_view(0, x)
        for _ in range(2):                                         # (the trace holds two calls of each: halve its sums)
            engine.fp64_bisil(xt, rc, cc, "euclidean")
            e.bisil(0, rc, cc, "euclidean")
    emit({"part": "once", "n": n, "m": m, "k": 3, "metric": "euclidean", "calls_of_each": 2})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="calls", choices=["calls", "once"])
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_bisil.jsonl"))
    a = ap.parse_args()
    (calls_part if a.part == "calls" else once_part)(a.quick)
    if a.part == "calls":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
