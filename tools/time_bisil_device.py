"""Wall times of the bisilhouette from cluster tensors (resnmtf_bisil_device) against what a caller
holding cluster tensors had to do before it, on one GPU.

    python tools/time_bisil_device.py [--quick] [--out FILE]

c2's shape (one 10000 x 2000 view) with planted clusters at k = 3 and k = 8, and one c5 view (50000 x 8000) at k = 64
(``--quick`` skips it); euclidean.  The cluster matrices are fp64 column-major tensors on the GPU, as ``finalise_device``
leaves them.  Medians of 5 calls after one warm-up call, wall time with ``torch.cuda.synchronize()`` before and after:
* host route: ``rc.cpu().numpy()``, ``cc.cpu().numpy()``, ``Engine.bisil``, ``bisil.view_score``;
* device route: ``Engine.bisil_device(..., silhouettes=False)`` (the score alone, as ``bisil.score`` asks for it) and
  ``Engine.bisil_device(...)`` (the silhouettes left on the device too).
Both routes must give the same score, which is checked.  Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd import bisil  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402

DEV = torch.device("cuda", 0)


def planted(n, m, k, seed):
    """k planted blocks (labels drawn uniformly) of height 2 on U(0, 0.2) noise, and their cluster matrices
    (tools/time_bisil.py)."""
    rng = np.random.default_rng(seed)
    rl = rng.integers(0, k, n); cl = rng.integers(0, k, m)
    x = rng.random((n, m), dtype=np.float32).astype(np.float64) * 0.2
    for j in range(k):                                          # one block at a time (memory)
        x[np.ix_(rl == j, cl == j)] += 2.0
    return x, np.eye(k)[rl], np.eye(k)[cl]


def median_time(fn, reps=5):
    fn()                                               # warm-up: first launches, allocations
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    plan = [("c2", 10000, 2000, 3), ("c2", 10000, 2000, 8)] + ([] if a.quick else [("c5v1", 50000, 8000, 64)])
    for name, n, m, k in plan:
        x, rc, cc = planted(n, m, k, k)
        trc, tcc = (torch.as_tensor(np.ascontiguousarray(c.T), device=DEV).T for c in (rc, cc))      # column-major
        with Engine([n], [m], [2]) as eng:
            eng.set_view(0, x)
            del x
            scores = {}

            def host_route():
                hr, hc = trc.cpu().numpy(), tcc.cpu().numpy()
                scores["host"] = bisil.view_score(hr, hc, *eng.bisil(0, hr, hc, "euclidean"))

            def device_score():
                scores["device"] = eng.bisil_device(0, trc, tcc, "euclidean", silhouettes=False)[2]

            hst = median_time(host_route)
            dev = median_time(device_score)
            full = median_time(lambda: eng.bisil_device(0, trc, tcc, "euclidean"))
            if scores["host"] != scores["device"]:
                raise SystemExit(f"{name} k={k}: the routes disagree: {scores}")
            rec = {"config": name, "n": n, "m": m, "k": k, "metric": "euclidean", "score": scores["device"],
                   "host_route_ms": 1e3 * hst[0], "host_route_min_max_ms": [1e3 * t for t in hst[1:]],
                   "device_score_ms": 1e3 * dev[0], "device_score_min_max_ms": [1e3 * t for t in dev[1:]],
                   "device_with_silhouettes_ms": 1e3 * full[0], "ratio": hst[0] / dev[0]}
            print(json.dumps(rec), flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
