"""Wall times of the bisilhouette silhouettes (resnmtf_bisil) on one GPU.

    python tools/time_bisil.py [--quick] [--out FILE]

c2's shape (one 10000 x 2000 view) with planted clusters at k = 3 ... 8, and one c5 view (50000 x 8000) at k = 64, each
for the three metrics.  The wall time is of Engine.bisil (host checks of the cluster matrices, the metadata upload,
the launches, the copy back; blocking), the median of --reps calls after one warm-up.  The distance terms counted are
sum_k |I_k| n |J_k| + sum_k |J_k| m |I_k| over the active biclusters.  Kernel times: run this under
``rocprofv3 --kernel-trace --stats`` (bisil_dist_kernel dominates).  --quick: c2 at k = 3 and 8 only, c5 euclidean.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd.engine import Engine  # noqa: E402


def planted(n, m, k, seed):
    """k planted blocks (labels drawn uniformly) of height 2 on U(0, 0.2) noise, and their cluster matrices."""
    rng = np.random.default_rng(seed)
    rl = rng.integers(0, k, n); cl = rng.integers(0, k, m)
    x = rng.random((n, m), dtype=np.float32).astype(np.float64) * 0.2
    for j in range(k):                                          # one block at a time (memory)
        x[np.ix_(rl == j, cl == j)] += 2.0
    return x, np.eye(k)[rl], np.eye(k)[cl]


def terms(rc, cc):
    act = (rc.sum(0) > 0) & (cc.sum(0) > 0)
    r, c = rc.sum(0)[act], cc.sum(0)[act]
    return float((r * rc.shape[0] * c).sum() + (c * cc.shape[0] * r).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    metrics = ["euclidean", "manhattan", "cosine"]
    plan = [("c2", 10000, 2000, k, metrics) for k in ((3, 8) if a.quick else range(3, 9))]
    plan.append(("c5v1", 50000, 8000, 64, metrics[:1] if a.quick else metrics))
    lines = []
    for name, n, m, k, mets in plan:
        x, rc, cc = planted(n, m, k, k)
        with Engine([n], [m], [2]) as eng:
            eng.set_view(0, x)
            del x
            for metric in mets:
                eng.bisil(0, rc, cc, metric)                     # warm-up
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    eng.bisil(0, rc, cc, metric)
                    ts.append(time.perf_counter() - t0)
                rec = {"config": name, "n": n, "m": m, "k": k, "metric": metric, "wall_ms": 1e3 * float(np.median(ts)),
                       "wall_ms_min": 1e3 * float(np.min(ts)), "terms": terms(rc, cc)}
                rec["terms_per_s"] = rec["terms"] / (rec["wall_ms"] / 1e3)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
