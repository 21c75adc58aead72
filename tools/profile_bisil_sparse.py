"""The silhouettes of one sparse view (resnmtf_bisil_sparse) or of its densified copy (resnmtf_bisil), for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_bisil_sparse.py --mode sparse
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_bisil_sparse.py --mode dense

c2's shape (10000 x 2000), k = 16 planted blocks (labels drawn uniformly) of height 2 on U(0, 0.2) noise, of which a
uniformly drawn --density share of the entries is kept.  One warm-up call, then --reps calls per metric; prints one JSON
line per metric with the median wall time of the call (host checks, metadata upload, launches, copy back; blocking).
The two modes hold the same fp32 values and return the same bits: bisil_scatter_kernel + the fill
against bisil_gather_kernel is the only difference in the trace."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd.engine import Engine  # noqa: E402


def planted_sparse(n, m, k, density, seed):
    rng = np.random.default_rng(seed)
    rl = rng.integers(0, k, n); cl = rng.integers(0, k, m)
    x = rng.random((n, m)) * 0.2 + 2.0 * (rl[:, None] == cl[None, :])
    x *= rng.random((n, m)) < density
    return sp.csc_matrix(x), np.eye(k)[rl], np.eye(k)[cl]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("sparse", "dense"), required=True)
    ap.add_argument("--shape", default="10000,2000")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, m = (int(t) for t in a.shape.split(","))
    xs, rc, cc = planted_sparse(n, m, a.k, a.density, 1)
    with Engine([n], [m], [2], nnz=[xs.nnz if a.mode == "sparse" else None]) as eng:
        if a.mode == "sparse":
            eng.set_view_sparse(0, xs, pre_processed=True)
            call = eng.bisil_sparse
        else:
            eng.set_view(0, xs.toarray())
            call = eng.bisil
        for metric in ("euclidean", "manhattan", "cosine"):
            call(0, rc, cc, metric)                              # warm-up
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                rs, cs = call(0, rc, cc, metric)
                ts.append(time.perf_counter() - t0)
            print(json.dumps({"mode": a.mode, "n": n, "m": m, "k": a.k, "nnz": int(xs.nnz), "metric": metric,
                              "wall_ms": 1e3 * float(np.median(ts)), "wall_ms_min": 1e3 * float(np.min(ts)),
                              "row_sil_sum": float(rs.sum()), "col_sil_sum": float(cs.sum())}), flush=True)


if __name__ == "__main__":
    main()
