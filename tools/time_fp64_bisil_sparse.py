"""Timings of the fp64 bisilhouette of sparse views (resnmtf_fp64_bisil_sparse) beside the dense
fp64 scorer on the densified view and the f32 engine's sparse scorer, on one GPU.

    python tools/time_fp64_bisil_sparse.py [--part calls|big] [--quick] [--reps 5] [--out profiles/time_fp64_bisil_sparse.jsonl]

calls:  c2's shape (10000 x 2000; --quick: 2000 x 500) at 1 % and 5 % stored, k = 3 and k = 8 planted blocks with some rows
        in two biclusters (time_fp64_bisil.py's `planted`, thinned to the stored share), euclidean and cosine.  Per case the
        median of `reps` blocking calls after a warm-up, all in this session, of
          engine.fp64_bisil_sparse from the host CSC (scipy.sparse) -- checked, CSR built and both copies uploaded per call,
          engine.fp64_bisil_sparse from a sparse_csc tensor on the device -- checked and sorted on the device per call,
          engine.fp64_bisil on the densified fp64 device tensor (row-major) -- what a caller had to do before,
          Engine.bisil_sparse on a handle that holds the view (its fp32 CSC / CSR copies are there already),
        whether the two fp64 results are bitwise equal, the largest |difference| to the f32 engine's silhouettes, and the
        workspace of the sparse call beside that of the dense one.
big:    one row at 200000 x 20000 with 20 M stored entries (1000 per column), k = 8, euclidean, for the three sparse routes
        only (the densified view would be 32 GB), with the workspace bytes.
Prints one JSON line per measurement and writes them to --out (--part big appends)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resnmtf_amd import engine  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402
from time_fp64_bisil import median_ms, planted, workspace_bytes  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def sparse_workspace_bytes(n, m, k, rc, cc, nnz):
    """The sparse call's one buffer, restated from resnmtf_bisil_plan.h: the dense call's regions without a copy of X, the
    two rank tables and the CSC and CSR copies (24 bytes per stored entry plus the pointers)."""
    return workspace_bytes(n, m, k, rc, cc, False) + 8 * ((n + m + 1) // 2 + (m + 1) + (n + 1) + 2 * nnz + 2 * ((nnz + 1) // 2))


def device_csc(xs, dev):
    import torch
    return torch.sparse_csc_tensor(torch.as_tensor(xs.indptr.astype(np.int64), device=dev), torch.as_tensor(xs.indices.astype(np.int64), device=dev),
                                   torch.as_tensor(xs.data, device=dev), xs.shape)


def calls_part(quick, reps):
    import torch
    dev = torch.device("cuda", 0)
    n, m = (2000, 500) if quick else (10000, 2000)
    for density in (0.01, 0.05):
        for k in (3, 8):
            x, rc, cc = planted(n, m, k)
            x = np.where(np.random.default_rng(5).random((n, m)) < density, x, 0.0)
            xs = sp.csc_matrix(x)
            xt, dense = device_csc(xs, dev), torch.as_tensor(x, device=dev)
            with Engine([n], [m], [2], nnz=[xs.nnz]) as e:
                e.set_view_sparse(0, xs, pre_processed=True)
                for metric in ("euclidean", "cosine"):
                    a = engine.fp64_bisil_sparse(xs, rc, cc, metric)
                    d = engine.fp64_bisil(dense, rc, cc, metric)
                    b = e.bisil_sparse(0, rc, cc, metric)
                    emit({"part": "calls", "n": n, "m": m, "stored": density, "nnz": int(xs.nnz), "k": k, "metric": metric,
                          "sparse_host_csc_ms": median_ms(lambda: engine.fp64_bisil_sparse(xs, rc, cc, metric), reps),
                          "sparse_device_csc_ms": median_ms(lambda: engine.fp64_bisil_sparse(xt, rc, cc, metric), reps),
                          "dense_fp64_device_ms": median_ms(lambda: engine.fp64_bisil(dense, rc, cc, metric), reps),
                          "f32_engine_sparse_ms": median_ms(lambda: e.bisil_sparse(0, rc, cc, metric), reps),
                          "columns": f"median, min, max of {reps} blocking calls after a warm-up",
                          "sparse_equals_dense_bitwise": bool(np.array_equal(a[0].view(np.uint64), d[0].view(np.uint64))
                                                              and np.array_equal(a[1].view(np.uint64), d[1].view(np.uint64))),
                          "max_abs_fp64_minus_f32_engine": float(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())),
                          "sparse_workspace_bytes": sparse_workspace_bytes(n, m, k, rc, cc, int(xs.nnz)),
                          "dense_workspace_bytes_device_x": workspace_bytes(n, m, k, rc, cc, False),
                          "dense_x_bytes": 8 * n * m})


def big_part(quick, reps):
    import torch
    dev = torch.device("cuda", 0)
    n, m, per_col, k = (20000, 2000, 100, 8) if quick else (200000, 20000, 1000, 8)
    rng = np.random.default_rng(9)
    step = n // per_col                                            # one stored row in each stretch of `step` rows: distinct, ascending
    rows = (np.arange(per_col, dtype=np.int64) * step)[None, :] + rng.integers(0, step, (m, per_col))
    xs = sp.csc_matrix((rng.random(m * per_col) + 0.01, rows.ravel().astype(np.int32), np.arange(m + 1, dtype=np.int64) * per_col), shape=(n, m))
    del rows
    rl, cl = rng.integers(0, k, n), rng.integers(0, k, m)
    rc, cc = np.eye(k)[rl], np.eye(k)[cl]
    rc[rng.random(n) < 0.05, 0] = 1.0
    xt = device_csc(xs, dev)
    metric = "euclidean"
    rec = {"part": "big", "n": n, "m": m, "nnz": int(xs.nnz), "k": k, "metric": metric,
           "sparse_host_csc_ms": median_ms(lambda: engine.fp64_bisil_sparse(xs, rc, cc, metric), reps),
           "sparse_device_csc_ms": median_ms(lambda: engine.fp64_bisil_sparse(xt, rc, cc, metric), reps)}
    print(json.dumps(rec), flush=True)                              # (progress: the third route follows)
    with Engine([n], [m], [2], nnz=[xs.nnz]) as e:
        e.set_view_sparse(0, xs, pre_processed=True)
        rec["f32_engine_sparse_ms"] = median_ms(lambda: e.bisil_sparse(0, rc, cc, metric), reps)
    rec.update({"columns": f"median, min, max of {reps} blocking calls after a warm-up",
                "sparse_workspace_bytes": sparse_workspace_bytes(n, m, k, rc, cc, int(xs.nnz)), "dense_x_bytes": 8 * n * m,
                "sparse_copies_bytes": 24 * int(xs.nnz) + 8 * (n + m + 2)})
    emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="calls", choices=["calls", "big"])
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_bisil_sparse.jsonl"))
    a = ap.parse_args()
    (calls_part if a.part == "calls" else big_part)(a.quick, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.part == "big" else "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
