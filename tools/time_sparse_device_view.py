"""Wall times of a sparse upload from device memory against the host route, on one GPU.

    python tools/time_sparse_device_view.py [--quick] [--out FILE]

For a sparse fp32 matrix that lies in device memory as a torch tensor, medians of 5 calls after a warm-up call, wall time
with ``torch.cuda.synchronize()`` before and after:
* ``Engine.set_view_sparse_device(t)`` -- the device route;
* what a caller had to do before it: the tensor's arrays ``.cpu()``, a ``scipy.sparse.csc_matrix`` of them,
  ``Engine.set_view_sparse`` (its canonical copy, the host checks, the host CSR, the upload).
Both normalise (``pre_processed=False``) into an open engine with k = 16.  Cases: c2's shape (10000 x 2000) at 1 % and 5 %,
and 200000 x 20000 at 0.5 % (20 M entries; ``--quick`` skips it); each as a CSC tensor in canonical order (the device
route's fast path: one sort) and as a COO tensor in random order (two sorts).  Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd.engine import Engine  # noqa: E402

DEV = torch.device("cuda", 0)


def random_entries(n, m, density, seed):
    """(rows, cols, values, column pointers) on the device, canonical CSC order: about density n m distinct positions,
    one per column at least, fp32 values in [0.05, 1.05)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    keys = torch.randint(0, n * m, (int(density * n * m),), device=DEV, generator=g, dtype=torch.int64)
    cols = torch.arange(m, device=DEV, dtype=torch.int64)
    keys = torch.unique(torch.cat([keys, cols * n + cols % n]))           # sorted: column-major positions c n + r
    rows, cols = keys % n, keys // n
    ccol = torch.zeros(m + 1, dtype=torch.int64, device=DEV)
    ccol[1:] = torch.cumsum(torch.bincount(cols, minlength=m), 0)
    vals = torch.rand(keys.numel(), device=DEV, generator=g, dtype=torch.float32) + 0.05
    return rows, cols, vals, ccol


def median_time(fn, reps=5):
    fn()                                               # warm-up: library load, first launches, allocations
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times))


def emit(rec, out):
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def time_case(n, m, density, out):
    rows, cols, vals, ccol = random_entries(n, m, density, 3)
    nnz = int(vals.numel())
    perm = torch.randperm(nnz, device=DEV)
    tensors = {"CSC, canonical order (one sort)": torch.sparse_csc_tensor(ccol, rows, vals, (n, m)),
               "COO, random order (two sorts)": torch.sparse_coo_tensor(torch.stack([rows[perm], cols[perm]]), vals[perm], (n, m),
                                                                         is_coalesced=True)}
    with Engine([n], [m], [16], nnz=[nnz]) as eng:
        for name, t in tensors.items():

            def host_route():
                if t.layout == torch.sparse_csc:
                    x = sp.csc_matrix((t.values().cpu().numpy(), t.row_indices().cpu().numpy(), t.ccol_indices().cpu().numpy()), shape=(n, m))
                else:
                    idx = t._indices().cpu().numpy()
                    x = sp.csc_matrix(sp.coo_matrix((t._values().cpu().numpy(), (idx[0], idx[1])), shape=(n, m)))
                eng.set_view_sparse(0, x, pre_processed=False)

            dev = median_time(lambda: eng.set_view_sparse_device(0, t, pre_processed=False))
            hst = median_time(host_route)
            emit({"case": f"{n} x {m} at {100 * density:g} %", "input": name, "nnz": nnz, "device_s": dev[0], "device_min_max_s": dev[1:],
                  "host_route_s": hst[0], "host_route_min_max_s": hst[1:], "ratio": hst[0] / dev[0]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    for n, m, density in ((10000, 2000, 0.01), (10000, 2000, 0.05)) + (() if a.quick else ((200000, 20000, 0.005),)):
        time_case(n, m, density, a.out)


if __name__ == "__main__":
    main()
