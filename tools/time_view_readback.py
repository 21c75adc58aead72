"""Wall times of the read-back routes through device memory against the host routes, on one GPU.

    python tools/time_view_readback.py [--quick] [--out FILE]

Medians of 5 calls after a warm-up call, wall time with ``torch.cuda.synchronize()`` before and after:
* dense: ``Engine.get_view_device(0)`` (fp32, row-major and column-major) against what a caller had to do before it,
  ``torch.from_numpy(eng.get_view(0)).cuda()``, at c2's shape (10000 x 2000) and c5's (50000 x 8000; ``--quick`` skips it);
* sparse: ``Engine.get_view_sparse_device(0)`` (csc, int64, fp32) against ``get_view_sparse`` followed by
  ``torch.sparse_csc_tensor(...).cuda()``, at c2's shape with 1 % and 5 % stored;
* reference clusters: ``Engine.set_reference_clusters_device`` of fp64 column-major 0 / 1 tensors (as
  ``finalise_device`` leaves them) against ``set_reference_clusters`` of the downloaded matrices, at c2's and c5's
  (n, m, k).
Prints one JSON line per measurement."""
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


def record(case, call, dev, hst, out, **more):
    emit({"case": case, "call": call, **more, "device_s": dev[0], "device_min_max_s": dev[1:], "host_route_s": hst[0],
          "host_route_min_max_s": hst[1:], "ratio": hst[0] / dev[0]}, out)


def time_dense(name, n, m, out):
    case = f"{name}: {n} x {m}"
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand((n, m), device=DEV, generator=g, dtype=torch.float32) + 0.05
    with Engine([n], [m], [2]) as eng:
        eng.set_view_device(0, x, raw=True)
        del x
        hst = median_time(lambda: torch.from_numpy(eng.get_view(0)).cuda())
        for order, label in (("C", "fp32 row-major"), ("F", "fp32 column-major")):
            buf = eng.get_view_device(0, order=order)          # (the caller's buffer: the copy alone is timed)
            dev = median_time(lambda: eng.get_view_device(0, out=buf))
            fresh = median_time(lambda: eng.get_view_device(0, order=order))
            record(case, "get_view_device", dev, hst, out, output=label, device_with_allocation_s=fresh[0])


def time_sparse(name, n, m, density, out):
    case = f"{name}: {n} x {m}, {100 * density:g} % stored"
    x = sp.random(n, m, density=density, random_state=7, format="csc", dtype=np.float64)
    x.data += 0.05
    with Engine([n], [m], [2], nnz=[x.nnz]) as eng:
        eng.set_view_sparse(0, x, pre_processed=True)

        def host_route():
            c = eng.get_view_sparse(0)
            return torch.sparse_csc_tensor(torch.from_numpy(c.indptr), torch.from_numpy(c.indices.astype(np.int64)),
                                           torch.from_numpy(c.data.astype(np.float32)), size=c.shape).cuda()
        hst = median_time(host_route)
        dev = median_time(lambda: eng.get_view_sparse_device(0))
        record(case, "get_view_sparse_device", dev, hst, out, output="csc int64 fp32", nnz=int(x.nnz))


def time_clusters(name, n, m, k, out):
    case = f"{name}: {n} x {m}, k = {k}"
    g = torch.Generator(device=DEV).manual_seed(9)
    rc, cc = ((torch.rand((k, rows), device=DEV, generator=g) < 0.3).double().T for rows in (n, m))      # column-major
    with Engine([n], [m], [2]) as eng:
        dev = median_time(lambda: eng.set_reference_clusters_device(0, rc, cc))
        hst = median_time(lambda: eng.set_reference_clusters(0, rc.cpu().numpy(), cc.cpu().numpy()))
        record(case, "set_reference_clusters_device", dev, hst, out, input="fp64 column-major")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    shapes = (("c2", 10000, 2000, 16),) + (() if a.quick else (("c5", 50000, 8000, 64),))
    for name, n, m, k in shapes:
        time_dense(name, n, m, a.out)
    for density in (0.01, 0.05):
        time_sparse("c2", 10000, 2000, density, a.out)
    for name, n, m, k in shapes:
        time_clusters(name, n, m, k, a.out)


if __name__ == "__main__":
    main()
