"""Wall times of device copies and sub-samples of sparse views ("Device copies and sub-samples")
on one GPU.

    python tools/time_sparse_subsample.py [--quick] [--out FILE]

At c2's shape (one 10000 x 2000 view), 1 % and 5 % density, sample rate 0.9, medians of 5 calls after a warm-up call:
* one device sub-sample -- the count, an engine of that capacity, Engine.subsample_view_sparse_from, the masks --
  against the host route: sparse.subsample of the host copy, an engine of its size, set_view_sparse;
* one device copy (Engine.copy_view_sparse_from) against one set_view_sparse of the host copy, into an open engine;
* stability_check (n_stability = 5, n_iters = 200, k = 16) with and without sparse_on_device;
* the k sweep k = 3 ... 8 (batched.k_sweep_on_device, n_iters = 200) with and without it (--quick skips the last two).
Prints one JSON line per measurement."""
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
from resnmtf_amd import api, batched, sparse, synth  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402


def planted_sparse(n, m, density, seed):
    """A planted view (synth.planted_view) with a random `density` of its entries kept, one per column at least."""
    rng = np.random.default_rng(seed)
    x = synth.planted_view(n, m, 8, seed)
    mask = rng.random((n, m)) < density
    mask[rng.integers(0, n, m), np.arange(m)] = True
    return sparse.check_data_one(sp.csc_matrix(np.where(mask, x, 0.0)))


def median_time(fn, reps=5):
    fn()                                               # warm-up: library load, first launches, allocations
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times))


def emit(rec, out):
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def time_entries(x, density, out):
    n, m = x.shape
    k = 16
    draws = iter(np.random.default_rng(s) for s in range(1, 100))
    with Engine([n], [m], [2], nnz=[x.nnz]) as src:
        src.set_view_sparse(0, x, pre_processed=True)

        def lists():
            rng = next(draws)
            return rng.choice(n, int(n * 0.9), replace=False), rng.choice(m, int(m * 0.9), replace=False)

        def device_sub():
            rows, cols = lists()
            with Engine([len(rows)], [len(cols)], [k], nnz=[src.subsample_count_sparse(0, rows, cols)]) as dst:
                dst.subsample_view_sparse_from(0, src, 0, rows, cols)
                dst.empty_lines(0)

        def host_sub():
            rows, cols = lists()
            sub = sparse.subsample(x, rows, cols)[0]
            with Engine([len(rows)], [len(cols)], [k], nnz=[sub.nnz]) as dst:
                dst.set_view_sparse(0, sub, pre_processed=True)

        dev, hst = median_time(device_sub), median_time(host_sub)
        emit({"case": "one sub-sample at rate 0.9, c2 shape", "density": density, "nnz": int(x.nnz), "device_s": dev[0],
              "device_min_max_s": dev[1:], "host_route_s": hst[0], "host_route_min_max_s": hst[1:], "ratio": hst[0] / dev[0]}, out)
        with Engine([n], [m], [k], nnz=[x.nnz]) as dst:
            dev = median_time(lambda: dst.copy_view_sparse_from(0, src, 0))
            hst = median_time(lambda: dst.set_view_sparse(0, x, pre_processed=True))
        emit({"case": "one copy, c2 shape", "density": density, "nnz": int(x.nnz), "device_s": dev[0], "device_min_max_s": dev[1:],
              "host_route_s": hst[0], "host_route_min_max_s": hst[1:], "ratio": hst[0] / dev[0]}, out)


def time_pipeline(x, density, out):
    k = 16
    zero = np.zeros((1, 1))
    res = api.res_nmtf_inner([x], None, None, k_vec=[k], spurious=False, seed=1, n_iters=200)

    def stability(**opt):
        return api.stability_check([x], res, k, zero, zero, zero, 200, False, 5, False, "euclidean", 0.9, 5, seed=3, **opt)

    off, on = median_time(stability), median_time(lambda: stability(sparse_on_device=True))
    emit({"case": "stability_check, n_stability = 5, n_iters = 200, k = 16", "density": density, "nnz": int(x.nnz),
          "host_route_s": off[0], "host_route_min_max_s": off[1:], "device_s": on[0], "device_min_max_s": on[1:],
          "ratio": off[0] / on[0]}, out)
    dev = batched.DeviceData([x], zero, zero, zero, pre_processed=True)
    try:
        off = median_time(lambda: batched.k_sweep_on_device(dev, 3, 8, 200, 1))
        on = median_time(lambda: batched.k_sweep_on_device(dev, 3, 8, 200, 1, sparse_on_device=True))
    finally:
        dev.close()
    emit({"case": "k sweep k = 3 ... 8, n_iters = 200", "density": density, "nnz": int(x.nnz), "host_route_s": off[0],
          "host_route_min_max_s": off[1:], "device_s": on[0], "device_min_max_s": on[1:], "ratio": off[0] / on[0]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    for density in (0.01, 0.05):
        x = planted_sparse(10000, 2000, density, 3)
        time_entries(x, density, a.out)
        if not a.quick:
            time_pipeline(x, density, a.out)


if __name__ == "__main__":
    main()
