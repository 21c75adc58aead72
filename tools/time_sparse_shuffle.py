"""Wall times of device shuffles of sparse views ("Sparse shuffles") on one GPU.

    python tools/time_sparse_shuffle.py [--quick] [--out FILE]

At c2's shape (one 10000 x 2000 view, k = 16), 1 % and 5 % density:
* one device shuffle (Engine.shuffle_view_sparse_from, re-normalised) against the host route -- the same shuffle built
  with NumPy / SciPy from the view's host copy (tests/shuffle_ref.py), normalised and uploaded with set_view_sparse --
  the median of 5 calls each after a warm-up call;
* remove_spurious (num_repeats = 5, shuffled fits guarded at 2000 sweeps) on the sparse view with shuffle_sparse=True
  against the same call on the densified view (--quick skips this part).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from resnmtf_amd import api, sparse, synth  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402
import shuffle_ref  # noqa: E402


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


def time_shuffle(x, density, out):
    n, m = x.shape
    with Engine([n], [m], [16], nnz=[x.nnz]) as src, Engine([n], [m], [16], nnz=[x.nnz]) as dst:
        src.set_view_sparse(0, x, pre_processed=True)
        seeds = iter(range(1, 100))

        def device():
            dst.shuffle_view_sparse_from(0, src, 0, seed=next(seeds))
            dst.empty_lines(0)

        def host():
            s = shuffle_ref.shuffle_csc(x, next(seeds))
            dst.set_view_sparse(0, s, pre_processed=False)

        dev, hst = median_time(device), median_time(host)
    emit({"case": "one shuffle, c2 shape", "density": density, "nnz": int(x.nnz), "device_s": dev[0], "device_min_max_s": dev[1:],
          "host_route_s": hst[0], "host_route_min_max_s": hst[1:], "ratio": hst[0] / dev[0]}, out)


def time_removal(x, density, out):
    res = api.res_nmtf_inner([x], None, None, k_vec=[16], spurious=False, seed=1, n_iters=500)
    dense = x.toarray()
    res_d = api.res_nmtf_inner([dense], None, None, k_vec=[16], spurious=False, seed=1, n_iters=500)
    api.remove_spurious([x], res, 2, seed=9, max_iters=50, shuffle_sparse=True)            # warm-up
    t0 = time.perf_counter()
    a = api.remove_spurious([x], res, 5, seed=0, max_iters=2000, shuffle_sparse=True)
    t_sparse = time.perf_counter() - t0
    api.remove_spurious([dense], res_d, 2, seed=9, max_iters=50)                           # warm-up
    t0 = time.perf_counter()
    b = api.remove_spurious([dense], res_d, 5, seed=0, max_iters=2000)
    t_dense = time.perf_counter() - t0
    emit({"case": "remove_spurious, c2 shape, k = 16, 5 repeats", "density": density, "nnz": int(x.nnz),
          "sparse_s": t_sparse, "densified_s": t_dense, "removed_sparse": int(a["spurious"]["removed"].sum()),
          "removed_densified": int(b["spurious"]["removed"].sum())}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    for density in (0.01, 0.05):
        x = planted_sparse(10000, 2000, density, 3)
        time_shuffle(x, density, a.out)
        if not a.quick:
            time_removal(x, density, a.out)


if __name__ == "__main__":
    main()
