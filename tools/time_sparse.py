"""Sweep rates and pass times of sparse data views on one GPU.

    python tools/time_sparse.py [--quick] [--huge] [--out FILE]

* c2 shape (10000 x 2000, k = 16) at 0.1 / 1 / 5 / 20 % density: sweeps/s of the sparse view against the dense path on
  the same (densified) matrix, and the per-pass times of both (time_kernels, eager launches);
* the skewed case: c2 shape at 0.1 % plus one row and one column at 60 % (sweep rate and pass times);
* a 200000 x 20000 view at 0.5 % density, k = 16 and k = 64: per-pass time and effective bytes/s (values + indices +
  pointers + gathered factor rows + slabs, resnmtf_pass_timings), and the SVD initialisation at sketch width 64, whose
  products are the same kernels without the k x k job's LDS (compare them in a kernel trace);
* --huge: one 10^6 x 10^5 view at 0.1 % (its dense images would need 800 GB): it factorises at all.
Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resnmtf_amd import synth  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402


def random_view(n, m, density, seed, dense_line=0.0):
    """Uniform random sparse view (one entry per column at least), column-normalised, canonical CSC.  dense_line > 0: row 7
    and column 11 also hold that fraction of their entries (the skewed case)."""
    rng = np.random.default_rng(seed)
    nnz = int(n * m * density)
    rows = [rng.integers(0, n, nnz), rng.integers(0, n, m)]
    cols = [rng.integers(0, m, nnz), np.arange(m)]
    if dense_line > 0:
        c = np.flatnonzero(rng.random(m) < dense_line); rows.append(np.full(c.size, 7)); cols.append(c)
        r = np.flatnonzero(rng.random(n) < dense_line); rows.append(r); cols.append(np.full(r.size, 11))
    rows = np.concatenate(rows).astype(np.int32)
    cols = np.concatenate(cols).astype(np.int32)
    vals = rng.uniform(0.1, 1.0, rows.size)
    x = sp.csc_matrix((vals, (rows, cols)), shape=(n, m))
    x.sum_duplicates()
    x.data /= np.repeat(np.add.reduceat(x.data, x.indptr[:-1]), np.diff(x.indptr))
    return x


def engine_for(x, k, seed, dense, **opts):
    n, m = x.shape
    e = Engine([n], [m], [k], nnz=None if dense else [x.nnz], **opts)
    if dense:
        e.set_view(0, x.toarray())
    else:
        e.set_view_sparse(0, x, pre_processed=True)
    f, s, g = synth.random_init(n, m, k, seed)
    e.set_factors(0, f, s, g)
    return e


def sweep_rate(x, k, dense, sweeps, seed=1):
    e = engine_for(x, k, seed, dense)
    try:
        e.run(sweeps)                          # warm-up: graphs captured, clocks up
        e.synchronize()
        t0 = time.perf_counter()
        e.run(sweeps)
        e.synchronize()
        dt = time.perf_counter() - t0
    finally:
        e.close()
    return sweeps / dt


def pass_times(x, k, dense, sweeps, seed=1):
    e = engine_for(x, k, seed, dense, time_kernels=True, use_graph=False)
    try:
        e.run(5)
        e.pass_timings(reset=True)
        e.run(sweeps)
        t = e.pass_timings()
    finally:
        e.close()
    xg = t["xg_ms_total"] / max(t["xg_launches"], 1)
    xtf = t["xtf_ms_total"] / max(t["xtf_launches"], 1)
    return {"xg_us": 1e3 * xg, "xtf_us": 1e3 * xtf, "xg_TBps": t["xg_bytes"] / (xg * 1e-3) / 1e12,
            "xtf_TBps": t["xtf_bytes"] / (xtf * 1e-3) / 1e12, "xg_bytes": t["xg_bytes"], "xtf_bytes": t["xtf_bytes"]}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--huge", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sweeps = 100 if a.quick else 500
    for density in (0.001, 0.01, 0.05, 0.2):
        x = random_view(10000, 2000, density, 7)
        rec = {"case": "c2", "density": density, "nnz": int(x.nnz), "k": 16,
               "sparse_sweeps_per_s": sweep_rate(x, 16, False, sweeps), "dense_sweeps_per_s": sweep_rate(x, 16, True, sweeps)}
        rec["sparse_us_per_sweep"] = 1e6 / rec["sparse_sweeps_per_s"]
        rec["dense_us_per_sweep"] = 1e6 / rec["dense_sweeps_per_s"]
        rec["sparse_passes"] = pass_times(x, 16, False, 20)
        rec["dense_passes"] = pass_times(x, 16, True, 20)
        emit(a.out, rec)
    # skewed: one row and one column at 60 % among lines at 0.1 % -- against the uniform 0.1 % case above
    x = random_view(10000, 2000, 0.001, 7, dense_line=0.6)
    rec = {"case": "c2 skewed", "density": 0.001, "dense_line": 0.6, "nnz": int(x.nnz), "k": 16,
           "sparse_sweeps_per_s": sweep_rate(x, 16, False, sweeps), "sparse_passes": pass_times(x, 16, False, 20)}
    rec["sparse_us_per_sweep"] = 1e6 / rec["sparse_sweeps_per_s"]
    emit(a.out, rec)
    x = random_view(200000, 20000, 0.005, 8)
    # occupancy probe: the SVD initialisation's products at sketch width 64 (k = 56) are spmm_kernel<64, *> launches WITHOUT
    # the k x k job's dynamic LDS (two workgroups per CU instead of one); a kernel trace sets them beside the sweep's
    e = Engine([x.shape[0]], [x.shape[1]], [56], nnz=[x.nnz])
    try:
        e.set_view_sparse(0, x, pre_processed=True)
        t0 = time.perf_counter()
        e.init_svd(0, seed=1, n_power=3)
        emit(a.out, {"case": "200000x20000 init_svd (L = 64)", "nnz": int(x.nnz), "wall_s": time.perf_counter() - t0})
    finally:
        e.close()
    for k in (16, 64):
        t0 = time.perf_counter()
        rec = {"case": "200000x20000", "density": 0.005, "nnz": int(x.nnz), "k": k, **pass_times(x, k, False, 10)}
        rec["wall_s"] = time.perf_counter() - t0
        emit(a.out, rec)
    if a.huge:
        t0 = time.perf_counter()
        x = random_view(1000000, 100000, 0.001, 9)
        t1 = time.perf_counter()
        e = engine_for(x, 16, 2, False)
        try:
            errs = e.run(10)
        finally:
            e.close()
        emit(a.out, {"case": "1e6x1e5", "density": 0.001, "nnz": int(x.nnz), "k": 16, "gen_s": t1 - t0,
                     "run_s": time.perf_counter() - t1, "all_error": [float(v) for v in errs],
                     "dense_image_bytes": 8.0 * 1e6 * 1e5})


if __name__ == "__main__":
    main()
