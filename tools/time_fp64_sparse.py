"""Timings of sparse views in the device-wide fp64 path (resnmtf_fp64_run_sparse), on one GPU, by
the protocol of tools/time_fp64.py.

    python tools/time_fp64_sparse.py [--part sweep|big|drift|all] [--out profiles/time_fp64_sparse.jsonl]

sweep: us per sweep of one view of c2's shape (10000 x 2000), k = 16, at 0.1 %, 1 %, 5 % and 20 % stored, through the
       sparse fp64 path and, in the same session, the dense fp64 path on the densified view and the f32 sparse engine
       (api.res_nmtf_inner).  Per path: the difference of two fixed-count runs divided by the difference of their sweep
       counts (upload, host preparation, launch set-up and download cancel out), best of three after a warm-up.
big:   the same for 200000 x 20000 at 0.5 %, k = 16 and 64 (the dense fp64 path is left out: its two images alone are
       64 GB), best of two.
drift: the f32 sparse engine against the sparse fp64 path at 200000 x 20000, 0.5 %, k = 16, over 100 sweeps from one
       explicit start: relative Frobenius distance of F, G, S and max |d All_Error|.  A recorded observation.
Prints one JSON line per measurement and writes them to --out."""
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
from resnmtf_amd import api, naming, sparse, synth  # noqa: E402
from resnmtf_amd.engine import fp64_run, fp64_sparse_plan  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def sparse_view(n, m, density, seed, blocks=8):
    """A pre-processed sparse view built without its dense image: per column about density * n distinct rows, the value
    10 inside the planted block of the column and 0.1 |N(0, 1)| + 0.01 outside, columns normalised."""
    rng = np.random.default_rng(seed)
    per_col = max(1, int(round(density * n)))
    rows = rng.integers(0, n, size=(m, per_col), dtype=np.int64).ravel()
    key = np.unique(np.repeat(np.arange(m, dtype=np.int64), per_col) * n + rows)      # (a row drawn twice: one entry)
    cols, rows = key // n, key % n
    vals = 0.1 * np.abs(rng.standard_normal(rows.size)) + 0.01
    vals += 10.0 * ((rows * blocks // n) == (cols * blocks // m))
    x = sparse.canonical_csc(sp.coo_matrix((vals, (rows, cols)), shape=(n, m)))
    colsum = np.add.reduceat(x.data, x.indptr[:-1])
    x.data /= np.repeat(colsum, np.diff(x.indptr))
    return x


def best_of(fn, reps=3):
    fn()                                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def per_sweep(fn, lo, hi, reps=3):
    t = {it: best_of(lambda it=it: fn(it), reps) for it in (lo, hi)}
    return (t[hi] - t[lo]) / (hi - lo) * 1e6


def engine_call(x, f, s, g, k, it):
    rn, cn = naming.give_names([x])
    return api.res_nmtf_inner([x], naming.shared_names(rn), naming.shared_names(cn), [f], [s], [g], [k], None, None, None, it,
                              spurious=False, row_names=rn, col_names=cn)


def time_case(part, n, m, k, density, seed, dense, reps, f64_counts, eng_counts):
    x = sparse_view(n, m, density, seed)
    f, s, g = synth.random_init(n, m, k, seed + 1)
    p = {"data": [x], "k": k, "init_f": [f], "init_s": [s], "init_g": [g]}
    rec = {"part": part, "n": n, "m": m, "k": k, "density": density, "nnz": int(x.nnz), "plan": fp64_sparse_plan(x, k)}
    rec["fp64_sparse_us_per_sweep"] = round(per_sweep(lambda it: fp64_run(dict(p, n_iters=it)), *f64_counts, reps=reps), 2)
    rec["fp64_dense_us_per_sweep"] = None
    if dense:
        xd = x.toarray()
        rec["fp64_dense_us_per_sweep"] = round(per_sweep(lambda it: fp64_run(dict(p, data=[xd], n_iters=it)), *f64_counts, reps=reps), 2)
        rec["sparse_below_dense"] = bool(rec["fp64_sparse_us_per_sweep"] < rec["fp64_dense_us_per_sweep"])
        del xd
    rec["f32_sparse_engine_us_per_sweep"] = round(per_sweep(lambda it: engine_call(x, f, s, g, k, it), *eng_counts, reps=reps), 2)
    emit(rec)


def rel_fro(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def drift_part(n=200000, m=20000, k=16, density=0.005, sweeps=100):
    x = sparse_view(n, m, density, 5)
    f, s, g = synth.random_init(n, m, k, 6)
    t0 = time.perf_counter()
    f32 = engine_call(x, f, s, g, k, sweeps)
    t1 = time.perf_counter()
    f64 = fp64_run({"data": [x], "k": k, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": sweeps})
    t2 = time.perf_counter()
    emit({"part": "drift", "n": n, "m": m, "k": k, "density": density, "nnz": int(x.nnz), "sweeps": sweeps,
          "rel_fro_f": rel_fro(f32["output_f"][0], f64["f"][0]), "rel_fro_g": rel_fro(f32["output_g"][0], f64["g"][0]),
          "rel_fro_s": rel_fro(f32["output_s"][0], f64["s"][0]),
          "max_abs_d_all_error": float(np.max(np.abs(f32["All_Error"] - f64["all_error"]))),
          "final_error_f32": float(f32["All_Error"][-1]), "final_error_fp64": float(f64["all_error"][-1]),
          "engine_call_s": round(t1 - t0, 3), "fp64_call_s": round(t2 - t1, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["sweep", "big", "drift", "all"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_sparse.jsonl"))
    a = ap.parse_args()
    if a.part in ("sweep", "all"):
        for density in (0.001, 0.01, 0.05, 0.2):
            time_case("sweep", 10000, 2000, 16, density, 1, True, 3, (10, 60), (10, 410))
    if a.part in ("big", "all"):
        for k in (16, 64):
            time_case("big", 200000, 20000, k, 0.005, 3, False, 2, (5, 25), (10, 110))
    if a.part in ("drift", "all"):
        drift_part()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
