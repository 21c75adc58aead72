"""Timings of the fp64 sub-sample of sparse views (resnmtf_fp64_subsample_sparse) beside the dense
fp64 sub-sample of the densified view, the f32 sparse route and SciPy indexing, and of stability_check(precision="fp64") on
sparse against densified views, on one GPU.

    python tools/time_fp64_subsample_sparse.py [--quick] [--reps 5] [--out profiles/time_fp64_subsample_sparse.jsonl]

subsample: c2's shape (10000 x 2000; --quick: 2000 x 500) at 1 % and 5 % stored, sample_rate 0.9, the lists in sample()
           order (drawn without replacement, unsorted).  Per case the median of `reps` blocking calls after a warm-up, all in
           this session, of one sub-sample by
             engine.fp64_subsample_sparse from a sparse_csc tensor on the device -- checked and sorted on the device per call,
             engine.fp64_subsample_sparse from the host CSC (scipy.sparse) -- checked on the host and uploaded per call,
             the same in count mode (from the device tensor),
             engine.fp64_subsample of the densified fp64 device tensor -- what a caller had to do before,
             the f32 route -- Engine.subsample_count_sparse, an engine of that capacity, subsample_view_sparse_from, empty_lines,
             SciPy indexing of the host matrix with the three arrays uploaded as a sparse_csc tensor,
           whether the sparse sub-sample equals the dense one bitwise, and the transient bytes of the sparse call beside the
           n_sub m_sub doubles of the dense sub-sample.
stability: stability_check(precision="fp64") with 5 repeats at the same shape and 5 % stored, k = 3, n_iters = 20: the view
           sparse (fp64_subsample_sparse=True) against the same view densified.
Prints one JSON line per measurement and writes them to --out."""
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
from resnmtf_amd import api, engine, naming  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402
from time_fp64_bisil import median_ms  # noqa: E402
from time_fp64_shuffle_sparse import device_csc, random_view  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def scipy_subsample(xs, rows, cols, dev):
    import torch
    s = sp.csc_matrix(xs[rows][:, cols])
    s.sort_indices()
    t = device_csc(s, dev)
    torch.cuda.synchronize()
    return t


def subsample_part(n, m, reps):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    rows, cols = rng.choice(n, int(n * 0.9), replace=False), rng.choice(m, int(m * 0.9), replace=False)
    ns, ms = len(rows), len(cols)
    r32, c32 = rows.astype(np.int32), cols.astype(np.int32)
    for density in (0.01, 0.05):
        xs = random_view(n, m, density, 5)
        xt, dense = device_csc(xs, dev), torch.as_tensor(xs.toarray(), device=dev)
        t, er, ec = engine.fp64_subsample_sparse(xt, rows, cols)
        d, dr, dc = engine.fp64_subsample(dense, rows, cols)
        got = sp.csc_matrix((t.values().cpu().numpy(), t.row_indices().cpu().numpy(), t.ccol_indices().cpu().numpy()), shape=(ns, ms))
        same = bool(np.array_equal(got.toarray().view(np.uint64), np.ascontiguousarray(d.cpu().numpy()).view(np.uint64))
                    and np.array_equal(er, dr) and np.array_equal(ec, dc))
        kept = int(t._nnz())
        with Engine([n], [m], [1], nnz=[xs.nnz]) as base:
            base.set_view_sparse(0, xs, pre_processed=True)

            def f32_route():
                with Engine([ns], [ms], [1], nnz=[base.subsample_count_sparse(0, r32, c32)]) as e:
                    e.subsample_view_sparse_from(0, base, 0, r32, c32)
                    return e.empty_lines(0)
            f32_ms = median_ms(f32_route, reps)
        emit({"part": "subsample", "n": n, "m": m, "n_sub": ns, "m_sub": ms, "stored": density, "nnz": int(xs.nnz), "nnz_sub": kept,
              "sparse_device_csc_ms": median_ms(lambda: engine.fp64_subsample_sparse(xt, rows, cols), reps),
              "sparse_host_csc_ms": median_ms(lambda: engine.fp64_subsample_sparse(xs, rows, cols), reps),
              "sparse_count_mode_ms": median_ms(lambda: engine.fp64_subsample_sparse(xt, rows, cols, count_only=True), reps),
              "dense_fp64_device_ms": median_ms(lambda: engine.fp64_subsample(dense, rows, cols), reps),
              "f32_sparse_route_ms": f32_ms,
              "scipy_indexing_and_upload_ms": median_ms(lambda: scipy_subsample(xs, rows, cols, dev), reps),
              "columns": f"median, min, max of {reps} blocking calls after a warm-up",
              "sparse_equals_dense_bitwise": same, "empty_rows": int(er.sum()), "empty_cols": int(ec.sum()),
              "sparse_transient_bytes_device_source": max(48 * int(xs.nnz) + 8 * (m + 1 + n + 1) + 24,
                                                          12 * int(xs.nnz) + 8 * (m + 1) + 24 + 64 * kept + 8 * (ms + 1 + ns + 1) + 24),
              "sparse_output_bytes": 16 * kept + 8 * (ms + 1), "dense_subsample_bytes": 8 * ns * ms})


def stability_part(n, m, reps):
    import time
    k, n_stab, iters = 3, 5, 20
    views = [random_view(n, m, 0.05, 11)]
    rn, cn = naming.give_names(views, None, None, None, None)
    fit = api.res_nmtf_inner(views, naming.shared_names(rn), naming.shared_names(cn), k_vec=[k], n_iters=iters, spurious=False,
                             row_names=rn, col_names=cn, seed=3, precision="fp64", fp64_sparse=True)
    z = np.zeros((1, 1))
    dense = [views[0].toarray()]

    def check(data, **kw):
        return api.stability_check(data, fit, k, z, z, z, iters, False, 5, False, "euclidean", 0.9, n_stab, 0.6, False, row_names=rn,
                                   col_names=cn, seed=3, precision="fp64", **kw)

    def once(fn):
        fn()                                                       # warm-up
        t0 = time.perf_counter()
        out = fn()
        return round((time.perf_counter() - t0) * 1e3, 1), out
    sparse_ms, a = once(lambda: check(views, fp64_subsample_sparse=True))
    dense_ms, b = once(lambda: check(dense))
    emit({"part": "stability", "n": n, "m": m, "stored": 0.05, "nnz": int(views[0].nnz), "k": k, "n_stability": n_stab, "n_iters": iters,
          "stability_check_fp64_sparse_view_ms": sparse_ms, "stability_check_fp64_densified_view_ms": dense_ms,
          "columns": "one call each, after a warm-up of both routes",
          "max_abs_relevance_difference": float(np.abs(a["relevance"] - b["relevance"]).max()),
          "decisions_at_0.6_equal": bool(np.array_equal(a["relevance"] < 0.6, b["relevance"] < 0.6))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_subsample_sparse.jsonl"))
    a = ap.parse_args()
    n, m = (2000, 500) if a.quick else (10000, 2000)
    subsample_part(n, m, a.reps)
    stability_part(n, m, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
