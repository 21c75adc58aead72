"""Timings of the fp64 shuffle of sparse views (resnmtf_fp64_shuffle_sparse) beside the dense fp64
shuffle of the densified view and a host shuffle of the stored entries, and of remove_spurious(precision="fp64") on sparse
against densified views, on one GPU.

    python tools/time_fp64_shuffle_sparse.py [--quick] [--reps 5] [--out profiles/time_fp64_shuffle_sparse.jsonl]

shuffle: c2's shape (10000 x 2000; --quick: 2000 x 500) at 1 % and 5 % stored, normalised draws.  Per case the median of
         `reps` blocking calls after a warm-up, all in this session, of
           engine.fp64_shuffle_sparse from a sparse_csc tensor on the device -- checked and sorted on the device per call,
           engine.fp64_shuffle_sparse from the host CSC (scipy.sparse) -- checked on the host and uploaded per call,
           engine.fp64_shuffle of the densified fp64 device tensor -- what a caller had to do before,
           a host shuffle a user would otherwise write: positions drawn without replacement with NumPy, a scipy.sparse CSC
           built of them, its columns normalised, the three arrays uploaded as a sparse_csc tensor,
         whether the sparse draw equals the dense one bitwise at the stored positions, and the transient bytes of the sparse
         call (68 per stored entry) beside the n m doubles of the dense draw.
removal: remove_spurious(precision="fp64") with 5 repeats at the same shape and 5 % stored, k = 3, every shuffled fit
         guarded by max_iters = 50: the views sparse (fp64_shuffle_sparse=True) against the same views densified.
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
from time_fp64_bisil import median_ms  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def device_csc(xs, dev):
    import torch
    return torch.sparse_csc_tensor(torch.as_tensor(xs.indptr.astype(np.int64), device=dev), torch.as_tensor(xs.indices.astype(np.int64), device=dev),
                                   torch.as_tensor(xs.data, device=dev), xs.shape)


def random_view(n, m, density, seed):
    """A pre-processed sparse view: uniform values at random positions, every column holding an entry, columns summing to 1."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < density
    mask[rng.integers(0, n, m), np.arange(m)] = True
    x = np.where(mask, rng.random((n, m)) + 0.05, 0.0)
    return sp.csc_matrix(x / x.sum(axis=0))


def host_shuffle(xs, seed, dev):
    n, m = xs.shape
    dst = np.random.default_rng(seed).choice(n * m, size=xs.nnz, replace=False)
    s = sp.csc_matrix((xs.data, (dst % n, dst // n)), shape=(n, m))
    s.sort_indices()
    colsum = np.add.reduceat(s.data, s.indptr[:-1])
    s.data = s.data / np.repeat(colsum, np.diff(s.indptr))
    return device_csc(s, dev)


def shuffle_part(n, m, reps):
    import torch
    dev = torch.device("cuda", 0)
    for density in (0.01, 0.05):
        xs = random_view(n, m, density, 5)
        xt, dense = device_csc(xs, dev), torch.as_tensor(xs.toarray(), device=dev)
        t, er, ec = engine.fp64_shuffle_sparse(xt, 7, normalise=True)
        d, _, dr, dc = engine.fp64_shuffle(dense, 7, normalise=True)
        ccol, rows, vals = t.ccol_indices().cpu().numpy(), t.row_indices().cpu().numpy(), t.values().cpu().numpy()
        at = d.cpu().numpy()[rows, np.repeat(np.arange(m), np.diff(ccol))]
        same = bool(np.array_equal(np.isnan(vals), np.isnan(at)) and np.array_equal(vals[~np.isnan(vals)].view(np.uint64), at[~np.isnan(at)].view(np.uint64))
                    and np.array_equal(er, dr) and np.array_equal(ec, dc))
        emit({"part": "shuffle", "n": n, "m": m, "stored": density, "nnz": int(xs.nnz),
              "sparse_device_csc_ms": median_ms(lambda: engine.fp64_shuffle_sparse(xt, 7, normalise=True), reps),
              "sparse_host_csc_ms": median_ms(lambda: engine.fp64_shuffle_sparse(xs, 7, normalise=True), reps),
              "dense_fp64_device_ms": median_ms(lambda: engine.fp64_shuffle(dense, 7, normalise=True), reps),
              "host_numpy_shuffle_and_upload_ms": median_ms(lambda: (host_shuffle(xs, 7, dev), torch.cuda.synchronize()), reps),
              "columns": f"median, min, max of {reps} blocking calls after a warm-up",
              "sparse_equals_dense_at_the_stored_positions_bitwise": same, "empty_rows": int(er.sum()), "empty_cols": int(ec.sum()),
              "sparse_transient_bytes": 68 * int(xs.nnz) + 8 * (2 * (m + 1) + n + 1) + 48, "sparse_output_bytes": 16 * int(xs.nnz) + 8 * (m + 1),
              "dense_draw_bytes": 8 * n * m})


def removal_part(n, m, reps):
    k, repeats, guard = 3, 5, 50
    views = [random_view(n, m, 0.05, 11)]
    rn, cn = naming.give_names(views, None, None, None, None)
    kw = dict(k_vec=[k], row_names=rn, col_names=cn, seed=3, max_iters=guard, precision="fp64")
    plain = api.res_nmtf_inner(views, naming.shared_names(rn), naming.shared_names(cn), n_iters=20, spurious=False, fp64_sparse=True, **kw)
    dense = [views[0].toarray()]
    more = dict(seed=3, precision="fp64", max_iters=guard)
    a = api.remove_spurious(views, plain, repeats, fp64_shuffle_sparse=True, **more)["spurious"]
    b = api.remove_spurious(dense, plain, repeats, **more)["spurious"]
    emit({"part": "removal", "n": n, "m": m, "stored": 0.05, "nnz": int(views[0].nnz), "k": k, "num_repeats": repeats, "max_iters": guard,
          "sparse_views_ms": median_ms(lambda: api.remove_spurious(views, plain, repeats, fp64_shuffle_sparse=True, **more), reps),
          "densified_views_ms": median_ms(lambda: api.remove_spurious(dense, plain, repeats, **more), reps),
          "columns": f"median, min, max of {reps} blocking calls after a warm-up",
          "removed_equal": bool(np.array_equal(a["removed"], b["removed"])),
          "max_abs_score_difference": float(np.abs(a["score"] - b["score"]).max())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_shuffle_sparse.jsonl"))
    a = ap.parse_args()
    n, m = (2000, 500) if a.quick else (10000, 2000)
    shuffle_part(n, m, a.reps)
    removal_part(n, m, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
