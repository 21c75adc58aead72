"""What the fp64 path gains from reading a SPARSE view where it lies in device memory (resnmtf_fp64_run_sparse_device,
DESIGN.md section 24), on one GPU.

    python tools/time_fp64_sparse_device.py [--quick] [--out profiles/time_fp64_sparse_device.jsonl]

Whole-call wall time of engine.fp64_run, 20 fixed sweeps at k = 16, from a sparse torch tensor on the GPU (checked, sorted
and copied on the device) against what a caller without the entry has to do with the same tensor: bring its arrays to the
host (.cpu()), build the scipy.sparse matrix, then engine.fp64_run on it (SciPy's canonical copy, the host check of every
entry, the host counting sort for the CSR copy, six uploads).  Both in this session, from host initial factors, best of
three after a warm-up (the 20 M entry case: best of two); the results of the two routes are compared bit for bit.
Cases: c2's shape (10000 x 2000) at 1 % and at 5 %, and section 22's showcase 200000 x 20000 at 0.5 %, each as a canonical
CSC tensor (one sort on the device) and as a COO tensor in random order (two sorts).
Prints one JSON line per measurement and writes them to --out.  Recorded figures, not assertions."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd import synth  # noqa: E402
from resnmtf_amd.engine import fp64_run  # noqa: E402

LINES = []
SWEEPS = 20
K = 16
CASES = [("c2 shape, 1 %", 10000, 2000, 0.01), ("c2 shape, 5 %", 10000, 2000, 0.05), ("200000 x 20000, 0.5 %", 200000, 20000, 0.005)]


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def case_entries(n, m, density, seed=0):
    """Distinct positions drawn on the device, in canonical CSC order, with column-normalised positive fp64 values (a
    column without an entry stays one: the view is taken as pre-processed either way)."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    want = int(n * m * density)
    pos = torch.unique(torch.randint(0, n * m, (int(want * 1.02) + 16,), generator=g, device=dev, dtype=torch.int64))[:want]
    cols, rows = pos // n, pos % n                                   # (sorted by c n + r: columns ascending, rows within them)
    vals = torch.rand(pos.numel(), generator=g, device=dev, dtype=torch.float64) + 0.05
    sums = torch.zeros(m, dtype=torch.float64, device=dev).index_add_(0, cols, vals)
    vals = vals / sums[cols]
    return rows, cols, vals


def tensors(rows, cols, vals, n, m, seed=1):
    """The canonical CSC tensor and a COO tensor of the same entries in random order."""
    import torch
    ccol = torch.zeros(m + 1, dtype=torch.int64, device=rows.device)
    ccol[1:] = torch.cumsum(torch.bincount(cols, minlength=m), 0)
    csc = torch.sparse_csc_tensor(ccol, rows, vals, (n, m))
    perm = torch.randperm(rows.numel(), generator=torch.Generator(device=rows.device).manual_seed(seed), device=rows.device)
    coo = torch.sparse_coo_tensor(torch.stack([rows[perm], cols[perm]]), vals[perm], (n, m), is_coalesced=True)
    return {"canonical CSC": csc, "COO, random order": coo}


def to_scipy(t):
    """What a caller does today with a sparse tensor on the GPU: its arrays to the host, the scipy.sparse matrix of them."""
    import scipy.sparse as sp
    import torch
    if t.layout == torch.sparse_csc:
        return sp.csc_matrix((t.values().cpu().numpy(), t.row_indices().cpu().numpy(), t.ccol_indices().cpu().numpy()), shape=tuple(t.shape))
    idx = t._indices().cpu().numpy()
    return sp.coo_matrix((t._values().cpu().numpy(), (idx[0], idx[1])), shape=tuple(t.shape))


def best_of(fn, reps):
    fn()                                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the two c2 cases alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_sparse_device.jsonl"))
    a = ap.parse_args()
    for name, n, m, density in CASES[:2] if a.quick else CASES:
        rows, cols, vals = case_entries(n, m, density)
        f, s, g = synth.random_init(n, m, K, 1)
        for form, t in tensors(rows, cols, vals, n, m).items():
            base = {"k": K, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": SWEEPS}
            out = {}

            def run_there():
                out["there"] = fp64_run(dict(base, data=[t]))

            def run_host():
                torch.cuda.synchronize()
                out["host"] = fp64_run(dict(base, data=[to_scipy(t)]))
            reps = 2 if t._nnz() >= 1 << 24 else 3
            torch.cuda.synchronize()
            t_there = best_of(run_there, reps)
            t_host = best_of(run_host, reps)
            same = all(np.array_equal(x, y, equal_nan=True) for key in ("f", "s", "g", "lambda", "mu")
                       for x, y in zip(out["there"][key], out["host"][key]))
            same = same and np.array_equal(out["there"]["all_error"], out["host"]["all_error"], equal_nan=True)
            emit({"case": name, "form": form, "n": n, "m": m, "k": K, "nnz": int(t._nnz()), "sweeps": SWEEPS,
                  "host_route_s": round(t_host, 4), "device_route_s": round(t_there, 4), "host_over_device": round(t_host / t_there, 2),
                  "bitwise_equal": bool(same)})
        del rows, cols, vals, t
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
