"""Timings and the f32 distance of the device-wide fp64 path (resnmtf_fp64_run), on one GPU.

    python tools/time_fp64.py [--part sweep|distance|all] [--quick] [--out profiles/time_fp64.jsonl]

sweep:    us per sweep of ONE job through the fp64 path, the grouped path (resnmtf_group_run, inside its limits) and the
          engine (api.res_nmtf_inner), all in this session: one view n x n, n = 64 .. 2048, k = 3, 8, 16 (the sizes of
          section 12's single-job table), then 4096 x 4096 and c2's shape (10000 x 2000), k = 16.  Per path: the difference
          of two fixed-count runs divided by the difference of their sweep counts (upload, launch set-up and download
          cancel out), best of three after a warm-up.  For c2 also the bytes one fp64 sweep moves and the GB/s achieved.
distance: c2 (synth.config("c2")), 500 fixed sweeps from its explicit start through the engine and through the fp64
          path: relative Frobenius distance of F, G, S and max |d All_Error| -- the acceptance protocol of BASELINE.json
          configs[1] at its own size.  A recorded measurement, not an assertion.
Prints one JSON line per measurement and writes them to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd import _lib, api, naming, synth  # noqa: E402
from resnmtf_amd.engine import fp64_plan, fp64_run, group_run  # noqa: E402

LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def one_view_problem(n, m, k, n_iters, seed=0):
    x = synth.planted_view(n, m, min(k, 8), seed)
    x = x / x.sum(axis=0)[None, :]
    f, s, g = synth.random_init(n, m, k, seed + 1)
    return {"data": [x], "k": k, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": n_iters}


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


def fp64_bytes_per_sweep(n, m, k):
    """What one fp64 sweep of one n x m view reads and writes in its three streaming kernels and their slabs: X once for
    X G, X^T once for X^T F, X once for the residual (padded images), each product's slab written and read once."""
    plan = fp64_plan(n, m, k)
    up = lambda x, a: (x + a - 1) // a * a                          # noqa: E731
    ldn, ldm = plan["ld"]
    image = ldn * up(m, 64) + ldm * up(n, 64) + ldn * up(m, 64)
    slabs = 2 * (plan["xg"][1] * ldn + plan["xtf"][1] * ldm) * plan["kp"]
    return 8 * (image + slabs)


def sweep_part(quick):
    in_group = lambda n, m, k: n * m <= _lib.GROUP_MAX_VIEW_ENTRIES and k <= _lib.GROUP_MAX_K      # noqa: E731
    cases = [(n, n, k) for k in (3, 8, 16) for n in ([64, 128, 256, 512, 1024, 2048] if not quick else [256, 1024])]
    cases += [(4096, 4096, 16), (10000, 2000, 16)]
    for n, m, k in cases:
        p = one_view_problem(n, m, k, 1)
        rn, cn = naming.give_names(p["data"])

        def eng(it):
            api.res_nmtf_inner(p["data"], naming.shared_names(rn), naming.shared_names(cn), p["init_f"], p["init_s"],
                               p["init_g"], [k], None, None, None, it, spurious=False, row_names=rn, col_names=cn)
        per_f64 = per_sweep(lambda it: fp64_run(dict(p, n_iters=it)), 10, 60)
        per_eng = per_sweep(eng, 10, 410)                           # (the engine's sweeps are short: a long difference)
        per_grp = None
        if in_group(n, m, k):
            lo, hi = (4, 14) if n >= 1024 else (10, 60)
            per_grp = per_sweep(lambda it: group_run([dict(p, n_iters=it)]), lo, hi, reps=2)
        rec = {"part": "sweep", "n": n, "m": m, "k": k, "fp64_us_per_sweep": round(per_f64, 2),
               "grouped_us_per_sweep": None if per_grp is None else round(per_grp, 2),
               "engine_us_per_sweep": round(per_eng, 2),
               "fp64_faster_than_grouped": None if per_grp is None else bool(per_f64 < per_grp), "plan": fp64_plan(n, m, k)}
        if (n, m) == (10000, 2000):
            b = fp64_bytes_per_sweep(n, m, k)
            rec.update(fp64_bytes_per_sweep=b, fp64_gb_per_s=round(b / per_f64 / 1e3, 1))
        emit(rec)


def rel_fro(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def distance_part(sweeps=500):
    prob = synth.config("c2")
    k = prob.init_f[0].shape[1]
    args = (prob.data, naming.shared_names(prob.row_names), naming.shared_names(prob.col_names), prob.init_f, prob.init_s,
            prob.init_g, [k] * len(prob.data), prob.phi, prob.xi, prob.psi, sweeps)
    kw = dict(spurious=False, row_names=prob.row_names, col_names=prob.col_names)
    t0 = time.perf_counter()
    f32 = api.res_nmtf_inner(*args, **kw)
    t1 = time.perf_counter()
    f64 = api.res_nmtf_inner(*args, precision="fp64", **kw)
    t2 = time.perf_counter()
    emit({"part": "distance", "config": "c2", "shape": list(prob.data[0].shape), "k": k, "sweeps": sweeps,
          "rel_fro_f": rel_fro(f32["output_f"][0], f64["output_f"][0]), "rel_fro_g": rel_fro(f32["output_g"][0], f64["output_g"][0]),
          "rel_fro_s": rel_fro(f32["output_s"][0], f64["output_s"][0]),
          "max_abs_d_all_error": float(np.max(np.abs(f32["All_Error"] - f64["All_Error"]))),
          "final_error_f32": float(f32["All_Error"][-1]), "final_error_fp64": float(f64["All_Error"][-1]),
          "engine_call_s": round(t1 - t0, 3), "fp64_call_s": round(t2 - t1, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["sweep", "distance", "all"])
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64.jsonl"))
    a = ap.parse_args()
    if a.part in ("distance", "all"):
        distance_part()
    if a.part in ("sweep", "all"):
        sweep_part(a.quick)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
