"""Timings of the grouped path (resnmtf_group_run) against the existing engine, on one GPU.

    python tools/time_group.py [--part crossover|throughput|pipeline|all] [--quick]

crossover:  the per-sweep time of ONE job alone in the grouped kernel and in the existing engine (api.res_nmtf_inner),
            one square view n x n, n = 64 .. 2048, k = 3, 8, 16: the difference of two fixed-count runs divided by the
            difference of their sweep counts (upload, launch and download cancel out); the engine over 400 sweeps.
throughput: 1, 8, 64, 256, 1024 copies of the planted 2 x 180 x 180, k = 3 job at a fixed 200 sweeps in one call:
            wall time, job-sweeps per second; then 1, 256, 1024 copies of it to convergence (default max_iters).
pipeline:   the planted problem's 6-job k sweep (k = 3..8) and 5-job shuffle list, to convergence: run_jobs_grouped
            against run_jobs (the existing engine, one job after another).
Every timed call follows an untimed warm-up of the same shape.  Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd import api, batched, naming, synth  # noqa: E402
from resnmtf_amd.engine import group_run  # noqa: E402
from resnmtf_amd.problem import pair_table  # noqa: E402


def planted():
    xs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        b = np.kron(np.eye(3), np.ones((60, 1)))
        xs.append(b @ np.diag([10.0] * 3) @ b.T + 0.1 * np.abs(rng.normal(size=(180, 180))))
    return xs


def one_view_problem(n, k, n_iters, seed=0):
    x = synth.planted_view(n, n, min(k, 8), seed)
    x = x / x.sum(axis=0)[None, :]
    f, s, g = synth.random_init(n, n, k, seed + 1)
    return {"data": [x], "k": k, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": n_iters}


def best_of(fn, reps=3):
    fn()                                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def crossover(quick):
    sizes = [64, 128, 256, 512, 1024, 2048] if not quick else [64, 256, 1024]
    for k in (3, 8, 16):
        for n in sizes:
            lo, hi = (4, 24) if n >= 1024 else (10, 110)
            t_grp = {it: best_of(lambda it=it: group_run([one_view_problem(n, k, it)])) for it in (lo, hi)}
            p = one_view_problem(n, k, 1)
            rn, cn = naming.give_names(p["data"])

            def eng(it):
                api.res_nmtf_inner(p["data"], naming.shared_names(rn), naming.shared_names(cn), p["init_f"], p["init_s"],
                                   p["init_g"], [k], None, None, None, it, spurious=False, row_names=rn, col_names=cn)
            e_lo, e_hi = 10, 410                   # (the engine's sweeps are short: a long difference keeps noise out)
            t_eng = {it: best_of(lambda it=it: eng(it)) for it in (e_lo, e_hi)}
            per_grp = (t_grp[hi] - t_grp[lo]) / (hi - lo) * 1e6
            per_eng = (t_eng[e_hi] - t_eng[e_lo]) / (e_hi - e_lo) * 1e6
            print(json.dumps({"part": "crossover", "n": n, "k": k, "grouped_us_per_sweep": round(per_grp, 2),
                              "engine_us_per_sweep": round(per_eng, 2), "grouped_faster": per_grp < per_eng}), flush=True)


def planted_problem(n_iters):
    data = naming.check_data(planted())
    init = api.svd_init(data, [3, 3], 3)
    rn, cn = naming.give_names(data)
    return {"data": data, "k": 3, "init_f": init[0], "init_s": init[1], "init_g": init[2], "init_lam": init[3],
            "init_mu": init[4], "phi": np.zeros((2, 2)), "xi": np.zeros((2, 2)), "psi": np.zeros((2, 2)),
            "row_pairs": pair_table(rn), "col_pairs": pair_table(cn), "n_iters": n_iters}


def throughput(quick):
    p = planted_problem(200)
    for copies in ([1, 8, 64, 256, 1024] if not quick else [1, 64, 256]):
        probs = [p] * copies
        t = best_of(lambda: group_run(probs), reps=2)
        print(json.dumps({"part": "throughput", "jobs": copies, "sweeps_each": 200, "wall_ms": round(t * 1e3, 2),
                          "job_sweeps_per_s": round(copies * 200 / t), "us_per_job_sweep": round(t / copies / 200 * 1e6, 3)}),
              flush=True)


def throughput_convergence(quick):
    """The same planted job to convergence (tol 1e-6, the default max_iters = 100000: every job's error history is
    sized by it on the device)."""
    p = planted_problem(None)
    for copies in ([1, 256, 1024] if not quick else [256]):
        probs = [p] * copies
        t = best_of(lambda: group_run(probs), reps=2)
        sweeps = group_run([p])[0]["iters"]
        print(json.dumps({"part": "throughput_convergence", "jobs": copies, "sweeps_each": sweeps,
                          "wall_ms": round(t * 1e3, 2), "us_per_job_sweep": round(t / copies / sweeps * 1e6, 3)}), flush=True)


def pipeline(quick):
    raw = planted()
    data = naming.check_data(raw)
    for name, jobs in (("k_sweep_3_8", batched.k_sweep_jobs(raw, 3, 8, seed=0)),
                       ("shuffles_5", batched.shuffled_jobs(data, 3, 5, seed=0))):
        t_grp = best_of(lambda: batched.run_jobs_grouped(jobs), reps=2)
        t_seq = best_of(lambda: batched.run_jobs(jobs), reps=1 if quick else 2)
        g = batched.run_jobs_grouped(jobs)
        s = batched.run_jobs(jobs)
        print(json.dumps({"part": "pipeline", "case": name, "jobs": len(jobs), "grouped_ms": round(t_grp * 1e3, 2),
                          "run_jobs_ms": round(t_seq * 1e3, 2), "speedup": round(t_seq / t_grp, 2),
                          "grouped_sweeps": [len(r["All_Error"]) for r in g],
                          "run_jobs_sweeps": [len(r["All_Error"]) for r in s]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["crossover", "throughput", "pipeline", "all"])
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.part in ("throughput", "all"):
        throughput(a.quick)
    if a.part in ("throughput", "all"):
        throughput_convergence(a.quick)
    if a.part in ("pipeline", "all"):
        pipeline(a.quick)
    if a.part in ("crossover", "all"):
        crossover(a.quick)


if __name__ == "__main__":
    main()
