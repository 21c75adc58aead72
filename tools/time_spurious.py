"""Wall times of spurious-bicluster scoring on one GPU.

    python tools/time_spurious.py [--quick] [--out FILE]

For the planted two-view problem (test-resnmtf.R, k = 3), c2 (one 10000 x 2000 view, k = 16) and c2's shape at k = 64:
the num_repeats = 5 shuffled factorisations (batched.shuffles_on_device, to convergence), the scoring of their F
columns (check_biclusters with those F's: one resnmtf_jsd_pairs call per view plus the host's mean and density mode),
the whole remove_spurious, and the NumPy restatement (tests/jsd_ref.py) on the CPU timed on a sample of the same pairs
and scaled to all of them.  --quick skips k = 64; --scoring-only times resnmtf_jsd_pairs alone on F-like pools.  Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resnmtf_amd  # noqa: E402
from resnmtf_amd import api, batched, naming, spurious, synth  # noqa: E402
from resnmtf_amd.engine import jsd_pairs  # noqa: E402


def planted():
    xs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        b = np.kron(np.eye(3), np.ones((60, 1)))
        xs.append(b @ np.diag([10.0] * 3) @ b.T + 0.1 * np.abs(rng.normal(size=(180, 180))))
    return xs


def measure(name, raw, k, R, n_iters, out):
    data = naming.check_data(raw)
    res = resnmtf_amd.apply_resnmtf(raw, k_val=k, spurious=False, stability=False, n_iters=n_iters, seed=1)
    dev = batched.DeviceData(data, pre_processed=True)
    try:
        batched.shuffles_on_device(dev, k, 1, seed=99)                          # warm-up (library load, first launches)
        t0 = time.perf_counter()
        reps = batched.shuffles_on_device(dev, k, R, seed=0)
        t_shuffle = time.perf_counter() - t0
    finally:
        dev.close()
    shuffled = [r["output_f"] for r in reps]
    sweeps = [len(r["All_Error"]) for r in reps]
    api.check_biclusters(data, res["output_f"], R, shuffled_f=shuffled)          # warm-up (library load, first launch)
    t0 = time.perf_counter()
    api.check_biclusters(data, res["output_f"], R, shuffled_f=shuffled)
    t_score = time.perf_counter() - t0
    null_p, score_p = spurious.pool_pairs(k, R)
    pairs = np.concatenate([null_p, score_p])
    pool = np.concatenate([res["output_f"][0]] + [f[0] for f in shuffled], axis=1)
    t0 = time.perf_counter()
    jsd_pairs(pool, pairs)
    t_call = time.perf_counter() - t0
    t0 = time.perf_counter()
    api.remove_spurious(data, res, R, seed=0)
    t_e2e = time.perf_counter() - t0
    import jsd_ref as J
    sample = pairs[np.linspace(0, len(pairs) - 1, min(8, len(pairs))).astype(int)]
    t0 = time.perf_counter()
    for a, b in sample:
        J.jsd_calc(pool[:, a], pool[:, b])
    t_ref = (time.perf_counter() - t0) / len(sample) * len(pairs) * len(data)
    rec = {"case": name, "views": len(data), "n": [d.shape[0] for d in data], "k": k, "num_repeats": R,
           "pairs_per_view": int(len(pairs)), "shuffle_sweeps": sweeps, "shuffles_s": t_shuffle,
           "scoring_s": t_score, "jsd_call_view0_s": t_call, "remove_spurious_s": t_e2e,
           "numpy_restatement_s_est": t_ref}
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--scoring-only", action="store_true",
                    help="only resnmtf_jsd_pairs on F-like pools of c2's shape, k = 16 and 64 (for a kernel trace)")
    a = ap.parse_args()
    if a.scoring_only:
        rng = np.random.default_rng(0)
        for k in (16, 64):
            f = rng.random((10000, 6 * k)) ** 6
            pool = f / f.sum(axis=0)
            null_p, score_p = spurious.pool_pairs(k, 5)
            pairs = np.concatenate([null_p, score_p])
            for _ in range(3):
                t0 = time.perf_counter()
                jsd_pairs(pool, pairs)
                print(json.dumps({"case": f"jsd_pairs c2 shape k={k}", "pairs": int(len(pairs)),
                                  "wall_s": time.perf_counter() - t0}), flush=True)
        return
    measure("planted", planted(), 3, 5, None, a.out)
    c2 = synth.config("c2")
    measure("c2 k=16", c2.data, 16, 5, 500, a.out)
    if not a.quick:
        measure("c2 shape k=64", c2.data, 64, 5, 500, a.out)


if __name__ == "__main__":
    main()
