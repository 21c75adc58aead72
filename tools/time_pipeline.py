"""Wall times of the reference's default pipeline with spurious removal inside it on one GPU.

    python tools/time_pipeline.py [--skip-c2] [--out FILE]

toy: the reference test's problem (test-resnmtf.R:38-52, two 180 x 180 views with three planted blocks),
``apply_resnmtf(data, k_sweep=True, spurious_on_device=True)`` -- k sweep 3..8, 5 shuffled repeats per k, 5 stability
draws, each with its own 5 shuffles.  c2: one 10000 x 2000 view (synth.config("c2")), ``apply_resnmtf(data, k_val=16,
spurious_on_device=True)``.  Each is run once to warm up, then timed end to end (host pre-processing included).  The
share of the shuffled factorisations is the time spent in ``problem.shuffled_engines`` (draws, SVD inits and the loops
to convergence; blocking), the scoring share the time in ``Engine.spurious_scores``.  Prints one JSON line per run."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import resnmtf_amd  # noqa: E402
from resnmtf_amd import problem, spurious, synth  # noqa: E402
from resnmtf_amd.engine import Engine  # noqa: E402

_T = {"shuffles": 0.0, "shuffle_fits": 0, "scores": 0.0, "score_calls": 0}


def _wrap():
    inner_sh, inner_sc = problem.shuffled_engines, Engine.spurious_scores

    def shuffled_engines(src, k, num_repeats, *a, **kw):
        t = time.perf_counter()
        out = inner_sh(src, k, num_repeats, *a, **kw)
        _T["shuffles"] += time.perf_counter() - t
        _T["shuffle_fits"] += num_repeats
        return out

    def spurious_scores(self, v, shuffles):
        t = time.perf_counter()
        out = inner_sc(self, v, shuffles)
        _T["scores"] += time.perf_counter() - t
        _T["score_calls"] += 1
        return out

    spurious.shuffled_engines = shuffled_engines          # (the name check_on_device calls)
    Engine.spurious_scores = spurious_scores


def planted(seed):
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1))); cc = np.kron(np.eye(3), np.ones((60, 1)))
    return rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + 0.1 * np.abs(rng.normal(size=(180, 180)))


def timed(name, fn):
    fn()                                                        # warm-up
    for key in _T:
        _T[key] = 0 if isinstance(_T[key], int) else 0.0
    t = time.perf_counter()
    res = fn()
    wall = time.perf_counter() - t
    out = {"case": name, "wall_s": round(wall, 4), "shuffle_s": round(_T["shuffles"], 4),
           "shuffle_share": round(_T["shuffles"] / wall, 4), "shuffle_fits": _T["shuffle_fits"],
           "scores_s": round(_T["scores"], 4), "score_calls": _T["score_calls"],
           "k": int(res["output_f"][0].shape[1]),
           "removed": [int(x) for x in np.asarray(res["spurious"]["removed"]).sum(axis=1)],
           "kept_row_clusters": [int(np.asarray(rc).any(axis=0).sum()) for rc in res["row_clusters"]]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-c2", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _wrap()
    rows = []
    toy = [planted(1), planted(2)]
    rows.append(timed("toy: 2 views 180x180, k sweep 3..8, 5 repeats, 5 stability draws",
                      lambda: resnmtf_amd.apply_resnmtf(toy, k_sweep=True, seed=7, spurious_on_device=True)))
    if not args.skip_c2:
        prob = synth.config("c2")
        rows.append(timed("c2: 1 view 10000x2000, k_val=16, 5 repeats, 5 stability draws",
                          lambda: resnmtf_amd.apply_resnmtf(prob.data, k_val=16, seed=7, spurious_on_device=True)))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
