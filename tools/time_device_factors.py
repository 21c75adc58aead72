"""Wall times of the factor routes through device memory against the host routes, on one GPU.

    python tools/time_device_factors.py [--quick] [--out FILE]

For initial factors that lie in device memory as torch tensors, medians of 5 calls after a warm-up call, wall time with
``torch.cuda.synchronize()`` before and after:
* ``Engine.set_factors_device(f, s, g)`` of fp64 column-major, fp64 row-major and fp32 row-major tensors -- the device
  route -- and once more with lambda and mu given (no column sums: the difference is the sequential sum's time);
* what a caller had to do before it: ``Engine.set_factors(*(t.double().cpu().numpy() for t in (f, s, g)))``;
* ``Engine.get_factors_device`` against ``Engine.get_factors``.
Shapes: c2's (10000 x 2000, k = 16) and c5's (50000 x 8000, k = 64; ``--quick`` skips it).  Prints one JSON line per
measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd.engine import Engine  # noqa: E402

DEV = torch.device("cuda", 0)


def median_time(fn, reps=5):
    fn()                                               # warm-up: library load, first launches, allocations
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times))


def emit(rec, out):
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def time_case(name, n, m, k, out):
    g = torch.Generator(device=DEV).manual_seed(5)
    f, s, w = (torch.rand(shape, device=DEV, generator=g, dtype=torch.float64) + 0.1 for shape in ((n, k), (k, k), (m, k)))
    inputs = {"fp64 column-major": [t.T.contiguous().T for t in (f, s, w)],
              "fp64 row-major": [f, s, w],
              "fp32 row-major": [t.float() for t in (f, s, w)]}
    lam, mu = f.sum(0), w.sum(0)
    case = f"{name}: {n} x {m}, k = {k}"
    with Engine([n], [m], [k]) as eng:
        for label, ts in inputs.items():
            dev = median_time(lambda: eng.set_factors_device(0, *ts))
            given = median_time(lambda: eng.set_factors_device(0, *ts, lam, mu))
            hst = median_time(lambda: eng.set_factors(0, *(t.double().cpu().numpy() for t in ts)))
            emit({"case": case, "call": "set_factors_device", "input": label, "device_s": dev[0], "device_min_max_s": dev[1:],
                  "device_given_lm_s": given[0], "host_route_s": hst[0], "host_route_min_max_s": hst[1:],
                  "ratio": hst[0] / dev[0]}, out)
        dev = median_time(lambda: eng.get_factors_device(0))
        hst = median_time(lambda: eng.get_factors(0))
        emit({"case": case, "call": "get_factors_device", "device_s": dev[0], "device_min_max_s": dev[1:], "host_route_s": hst[0],
              "host_route_min_max_s": hst[1:], "ratio": hst[0] / dev[0]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    for name, n, m, k in (("c2", 10000, 2000, 16),) + (() if a.quick else (("c5", 50000, 8000, 64),)):
        time_case(name, n, m, k, a.out)


if __name__ == "__main__":
    main()
