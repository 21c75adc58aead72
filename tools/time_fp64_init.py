"""Wall time and peak transient device memory of the START of an fp64 fit: engine.fp64_init_svd
(what res_nmtf_inner(precision="fp64", fp64_init=True) calls) against the route the fp64 path took before -- a
short-lived f32 Engine built, loaded, resnmtf_init_svd, the factors read back, the engine closed -- on one GPU.

    python tools/time_fp64_init.py [--quick] [--reps 5] [--out profiles/time_fp64_init.jsonl]

Shapes: 10000 x 2000 at k = 16 and 50000 x 8000 at k = 64 (dense), 10000 x 2000 at k = 16 with 1 % and 5 % stored (sparse);
--quick: 2000 x 500 at k = 16 and one sparse 2000 x 500.  Each shape from host memory (a NumPy array, a scipy.sparse CSC;
the start returned as NumPy arrays) and from device memory (an fp64 tensor, a sparse_csc tensor; the start left on the
device).  Per route the median, minimum and maximum of `reps` blocking calls after a warm-up, all in this session, and the
peak of (free device memory before the call) - (free device memory during it), sampled by a thread every 0.2 ms through
hipMemGetInfo: a lower bound of the true peak.  Prints one JSON line per measurement and writes them to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

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


def engine_route(view, k, on_device):
    """The start of res_nmtf_inner(precision="fp64") without fp64_init: api._res_nmtf_inner_fp64's own steps."""
    data = api._views([view])
    sp_view = hasattr(data[0], "nnz")
    more = {"nnz": [data[0].nnz]} if sp_view else {}
    rn, cn = naming.give_names(data, None, None, None, None)
    z = np.zeros((1, 1))
    eng = Engine([data[0].shape[0]], [data[0].shape[1]], [k], **more)
    try:
        api._load_engine(eng, data, None, None, None, None, None, z, z, z, rn, cn, naming.shared_names(rn), naming.shared_names(cn), seed=1)
        return (eng.get_factors_device if on_device else eng.get_factors)(0)
    finally:
        eng.close()


def fp64_route(view, k, on_device):
    return engine.fp64_init_svd([view], k, seed=1, output="torch" if on_device else "numpy")[0]


def peak_bytes(fn):
    """Free device memory before the call minus the least seen during it (sampled: a lower bound)."""
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    least, stop = [before], threading.Event()

    def sample():
        while not stop.is_set():
            least[0] = min(least[0], torch.cuda.mem_get_info()[0])
            time.sleep(2e-4)
    t = threading.Thread(target=sample)
    t.start()
    try:
        out = fn()
    finally:
        stop.set()
        t.join()
    del out
    return int(before - least[0])


def one_shape(name, host_view, device_view, k, reps):
    for where, view, on_device in (("host", host_view, False), ("device", device_view, True)):
        rec = {"shape": name, "source": where, "k": k, "columns": f"median, min, max of {reps} blocking calls after a warm-up"}
        for route, fn in (("fp64_init_svd", fp64_route), ("f32_engine_route", engine_route)):
            rec[route + "_ms"] = median_ms(lambda: fn(view, k, on_device), reps)
            rec[route + "_peak_transient_bytes"] = peak_bytes(lambda: fn(view, k, on_device))
        rec["fp64_over_engine"] = round(rec["fp64_init_svd_ms"][0] / rec["f32_engine_route_ms"][0], 3)
        emit(rec)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_init.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    dense = [(2000, 500, 16)] if a.quick else [(10000, 2000, 16), (50000, 8000, 64)]
    for n, m, k in dense:
        x = rng.random((n, m)) + 0.01
        x = np.asfortranarray(x / x.sum(axis=0))
        t = torch.as_tensor(x, device=dev)
        one_shape(f"dense {n} x {m}", x, t, k, a.reps)
        del x, t
    n, m = (2000, 500) if a.quick else (10000, 2000)
    for density in ((0.05,) if a.quick else (0.01, 0.05)):
        xs = random_view(n, m, density, 5)
        one_shape(f"sparse {n} x {m}, {density:.0%} stored ({xs.nnz} entries)", xs, device_csc(xs, dev), 16, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
