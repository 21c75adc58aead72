"""What the fp64 path gains from reading device memory (resnmtf_fp64_run_device), on one GPU.

    python tools/time_fp64_device.py [--part calls|images|colsum|all] [--quick] [--out profiles/time_fp64_device.jsonl]

calls:   whole-call wall time of engine.fp64_run, 20 fixed sweeps, from host arrays (the host staging: two padded images
         built on the host and copied over the bus, results downloaded) against the SAME values as device tensors
         (output="torch": nothing of size n or m crosses the bus), in this session: c2's shape (10000 x 2000, k = 16) as
         fp64 row-major and as fp32 row-major, 4096 x 4096 (k = 16) and one c5 view (50000 x 8000, k = 64) when the
         device and the host have room.  Best of three after a warm-up (the c5 view: one run after a warm-up); the
         device route is synchronised before the clock stops.  The results of the two routes are compared bit for bit.
images:  fp64_images_kernel alone, from the kernel trace of a child process (rocprofv3 --kernel-trace --stats; the child
         makes one device-route call per case): GB/s over bytes read + bytes of both images written, beside a
         hipMemcpyDtoD that moves the same number of bytes (half of them read, half written) timed in this session.
colsum:  the whole-call cost of leaving lambda / mu to fp64_colsum_seq_kernel at 50000 x 64 (section 17's shape): a
         device-route call with them given against one without, one sweep each, and the kernel's own time from the trace.
Prints one JSON line per measurement and writes them to --out.  Recorded figures, not assertions."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd import synth  # noqa: E402
from resnmtf_amd.engine import fp64_plan, fp64_run  # noqa: E402

LINES = []
SWEEPS = 20
CASES = [("c2 fp64 row-major", 10000, 2000, 16, "float64"), ("c2 fp32 row-major", 10000, 2000, 16, "float32"),
         ("4096 x 4096", 4096, 4096, 16, "float64"), ("c5 view", 50000, 8000, 64, "float64")]


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def case_tensors(n, m, k, dtype, seed=0):
    """A column-normalised non-negative view of the dtype, row-major on the device, and its start (fp64, on the device)."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    x = rng.random((n, m), dtype=np.float32 if dtype == "float32" else np.float64)
    x /= x.sum(axis=0, dtype=np.float64)[None, :].astype(x.dtype)
    f, s, g = synth.random_init(n, m, k, seed + 1)
    view = torch.as_tensor(x, device=dev)
    return view, [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (f, s, g)]


def best_of(fn, reps):
    fn()                                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def image_bytes(n, m, k, itemsize):
    """Bytes fp64_images_kernel reads (the source once) and writes (the n x m entries of both images)."""
    return n * m * itemsize, 2 * n * m * 8


def calls_part(quick):
    import torch
    for name, n, m, k, dtype in CASES[:3] if quick else CASES:
        try:
            view, (f, s, g) = case_tensors(n, m, k, dtype)
            there = {"data": [view], "k": k, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": SWEEPS}
            # (column-major already, as the C entry reads it: the host call is charged its staging, not a re-layout)
            host = {key: [np.asfortranarray(t.double().cpu().numpy()) for t in val] if isinstance(val, list) else val
                    for key, val in there.items()}
            big = n * m >= 1 << 28
            out = {}

            def run_there():
                out["there"] = fp64_run(there, output="torch")
                torch.cuda.synchronize()

            def run_host():
                out["host"] = fp64_run(host)
            t_there = best_of(run_there, 1 if big else 3)
            t_host = best_of(run_host, 1 if big else 3)
            same = all(np.array_equal(a.cpu().numpy(), b) for key in ("f", "s", "g", "lambda", "mu")
                       for a, b in zip(out["there"][key], out["host"][key])) and np.array_equal(out["there"]["all_error"], out["host"]["all_error"])
            emit({"part": "calls", "case": name, "n": n, "m": m, "k": k, "dtype": dtype, "sweeps": SWEEPS,
                  "host_call_s": round(t_host, 4), "device_call_s": round(t_there, 4), "host_over_device": round(t_host / t_there, 2),
                  "bitwise_equal": bool(same), "ld": fp64_plan(n, m, k)["ld"]})
            del view, f, s, g, there, host, out
            torch.cuda.empty_cache()
        except (MemoryError, RuntimeError) as exc:                  # (no room for the c5 view: said, not hidden)
            emit({"part": "calls", "case": name, "n": n, "m": m, "k": k, "dtype": dtype, "skipped": str(exc)[:200]})


def memcpy_dtod_gb_per_s(total_bytes):
    """hipMemcpyDtoD of total_bytes / 2 (as many bytes read, as many written: total_bytes moved), best of five."""
    import torch
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    hip.hipDeviceSynchronize.argtypes = []
    half = total_bytes // 2
    src = torch.ones(half // 8 + 1, dtype=torch.float64, device="cuda:0")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()

    def copy():
        assert hip.hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), half) == 0
        assert hip.hipDeviceSynchronize() == 0
    t = best_of(copy, 5)
    return 2 * half / t / 1e9, t


def traced_child(part, quick):
    """Run this tool's child part under the kernel trace; {kernel name: (calls, average ns, min ns)} of its stats."""
    out_dir = tempfile.mkdtemp(prefix="time_fp64_device_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable,
           os.path.abspath(__file__), "--part", part] + (["--quick"] if quick else [])
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                rows[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]))
    return rows


def images_child(quick):
    """One device-route call per case, one sweep: each launches fp64_images_kernel once (distinct template instances or
    call order tell the cases apart: the trace lists fp64 and fp32 sources under their own names)."""
    for name, n, m, k, dtype in CASES[:3] if quick else CASES:
        try:
            view, (f, s, g) = case_tensors(n, m, k, dtype)
            fp64_run({"data": [view], "k": k, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": 1}, output="torch")
        except (MemoryError, RuntimeError):
            pass


def images_part(quick):
    """The fp32 case has an instance of its own; the fp64 cases share one, so each is traced in a child of its own."""
    for case in (CASES[:3] if quick else CASES):
        name, n, m, k, dtype = case
        rows = traced_child("images-child:" + name, quick)
        hits = {kn: v for kn, v in rows.items() if "fp64_images_kernel" in kn}
        if len(hits) != 1:
            emit({"part": "images", "case": name, "skipped": f"{len(hits)} fp64_images_kernel rows in the trace"})
            continue
        (kernel, (calls, avg_ns, min_ns)), = hits.items()
        rd, wr = image_bytes(n, m, k, 4 if dtype == "float32" else 8)
        copy_gbs, copy_s = memcpy_dtod_gb_per_s(rd + wr)
        emit({"part": "images", "case": name, "n": n, "m": m, "dtype": dtype, "kernel": kernel, "calls": calls,
              "kernel_us": round(avg_ns / 1e3, 1), "bytes_read": rd, "bytes_written": wr,
              "kernel_gb_per_s": round((rd + wr) / avg_ns, 1), "memcpy_dtod_us": round(copy_s * 1e6, 1),
              "memcpy_dtod_gb_per_s": round(copy_gbs, 1), "kernel_over_memcpy": round((rd + wr) / avg_ns / copy_gbs, 3)})


def colsum_problem(with_lm):
    import torch
    n, m, k = 50000, 64, 64
    view, (f, s, g) = case_tensors(n, m, k, "float64", seed=3)
    p = {"data": [view], "k": k, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": 1}
    if with_lm:
        p.update(init_lam=[f.sum(0)], init_mu=[g.sum(0)])
    torch.cuda.synchronize()
    return p


def colsum_part(quick):
    import torch

    def call(p):
        fp64_run(p, output="torch")
        torch.cuda.synchronize()
    given, summed = colsum_problem(True), colsum_problem(False)
    t_given, t_summed = best_of(lambda: call(given), 5), best_of(lambda: call(summed), 5)
    rows = traced_child("colsum-child", quick)
    hits = [v for kn, v in rows.items() if "fp64_colsum_seq_kernel" in kn]
    emit({"part": "colsum", "n": 50000, "m": 64, "k": 64, "call_given_ms": round(t_given * 1e3, 3),
          "call_summed_ms": round(t_summed * 1e3, 3), "kernel_us": round(hits[0][1] / 1e3, 1) if hits else None,
          "kernel_calls": hits[0][0] if hits else 0})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fp64_device.jsonl"))
    a = ap.parse_args()
    if a.part.startswith("images-child:"):                          # (under the kernel trace: no output file)
        global CASES
        CASES = [c for c in CASES if c[0] == a.part.split(":", 1)[1]]
        return images_child(False)
    if a.part == "colsum-child":
        return fp64_run(colsum_problem(False), output="torch")
    if a.part not in ("calls", "images", "colsum", "all"):
        ap.error("--part must be calls, images, colsum or all")
    if a.part in ("calls", "all"):
        calls_part(a.quick)
    if a.part in ("images", "all"):
        images_part(a.quick)
    if a.part in ("colsum", "all"):
        colsum_part(a.quick)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
