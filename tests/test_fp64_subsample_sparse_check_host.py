"""The host-only half of resnmtf_fp64_subsample_sparse (csrc/resnmtf_fp64_subsample_sparse_job.h)
from plain C++: tests/host/fp64_subsample_sparse_check.cpp is compiled with g++ -std=c++17 against that header and
include/resnmtf_hip.h alone -- no HIP, no library -- and run.  It checks the struct refusals with their texts, count mode
against fill mode, the index-list checks, the extents and overlaps of the outputs and of a device view's arrays, that
every region of the workspace is claimed once and is large enough, and the transient byte count.  The second test builds
the same stand-alone program under AddressSanitizer and UBSan and runs it clean."""
import os
import subprocess

from helpers import ROOT

SRC = os.path.join(ROOT, "tests", "host", "fp64_subsample_sparse_check.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "resnmtf_amd", "csrc")]
DONE = "fp64_subsample_sparse_check: 23 refusals, 3 list refusals, 70 workspace cases, all checks passed"


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert DONE in r.stdout
    return r


def test_fp64_subsample_sparse_check_compiles_without_hip_and_passes(tmp_path):
    _build_and_run(tmp_path, "fp64_subsample_sparse_check", ["-O1"])


def test_fp64_subsample_sparse_check_runs_clean_under_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, "fp64_subsample_sparse_check_san",
                       ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
