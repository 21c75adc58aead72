"""The host-only half of a bisilhouette call (csrc/resnmtf_bisil_plan.h) from plain C++:
tests/host/fp64_bisil_check.cpp is compiled with g++ -std=c++17 against that header and include/resnmtf_hip.h alone -- no
HIP, no library -- and run.  It checks the index lists (U, masks, members, features, counts) entry by entry against
their definition over a table of cluster matrices, the chunk rule by search, the kq table, the choice of the gather
kernel from the strides, and the workspace of resnmtf_fp64_bisil: every region of the packed lists claimed once, G and the
partials large enough for every side and bicluster."""
import os
import subprocess

from helpers import ROOT


def test_fp64_bisil_check_compiles_without_hip_and_passes(tmp_path):
    exe = str(tmp_path / "fp64_bisil_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "resnmtf_amd", "csrc"), os.path.join(ROOT, "tests", "host", "fp64_bisil_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "fp64_bisil_check: 98 chunk rules, 20 list cases, all checks passed" in r.stdout
