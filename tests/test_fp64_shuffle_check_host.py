"""The host-only half of resnmtf_fp64_shuffle (csrc/resnmtf_fp64_shuffle_job.h, csrc/resnmtf_feistel.h; DESIGN.md section
27) from plain C++: tests/host/fp64_shuffle_check.cpp is compiled with g++ -std=c++17 against those headers and
include/resnmtf_hip.h alone -- no HIP, no library -- and run.  It checks every struct refusal, the extents, the overlap
test, the workspace layout, and the Feistel permutation both translation units and this program share: a bijection on
[0, count) for every count in 1 .. 4100 and three seeds, inverse after forward the identity."""
import os
import subprocess

from helpers import ROOT


def test_fp64_shuffle_check_compiles_without_hip_and_passes(tmp_path):
    exe = str(tmp_path / "fp64_shuffle_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "resnmtf_amd", "csrc"), os.path.join(ROOT, "tests", "host", "fp64_shuffle_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "fp64_shuffle_check: 15 refusals, 4100 counts (4094 with a cycle walk) x 3 seeds, all checks passed" in r.stdout
