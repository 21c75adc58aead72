"""The host-only description of an fp64 job (csrc/resnmtf_fp64_job.h) from plain C++:
tests/host/fp64_job_check.cpp is compiled with g++ -std=c++17 against that header and include/resnmtf_hip.h alone -- no
HIP, no library -- and run.  It checks the layout of the job's one device buffer over a table of jobs (every region
inside the buffer, disjoint at the extent its consumer addresses), the CSC check, the CSR build and the two struct
checks that need no device."""
import os
import subprocess

from helpers import ROOT


def test_fp64_job_check_compiles_without_hip_and_passes(tmp_path):
    exe = str(tmp_path / "fp64_job_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "resnmtf_amd", "csrc"), os.path.join(ROOT, "tests", "host", "fp64_job_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "fp64_job_check: 10 jobs, all checks passed" in r.stdout
