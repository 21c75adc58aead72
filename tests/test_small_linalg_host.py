"""The L x L linear algebra of the SVD initialisation (csrc/resnmtf_small_linalg.h) from plain C++:
tests/host/small_linalg_check.cpp is compiled with g++ -std=c++17 against that header alone -- no HIP, no library -- twice,
plainly and with the host's address and undefined-behaviour sanitizers, and both programs are run.  It checks
cholesky_upper (with a cut column, and the NaN return), invert_upper and jacobi_eigen against brute force at 16 x 16 ...
64 x 64, two of the matrices rank-deficient.  The header is the one text both translation units include."""
import os
import subprocess

import pytest

from helpers import ROOT

SOURCE = os.path.join(ROOT, "tests", "host", "small_linalg_check.cpp")
HEADER = os.path.join(ROOT, "resnmtf_amd", "csrc", "resnmtf_small_linalg.h")


@pytest.mark.parametrize("name, flags", [("plain", ["-O1"]),
                                         ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_small_linalg_check_compiles_without_hip_and_passes(tmp_path, name, flags):
    exe = str(tmp_path / ("small_linalg_check_" + name))
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + os.path.join(ROOT, "resnmtf_amd", "csrc"), SOURCE,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "small_linalg_check: 7 cases, all checks passed" in r.stdout


def test_one_text_for_both_translation_units():
    """The three functions are defined in the header alone, and both units include it."""
    csrc = os.path.dirname(HEADER)
    header = open(HEADER).read()
    assert "#include <hip" not in header and "__global__" not in header
    for fn in ("cholesky_upper(const", "invert_upper(const", "jacobi_eigen(std::vector"):
        assert header.count(fn) == 1
        for unit in ("resnmtf_hip.hip", "resnmtf_fp64.hip"):
            assert fn not in open(os.path.join(csrc, unit)).read(), (fn, unit)
    for unit in ("resnmtf_hip.hip", "resnmtf_fp64.hip"):
        assert '#include "resnmtf_small_linalg.h"' in open(os.path.join(csrc, unit)).read()
