"""The host-only description of an fp64 job (csrc/resnmtf_fp64_job.h) from plain C++:
tests/host/fp64_job_check.cpp is compiled with g++ -std=c++17 against that header and include/resnmtf_hip.h alone -- no
HIP, no library -- and run.  It checks the layout of the job's one device buffer over a table of jobs (every region
inside the buffer, disjoint at the extent its consumer addresses), the CSC check, the CSR build and the two struct
checks that need no device.

It also prints ``fp64_col_sum`` of every column of a fixed non-dyadic V x V matrix for V = 1 .. 8; this file rebuilds the
matrix and requires each sum to be ``np.sum`` of that column bit for bit -- the oracle branches on those sums and puts
them into every denominator, and at V = 8 numpy leaves the sequential order for its 8-accumulator pairwise form, which
no entry-by-entry bar of a GPU test can see."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT


@pytest.fixture(scope="module")
def printout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fp64_job_check") / "fp64_job_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "resnmtf_amd", "csrc"), os.path.join(ROOT, "tests", "host", "fp64_job_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout


def test_fp64_job_check_compiles_without_hip_and_passes(printout):
    assert "fp64_job_check: 10 jobs, all checks passed" in printout


def restriction(V: int) -> np.ndarray:
    """The matrix of check_col_sums: R[w, v] = 1 / (3 + 6 w + 10 v): odd denominators, so no entry is dyadic; one correctly
    rounded division per entry."""
    w, v = np.meshgrid(np.arange(V), np.arange(V), indexing="ij")
    return 1.0 / (3 + 6 * w + 10 * v).astype(np.float64)


def _sequential(col) -> float:
    s = 0.0
    for x in col:
        s += float(x)
    return s


def test_col_sums_are_numpys_bit_for_bit(printout):
    got = {(int(V), int(v)): float.fromhex(h) for V, v, h in re.findall(r"^colsum V (\d+) v (\d+): (\S+)$", printout, re.M)}
    assert sorted(got) == [(V, v) for V in range(1, 9) for v in range(V)]
    differs = 0
    for V in range(1, 9):
        M = restriction(V)
        assert np.all(np.frexp(M)[0] != 0.5), "a dyadic entry"
        for v in range(V):
            want = float(np.sum(M[:, v]))
            assert np.float64(got[V, v]).tobytes() == np.float64(want).tobytes(), (V, v, got[V, v].hex(), want.hex())
            if V < 8:
                assert want == _sequential(M[:, v])                 # (numpy itself is sequential below 8 entries)
            else:
                differs += want != _sequential(M[:, v])
    # at V = 8 the two orders must differ somewhere, or the equality above pins nothing
    assert differs >= 1, "no column of the V = 8 matrix tells numpy's pairwise sum from the sequential one"


def test_the_eight_view_cases_meet_the_pairwise_branch():
    """The restriction matrices of ``update_cases``' 8-view bucket problem are among those whose column sums depend on
    the order: on such weights the sequential form would give other bits (the 8-view problem of the fp64 cases is checked
    the same way in tests/test_fp64_update_cases_host.py)."""
    import update_cases as U
    prob = U.bucket_problem(8, 8, 808)
    for name, mat, cols in (("phi", prob.phi, (0, 1)), ("psi", prob.psi, (6,)), ("xi", prob.xi, (0, 3))):
        for v in cols:
            assert float(np.sum(mat[:, v])) != _sequential(mat[:, v]), (name, v)
