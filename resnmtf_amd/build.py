"""In-tree build of libresnmtf_hip.so for gfx950 (hipcc cross-compiles without a GPU).

    python -m resnmtf_amd.build [--force]

compile_units() is the project's one compile recipe: the product build below, tools/build_variant.py and the stamp builds
of tools/stamps*.py all go through it.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libresnmtf_hip.so")
# the main unit: the host side and every kernel but the k <= 16 streaming pass
SWEEP = "resnmtf_hip.hip"
# the k <= 16 streaming pass: a translation unit of its own, compiled with the max-ILP machine scheduler (csrc/resnmtf_split_tu.h)
PASS_K16 = "resnmtf_pass_k16.hip"
PASS_K16_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# the device-wide fp64 path (resnmtf_fp64_run): host side and kernels in a unit, and so a code object, of their own
FP64 = "resnmtf_fp64.hip"
UNITS = [SWEEP, PASS_K16, FP64]
ARCH = "--offload-arch=gfx950"


def deps() -> list:
    """Everything a unit may include: the whole of csrc/ and the public header."""
    return [os.path.join(CSRC, name) for name in sorted(os.listdir(CSRC))] + [os.path.join(ROOT, "include", "resnmtf_hip.h")]


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def needs_build() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in deps())


def compile_units(out: str, defines=(), unit_flags=None, one_code_object: bool = False, verbose: bool = True) -> str:
    """Compile the units, side by side, and link them into `out`.

    defines: extra -D... of every unit.  unit_flags: {unit: extra flags}; PASS_K16_FLAGS is the default for PASS_K16.
    one_code_object: the main unit instantiates the k <= 16 passes itself (no -DRESNMTF_SPLIT_TU) and PASS_K16 is left
    out, so that every kernel of the sweep sits in one code object (the stamp builds: their buffer is per code object).
    Objects go to a temporary directory; `out` is replaced only by a library that linked."""
    flags = {PASS_K16: PASS_K16_FLAGS, **(unit_flags or {})}
    units = [u for u in UNITS if not (one_code_object and u == PASS_K16)]
    common = [hipcc_path(), ARCH, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + list(defines)
    tmp = tempfile.mkdtemp(prefix="resnmtf_build_")
    staged = out + ".%d.tmp" % os.getpid()      # (same directory as `out`: os.replace does not cross file systems)
    try:
        objs = [os.path.join(tmp, u + ".o") for u in units]
        cmds = [common + ([] if one_code_object or u != SWEEP else ["-DRESNMTF_SPLIT_TU"]) + list(flags.get(u, [])) +
                ["-c", os.path.join(CSRC, u), "-o", obj] for u, obj in zip(units, objs)]
        linked = os.path.join(tmp, os.path.basename(out))
        link = [hipcc_path(), ARCH, "-fPIC", "-shared", "-o", linked] + objs
        if verbose:
            for cmd in cmds:
                print("[resnmtf_amd.build]", " ".join(cmd), flush=True)
        procs = [subprocess.Popen(cmd) for cmd in cmds]      # (one process per unit)
        codes = [p.wait() for p in procs]
        for code, cmd in zip(codes, cmds):
            if code != 0:
                raise subprocess.CalledProcessError(code, cmd)
        if verbose:
            print("[resnmtf_amd.build]", " ".join(link), flush=True)
        subprocess.run(link, check=True)
        shutil.move(linked, staged)
        os.replace(staged, out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        if os.path.exists(staged):
            os.remove(staged)
    return out


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not needs_build():
        return OUT
    return compile_units(OUT, verbose=verbose)


if __name__ == "__main__":
    build(force="--force" in sys.argv)
