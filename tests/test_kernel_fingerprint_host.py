"""The device code of the built library is the committed baseline, kernel by kernel: a
change that is meant to leave the kernels alone finds out here, on a machine without a GPU, whether it did; a change
that is meant to touch them regenerates ``profiles/kernel_fingerprint.txt`` (``tools/kernel_fingerprint.py``) and the diff
of that file shows the reviewer which kernels moved."""
import contextlib
import importlib.util
import io
import os

import pytest

from helpers import ROOT

BASELINE = os.path.join(ROOT, "profiles", "kernel_fingerprint.txt")


def _tool_module():
    spec = importlib.util.spec_from_file_location("kernel_fingerprint", os.path.join(ROOT, "tools", "kernel_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_built_library_matches_the_committed_fingerprint(tmp_path):
    fp = _tool_module()
    try:
        for name in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
            fp.tool(name)
    except SystemExit as e:
        pytest.skip(str(e))
    from resnmtf_amd import build
    lines = fp.fingerprint(build.build(verbose=False))
    fresh = tmp_path / "kernel_fingerprint.txt"
    fresh.write_text("\n".join(lines) + "\n")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = fp.diff(BASELINE, str(fresh))
    assert rc == 0, "the built device code is not profiles/kernel_fingerprint.txt:\n" + out.getvalue()
