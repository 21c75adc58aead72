#!/usr/bin/env python3
"""Diagnostic: build the library with other compiler flags per translation unit, for A/B runs through tools/run_with_lib.py:
    python tools/build_variant.py <tag> "<flags of the main unit>" "<flags of the k <= 16 pass unit>"
-> tools/micro/libresnmtf_<tag>.so   (empty string = none; the product's own flags: resnmtf_amd/build.py)"""
import os
import shlex
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnmtf_amd import build as B  # noqa: E402

tag, main_flags, k16_flags = sys.argv[1], shlex.split(sys.argv[2]), shlex.split(sys.argv[3])
out = os.path.join(ROOT, "tools", "micro", f"libresnmtf_{tag}.so")
B.compile_units(out, unit_flags={B.SWEEP: main_flags, B.PASS_K16: k16_flags})
print("built", out)
