#!/usr/bin/env python3
"""Fingerprint of the device code in a built libresnmtf_hip.so, to show that a host-side change left the kernels alone:

    python tools/kernel_fingerprint.py [resnmtf_amd/libresnmtf_hip.so] > profiles/kernel_fingerprint.txt
    python tools/kernel_fingerprint.py --diff OLD.txt NEW.txt

The library's .hip_fatbin section holds one offload bundle per translation unit.  Each bundle's gfx950 code object is
unbundled and, per kernel symbol, one line is printed: a SHA-256 (first 16 hex digits) of its disassembled instruction text
with the addresses and encodings stripped, and its register / LDS / scratch figures from the code object's metadata note.
Equal lines = the same instructions and the same resources.  Needs the LLVM tools of the ROCm installation."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def tool(name):
    for cand in (shutil.which(name), "/opt/rocm/llvm/bin/" + name, "/opt/rocm/lib/llvm/bin/" + name):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit(name + " not found (ROCm LLVM tools)")


def code_objects(so, tmp):
    """The gfx950 code object of every offload bundle in the library, in file order."""
    fatbin = os.path.join(tmp, "fatbin")
    subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, so, os.path.join(tmp, "copy.so")], check=True)
    blob = open(fatbin, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    out = []
    for i, s in enumerate(starts):
        bundle, co = os.path.join(tmp, f"bundle{i}"), os.path.join(tmp, f"unit{i}.co")
        with open(bundle, "wb") as f:
            f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle,
                        "--output=" + co], check=True)
        out.append(co)
    return out


def kernel_resources(co):
    """{kernel name: resource figures} from the amdhsa.kernels metadata."""
    notes = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    res = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk

        def get(key):
            m = re.search(r"\." + key + r":\s+(\S+)", blk)
            return m.group(1) if m else "?"
        res[get("name").strip("'\"")] = " ".join(f"{key}={get(key)}" for key in RESOURCES)
    return res


def kernel_hashes(co, names):
    """{kernel name: hash of its instruction text}: mnemonic and operands of every line between the symbol's label and the next."""
    dis = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
                         capture_output=True, text=True).stdout
    hashes, cur, acc = {}, None, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            if cur in names:
                hashes[cur] = acc.hexdigest()[:16]
            cur, acc = m.group(1), hashlib.sha256()
            continue
        if cur is None or not line.strip():
            continue
        text = re.sub(r"\s*//.*$", "", line).strip()      # (the trailing comment carries the address and the encoding)
        acc.update((text + "\n").encode())
    if cur in names:
        hashes[cur] = acc.hexdigest()[:16]
    return hashes


def fingerprint(so):
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for unit, co in enumerate(code_objects(so, tmp)):
            res = kernel_resources(co)
            hashes = kernel_hashes(co, set(res))
            # kernel_resources relies on `.agpr_count` opening each kernel's map in the note and on `.name` of the kernel
            # being the first `.name` after it (kernel arguments carry none): refuse to print a baseline if that breaks
            for name in sorted(res):
                if name == "?" or "?" in res[name] or name not in hashes:
                    raise SystemExit(f"unit{unit}: kernel {name!r}: metadata or disassembly not understood ({res[name]})")
                lines.append(f"unit{unit} {name} {hashes[name]} {res[name]}")
    if not lines:
        raise SystemExit("no kernels found in " + so)
    return lines


def diff(old, new):
    def load(path):
        return {" ".join(l.split()[:2]): l.strip() for l in open(path) if l.strip() and not l.startswith("#")}
    a, b = load(old), load(new)
    bad = 0
    for key in sorted(set(a) | set(b)):
        if key not in b:
            print("dropped ", key)
        elif key not in a:
            print("added   ", key)
        elif a[key] != b[key]:
            print("changed ", a[key], "\n      -> ", b[key])
        else:
            continue
        bad += 1
    print(f"{len(a)} kernels before, {len(b)} after, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        raise SystemExit(diff(sys.argv[2], sys.argv[3]))
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "resnmtf_amd", "libresnmtf_hip.so")
    print("# tools/kernel_fingerprint.py: <unit> <kernel symbol> <hash of instruction text> <resources>")
    print("\n".join(fingerprint(so)))
