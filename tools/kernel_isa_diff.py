#!/usr/bin/env python3
"""tools/kernel_isa_diff.py — are the kernels of two builds the same machine code? Runs without a GPU.

    python tools/kernel_isa_diff.py <build dir A> <build dir B> [object name ...]

For every named object (default: the four winner-only translation units of polar_kernels.hip and polar_kernels_sc.hip) the gfx950
code object is extracted from both builds (llvm-objdump --offloading) and disassembled; every function symbol is compared
instruction by instruction — mnemonic, operands and encoding, the address column dropped. Prints one line per object and
the symbols that differ, are missing or are new; exit status 1 if any kernel differs.
"""
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
DEFAULT = ["polar_kernels.hip.o", "polar_kernels.hip.ed.o", "polar_kernels.hip.ed32.o", "polar_kernels.hip.lat.o", "polar_kernels_sc.hip.o"]


def kernels(obj):
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, os.path.basename(obj))
        subprocess.check_call(["cp", obj, tmp])
        subprocess.check_call([OBJDUMP, "--offloading", tmp], stdout=subprocess.DEVNULL, cwd=d)
        co = [f for f in os.listdir(d) if "amdgcn" in f]
        assert co, "no device code object in " + obj
        text = subprocess.check_output([OBJDUMP, "-d", os.path.join(d, co[0])], text=True)
    out = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, flags=re.S | re.M):
        body = []
        for l in m.group(2).split("\n"):
            q = re.match(r"\s+(.*?)\s*//\s*[0-9A-F]+:\s*(.*)$", l)
            if q:
                body.append((q.group(1), q.group(2)))
        out[m.group(1)] = body
    return out


def main():
    a, b = sys.argv[1], sys.argv[2]
    bad = 0
    for name in sys.argv[3:] or DEFAULT:
        ka, kb = kernels(os.path.join(a, name)), kernels(os.path.join(b, name))
        diff = sorted(k for k in ka if k in kb and ka[k] != kb[k])
        gone, new = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        print("%-28s %3d symbols, %7d instructions: %d differ, %d missing, %d new" %
              (name, len(ka), sum(len(v) for v in ka.values()), len(diff), len(gone), len(new)))
        for k in diff + gone + new:
            print("    ", "differs" if k in diff else "missing" if k in gone else "new", k)
        bad += len(diff) + len(gone) + len(new)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
