#!/usr/bin/env python3
"""Which kernels of the library's code object changed between two source trees: compiles ecfft_capi.hip of both to gfx950 assembly
(device only) and compares every kernel's instruction stream with label numbers and comments stripped.  Prints the kernels that
differ, the new ones and the ones that are gone, and the count of identical ones.
usage: kernel_isa_diff.py OTHER_ROOT [-DFLAG ...]   (OTHER_ROOT: a checkout of the commit to compare with, e.g. a git worktree)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(root, flags, d, tag):
    asm = os.path.join(d, tag + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "-S", "--cuda-device-only", "-o", asm,
                    os.path.join(root, "ecfft_amd", "csrc", "ecfft_capi.hip")] + flags, check=True, stderr=subprocess.DEVNULL)
    out = {}
    for m in re.finditer(r"^\t\.globl\t(\S+)\n.*?^\1:[^\n]*\n(.*?)^\.Lfunc_end\d+:", open(asm).read(), re.S | re.M):
        out[m.group(1)] = re.sub(r";.*", "", re.sub(r"\.L\w+", ".L", m.group(2)))
    return out


with tempfile.TemporaryDirectory() as d:
    a, b = kernels(sys.argv[1], sys.argv[2:], d, "other"), kernels(ROOT, sys.argv[2:], d, "this")
names = sorted(set(a) | set(b))
dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()))
same = 0
for n in names:
    if n in a and n in b and a[n] == b[n]:
        same += 1
    else:
        print(("differs" if n in a and n in b else "new" if n in b else "gone") + ": " + re.sub(r"^void ", "", dem[n])[:180])
print(f"{same} kernels identical apart from label numbers; {len(a)} in {sys.argv[1]}, {len(b)} in this tree")
