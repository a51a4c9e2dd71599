#!/usr/bin/env python3
"""Instruction-level comparison of every gfx950 kernel of two built libraries (no GPU needed):
    python tools/disassembly_diff.py [--histogram] parent/libmmdx.so [new/libmmdx.so]
Unbundles the code object of every translation unit (as tools/kernel_resources.py does), disassembles it with llvm-objdump, drops
addresses and encodings, and prints: kernels that differ (with a unified diff), the counts, and the kernels only the new library
has.  Kernels are keyed by (code object index, mangled name).
--histogram: for every kernel that differs, the per-mnemonic instruction counts that changed, instead of the unified diff; register
moves, waits and no-ops (s_mov*, v_mov*, s_waitcnt, s_nop) are left out, so a kernel whose instructions were only reordered or
renumbered prints "same mix"."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels_of(so):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        data = open(fat, "rb").read()
        starts = [i for i in range(len(data)) if data.startswith(magic, i)]
        for k, (b, e) in enumerate(zip(starts, starts[1:] + [len(data)])):
            one, co = os.path.join(d, "fat%d.bin" % k), os.path.join(d, "gfx950_%d.co" % k)
            open(one, "wb").write(data[b:e])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + one,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                                  check=True).stdout
            name = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = (k, m.group(1))
                    out[name] = []
                elif name and line.strip():
                    ins = re.sub(r"\s*//.*$", "", line).strip()                 # the address comment
                    ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
                    out[name].append(re.sub(r"\s+", " ", ins))
    return {k: v for k, v in out.items() if not k[1].startswith("__hip_cuid")}


def mix(instructions):
    """Instructions per mnemonic, without the ones that only move registers or wait."""
    names = (i.split(" ", 1)[0] for i in instructions)
    return collections.Counter(n for n in names if not n.startswith(("s_mov", "v_mov", "s_waitcnt", "s_nop")))


def main():
    args = [a for a in sys.argv[1:] if a != "--histogram"]
    histogram = len(args) != len(sys.argv) - 1
    parent = kernels_of(args[0])
    new = kernels_of(args[1] if len(args) > 1 else os.path.join(ROOT, "simple_mmd_renderer_amd", "libmmdx.so"))
    differ = [k for k in parent if k in new and parent[k] != new[k]]
    for k in differ:
        print("DIFF", k, len(parent[k]), len(new[k]))
    only_new = sorted(k for k in new if k not in parent)
    gone = sorted(k for k in parent if k not in new)
    print("parent functions %d identical %d different %d new-only %d parent-only %d" %
          (len(parent), sum(1 for k in parent if k in new and parent[k] == new[k]), len(differ), len(only_new), len(gone)))
    for k in only_new:
        print(" new", k, len(new[k]))
    for k in gone:
        print(" gone", k, len(parent[k]))
    for k in differ:
        print("=====", k)
        if histogram:
            a, b = mix(parent[k]), mix(new[k])
            changed = ["%s %d -> %d" % (n, a[n], b[n]) for n in sorted(set(a) | set(b)) if a[n] != b[n]]
            print("\n".join(changed) if changed else "same mix")
        else:
            print("\n".join(difflib.unified_diff(parent[k], new[k], lineterm="", n=1)))


if __name__ == "__main__":
    main()
