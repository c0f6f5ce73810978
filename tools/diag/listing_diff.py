#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device listings of any unit under video-blade_amd/csrc (a
refactor check: does the GPU still execute the same instructions?). No GPU needed.

Produce a listing of the unit with the Makefile's flags for that file, e.g. for the predictor

  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Iinclude -Ivideo-blade_amd/csrc \\
        -fno-honor-nans --cuda-device-only -S video-blade_amd/csrc/vb_predict.hip -o new.s

(vb_attn_bwd.hip: -mllvm -amdgpu-sched-strategy=iterative-ilp; vb_attn_bwd_kv.hip:
-fno-slp-vectorize; vb_attn_fwd.hip: -fno-slp-vectorize -fno-honor-nans and the scheduler flag),
then, with old.s made the same way at the commit to compare against:

  python tools/diag/listing_diff.py old.s new.s            # expects no differing line
  python tools/diag/listing_diff.py old.s new.s --kernarg  # a kernel-argument field went or came

Per kernel the instruction stream with its .amdhsa_kernel descriptor and its metadata entry (VGPR,
SGPR, LDS and scratch sizes) are compared line for line after normalising three things only: the
predictor score kernel's mangled name (its template arguments become <D,T,long,keep,rule>, whatever further
bool parameters a side has), the ordinal that local labels take from the kernel's place in the unit
(.LBB<n>_<m> and BB<n>_<m> in loop comments, .Lfunc_end<n>, .Lpost_getpc<n>; the blanks in front of
a label's comment, which move with the ordinal's width, count as one) and .file/.ident lines. With --kernarg, lines that differ only in a kernel-argument size or offset (the
scalar loads off the kernarg pointer, .amdhsa_kernarg_size, the metadata's .size/.offset/
.kernarg_segment_size) are counted apart. Exit status 0: no other line differs and both sides hold
the same kernels."""
import re
import sys

NAME = re.compile(r"mask_predict_kernelILi(\d+)ENS_\d(BF16|F16)E(?:Lb[01]E)*?Lb([01])ELi(\d+)ELb([01])EE")
ORD = re.compile(r"\.?\b(LBB|BB|Lfunc_begin|Lfunc_end|Lpost_getpc)\d+")
KERNARG = re.compile(r"^\s*(s_load_\w+ s\S+ s\[\d+:\d+\], |\.amdhsa_kernarg_size |\.kernarg_segment_size: |"
                     r"\.size: |- \.offset: |\.offset: )")
NUM = re.compile(r"\b(0x[0-9a-f]+|\d+)\s*$")


def norm(line):
    line = NAME.sub(lambda m: "mask_predict_kernel<%s,%s,%s,%s,%s>" % m.groups(), line.rstrip())
    line = ORD.sub(lambda m: "." + m.group(1) + "#", line)
    return re.sub(r"\s+;", " ;", line)   # the column of a label's comment moves with the ordinal's width


def kernels(path):
    """{kernel: lines of its code and descriptor + lines of its metadata entry}"""
    out, cur, meta, entries = {}, None, False, []
    for raw in open(path):
        line = norm(raw)
        if re.match(r"\s*\.(file|ident)\b", line):
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(line)
            if line.strip() == ".end_amdhsa_kernel":
                cur = None
        if line.startswith("amdhsa.kernels:"):
            meta = True
        elif meta and line.startswith("  - "):
            entries.append([line])
        elif meta and line.startswith("    "):
            entries[-1].append(line)
        elif meta:
            meta = False
    for e in entries:
        name = [re.sub(r"^\s+\.name:\s+", "", x).strip("'") for x in e if re.match(r"\s+\.name:", x)][0]
        out[name].extend(e)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernarg = "--kernarg" in sys.argv
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels(args[0]), kernels(args[1])
    bad = sorted(set(old) ^ set(new))
    for k in bad:
        print("only in %s: %s" % ("old" if k in old else "new", k))
    other = arg_only = 0
    for k in sorted(set(old) & set(new)):
        a, b = old[k], new[k]
        if len(a) != len(b):
            print("%s: %d lines against %d" % (k, len(a), len(b)))
            other += 1
            continue
        for x, y in zip(a, b):
            if x == y:
                continue
            if kernarg and KERNARG.match(x) and KERNARG.match(y) and NUM.sub("", x) == NUM.sub("", y):
                arg_only += 1
                continue
            other += 1
            if other <= 20:
                print("%s:\n  - %s\n  + %s" % (k, x, y))
    print("%d kernels on each side compared (old %d, new %d): %d kernel-argument lines differ, %d other lines differ"
          % (len(set(old) & set(new)), len(old), len(new), arg_only, other))
    sys.exit(1 if bad or other else 0)


if __name__ == "__main__":
    main()
