#!/usr/bin/env python3
"""Per-kernel digests of the gfx950 assembly of the MFMA GEMM family (csrc/gemm.hip, gemm_bf16.hip, gemm_bf16_split.hip,
gemm_bf16_resident.hip): the check of a change that is meant to move text and leave every kernel's instructions alone.

Each file is compiled with the command the tree's Makefile would run for its object (`make -n -B`), with `-c ... -o x.o` replaced by
`--offload-device-only -S`.  The lines that carry the compile's random `__hip_cuid_` symbol are dropped, the text is cut per kernel
symbol -- the function from its .type line to its .size line, and its .amdhsa_kernel descriptor (registers, LDS, scratch) -- and
one line per kernel is printed, sorted:   file  kernel-symbol  sha256  instruction-line-count
Block labels and the comments that name them carry the function's ordinal in the file (.LBB7_3, "Header=BB7_2"), and the comments'
column depends on the label's width; the ordinal is dropped and white space collapsed before hashing, so that a kernel's digest does
not depend on what stands before it in the file.  The tool reads text and runs the compiler; it does not look at what the instructions are.

    tools/gemm_isa_digest.py                       digests of this tree
    tools/gemm_isa_digest.py --against OTHER_TREE  both lists, the kernels whose digests differ, and "kernels differing: N"
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

FILES = ("gemm.hip", "gemm_bf16.hip", "gemm_bf16_split.hip", "gemm_bf16_resident.hip")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_command(tree, name, out):
    obj = "dorylus_amd/csrc/" + name[:-4] + ".o"
    line = [l for l in subprocess.run(["make", "-n", "-B", obj], cwd=tree, check=True, capture_output=True, text=True).stdout.splitlines()
            if name in l]
    assert len(line) == 1, line
    cmd = shlex.split(line[0])
    at = cmd.index("-o")
    del cmd[at:at + 2]
    cmd.remove("-c")
    return cmd + ["--offload-device-only", "-S", "-o", out]


def kernels(asm):
    """{symbol: (sha256, instruction lines)} of the kernels in one file's assembly"""
    lines = [l for l in asm.splitlines() if "__hip_cuid_" not in l]
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    out = {}
    for sym in names:
        first = next(i for i, l in enumerate(lines) if re.match(r"\s*\.type\s+%s,@function" % re.escape(sym), l))
        last = next(i for i, l in enumerate(lines) if i > first and re.match(r"\s*\.size\s+%s," % re.escape(sym), l))
        d0 = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+%s$" % re.escape(sym), l))
        d1 = next(i for i, l in enumerate(lines) if i > d0 and ".end_amdhsa_kernel" in l)
        text = lines[first:last + 1] + lines[d0:d1 + 1]
        text = [" ".join(re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp)\d+", r"\1\2", l).split()) for l in text]
        body = [l.strip() for l in lines[first:last + 1]]
        count = sum(1 for l in body if l and l[0] not in ".;" and not l.split(";")[0].rstrip().endswith(":"))
        out[sym] = (hashlib.sha256("\n".join(text).encode()).hexdigest(), count)
    return out


def digest(tree):
    tree = os.path.abspath(tree)
    with tempfile.TemporaryDirectory() as tmp:
        def one(name):
            out = os.path.join(tmp, name + ".s")
            subprocess.run(compile_command(tree, name, out), cwd=tree, check=True)
            with open(out) as f:
                return name, kernels(f.read())
        with concurrent.futures.ThreadPoolExecutor(len(FILES)) as ex:
            return {(name, sym): v for name, ks in ex.map(one, FILES) for sym, v in ks.items()}


def show(title, d):
    print("== %s: %d kernels" % (title, len(d)))
    for (name, sym), (h, n) in sorted(d.items()):
        print("%s  %s  %s  %d" % (name, sym, h, n))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=HERE, help="the tree to digest (default: the one this file is in)")
    ap.add_argument("--against", help="another tree: print both lists and the kernels whose digests differ")
    a = ap.parse_args()
    mine = digest(a.tree)
    show("tree", mine)
    if not a.against:
        return 0
    other = digest(a.against)
    show("against", other)
    diff = sorted(k for k in set(mine) | set(other) if mine.get(k) != other.get(k))
    for name, sym in diff:
        print("differs: %s  %s  %s" % (name, sym, "in both" if (name, sym) in mine and (name, sym) in other
                                     else "only in tree" if (name, sym) in mine else "only in against"))
    print("kernels differing: %d" % len(diff))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
