#!/usr/bin/env python3
"""ISA comparison of the text scan kernels (kernels_tbl.hip, kernels_csv.hip) between this checkout and another one (e.g. the
parent commit), CPU only: compiles both files of both trees for gfx950 with the Makefile's flags (--cuda-device-only -S) and
prints, per kernel, "identical" when the instruction streams are equal line for line (comments dropped, the names of the power-of-ten
table, of the byte readers, of the plan type and of the string-copy kernel normalised: another checkout may still have TEXT_POW10,
TblPlan / CsvPlan and csv_copy_strings_kernel) and the resources are the same, or the resources of both sides and the number of instruction lines that differ.

    python tools/isa_text_scan.py OTHER_TREE [--keep DIR]

Exit status 1 when a kernel of this checkout has scratch that the other side's does not.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "--cuda-device-only", "-S"]
FILES = ["kernels_tbl.hip", "kernels_csv.hip"]
KEYS = [".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size"]


def compile_tree(tree, tmp, tag):
    """-> {demangled kernel name: (instruction lines, {resource: value})}"""
    out = {}
    for f in FILES:
        asm = os.path.join(tmp, f"{tag}_{f}.s")
        subprocess.run([HIPCC] + FLAGS + [os.path.join(tree, "ballista_amd", "csrc", f), "-o", asm], check=True)
        text = open(asm).read()
        text = re.sub(r"(?:__const\.)?_ZN4bhip\w*(?:POW10E|pow10Ei\.t)\b", "POW10", text)
        text = re.sub(r"7(?:Tbl|Csv)Plan", "8TextPlan", text)                            # the plan type inside mangled kernel names
        text = text.replace("23csv_copy_strings_kernel", "24text_copy_strings_kernel")  # the one copy kernel was CSV's
        text = re.sub(r"\d+(Tbl|Csv|Text)(Global|Lds)Reader", r"\2Reader", text)       # the readers' names inside mangled symbols
        bodies, cur = {}, None
        for line in text.splitlines():
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur = m.group(1)
                bodies[cur] = []
            elif cur and line.startswith(".Lfunc_end"):
                cur = None
            elif cur:
                s = line.split(";")[0].strip()
                if s and not s.startswith((".p2align", ".loc", ".file", ".cfi")):
                    bodies[cur].append(s)
        res = {}
        for m in re.finditer(r"^  - (?:\.\w+:.*\n(?:    .*\n)*)+", text, re.M):
            block = m.group(0)
            name = re.search(r"^    \.name:\s+(\S+)", block, re.M) or re.search(r"\.name:\s+(_Z\S+)", block)
            if name and name.group(1) in bodies:
                res[name.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
        names = sorted(res)
        dm = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        for n, d in zip(names, dm):
            out[d.split("(")[0].replace("void ", "").replace("bhip::", "")] = (bodies[n], res[n])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("other")
    ap.add_argument("--keep", help="directory for the .s files (default: a temporary one)")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_text_")
    os.makedirs(tmp, exist_ok=True)
    old, new = compile_tree(os.path.abspath(a.other), tmp, "other"), compile_tree(ROOT, tmp, "this")
    fmt = lambda r: "  ".join(f"{k[1:]}={r[k]}" for k in KEYS)
    bad = False
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name:32s} only in {'this checkout' if name in new else 'the other'}")
            continue
        (b0, r0), (b1, r1) = old[name], new[name]
        if b0 == b1 and r0 == r1:
            print(f"{name:32s} identical  ({len(b1)} lines; {fmt(r1)})")
            continue
        changed = sum(1 for l in difflib.ndiff(b0, b1) if l[0] in "+-")
        print(f"{name:32s} DIFFERS: {changed} lines of {len(b0)} -> {len(b1)}\n{'':34s}other {fmt(r0)}\n{'':34s}this  {fmt(r1)}")
        bad |= r1[".private_segment_fixed_size"] > 0 and r0[".private_segment_fixed_size"] == 0
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
