#!/usr/bin/env python3
"""ISA check of the lean scan + aggregate kernels (lean_kernel.h, lean_spec_kernel.h), CPU only: compiles their
instantiation files for gfx950 with the Makefile's flags plus --save-temps -Rpass-analysis=kernel-resource-usage and
prints, per kernel, its resources (VGPRs, SGPRs, spills, scratch, LDS, occupancy) and the memory waits of its main loop.

The main loop is the natural loop (control-flow graph of the .s, back edge = branch to a dominator) that holds the most
global_load_dwordx4.  Its fast path is that loop without the key-append path of the lookup (the region below the block
that takes the LDS lock).  For the fast path the tool prints its global loads, the sequence of loads and
s_waitcnt vmcnt(N) in layout order, the number of vmcnt(0) waits, and the waits of the latch (the back edge's block).

    python tools/isa_lean_waits.py [--keep DIR] [files ...]      (default: kernels_lean_g1/g4.hip, kernels_lean_spec.hip)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ballista_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
         "-Wno-unused-function", "--save-temps", "-Rpass-analysis=kernel-resource-usage"]
DEFAULT = ["kernels_lean_g1.hip", "kernels_lean_g4.hip", "kernels_lean_spec.hip"]
KEYS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("SGPRs Spill", "SGPR spill"),
        ("VGPRs Spill", "VGPR spill"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
        ("Occupancy [waves/SIMD]", "occupancy")]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def resources(stderr):
    res, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark: .*?:\s+([A-Za-z][^:]*): (\S+) \[", line)
        if m and cur:
            res[cur][m.group(1).strip()] = m.group(2)
    return res


def functions(asm):
    """mangled name -> list of instruction / label lines of its body"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"^\s*\.Lfunc_end", line) or line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].rstrip()
        if s.strip():
            out[cur].append(s.strip())
    return out


def cfg(body):
    """basic blocks of a function body: list of (label, lines), successor lists"""
    blocks, cur = [], None
    for l in body:
        if re.match(r"^\.LBB\w+:$", l):
            cur = (l[:-1], [])
            blocks.append(cur)
            continue
        if cur is None or (cur[1] and re.match(r"^s_(branch|cbranch_\w+|endpgm|setpc_b64)\b", cur[1][-1])):
            cur = (None, [])
            blocks.append(cur)
        cur[1].append(l)
    index = {lab: i for i, (lab, _) in enumerate(blocks) if lab}
    succ = []
    for i, (_, lines) in enumerate(blocks):
        last = lines[-1] if lines else ""
        m = re.match(r"^s_(branch|cbranch_\w+)\s+(\.LBB\w+)$", last)
        out = []
        if m and m.group(2) in index:
            out.append(index[m.group(2)])
        if not (m and m.group(1) == "branch") and not last.startswith("s_endpgm") and i + 1 < len(blocks):
            out.append(i + 1)
        succ.append(out)
    return blocks, succ


def dominators(n, succ):
    pred = [[] for _ in range(n)]
    for i, ss in enumerate(succ):
        for j in ss:
            pred[j].append(i)
    full = set(range(n))
    dom = [full] * n
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for i in range(1, n):
            ps = [dom[p] for p in pred[i]]
            d = (set.intersection(*ps) if ps else set()) | {i}
            if d != dom[i]:
                dom[i], changed = d, True
    return dom, pred


def natural_loop(h, t, pred):
    body, stack = {h, t}, ([t] if t != h else [])
    while stack:
        x = stack.pop()
        for p in pred[x]:
            if p not in body:
                body.add(p)
                stack.append(p)
    return body


def main_loop(body):
    """(blocks, fast-path block indices in layout order, latch index) of the loop with the most global_load_dwordx4, or
    None.  The fast path leaves out the key-append path of the lookup: for each block that takes the LDS lock (ds_cmpst*),
    the region dominated by its highest dominator that dominates none of the loop's global_load_dwordx4 blocks"""
    blocks, succ = cfg(body)
    n = len(blocks)
    dom, pred = dominators(n, succ)
    best = None
    for t in range(n):
        for h in succ[t]:
            if h in dom[t]:
                lp = natural_loop(h, t, pred)
                x4 = sum(1 for i in lp for l in blocks[i][1] if l.startswith("global_load_dwordx4"))
                if best is None or (x4, -len(lp)) > (best[0], -len(best[1])):
                    best = (x4, lp, t)
    if not best or best[0] == 0:
        return None
    _, lp, latch = best
    x4_blocks = [i for i in lp if any(l.startswith("global_load_dwordx4") for l in blocks[i][1])]
    rare = set()
    for c in lp:
        if any(l.startswith("ds_cmpst") for l in blocks[c][1]):
            chain = sorted(dom[c], key=lambda d: -len(dom[d]))      # c .. root
            entry = c
            for d in chain:
                if d not in lp or any(d in dom[x] for x in x4_blocks):
                    break
                entry = d
            rare |= {i for i in lp if entry in dom[i]}
    return blocks, [i for i in sorted(lp) if i not in rare], latch


def wait_of(line):
    m = re.match(r"^s_waitcnt\s+(.*)$", line)
    if not m:
        return None
    v = re.search(r"vmcnt\((\d+)\)", m.group(1))
    return int(v.group(1)) if v else None


def report(name, res, body):
    r = res.get(name, {})
    print(" ", "  ".join(f"{short}={r.get(k, '?')}" for k, short in KEYS))
    loop = main_loop(body)
    if not loop:
        print("  main loop: none found")
        return
    blocks, fast, latch = loop
    seq, loads = [], {}
    for i in fast:
        for l in blocks[i][1]:
            op = l.split()[0]
            if op.startswith("global_load") or op.startswith("buffer_load"):
                loads[op] = loads.get(op, 0) + 1
                seq.append("L4" if op == "global_load_dwordx4" else "l")
            w = wait_of(l)
            if w is not None:
                seq.append(f"w{w}")
    comp, prev, run = [], None, 0
    for t in seq + ["end"]:
        if t == prev and t in ("l", "L4"):
            run += 1
            continue
        if prev in ("l", "L4"):
            comp.append(f"{prev}x{run}" if run > 1 else prev)
        prev, run = t, 1
        if t not in ("l", "L4", "end"):
            comp.append(t)
            prev = None
    latch_w = [wait_of(l) for l in blocks[latch][1] if wait_of(l) is not None]
    n0 = sum(1 for t in seq if t == "w0")
    print(f"  main loop fast path: {len(fast)} blocks, {sum(loads.values())} global loads "
          f"({', '.join(f'{v} {k}' for k, v in sorted(loads.items()))})")
    print(f"  vmcnt(0) on the fast path: {n0};  latch block waits: {latch_w or 'none'}")
    print("  sequence (L4: global_load_dwordx4, l: other global load, xN: N in a row, w<N>: s_waitcnt vmcnt(N)):")
    line = "   "
    for t in comp:
        if len(line) + len(t) > 116:
            print(line)
            line = "   "
        line += " " + t
    print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("files", nargs="*", default=DEFAULT)
    ap.add_argument("--keep", help="directory for the .s / .o files (default: a temporary one)")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_lean_")
    os.makedirs(tmp, exist_ok=True)
    for f in a.files:
        src = os.path.join(CSRC, f)
        p = subprocess.run([HIPCC] + FLAGS + ["-c", src, "-o", os.path.join(tmp, os.path.basename(f) + ".o")], cwd=tmp,
                           capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            return 1
        res = resources(p.stderr)
        stem = os.path.splitext(os.path.basename(f))[0]
        asm_path = os.path.join(tmp, f"{stem}-hip-amdgcn-amd-amdhsa-gfx950.s")
        with open(asm_path) as fh:
            funcs = functions(fh.read())
        kernels = [n for n in funcs if "scan_agg_lean" in n]
        dm = demangle(kernels)
        print(f"== {f}")
        for n in kernels:
            print(f"{dm[n].split('(')[0]}")
            report(n, res, funcs[n])
    return 0


if __name__ == "__main__":
    sys.exit(main())
