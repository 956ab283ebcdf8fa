#!/usr/bin/env python3
"""substr(s, 1, 2) beside trim(s) at size (run on the GPU box): the device time of the lengths and write kernels of each, read from
bhip_ctx_kernel_stats (BHIP_KERNEL_TIMING=1), over one resident column of `rows` 15-byte phone-like ASCII strings.

    python tools/exp_string_fns.py [rows] [--fn trim|substr|both] [--runs 5] [--out FILE]      (default 64 Mi rows, both)

Each function is run once to warm up (code objects, the allocator) and then `--runs` times, the two alternating; a run is one
fresh ProjectionExec and collect(), and its figure is the sum of the two kernels' times of that run.  The result's first rows are
checked.  --fn trim with BHIP_LIB_PATH set to another build's library times that build's trim: the yardstick of
profiles/string_fns.txt is the commit before substr, run that way."""
import argparse, os, sys
os.environ.setdefault("BHIP_KERNEL_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col

ap = argparse.ArgumentParser()
ap.add_argument("rows", nargs="?", type=int, default=64 << 20)
ap.add_argument("--fn", default="both", choices=("trim", "substr", "both"))
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
n = args.rows
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


# "CC-DDD-DDD-DDDD": 15 bytes, country codes 10 .. 34 as in TPC-H's c_phone; built from its buffers, no Python string per row
rng = np.random.default_rng(22)
data = rng.integers(ord("0"), ord("9") + 1, (n, 15), dtype=np.uint8)
code = rng.integers(10, 35, n)
data[:, 0], data[:, 1] = ord("0") + code // 10, ord("0") + code % 10
data[:, [2, 6, 10]] = ord("-")
phones = pa.StringArray.from_buffers(n, pa.py_buffer(np.arange(n + 1, dtype=np.int32) * 15), pa.py_buffer(data.reshape(-1)))
first = phones.slice(0, 2000).to_pylist()

ctx = ba.Context(0)
batch = ba.RecordBatch.from_pyarrow(ctx, pa.RecordBatch.from_arrays([phones], names=["s"]))
FNS = {"trim": (E.ScalarFunctionExpr("trim", [col("s")]), ("str_transform_lengths", "str_transform_write"), first),
       "substr": (None, ("str_range_lengths", "str_range_write"), [p[:2] for p in first])}
if args.fn != "trim":
    FNS["substr"] = (E.ScalarFunctionExpr("substr", [col("s"), E.Literal(1, "Int64"), E.Literal(2, "Int64")]),) + FNS["substr"][1:]
names = ["trim", "substr"] if args.fn == "both" else [args.fn]


def one_run(name):
    expr, kernels, want = FNS[name]
    plan = ba.ProjectionExec([(expr, "v")], ba.MemoryExec([[batch]], ctx))
    ctx.synchronize()
    ctx.kernel_stats(reset=True)
    out = plan.collect()
    ctx.synchronize()
    ks = ctx.kernel_stats(reset=True)
    assert out[0].num_rows == n and out[0].to_pyarrow().column(0).slice(0, 2000).to_pylist() == want, name + " result differs"
    assert all(k in ks and ks[k][1] == 1 for k in kernels), (name, sorted(ks))
    return [ks[k][0] for k in kernels]


say(f"rows {n}, 15 B per value; library {os.environ.get('BHIP_LIB_PATH') or 'this build'}")
times = {name: [] for name in names}
for name in names:
    one_run(name)                                   # warm-up, not counted
for _ in range(args.runs):
    for name in names:                              # alternating
        times[name].append(one_run(name))
for name in names:
    sums = [a + b for a, b in times[name]]
    say(f"{name:7s} {FNS[name][1][0]} + {FNS[name][1][1]}, ms per run: " + "  ".join(f"{a:.3f}+{b:.3f}={a + b:.3f}" for a, b in times[name]))
    say(f"{name:7s} min {min(sums):.3f}  median {sorted(sums)[len(sums) // 2]:.3f}  max {max(sums):.3f}  range {max(sums) - min(sums):.3f} ms")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
