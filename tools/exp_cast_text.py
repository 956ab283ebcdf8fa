#!/usr/bin/env python3
"""CAST(Utf8 -> Int64) and CAST(Int64 -> Utf8) at size (run on the GPU box): decimal strings of 1-10 digits, each direction as one
ProjectionExec; the median of 10 fresh plans, rows/s and the GB/s of the bytes the direction reads plus writes, beside
`pyarrow.compute.cast` on the same data on the box's 16 threads.

    python tools/exp_cast_text.py [rows]          (default 64 M; the results are checked against pyarrow's)"""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64 << 20
pa.set_cpu_count(16)
rng = np.random.default_rng(11)
digits = rng.integers(1, 11, n)
values = (rng.random(n) * 9 * 10.0 ** (digits - 1) + 10.0 ** (digits - 1)).astype(np.int64)      # `digits` digits each
values[digits == 1] = rng.integers(0, 10, int((digits == 1).sum()))
ints = pa.array(values)
text = pc.cast(ints, pa.string())
text_bytes = text.buffers()[2].size
ctx = ba.Context(0)
t_text = ba.RecordBatch.from_pyarrow(ctx, pa.RecordBatch.from_arrays([text], names=["s"]))
t_ints = ba.RecordBatch.from_pyarrow(ctx, pa.RecordBatch.from_arrays([ints], names=["k"]))


def timed(make_plan, reps=10):
    ms, out = [], None
    for _ in range(reps + 1):                      # the first run warms the allocator and the code objects
        plan = make_plan()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = plan.collect()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[1:]), min(ms[1:]), max(ms[1:]), out


def cpu(f, reps=3):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), out


def line(name, ms, lo, hi, nbytes):
    print(f"{name:28s} {ms:9.2f} ms (min {lo:.2f} .. max {hi:.2f})  {n / ms / 1e6:8.3f} G rows/s  {nbytes / ms / 1e6:8.1f} GB/s of {nbytes / 1e6:.0f} MB read + written", flush=True)


print(f"rows {n}, text bytes {text_bytes} ({text_bytes / n:.2f} per row)")
# Utf8 -> Int64: offsets + text in, values + validity bits out
parse_bytes = 4 * (n + 1) + text_bytes + 8 * n + n // 8
ms, lo, hi, out = timed(lambda: ba.ProjectionExec([(E.CastExpr(col("s"), "Int64"), "v")], ba.MemoryExec([[t_text]], ctx)))
line("CAST(Utf8 -> Int64) GPU", ms, lo, hi, parse_bytes)
dtype, got, valid = out[0].column(0)
assert dtype == "Int64" and np.array_equal(got, values) and (valid is None or valid.all()), "parse result differs"
cms, ref = cpu(lambda: pc.cast(text, pa.int64()))
line("pyarrow.compute.cast, 16 thr", cms, cms, cms, parse_bytes)
assert ref.equals(ints)
# Int64 -> Utf8: values in, lengths out; lengths in, offsets out (scan); values + offsets in, text out
format_bytes = 8 * n + 4 * n + 4 * n + 4 * (n + 1) + 8 * n + 4 * (n + 1) + text_bytes
ms, lo, hi, out = timed(lambda: ba.ProjectionExec([(E.CastExpr(col("k"), "Utf8"), "s")], ba.MemoryExec([[t_ints]], ctx)))
line("CAST(Int64 -> Utf8) GPU", ms, lo, hi, format_bytes)
back = out[0].to_pyarrow().column(0)
assert back.equals(text), "format result differs"
cms, ref = cpu(lambda: pc.cast(ints, pa.string()))
line("pyarrow.compute.cast, 16 thr", cms, cms, cms, format_bytes)
