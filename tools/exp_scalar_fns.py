#!/usr/bin/env python3
"""concat, to_timestamp and date_trunc at size (run on the GPU box), each as one ProjectionExec over `rows` rows: the median of 10
fresh plans, and the GB/s of the bytes the kernels of the node read plus write (counted from the shapes, below).  Beside them, on
the same build: lower(comment) as the yardstick for a string node, and a device-to-device copy of the same byte count as the floor.

    python tools/exp_scalar_fns.py [rows] [--out profiles/scalar_fns.txt]       (default 10 M rows; results are spot-checked)

The table: 18-byte names, 40-100-byte comments (ASCII), 19-29-byte timestamp texts (0, 3, 6 or 9 fraction digits, with and without
a Z), nanosecond timestamps of 1990-2030."""
import argparse, os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import torch
import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit

ap = argparse.ArgumentParser()
ap.add_argument("rows", nargs="?", type=int, default=10_000_000)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scalar_fns.txt"))
args = ap.parse_args()
n = args.rows
rng = np.random.default_rng(21)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def utf8_array(lengths, fill):
    """a pyarrow string array of the given byte lengths, built from its buffers (no Python string per row)"""
    off = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(lengths, out=off[1:])
    data = fill(int(off[-1]))
    return pa.StringArray.from_buffers(len(lengths), pa.py_buffer(off), pa.py_buffer(data))


letters = lambda k: rng.integers(ord("a"), ord("z") + 1, k, dtype=np.uint8)
names = utf8_array(np.full(n, 18, np.int64), letters)
comment_len = rng.integers(40, 101, n)
comments = utf8_array(comment_len, letters)
ns = rng.integers(631152000, 1893456000, n) * 10**9 + rng.integers(0, 10**9, n)
# texts of 19 / 23 / 26 / 29 bytes (+ 'Z' on a third of them): numpy writes them, in four groups by fraction width
unit = rng.integers(0, 4, n)
texts = np.empty(n, dtype="U30")
for k, code in enumerate(("s", "ms", "us", "ns")):
    sel = unit == k
    texts[sel] = np.datetime_as_string(ns[sel].view("datetime64[ns]").astype(f"datetime64[{code}]"))
zed = rng.random(n) < 1 / 3
texts[zed] = np.char.add(texts[zed], "Z")
text_arr = pa.array(texts)
if isinstance(text_arr, pa.ChunkedArray):
    text_arr = text_arr.combine_chunks()
width = np.array([19, 23, 26, 29])[unit]
text_ns = ns - ns % (10 ** (9 - np.array([0, 3, 6, 9])[unit]))
text_bytes, name_bytes, comment_bytes = int(width.sum() + zed.sum()), 18 * n, int(comment_len.sum())

ctx = ba.Context(0)
batch = ba.RecordBatch.from_pyarrow(ctx, pa.RecordBatch.from_arrays(
    [names, comments, text_arr, pa.array(ns, pa.timestamp("ns"))], names=["name", "comment", "text", "t"]))
say(f"rows {n}; name 18 B, comment {comment_bytes / n:.1f} B, timestamp text {text_bytes / n:.1f} B per row")


def timed(expr, reps=10):
    ms, out = [], None
    for _ in range(reps + 1):                      # the first run warms the allocator and the code objects
        plan = ba.ProjectionExec([(expr, "v")], ba.MemoryExec([[batch]], ctx))
        ctx.synchronize()
        t0 = time.perf_counter()
        out = plan.collect()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[1:]), min(ms[1:]), max(ms[1:]), out


def copy_floor(nbytes, reps=10):
    """a device-to-device copy that reads nbytes / 2 and writes nbytes / 2"""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ms = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[1:])


def report(name, expr, nbytes, check):
    ms, lo, hi, out = timed(expr)
    check(out[0])
    floor = copy_floor(nbytes)
    say(f"{name:42s} {ms:8.2f} ms (min {lo:.2f} .. max {hi:.2f})  {nbytes / ms / 1e6:7.1f} GB/s of {nbytes / 1e6:6.0f} MB read + written;"
        f"  D2D copy of as many bytes {floor:6.2f} ms ({nbytes / floor / 1e6:.0f} GB/s)")
    return nbytes / ms / 1e6


def first_rows(rb, k=2000):
    return rb.to_pyarrow().column(0).slice(0, k).to_pylist()


def check_concat(rb):
    want = [a + "#" + b for a, b in zip(names.slice(0, 2000).to_pylist(), comments.slice(0, 2000).to_pylist())]
    assert rb.num_rows == n and first_rows(rb) == want, "concat result differs"


def check_lower(rb):
    assert rb.num_rows == n and first_rows(rb) == comments.slice(0, 2000).to_pylist(), "lower result differs"


def check_values(want):
    def check(rb):
        dtype, got, valid = rb.column(0)
        assert dtype == "Timestamp(Nanosecond)" and np.array_equal(got, want) and (valid is None or valid.all()), "result differs"
    return check


# concat: lengths (2 offsets arrays in, lengths out), scan (lengths in, offsets out), bytes (3 offsets arrays + both values in, values out)
concat_bytes = (8 + 4) * n + 8 * n + 12 * n + (name_bytes + comment_bytes) + (name_bytes + comment_bytes + n)
c = report("concat(name, '#', comment)", E.ScalarFunctionExpr("concat", [col("name"), lit("#"), col("comment")]), concat_bytes, check_concat)
# lower: lengths (offsets in, lengths out), scan, bytes (2 offsets arrays + values in, values out)
lower_bytes = 8 * n + 8 * n + 8 * n + 2 * comment_bytes
lo = report("lower(comment)", E.ScalarFunctionExpr("lower", [col("comment")]), lower_bytes, check_lower)
report("to_timestamp(text)", E.ScalarFunctionExpr("to_timestamp", [col("text")]), 4 * n + text_bytes + 8 * n, check_values(text_ns))
month = ns.view("datetime64[ns]").astype("datetime64[M]").astype("datetime64[ns]").astype(np.int64)
report("date_trunc('month', t)", E.ScalarFunctionExpr("date_trunc", [lit("month"), col("t")]), 16 * n + n // 8, check_values(month))
say(f"concat moves {c / lo:.2f} x the bytes per second of lower(comment)")
say("how taken: one ProjectionExec per line over one resident batch, wall clock around collect() between two device synchronises,"
    " median of 10 fresh plans after one warm-up; bytes counted from the shapes as the comments of tools/exp_scalar_fns.py say;"
    " each node also waits for the host once or twice per batch (the byte total of a string result, to_timestamp's status word)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
