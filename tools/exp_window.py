#!/usr/bin/env python3
"""What WindowAggExec costs on top of the sort beneath it (run on the GPU box).

2^26 rows (ROWS overrides) of an Int64 partition key with about 2^16 values, an Int64 order key and a Float64 argument, in one batch.
Three plans, a fresh plan per step as bench.py does, WARMUP untimed steps and then RUNS timed ones (host clock around collect() and
a device synchronise):
  SortExec([p, o])                                              the sort alone, over the keys the operator sorts by
  WindowAggExec([p], [o], [ROW_NUMBER, RANK])
  WindowAggExec([p], [o], [SUM(v) ROWS_TO_CURRENT, LAG(v, 1)])
Prints each median, the window pass as the difference from the sort, the GB/s that difference amounts to against the bytes the pass
must read and write (the two keys, the argument, and the columns it adds), and the per-launch totals of every window_* launch and of
the gathers from the context's kernel statistics (BHIP_KERNEL_TIMING=1).
  tools/exp_window.py > profiles/window.txt

`frames`: the sliding ROWS frames over the same input, every plan one aggregate:
  SortExec([p, o]); SUM(v) ROWS_TO_CURRENT (the running sum, for comparison); SUM(v) over (-6, 0), (-63, 0) and (-4095, 0); MIN(v) over
  (-6, 0); SUM(o) over (-6, 0) (an Int64 argument: the difference of running sums)
The plans alternate inside every round (one step of each, RUNS rounds after WARMUP untimed ones), so a difference between two of them
is not a difference between two moments of a shared machine.  Prints what the first form prints, per plan.
  tools/exp_window.py frames > profiles/window_frames.txt

`value_frames`: RANGE and GROUPS frames over the same input, the plans alternating as in `frames`, each beside the ROWS (-6, 0) pass of
the same run:
  SortExec([p, o]); SUM(v) over ROWS (-6, 0), RANGE (-6, 0) and GROUPS (-1, 1); COUNT(v) over RANGE (-6, 0); SUM(v) over a RANGE frame
  about 1000 rows wide.  RANGE offsets are in units of the mean key distance between two rows (see value_frames)
  tools/exp_window.py value_frames > profiles/window_value_frames.txt"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BHIP_KERNEL_TIMING", "1")

import numpy as np

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col


def alternate(ctx, n, plans, runs, warmup):
    """one step of each plan per round, `warmup` untimed rounds and then `runs` timed ones; prints per plan the median, the steps, the
    window pass (the difference from the plan named "sort") and the per-launch totals -> the medians"""
    print(json.dumps(dict(rows=n, partitions=1 << 16, runs=runs, warmup=warmup, tile_rows=ba.plan.WINDOW_TILE_ROWS,
                          slide_max_rows=ba.plan.WINDOW_SLIDE_MAX_ROWS, cus=ctx.device_cus())), flush=True)
    ms = {name: [] for name in plans}
    launches = {name: {} for name in plans}
    for it in range(warmup + runs):
        for name, make in plans.items():
            plan = make()
            ctx.synchronize()
            ctx.kernel_stats(reset=True)
            t0 = time.perf_counter()
            out = plan.collect()
            ctx.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert sum(b.num_rows for b in out) == n
            del plan, out
            if it >= warmup:
                ms[name].append(dt)
                for k, (t, count, _) in ctx.kernel_stats(reset=True).items():
                    acc = launches[name].setdefault(k, [0.0, 0])
                    acc[0] += t
                    acc[1] += count
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    for name in plans:
        line = dict(plan=name, ms_median=round(med[name], 3), ms=[round(x, 3) for x in ms[name]])
        if name != "sort":
            line.update(window_pass_ms=round(med[name] - med["sort"], 3))
        print(json.dumps(line), flush=True)
        ks = launches[name]
        for k in sorted(ks, key=lambda k: -ks[k][0]):
            if name == "sort" or k.startswith("window_") or k.startswith("take_") or k == "scan_project":
                print(f"    {k:36s} {ks[k][0] / runs:9.3f} ms/step  {ks[k][1] // runs:4d} launches/step", flush=True)
    return med


def frames():
    n = int(os.environ.get("ROWS", 1 << 26))
    runs, warmup = int(os.environ.get("RUNS", 7)), int(os.environ.get("WARMUP", 1))
    rng = np.random.default_rng(1)
    ctx = ba.Context(0)
    batch = ba.RecordBatch.from_columns(ctx, [("p", "Int64", rng.integers(0, 1 << 16, n), None), ("o", "Int64", rng.integers(0, 1 << 40, n), None),
                                              ("v", "Float64", rng.uniform(0.5, 2.0, n), None)])
    keys = [E.PhysicalSortExpr(col("p")), E.PhysicalSortExpr(col("o"))]
    leaf = lambda: ba.MemoryExec([[batch]], ctx)
    one = lambda fun, arg, frame: (lambda: ba.WindowAggExec([col("p")], keys[1:], [E.WindowExpr(fun, col(arg), "w", frame=frame)], leaf()))
    plans = {"sort": lambda: ba.SortExec(keys, leaf()),
             "SUM(v) ROWS_TO_CURRENT": one("SUM", "v", "ROWS_TO_CURRENT"),
             "SUM(v) (-6, 0)": one("SUM", "v", E.RowsFrame(-6, 0)),
             "SUM(v) (-63, 0)": one("SUM", "v", E.RowsFrame(-63, 0)),
             "SUM(v) (-4095, 0)": one("SUM", "v", E.RowsFrame(-4095, 0)),
             "MIN(v) (-6, 0)": one("MIN", "v", E.RowsFrame(-6, 0)),
             "SUM(o) (-6, 0)": one("SUM", "o", E.RowsFrame(-6, 0))}
    med = alternate(ctx, n, plans, runs, warmup)
    running, sliding = med["SUM(v) ROWS_TO_CURRENT"] - med["sort"], med["SUM(v) (-6, 0)"] - med["sort"]
    print(json.dumps(dict(running_sum_pass_ms=round(running, 3), sliding_sum_6_0_pass_ms=round(sliding, 3), ratio=round(sliding / running, 3),
                          not_slower_within_10_percent=bool(sliding <= 1.1 * running))), flush=True)


def value_frames():
    """RANGE / GROUPS frames beside the ROWS frame of the same run.  The order key of the frames input is uniform over 2^40 with about
    1024 rows per partition, so one row is worth 2^30 of key on average: RANGE offsets are given in that unit, and "RANGE (-6, 0)" is
    6 * 2^30 PRECEDING .. CURRENT ROW, seven rows on average like ROWS (-6, 0).  The wide frame reaches 1000 units either way: nearly
    the whole partition, about 1000 rows."""
    n = int(os.environ.get("ROWS", 1 << 26))
    runs, warmup = int(os.environ.get("RUNS", 7)), int(os.environ.get("WARMUP", 1))
    rng = np.random.default_rng(1)
    ctx = ba.Context(0)
    batch = ba.RecordBatch.from_columns(ctx, [("p", "Int64", rng.integers(0, 1 << 16, n), None), ("o", "Int64", rng.integers(0, 1 << 40, n), None),
                                              ("v", "Float64", rng.uniform(0.5, 2.0, n), None)])
    keys = [E.PhysicalSortExpr(col("p")), E.PhysicalSortExpr(col("o"))]
    leaf = lambda: ba.MemoryExec([[batch]], ctx)
    one = lambda fun, arg, frame: (lambda: ba.WindowAggExec([col("p")], keys[1:], [E.WindowExpr(fun, col(arg), "w", frame=frame)], leaf()))
    unit = (1 << 40) // max(1, n >> 16)
    plans = {"sort": lambda: ba.SortExec(keys, leaf()),
             "SUM(v) ROWS (-6, 0)": one("SUM", "v", E.RowsFrame(-6, 0)),
             "SUM(v) RANGE (-6, 0)": one("SUM", "v", E.RangeFrame(-6 * unit, 0)),
             "SUM(v) GROUPS (-1, 1)": one("SUM", "v", E.GroupsFrame(-1, 1)),
             "COUNT(v) RANGE (-6, 0)": one("COUNT", "v", E.RangeFrame(-6 * unit, 0)),
             "SUM(v) RANGE (-1000, 1000)": one("SUM", "v", E.RangeFrame(-1000 * unit, 1000 * unit))}
    med = alternate(ctx, n, plans, runs, warmup)
    rows = med["SUM(v) ROWS (-6, 0)"] - med["sort"]
    print(json.dumps(dict(range_unit=unit, stage_rows=ba.plan.WINDOW_SLIDE_STAGE_ROWS, rows_sum_6_0_pass_ms=round(rows, 3),
                          **{name + " / ROWS (-6, 0)": round((med[name] - med["sort"]) / rows, 3) for name in plans if "RANGE" in name or "GROUPS" in name})), flush=True)


def main():
    n = int(os.environ.get("ROWS", 1 << 26))
    runs, warmup = int(os.environ.get("RUNS", 5)), int(os.environ.get("WARMUP", 1))
    rng = np.random.default_rng(1)
    ctx = ba.Context(0)
    batch = ba.RecordBatch.from_columns(ctx, [("p", "Int64", rng.integers(0, 1 << 16, n), None), ("o", "Int64", rng.integers(0, 1 << 40, n), None),
                                              ("v", "Float64", rng.uniform(0.5, 2.0, n), None)])
    keys = [E.PhysicalSortExpr(col("p")), E.PhysicalSortExpr(col("o"))]
    leaf = lambda: ba.MemoryExec([[batch]], ctx)
    plans = {
        "sort": (lambda: ba.SortExec(keys, leaf()), 0),
        # read p, o; write two UInt64 columns
        "row_number+rank": (lambda: ba.WindowAggExec([col("p")], keys[1:], [E.WindowExpr("ROW_NUMBER", None, "rn"), E.WindowExpr("RANK", None, "rk")], leaf()),
                            16 + 16),
        # read p, o, v; write a Float64 sum and a Float64 lag, each with a validity bit
        "running_sum+lag": (lambda: ba.WindowAggExec([col("p")], keys[1:], [E.WindowExpr("SUM", col("v"), "s", frame="ROWS_TO_CURRENT"),
                                                                            E.WindowExpr("LAG", col("v"), "l", 1)], leaf()), 24 + 16.25),
    }
    print(json.dumps(dict(rows=n, partitions=1 << 16, runs=runs, warmup=warmup, tile_rows=ba.plan.WINDOW_TILE_ROWS, cus=ctx.device_cus())), flush=True)
    medians = {}
    for name, (make, bytes_per_row) in plans.items():
        ms = []
        for it in range(warmup + runs):
            plan = make()
            ctx.synchronize()
            if it == warmup:
                ctx.kernel_stats(reset=True)
            t0 = time.perf_counter()
            out = plan.collect()
            ctx.synchronize()
            if it >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            assert sum(b.num_rows for b in out) == n
            del plan, out
        medians[name] = sorted(ms)[len(ms) // 2]
        line = dict(plan=name, ms_median=round(medians[name], 3), ms=[round(x, 3) for x in ms])
        if name != "sort":
            extra = medians[name] - medians["sort"]
            line.update(window_pass_ms=round(extra, 3), pass_bytes_per_row=bytes_per_row,
                        pass_GBps=round(n * bytes_per_row / (extra * 1e-3) / 1e9, 1) if extra > 0 else None)
        print(json.dumps(line), flush=True)
        ks = ctx.kernel_stats(reset=True)
        for k in sorted(ks, key=lambda k: -ks[k][0]):
            if name == "sort" or k.startswith("window_") or k.startswith("take_") or k == "scan_project":
                print(f"    {k:36s} {ks[k][0] / runs:9.3f} ms/step  {ks[k][1] // runs:4d} launches/step", flush=True)


if __name__ == "__main__":
    {"frames": frames, "value_frames": value_frames}.get(" ".join(sys.argv[1:]), main)()
