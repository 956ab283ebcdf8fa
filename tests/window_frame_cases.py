"""Sliding ROWS frames of WindowAggExec restated row by row (test_window_frames_cpu.py checks this against sqlite3, test_window_frames_gpu.py
checks the device against it).

Written from the contract (DESIGN.md "Window functions", sliding frames), not from the host code.  For row i of a partition [ps, pe] and
a frame (start, end) — offsets from the current row, None = unbounded — the frame is rows lo .. hi with lo = max(ps, i + start) (ps when
unbounded) and hi = min(pe, i + end) (pe when unbounded); it is empty when lo > hi: COUNT is 0 there, everything else NULL.

Float sums.  With two finite ends SUM of floats and every AVG is DEFINED: the accumulator starts at +0.0 and takes the frame's non-NULL
values in row order, in Float64 — here one numpy step per frame offset k ascending, `acc = where(in_frame & valid, acc + x, acc)`, which
is the same IEEE additions in the same order for every row.  A frame that starts UNBOUNDED PRECEDING reads the running state of the
existing restatement (math.fsum: the correctly rounded sum), as ROWS_TO_CURRENT does.

The rows are ALREADY in the operator's order; named frames and every function without a frame go to window_cases.restate."""
import math
from collections import OrderedDict

import numpy as np

from ballista_amd import expr as E
from oracle import engine as og
from oracle.engine import OCol
from tests import window_cases as K
from tests.window_cases import W, asc, bounds, table                     # noqa: F401  (the frame tests take them from here)

F = E.RowsFrame
FRAMED = K.AGGREGATES + ("FIRST_VALUE", "LAST_VALUE")                    # what a rows frame moves


def frame_bounds(part_start, part_end, frame):
    """(lo, hi) per row; (None, None): the empty frame"""
    lo, hi = [], []
    for i, (ps, pe) in enumerate(zip(part_start, part_end)):
        a = ps if frame.start is None else max(ps, i + frame.start)
        b = pe if frame.end is None else min(pe, i + frame.end)
        lo.append(a if a <= b else None)
        hi.append(b if a <= b else None)
    return lo, hi


def canonical(frame):
    """the two rows frames that ARE named frames (and run and display as them)"""
    if isinstance(frame, F) and frame.start is None and frame.end is None:
        return "PARTITION"
    if isinstance(frame, F) and frame.start is None and frame.end == 0:
        return "ROWS_TO_CURRENT"
    return frame


def can_be_empty(frame):
    return (frame.start is not None and frame.start > 0) or (frame.end is not None and frame.end < 0)


def _ordered_float_sums(x, valid, lo, hi, frame):
    """per row (sum, count) of the non-NULL x[lo .. hi] added to +0.0 in row order; x: float64 array"""
    n = len(x)
    acc, cnt = np.zeros(n, np.float64), np.zeros(n, np.int64)
    i = np.arange(n, dtype=np.int64)
    lo_a = np.array([n if v is None else v for v in lo], np.int64)      # an empty frame holds no j
    hi_a = np.array([-1 if v is None else v for v in hi], np.int64)
    # only offsets that can reach a row: |k| < n
    for k in range(max(frame.start, -n), (n if frame.end is None else min(frame.end, n)) + 1):
        j = i + k
        inside = (j >= lo_a) & (j <= hi_a)
        jc = np.clip(j, 0, max(n - 1, 0))
        take = inside & valid[jc]
        with np.errstate(all="ignore"):
            acc = np.where(take, acc + x[jc], acc)
        cnt += take
    return acc, cnt


def _as_f64(dtype, values):
    """the argument as Float64, the way the device's Float64 add takes it: Float32 widened, integers converted (round to nearest)"""
    return np.array([0.0 if v is None else float(v) for v in values], np.float64)


def _aggregate(fun, dtype, values, lo, hi, part_start, frame):
    n = len(values)
    if frame.start is None:                                               # the running state at hi
        run = K._running(fun, dtype, values, part_start)
        return [(0 if fun == "COUNT" else None) if hi[i] is None else run[hi[i]] for i in range(n)]
    floating = fun == "AVG" or (fun == "SUM" and dtype in K.FLOATS)
    if floating:
        valid = np.array([v is not None for v in values], bool)
        acc, cnt = _ordered_float_sums(_as_f64(dtype, values), valid, lo, hi, frame)
        with np.errstate(all="ignore"):
            res = acc / cnt if fun == "AVG" else acc
        return [None if cnt[i] == 0 else float(res[i]) for i in range(n)]
    out = []
    for i in range(n):
        rows = [] if lo[i] is None else [v for v in values[lo[i]:hi[i] + 1] if v is not None]
        if fun == "COUNT":
            out.append(len(rows))
        elif not rows:
            out.append(None)
        elif fun == "SUM":
            w = sum(rows) & (2**64 - 1)                                    # integer sums wrap
            out.append(w if dtype in K.UNSIGNED else w - 2**64 if w >= 2**63 else w)
        else:
            numbers = [v for v in rows if v == v]                          # a NaN counts only when nothing else is there
            out.append((min(numbers) if fun == "MIN" else max(numbers)) if numbers else math.nan)
    return out


def restate(batch, partition_by, order_by, window_exprs):
    """window_cases.restate for expressions with named frames; the rows frames from the definitions above.  Columns in the operator's
    order: the input's, then one per expression."""
    n = og.batch_len(batch)
    part_start, part_end, _, _ = bounds(batch, partition_by, order_by)
    out = OrderedDict(batch)
    for w in window_exprs:
        frame = canonical(w.frame)
        if not isinstance(frame, F) or w.fun not in FRAMED:
            # (a rows frame on a function without a frame is ignored)
            named = E.WindowExpr(w.fun, w.expr, w.name, w.offset, frame if not isinstance(frame, F) else "DEFAULT")
            out[w.name] = K.restate(batch, partition_by, order_by, [named])[w.name]
            continue
        lo, hi = frame_bounds(part_start, part_end, frame)
        arg = og.evaluate(w.expr, batch)
        if w.fun in ("FIRST_VALUE", "LAST_VALUE"):
            src = lo if w.fun == "FIRST_VALUE" else hi
            idx = np.array([j if j is not None else 0 for j in src], dtype=np.int64)
            inside = np.array([j is not None for j in src], dtype=bool)
            out[w.name] = OCol(arg.dtype, arg.values[idx] if n else arg.values, arg.is_valid()[idx] & inside if n else None)
            continue
        res = _aggregate(w.fun, arg.dtype, arg.to_pylist(), lo, hi, part_start, frame)
        out[w.name] = K._column(K.result_type(w.fun, arg.dtype), res)
    return out
