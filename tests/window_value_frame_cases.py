"""RANGE and GROUPS frames of WindowAggExec restated row by row (test_window_value_frames_cpu.py checks this against sqlite3 and pins
what sqlite cannot express, test_window_value_frames_gpu.py checks the device against it).

Written from the contract ("Frames measured in values and in peer groups"), not from the host code.  A frame has two
sides, each None (UNBOUNDED), E.CURRENT_ROW or a signed offset.  For row i of the partition [ps, pe], in the operator's order:

  UNBOUNDED    ps / pe
  CURRENT ROW  i's first / last peer
  GROUPS       the partition's peer groups are numbered 0 .. G-1 and i lies in group g: lo = the first row of group max(g + start, 0),
               none when g + start > G-1; hi = the last row of group min(g + end, G-1), none when g + end < 0
  RANGE        one order key; s = +1 ascending, -1 descending.  The rows that QUALIFY are found by brute force over the partition:
               integer-typed keys  s (key_j - key_i) >= start  /  <= end, in Python integers (nothing wraps);
               float keys          t = key_i + s offset as one np.float64 addition; key_j >= t / key_j <= t ascending, mirrored
                                   descending, by IEEE comparison (-0.0 == +0.0);
               only a row whose key is a number qualifies (not NULL, not NaN); lo = the first such row, hi = the last.  A row i whose own
               key is NULL or NaN takes its peer bound.
  The frame is lo .. hi when both exist and lo <= hi, else empty: COUNT 0, NULL elsewhere.

The results then go through the loops of window_frame_cases: the gathers, the integer loops, and for float SUM / AVG without an unbounded
start the left-to-right Float64 sum from +0.0 (a frame that starts UNBOUNDED reads the running state, math.fsum)."""
import math
from collections import OrderedDict

import numpy as np

from ballista_amd import expr as E
from oracle import engine as og
from oracle.engine import OCol
from tests import window_cases as K, window_frame_cases as FK
from tests.window_cases import W, asc, bounds                            # noqa: F401  (the tests take them from here)

R, G, CUR, F = E.RangeFrame, E.GroupsFrame, E.CURRENT_ROW, E.RowsFrame
FRAMED = FK.FRAMED
INTEGER_KEYS = ("Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64", "Date32", "Date64", "Timestamp(Second)",
                "Timestamp(Millisecond)", "Timestamp(Microsecond)", "Timestamp(Nanosecond)")


def is_offset(side):
    return side is not None and side is not CUR


def canonical(frame, fun="SUM"):
    """the value frames that ARE other frames (and run and display as them); a function without a frame ignores it"""
    if not isinstance(frame, (R, G)):
        return frame
    if fun not in FRAMED:
        return "DEFAULT"
    start, end = frame.start, frame.end
    if isinstance(frame, G):                                               # under GROUPS, CURRENT ROW is offset 0
        start, end = (0 if start is CUR else start), (0 if end is CUR else end)
    if start is None and end is None:
        return "PARTITION"
    if start is None and (end is CUR or (isinstance(frame, G) and end == 0)):
        return "RANGE_TO_CURRENT"
    return type(frame)(start, end)


def can_be_empty(frame):
    return (is_offset(frame.start) and frame.start > 0) or (is_offset(frame.end) and frame.end < 0)


def _range_side(keys, numeric, ps, pe, offset, descending, is_end, floating):
    """one OFFSET side for every row i of the partition ps .. pe at once: the rows j that qualify, by the definition, as a matrix
    (i, j) taken 512 rows i at a time -> per row the first (start) / last (end) qualifying row, -1: none"""
    k = keys[ps:pe + 1]
    out = np.full(pe - ps + 1, -1, np.int64)
    for at in range(0, len(k), 512):
        mine = k[at:at + 512, None]
        if floating:
            with np.errstate(all="ignore"):
                t = mine - np.float64(offset) if descending else mine + np.float64(offset)       # one Float64 addition per row i
                ok = (k[None, :] <= t) if (is_end != descending) else (k[None, :] >= t)
        else:
            d = (k[None, :] - mine) * (-1 if descending else 1)           # object arrays of Python integers, or int64 far from overflow
            ok = (d <= offset) if is_end else (d >= offset)
        ok = np.asarray(ok, bool) & numeric[None, ps:pe + 1]
        some = ok.any(axis=1)
        where = (ok.shape[1] - 1 - np.argmax(ok[:, ::-1], axis=1)) if is_end else np.argmax(ok, axis=1)
        out[at:at + 512] = np.where(some, ps + where, -1)
    return out


def frame_bounds(batch, partition_by, order_by, frame):
    """(lo, hi) per row of the already sorted batch; (None, None): the empty frame"""
    n = og.batch_len(batch)
    part_start, part_end, peer_start, peer_end = bounds(batch, partition_by, order_by)
    lo, hi = [None] * n, [None] * n
    ranged = isinstance(frame, R) and (is_offset(frame.start) or is_offset(frame.end))
    if ranged:
        assert len(order_by) == 1, "a RANGE offset needs exactly one order key"
        col = og.evaluate(order_by[0].expr, batch)
        floating = col.dtype in K.FLOATS
        assert floating or col.dtype in INTEGER_KEYS, col.dtype
        valid = col.is_valid()
        if floating:
            keys = np.asarray(col.values, np.float64)                     # Float32 widened
            numeric = valid & ~np.isnan(keys)
        else:
            exact = [int(v) for v in col.values]
            far = max([abs(v) for v in exact] + [abs(o) for o in (frame.start, frame.end) if is_offset(o)] + [0]) >= 2**61
            keys = np.array(exact, dtype=object if far else np.int64)
            numeric = valid.copy()
        descending = order_by[0].descending
    # the number of the row's peer group inside its partition
    group = [0] * n
    for i in range(1, n):
        group[i] = 0 if part_start[i] == i else group[i - 1] + (1 if peer_start[i] == i else 0)
    for ps in sorted(set(part_start)):
        pe = part_end[ps]
        firsts = [j for j in range(ps, pe + 1) if peer_start[j] == j]      # the first row of each peer group
        n_groups = len(firsts)
        searched = {}
        if ranged:
            for side, is_end in ((frame.start, False), (frame.end, True)):
                if is_offset(side):
                    searched[is_end] = _range_side(keys, numeric, ps, pe, side, descending, is_end, floating)
        for i in range(ps, pe + 1):
            ends = []
            for side, is_end in ((frame.start, False), (frame.end, True)):
                if side is None:
                    ends.append(pe if is_end else ps)
                elif side is CUR:
                    ends.append(peer_end[i] if is_end else peer_start[i])
                elif isinstance(frame, G):
                    g = group[i] + side
                    if is_end:
                        ends.append(None if g < 0 else peer_end[firsts[min(g, n_groups - 1)]])
                    else:
                        ends.append(None if g > n_groups - 1 else firsts[max(g, 0)])
                elif not numeric[i]:
                    ends.append(peer_end[i] if is_end else peer_start[i])
                else:
                    j = int(searched[is_end][i - ps])
                    ends.append(None if j < 0 else j)
            a, b = ends
            if a is not None and b is not None and a <= b:
                lo[i], hi[i] = a, b
    return lo, hi


def _ordered_float_sums(x, valid, lo, hi):
    """per row (sum, count) of the non-NULL x[lo .. hi] added to +0.0 in row order: window_frame_cases._ordered_float_sums — one numpy
    step per position, `acc = where(in_frame & valid, acc + x, acc)`, the same IEEE additions in the same order for every row —
    stepped from the frame's first row instead of from the row itself, since a value frame may lie thousands of rows from its row"""
    n = len(x)
    acc, cnt = np.zeros(n, np.float64), np.zeros(n, np.int64)
    lo_a = np.array([0 if v is None else v for v in lo], np.int64)
    width = np.array([0 if a is None else b - a + 1 for a, b in zip(lo, hi)], np.int64)
    for k in range(int(width.max()) if n else 0):
        inside = k < width
        j = np.where(inside, lo_a + k, 0)
        take = inside & valid[j]
        with np.errstate(all="ignore"):
            acc = np.where(take, acc + x[j], acc)
        cnt += take
    return acc, cnt


def _aggregate(fun, dtype, values, lo, hi, part_start, start_unbounded):
    """window_frame_cases._aggregate over any (lo, hi): its running state and its integer / MIN / MAX loops as they are (they read lo
    and hi alone); the ordered float sum from the loop above"""
    if (fun == "AVG" or (fun == "SUM" and dtype in K.FLOATS)) and not start_unbounded:
        valid = np.array([v is not None for v in values], bool)
        acc, cnt = _ordered_float_sums(FK._as_f64(dtype, values), valid, lo, hi)
        with np.errstate(all="ignore"):
            res = acc / cnt if fun == "AVG" else acc
        return [None if cnt[i] == 0 else float(res[i]) for i in range(len(values))]
    if fun == "COUNT" or (fun == "SUM" and not start_unbounded):
        # its loop over values[lo .. hi] as a difference of prefix totals in Python integers: exact, so the same numbers, and a frame
        # that runs to the partition's end does not cost its width per row
        count, total = [0], [0]
        for v in values:
            count.append(count[-1] + (v is not None))
            total.append(total[-1] + (0 if v is None or fun == "COUNT" else v))
        out = []
        for a, b in zip(lo, hi):
            c = 0 if a is None else count[b + 1] - count[a]
            w = (0 if a is None else total[b + 1] - total[a]) & (2**64 - 1)                    # integer sums wrap
            out.append(c if fun == "COUNT" else None if c == 0 else w if dtype in K.UNSIGNED else w - 2**64 if w >= 2**63 else w)
        return out
    return FK._aggregate(fun, dtype, values, lo, hi, part_start, F(None if start_unbounded else 0, 0))


def restate(batch, partition_by, order_by, window_exprs):
    """window_frame_cases.restate for everything but the RANGE / GROUPS frames that stay such; those from the definitions above.
    Columns in the operator's order: the input's, then one per expression."""
    n = og.batch_len(batch)
    part_start, _, _, _ = bounds(batch, partition_by, order_by)
    out = OrderedDict(batch)
    made = {}
    for w in window_exprs:
        frame = canonical(w.frame, w.fun)
        if not isinstance(frame, (R, G)):
            same = E.WindowExpr(w.fun, w.expr, w.name, w.offset, frame)
            out[w.name] = FK.restate(batch, partition_by, order_by, [same])[w.name]
            continue
        if frame not in made:
            made[frame] = frame_bounds(batch, partition_by, order_by, frame)
        lo, hi = made[frame]
        arg = og.evaluate(w.expr, batch)
        if w.fun in ("FIRST_VALUE", "LAST_VALUE"):
            src = lo if w.fun == "FIRST_VALUE" else hi
            idx = np.array([j if j is not None else 0 for j in src], dtype=np.int64)
            inside = np.array([j is not None for j in src], dtype=bool)
            out[w.name] = OCol(arg.dtype, arg.values[idx] if n else arg.values, arg.is_valid()[idx] & inside if n else None)
            continue
        res = _aggregate(w.fun, arg.dtype, arg.to_pylist(), lo, hi, part_start, frame.start is None)
        out[w.name] = K._column(K.result_type(w.fun, arg.dtype), res)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

# key type -> (the key of order id o, what one step of the order id is worth in the key's units)
KEY_TYPES = OrderedDict([
    ("Int64", (lambda o: (o - 7).astype(np.int64), 1)),
    ("Int32", (lambda o: (o - 7).astype(np.int32), 1)),
    ("UInt64", (lambda o: o.astype(np.uint64) + np.uint64(2**63 + 5), 1)),                    # every value above 2^63
    ("Date32", (lambda o: (o + 18000).astype(np.int32), 1)),
    ("Timestamp(Microsecond)", (lambda o: (o * 1000 - 5000).astype(np.int64), 1000)),
    ("Float64", (lambda o: o * 0.5 - 3.0, 0.5)),
    ("Float32", (lambda o: (o * 0.25 - 2.0).astype(np.float32), 0.25)),
])


def table(n, shape, seed, key="Int64"):
    """window_cases.table with the order key `o` of type `key`: ties (peer groups of 1 .. 4 rows, 6 under peer_straddle) AND gaps (every
    third distinct value is followed by a hole of two steps), NULL in the first peer group of every third partition"""
    t = K.table(n, shape, seed)
    o = t["o"]
    ids = np.asarray(o.values, np.int64)
    make, _ = KEY_TYPES[key]
    t["o"] = OCol(key, make(ids + 2 * (ids // 3)), o.is_valid().copy())
    return t


def step(key, m):
    """m steps of the order id as an offset over a key of type `key`"""
    unit = KEY_TYPES[key][1]
    return m * unit if isinstance(unit, int) else float(m * unit)
