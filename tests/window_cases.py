"""WindowAggExec restated row by row, and the inputs the window tests share (test_window_cases_cpu.py checks the restatement against
sqlite3 and against pinned values; test_window_gpu.py checks the device against the restatement).

The restatement is written from the contract (DESIGN.md "Window functions"), not from the host code: plain loops over rows that are
ALREADY in the operator's order — the order itself comes from the oracle's SortExec (sorted_input) — and math.fsum for every
floating-point sum, so a float result here is the correctly rounded sum of the frame.

Equality of keys is the GROUP BY rule: NULL equals NULL, floats compare by bit pattern, Utf8 by bytes."""
import math
from collections import OrderedDict

import numpy as np

from ballista_amd import expr as E
from ballista_amd.plan import WINDOW_TILE_ROWS
from oracle import engine as og
from oracle.engine import OCol

T = WINDOW_TILE_ROWS
# the second level of the scans takes this many tile summaries per step (csrc/window_kernels.h WINDOW_SUMMARY_STEP; pinned against the
# header by test_window_cases_cpu.py), so S rows is the smallest count whose summaries need a second step
SUMMARY_STEP = 256
S = T * SUMMARY_STEP + 1
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, S + 1]

FLOATS = ("Float64", "Float32")
UNSIGNED = ("UInt8", "UInt16", "UInt32", "UInt64")
RANKING = ("ROW_NUMBER", "RANK", "DENSE_RANK")
AGGREGATES = ("SUM", "AVG", "COUNT", "MIN", "MAX")


def W(fun, expr, name, offset=1, frame="DEFAULT"):
    return E.WindowExpr(fun, E.col(expr) if isinstance(expr, str) else expr, name, offset, frame)


def asc(name, descending=False, nulls_first=True):
    return E.PhysicalSortExpr(E.col(name) if isinstance(name, str) else name, descending, nulls_first)


def sort_keys(partition_by, order_by):
    """what the operator sorts by: the partition keys ASC NULLS FIRST, then the order keys as given"""
    return [E.PhysicalSortExpr(e, False, True) for e in partition_by] + list(order_by)


def sorted_input(batch, partition_by, order_by):
    keys = sort_keys(partition_by, order_by)
    return og.sort_batch(batch, keys) if keys else batch


def result_type(fun, arg_dtype):
    """(Arrow type, nullable given the argument's nullability) of a window function"""
    if fun in RANKING or fun == "COUNT":
        return "UInt64"
    if fun == "AVG" or (fun == "SUM" and arg_dtype in FLOATS):
        return "Float64"
    if fun == "SUM":
        return "UInt64" if arg_dtype in UNSIGNED else "Int64"
    return arg_dtype


def _images(col):
    """per row, a value that is equal exactly when two keys are equal under the GROUP BY rule"""
    valid = col.is_valid()
    if col.dtype in FLOATS:
        bits = np.ascontiguousarray(col.values).view(np.uint64 if col.dtype == "Float64" else np.uint32)
        vals = [int(b) for b in bits]
    elif col.dtype == "Utf8":
        vals = [s.encode("utf-8") for s in col.values]
    else:
        vals = [v.item() for v in col.values]
    return [(True, v) if ok else (False, None) for v, ok in zip(vals, valid)]


def bounds(batch, partition_by, order_by):
    """part_start, part_end, peer_start, peer_end of every (already sorted) row, by comparing neighbours"""
    n = og.batch_len(batch)
    pk = [_images(og.evaluate(e, batch)) for e in partition_by]
    ok = [_images(og.evaluate(s.expr, batch)) for s in order_by]
    part_start, peer_start = [0] * n, [0] * n
    for i in range(1, n):
        same_part = all(k[i] == k[i - 1] for k in pk)
        same_peer = same_part and all(k[i] == k[i - 1] for k in ok)
        part_start[i] = part_start[i - 1] if same_part else i
        peer_start[i] = peer_start[i - 1] if same_peer else i
    part_end, peer_end = [n - 1] * n, [n - 1] * n
    for i in range(n - 2, -1, -1):
        part_end[i] = part_end[i + 1] if part_start[i + 1] == part_start[i] else i
        peer_end[i] = peer_end[i + 1] if peer_start[i + 1] == peer_start[i] else i
    return part_start, part_end, peer_start, peer_end


class _ExactSum:
    """the running sum of floats held exactly (Shewchuk's non-overlapping partials, what math.fsum keeps); value() = math.fsum of
    the partials = the correctly rounded sum so far.  Infinities and NaNs are added apart, as IEEE adds them."""

    def __init__(self):
        self.partials, self.special = [], None

    def add(self, x):
        if math.isinf(x) or math.isnan(x):
            self.special = x if self.special is None else self.special + x
            return
        i = 0
        for y in self.partials:
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo:
                self.partials[i] = lo
                i += 1
            x = hi
        self.partials[i:] = [x]

    def value(self):
        return self.special if self.special is not None else math.fsum(self.partials)


def _running(fun, dtype, values, part_start):
    """per row the aggregate over rows part_start[i] .. i (None: no non-NULL value there), and for AVG / COUNT what they need"""
    out = [None] * len(values)
    for i, v in enumerate(values):
        if i == part_start[i]:
            count, isum, fsum_, best, saw_nan = 0, 0, _ExactSum(), None, False
        if v is not None:
            count += 1
            if fun in ("SUM", "AVG"):
                if dtype in FLOATS or fun == "AVG":
                    fsum_.add(float(v))
                else:
                    isum += v
            elif fun in ("MIN", "MAX"):
                if dtype in FLOATS and v != v:
                    saw_nan = True                       # a NaN counts only when nothing else is there
                elif best is None or (v < best if fun == "MIN" else v > best):
                    best = v
        if fun == "COUNT":
            out[i] = count
        elif count == 0:
            out[i] = None
        elif fun == "AVG":
            out[i] = fsum_.value() / count
        elif fun == "SUM":
            if dtype in FLOATS:
                out[i] = fsum_.value()
            else:
                w = isum & (2**64 - 1)                    # integer sums wrap
                out[i] = w if dtype in UNSIGNED else w - 2**64 if w >= 2**63 else w
        else:
            out[i] = best if best is not None else math.nan
    return out


def _column(dtype, values):
    valid = np.array([v is not None for v in values], bool)
    if dtype == "Utf8":
        return OCol(dtype, [v if v is not None else "" for v in values], valid)
    return OCol(dtype, np.array([v if v is not None else 0 for v in values], dtype=og.NP_TYPES[dtype]), valid)


def restate(batch, partition_by, order_by, window_exprs):
    """`batch` (dict name -> OCol, rows already in the operator's order) -> its columns plus one per window expression"""
    n = og.batch_len(batch)
    part_start, part_end, peer_start, peer_end = bounds(batch, partition_by, order_by)
    out = OrderedDict(batch)
    for w in window_exprs:
        frame = w.frame if w.frame != "DEFAULT" else ("RANGE_TO_CURRENT" if order_by else "PARTITION")
        frame_end = list(range(n)) if frame == "ROWS_TO_CURRENT" else peer_end if frame == "RANGE_TO_CURRENT" else part_end
        if w.fun in RANKING:
            res, dense = [], 0
            for i in range(n):
                dense = 1 if i == part_start[i] else dense + (1 if i == peer_start[i] else 0)
                res.append(i - part_start[i] + 1 if w.fun == "ROW_NUMBER" else peer_start[i] - part_start[i] + 1 if w.fun == "RANK" else dense)
            out[w.name] = _column("UInt64", res)
            continue
        arg = og.evaluate(w.expr, batch)
        if w.fun not in AGGREGATES:
            # the row each row reads (None: outside the partition); the values are then copied as they are, bit for bit
            if w.fun == "LAG":
                src = [i - w.offset if i - w.offset >= part_start[i] else None for i in range(n)]
            elif w.fun == "LEAD":
                src = [i + w.offset if i + w.offset <= part_end[i] else None for i in range(n)]
            elif w.fun == "FIRST_VALUE":
                src = [part_start[i] for i in range(n)]
            else:
                src = [frame_end[i] for i in range(n)]
            idx = np.array([j if j is not None else 0 for j in src], dtype=np.int64)
            inside = np.array([j is not None for j in src], dtype=bool)
            out[w.name] = OCol(arg.dtype, arg.values[idx] if n else arg.values, arg.is_valid()[idx] & inside if n else None)
            continue
        run = _running(w.fun, arg.dtype, arg.to_pylist(), part_start)
        res = [run[frame_end[i]] for i in range(n)]
        out[w.name] = _column(result_type(w.fun, arg.dtype), res)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

SHAPES = ("one_partition", "every_row", "tile_ends", "last_row", "three_tiles", "peer_straddle")


def partition_ids(shape, n):
    """partition id of the row at each SORTED position (ids rise with the position)"""
    i = np.arange(n, dtype=np.int64)
    if shape == "one_partition":            # the carry crosses every tile
        return np.zeros(n, np.int64)
    if shape == "every_row":
        return i
    if shape == "tile_ends":                # every tile's last row ends a partition; a second cut inside each tile
        return (i // T) * 2 + (i % T >= T // 3)
    if shape == "last_row":                 # a partition that begins on the very last row
        return (i == n - 1).astype(np.int64)
    if shape == "three_tiles":              # rows T/2 .. T/2 + 3T + 7 are one partition: whole tiles without a head
        return (i >= T // 2).astype(np.int64) + (i >= T // 2 + 3 * T + 7)
    if shape == "peer_straddle":            # few, long partitions; the peer groups are what matters (order_ids)
        return i // (2 * T + 77)
    raise ValueError(shape)


def order_ids(shape, n, rng):
    """order key of the row at each sorted position, non-decreasing inside a partition.  peer_straddle: groups of 6 rows laid so that
    rows T - 3 .. T + 2 are one group, and no group starts on any multiple of T: every tile boundary falls inside a peer group, so
    RANGE_TO_CURRENT reads the next tile.  Elsewhere: groups of 1 .. 4 rows."""
    i = np.arange(n, dtype=np.int64)
    if shape == "peer_straddle":
        return (i + (-(T - 3)) % 6) // 6
    return np.cumsum(rng.integers(0, 4, n) == 0)


def table(n, shape, seed, strings=False):
    """n rows whose sorted form has the partitions of `shape`, handed over in a random order.  rn: the INPUT row number.
    p / o: partition and order key (o: NULL in its first peer group of every third partition); i64 with NULLs, f (exact: eighths),
    u (positive uniform), g (Int32, every row of every fifth partition NULL: an all-NULL frame)."""
    rng = np.random.default_rng(seed)
    p, o = partition_ids(shape, n), order_ids(shape, n, rng)
    first_group = np.zeros(n, bool)
    if n:
        starts = np.r_[True, p[1:] != p[:-1]]
        first_row = np.maximum.accumulate(np.where(starts, np.arange(n), 0))         # of the row's partition
        first_group = (o == o[first_row]) & (p % 3 == 0)
    cols = OrderedDict()
    cols["p"] = OCol("Int64", p)
    cols["o"] = OCol("Int32", o.astype(np.int32), ~first_group)          # NULLS FIRST keeps them at the head of the partition
    cols["i64"] = OCol("Int64", rng.integers(-10**6, 10**6, n), rng.random(n) > 0.1)
    cols["f"] = OCol("Float64", rng.integers(-1024, 1025, n) / 8.0, rng.random(n) > 0.1)
    cols["u"] = OCol("Float64", rng.uniform(0.5, 2.0, n))
    cols["g"] = OCol("Int32", rng.integers(-100, 100, n).astype(np.int32), p % 5 != 0)
    if strings:
        cols["s"] = OCol("Utf8", ["s%d" % v if v % 7 else "" for v in rng.integers(0, 50, n)], rng.random(n) > 0.1)
    perm = rng.permutation(n)
    # ties of (p, o) keep input order: the permutation decides which row of a peer group comes first
    out = OrderedDict((k, c.take(perm)) for k, c in cols.items())
    out["rn"] = OCol("Int64", np.arange(n, dtype=np.int64))
    return out


def standard_exprs(strings=False, full=True):
    """what every (size, shape) case computes.  full=False: the subset the largest size runs (the restatement is plain Python)"""
    ws = [W("ROW_NUMBER", None, "row_number"), W("DENSE_RANK", None, "dense_rank"), W("LEAD", "i64", "lead2", 2),
          W("SUM", "f", "run_f", frame="ROWS_TO_CURRENT"), W("COUNT", "i64", "cnt_range"), W("MIN", "g", "min_part", frame="PARTITION"),
          W("SUM", "i64", "sum_range")]
    if full:
        ws += [W("RANK", None, "rank"), W("LAG", "i64", "lag1", 1), W("LAG", "f", "lag0", 0), W("LEAD", "g", "lead_far", 10**7),
               W("FIRST_VALUE", "i64", "first"), W("LAST_VALUE", "f", "last_range"), W("LAST_VALUE", "i64", "last_part", frame="PARTITION"),
               W("LAST_VALUE", "g", "last_rows", frame="ROWS_TO_CURRENT"), W("AVG", "f", "avg_part", frame="PARTITION"),
               W("AVG", "i64", "avg_rows", frame="ROWS_TO_CURRENT"), W("MAX", "f", "max_range"), W("MAX", "g", "max_rows", frame="ROWS_TO_CURRENT"),
               E.count_star("count_star"), W("SUM", "g", "sum_g", frame="PARTITION")]
    if strings:
        ws += [W("LAG", "s", "lag_s", 1), W("FIRST_VALUE", "s", "first_s"), W("COUNT", "s", "count_s", frame="ROWS_TO_CURRENT")]
    return ws


def every_type_table(n, seed):
    """one argument column of every type the operator takes, with NULLs; p: 7 partitions, o: an order key with ties.  The signed ranges
    keep every sum of n values below 2^53, so AVG (a sum of doubles) is exact; UInt64 takes its whole range: its SUM wraps"""
    rng = np.random.default_rng(seed)
    cols = OrderedDict()
    cols["p"] = OCol("Int32", rng.integers(0, 7, n).astype(np.int32))
    cols["o"] = OCol("Int64", rng.integers(0, n // 3 + 1, n))
    ranges = {"Int8": (-128, 128), "Int16": (-2**15, 2**15), "Int32": (-2**31, 2**31), "Int64": (-2**40, 2**40), "UInt8": (0, 256),
              "UInt16": (0, 2**16), "UInt32": (0, 2**32), "Date32": (-10**5, 10**5), "Date64": (-10**12, 10**12),
              "Timestamp(Second)": (-10**9, 10**9), "Timestamp(Millisecond)": (-10**12, 10**12), "Timestamp(Microsecond)": (-10**13, 10**13),
              "Timestamp(Nanosecond)": (-10**13, 10**13)}
    for t, (lo, hi) in ranges.items():
        cols["c_" + t] = OCol(t, rng.integers(lo, hi, n).astype(og.NP_TYPES[t]), rng.random(n) > 0.15)
    cols["c_UInt64"] = OCol("UInt64", rng.integers(0, 2**64, n, dtype=np.uint64), rng.random(n) > 0.15)
    cols["c_Float64"] = OCol("Float64", rng.integers(-4096, 4096, n) / 16.0, rng.random(n) > 0.15)
    cols["c_Float32"] = OCol("Float32", (rng.integers(-4096, 4096, n) / 16.0).astype(np.float32), rng.random(n) > 0.15)
    cols["c_Boolean"] = OCol("Boolean", rng.random(n) > 0.5, rng.random(n) > 0.15)
    cols["c_Utf8"] = OCol("Utf8", ["v%d" % v for v in rng.integers(0, 30, n)], rng.random(n) > 0.15)
    cols["rn"] = OCol("Int64", np.arange(n, dtype=np.int64))
    return cols


def every_type_exprs(batch):
    ws = []
    for name, c in batch.items():
        if not name.startswith("c_"):
            continue
        t = name[2:]
        ws += [W("LAG", name, "lag_" + t, 1), W("LEAD", name, "lead_" + t, 3), W("FIRST_VALUE", name, "first_" + t),
               W("LAST_VALUE", name, "last_" + t), W("COUNT", name, "count_" + t)]
        if t not in ("Boolean", "Utf8"):
            ws += [W("SUM", name, "sum_" + t, frame="ROWS_TO_CURRENT"), W("AVG", name, "avg_" + t, frame="PARTITION"),
                   W("MIN", name, "min_" + t), W("MAX", name, "max_" + t, frame="ROWS_TO_CURRENT")]
    return ws
