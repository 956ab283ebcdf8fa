"""CPU tier of WindowAggExec: no GPU work.

1. the row-by-row restatement (tests/window_cases.py) against the standard library's sqlite3 on tables SQLite can hold (integers within
   Int63, small dyadic floats whose sums are exact, no NaN).  What depends on the order of ties (ROW_NUMBER, LAG / LEAD, FIRST / LAST_VALUE,
   the ROWS frame) is asked of SQLite with the input row number as an extra last order key — the operator's stable sort keeps ties in
   input order; what depends on peers (RANK, DENSE_RANK, the RANGE frame) without it;
2. the values SQLite cannot check, against hand-written expectations: NaN rules, UInt64 above 2^63, wrapping sums, -0.0 / +0.0;
3. plan-time behaviour over a leaf decoded from a wire plan with no context: schema, display, with_new_children, every refusal;
4. the tile constants of the Python mirror and of this file's tables against csrc/window_kernels.h."""
import math
import os
import re
import sqlite3
import struct

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle.engine import OCol
from tests import plan_nodes as N, proto_encode as pe, window_cases as K
from tests.window_cases import W, asc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against SQLite -------------------------------------------------------------------------------------------

def sqlite_table(n=400, seed=7):
    rng = np.random.default_rng(seed)
    def nulls(share):
        return rng.random(n) > share
    return {"p": OCol("Int64", rng.integers(0, 6, n), nulls(0.1)),
            "q": OCol("Utf8", [("k%d" % v) for v in rng.integers(0, 3, n)], nulls(0.15)),
            "o": OCol("Int64", rng.integers(-5, 12, n), nulls(0.1)),
            "x": OCol("Int64", rng.integers(-10**9, 10**9, n), nulls(0.2)),
            "f": OCol("Float64", rng.integers(-2000, 2000, n) / 16.0, nulls(0.2)),
            "s": OCol("Utf8", ["t%d" % v for v in rng.integers(0, 40, n)], nulls(0.2)),
            "rn": OCol("Int64", np.arange(n, dtype=np.int64))}


SPECS = {
    "one_key_asc": (["p"], [asc("o")]),
    "two_keys_desc_nulls_last": (["p", "q"], [asc("o", True, False)]),
    "no_partition_two_order_keys": ([], [asc("o", False, False), asc("x", True, True)]),
    "no_order": (["q"], []),
    "nothing": ([], []),
}

SQL_FRAME = {"ROWS_TO_CURRENT": "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW", "PARTITION": "ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING",
             "RANGE_TO_CURRENT": "RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW"}


def sql_for(w, partition_by, order_by):
    """one SELECT item computing window expression `w` the SQL way"""
    order_sql = [f"{s.expr.name} {'DESC' if s.descending else 'ASC'} NULLS {'FIRST' if s.nulls_first else 'LAST'}" for s in order_by]
    part_sql = ("PARTITION BY " + ", ".join(partition_by) + " ") if partition_by else ""
    tie = part_sql + "ORDER BY " + ", ".join(order_sql + ["rn"])                       # ties in input order
    peer = part_sql + ("ORDER BY " + ", ".join(order_sql) if order_sql else "")
    frame = w.frame if w.frame != "DEFAULT" else ("RANGE_TO_CURRENT" if order_by else "PARTITION")
    arg = "*" if isinstance(w.expr, E.Literal) else w.expr.name if w.expr is not None else ""
    if w.fun == "ROW_NUMBER":
        return f"row_number() OVER ({tie})"
    if w.fun in ("RANK", "DENSE_RANK"):
        return f"{w.fun.lower()}() OVER ({peer})"
    if w.fun in ("LAG", "LEAD"):
        return f"{w.fun.lower()}({arg}, {w.offset}) OVER ({tie})"
    if w.fun == "FIRST_VALUE":
        return f"first_value({arg}) OVER ({tie})"
    if w.fun == "LAST_VALUE" and frame == "RANGE_TO_CURRENT":
        # the last peer in input order: no window function says that once rn is an order key, so a correlated subquery does
        same = " AND ".join(f"t2.{k} IS t.{k}" for k in partition_by + [s.expr.name for s in order_by]) or "1"
        return f"(SELECT t2.{arg} FROM t t2 WHERE {same} ORDER BY t2.rn DESC LIMIT 1)"
    if w.fun == "LAST_VALUE":
        return f"last_value({arg}) OVER ({tie} {SQL_FRAME[frame]})"
    fn = {"SUM": "sum", "AVG": "avg", "COUNT": "count", "MIN": "min", "MAX": "max"}[w.fun]
    return f"{fn}({arg}) OVER ({tie if frame == 'ROWS_TO_CURRENT' else peer} {SQL_FRAME[frame]})"


def sqlite_exprs():
    ws = [W("ROW_NUMBER", None, "rnum"), W("RANK", None, "rnk"), W("DENSE_RANK", None, "dense"),
          W("LAG", "x", "lag1", 1), W("LAG", "s", "lag2", 2), W("LAG", "f", "lag0", 0), W("LEAD", "f", "lead1", 1), W("LEAD", "x", "lead50", 50),
          W("FIRST_VALUE", "s", "first_s"), W("FIRST_VALUE", "x", "first_x"), E.count_star("star_rows", "ROWS_TO_CURRENT"), E.count_star("star")]
    for frame in ("DEFAULT", "PARTITION", "ROWS_TO_CURRENT", "RANGE_TO_CURRENT"):
        ws += [W("LAST_VALUE", "s", "last_s_" + frame, frame=frame), W("LAST_VALUE", "f", "last_f_" + frame, frame=frame)]
        for fun in K.AGGREGATES:
            ws += [W(fun, "x", f"{fun}_x_{frame}", frame=frame), W(fun, "f", f"{fun}_f_{frame}", frame=frame)]
        ws += [W("COUNT", "s", "count_s_" + frame, frame=frame)]
    return ws


@pytest.mark.parametrize("spec", list(SPECS))
def test_the_restatement_agrees_with_sqlite(spec):
    assert sqlite3.sqlite_version_info >= (3, 30), sqlite3.sqlite_version
    partition_by, order_by = SPECS[spec]
    batch = sqlite_table()
    n = len(batch["rn"])
    ws = sqlite_exprs()
    got = K.restate(K.sorted_input(batch, [col(k) for k in partition_by], order_by), [col(k) for k in partition_by], order_by, ws)
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE t (p, q, o, x, f, s, rn)")
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?, ?, ?)", list(zip(*[batch[k].to_pylist() for k in ("p", "q", "o", "x", "f", "s", "rn")])))
    want = {r[0]: r[1:] for r in db.execute("SELECT rn, " + ", ".join(sql_for(w, partition_by, order_by) for w in ws) + " FROM t t")}
    assert len(want) == n
    rns = got["rn"].to_pylist()
    for k, w in enumerate(ws):
        mine = got[w.name].to_pylist()
        bad = [(rn, mine[i], want[rn][k]) for i, rn in enumerate(rns) if mine[i] != want[rn][k] or type(mine[i]) is not type(want[rn][k])]
        assert not bad, (w.name, sql_for(w, partition_by, order_by), bad[:5])
    # the table exercises what it is there for: NULL results, ties, more than one partition
    assert None in got["lag1"].to_pylist() and None in got["MIN_f_PARTITION"].to_pylist() + got["lead1"].to_pylist()
    assert max(got["rnum"].to_pylist()) > max(got["dense"].to_pylist()) or not order_by


# ---- 2. what SQLite cannot hold: pinned by hand -------------------------------------------------------------------------------------

NAN = math.nan


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def run(cols, partition_by, order_by, ws):
    batch = dict(cols)
    batch["rn"] = OCol("Int64", np.arange(len(next(iter(cols.values()))), dtype=np.int64))
    pb = [col(k) for k in partition_by]
    return K.restate(K.sorted_input(batch, pb, order_by), pb, order_by, ws)


def same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and (x == y or (x != x and y != y))) for x, y in zip(a, b))


def test_nan_rules_are_pinned():
    v = OCol("Float64", [NAN, 1.0, NAN, -2.0, NAN, NAN], np.array([True, True, True, True, False, True]))
    got = run({"p": OCol("Int32", [0, 0, 0, 0, 1, 1]), "v": v}, ["p"], [],
              [W("MIN", "v", "mn", frame="ROWS_TO_CURRENT"), W("MAX", "v", "mx", frame="ROWS_TO_CURRENT"), W("MIN", "v", "mn_all"),
               W("SUM", "v", "sm", frame="ROWS_TO_CURRENT"), W("COUNT", "v", "ct", frame="ROWS_TO_CURRENT")])
    assert same(got["mn"].to_pylist(), [NAN, 1.0, 1.0, -2.0, None, NAN])          # a NaN only while nothing else is there
    assert same(got["mx"].to_pylist(), [NAN, 1.0, 1.0, 1.0, None, NAN])
    assert same(got["mn_all"].to_pylist(), [-2.0] * 4 + [NAN] * 2)
    assert same(got["sm"].to_pylist(), [NAN] * 4 + [None, NAN])                    # a sum takes the NaN like any addition
    assert got["ct"].to_pylist() == [1, 2, 3, 4, 0, 1]


def test_float_keys_compare_by_bit_pattern():
    """-0.0 and +0.0 are two partitions, two NaNs are one partition only when their bits agree; NULL equals NULL"""
    keys = OCol("Float64", [0.0, -0.0, f64(0x7FF8000000000000), 0.0, f64(0x7FF8000000000001), f64(0x7FF8000000000000), -0.0, 5.0, 6.0],
                np.array([True] * 7 + [False] * 2))
    got = run({"k": keys}, ["k"], [], [E.count_star("c"), W("ROW_NUMBER", None, "r")])
    # sorted: NULL NULL | -0.0 -0.0 | +0.0 +0.0 | NaN NaN | NaN(payload 1)
    assert got["rn"].to_pylist() == [7, 8, 1, 6, 0, 3, 2, 5, 4]
    assert got["c"].to_pylist() == [2, 2, 2, 2, 2, 2, 2, 2, 1]
    assert got["r"].to_pylist() == [1, 2, 1, 2, 1, 2, 1, 2, 1]
    # the same values as ORDER keys: peers by bit pattern
    got = run({"k": keys}, [], [asc("k")], [W("RANK", None, "rank"), W("DENSE_RANK", None, "dense"), E.count_star("upto")])
    assert got["rank"].to_pylist() == [1, 1, 3, 3, 5, 5, 7, 7, 9]
    assert got["dense"].to_pylist() == [1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert got["upto"].to_pylist() == [2, 2, 4, 4, 6, 6, 8, 8, 9]


def test_uint64_and_wrapping_sums_are_pinned():
    u = OCol("UInt64", np.array([2**63, 2**63, 5, 2**64 - 1], np.uint64))
    i = OCol("Int64", np.array([2**63 - 1, 1, -2**63, -1], np.int64))
    got = run({"u": u, "i": i}, [], [], [W("SUM", "u", "su", frame="ROWS_TO_CURRENT"), W("MAX", "u", "mu", frame="ROWS_TO_CURRENT"),
                                        W("MIN", "u", "nu", frame="ROWS_TO_CURRENT"), W("SUM", "i", "si", frame="ROWS_TO_CURRENT"),
                                        W("MIN", "i", "ni", frame="ROWS_TO_CURRENT"), W("AVG", "u", "au", frame="ROWS_TO_CURRENT")])
    assert got["su"].dtype == "UInt64" and got["su"].to_pylist() == [2**63, 0, 5, 4]
    assert got["mu"].to_pylist() == [2**63, 2**63, 2**63, 2**64 - 1] and got["nu"].to_pylist() == [2**63, 2**63, 5, 5]      # no negative numbers
    assert got["si"].dtype == "Int64" and got["si"].to_pylist() == [2**63 - 1, -2**63, 0, -1]
    assert got["ni"].to_pylist() == [2**63 - 1, 1, -2**63, -2**63]
    assert got["au"].to_pylist()[:2] == [2.0**63, 2.0**63]                                                                  # AVG sums doubles: no wrap


def test_offsets_frames_and_ties_are_pinned():
    """a table small enough to do by hand: p = a a a a b | o = 1 1 2 NULL 1, given in the order rn = 0 .. 4"""
    got = run({"p": OCol("Utf8", ["a", "a", "a", "a", "b"]), "o": OCol("Int32", [1, 1, 2, 0, 1], np.array([True, True, True, False, True])),
               "v": OCol("Int64", [10, 20, 30, 40, 50], np.array([True, False, True, True, True]))}, ["p"], [asc("o")],
              [W("ROW_NUMBER", None, "r"), W("RANK", None, "k"), W("DENSE_RANK", None, "d"), W("LAG", "v", "lag", 1), W("LEAD", "v", "lead", 2),
               W("LAG", "v", "lag0", 0), W("SUM", "v", "range"), W("SUM", "v", "rows", frame="ROWS_TO_CURRENT"), W("SUM", "v", "part", frame="PARTITION"),
               W("LAST_VALUE", "v", "last"), W("FIRST_VALUE", "v", "first"), W("COUNT", "v", "cnt"), W("AVG", "v", "avg")])
    assert got["rn"].to_pylist() == [3, 0, 1, 2, 4]                       # NULLS FIRST; the tie of o = 1 in input order
    assert got["r"].to_pylist() == [1, 2, 3, 4, 1] and got["k"].to_pylist() == [1, 2, 2, 4, 1] and got["d"].to_pylist() == [1, 2, 2, 3, 1]
    assert got["lag"].to_pylist() == [None, 40, 10, None, None] and got["lead"].to_pylist() == [None, 30, None, None, None]
    assert got["lag0"].to_pylist() == [40, 10, None, 30, 50]
    assert got["range"].to_pylist() == [40, 50, 50, 80, 50] and got["rows"].to_pylist() == [40, 50, 50, 80, 50] and got["part"].to_pylist() == [80] * 4 + [50]
    assert got["last"].to_pylist() == [40, None, None, 30, 50] and got["first"].to_pylist() == [40] * 4 + [50]
    assert got["cnt"].to_pylist() == [1, 2, 2, 3, 1] and got["avg"].to_pylist() == [40.0, 25.0, 25.0, 80 / 3, 50.0]


# ---- 3. plan time, with no GPU ------------------------------------------------------------------------------------------------------

def leaf(partitions=1):
    """a plan to build on, made with no context"""
    b = {"s": OCol("Utf8", ["a", ""], np.array([True, False])), "u": OCol("Utf8", ["b", "c"]), "k": OCol("Int64", [1, 2]),
         "kn": OCol("Int64", [1, 2], np.array([True, False])), "i": OCol("Int32", [1, 2]), "u8": OCol("UInt8", [1, 2]), "f": OCol("Float64", [1.0, 2.0]),
         "f32": OCol("Float32", [1.0, 2.0]), "b": OCol("Boolean", [True, False]), "d": OCol("Date32", np.array([1, 2], np.int32))}
    m = N.MemoryExec([[b]] * partitions)
    m.name = "mem://window"
    return ba.ExecutionPlan.from_proto(None, pe.plan(m))


def raw(fun, expr, name, offset=1, frame="DEFAULT"):
    w = object.__new__(E.WindowExpr)          # past the host mirror's own checks: the C ABI can be handed any number
    w.fun, w.expr, w.name, w.offset, w.frame = fun, expr, name, offset, frame
    return w


def test_schema_nullability_and_display():
    ws = [W("ROW_NUMBER", None, "rn"), W("RANK", None, "rk"), W("DENSE_RANK", None, "dr"), W("LAG", "u", "lag_u", 2), W("LEAD", "b", "lead_b", 0),
          W("FIRST_VALUE", "u", "first_u"), W("FIRST_VALUE", "kn", "first_kn"), W("LAST_VALUE", "d", "last_d"), W("SUM", "i", "sum_i"),
          W("SUM", "u8", "sum_u8"), W("SUM", "f32", "sum_f32"), W("AVG", "i", "avg_i"), W("COUNT", "s", "count_s"), E.count_star("star"),
          W("MIN", "f32", "min_f32"), W("MAX", "d", "max_d", frame="ROWS_TO_CURRENT"), W("MAX", "kn", "max_kn", frame="PARTITION"),
          W("LAG", E.ScalarFunctionExpr("lower", [col("s")]), "lag_lower", 1)]
    plan = ba.WindowAggExec([col("k"), E.ScalarFunctionExpr("lower", [col("u")])], [asc("f", True, False), asc("i")], ws, leaf())
    assert plan.as_any() == "WindowAggExec" and plan.output_partitioning().count == 1
    assert plan.schema() == leaf().schema() + [
        ("rn", "UInt64", False), ("rk", "UInt64", False), ("dr", "UInt64", False), ("lag_u", "Utf8", True), ("lead_b", "Boolean", True),
        ("first_u", "Utf8", False), ("first_kn", "Int64", True), ("last_d", "Date32", False), ("sum_i", "Int64", True), ("sum_u8", "UInt64", True),
        ("sum_f32", "Float64", True), ("avg_i", "Float64", True), ("count_s", "UInt64", False), ("star", "UInt64", False),
        ("min_f32", "Float32", True), ("max_d", "Date32", True), ("max_kn", "Int64", True), ("lag_lower", "Utf8", True)]
    text = plan.display()
    for part in ("WindowAggExec: partition_by=[k, lower(u)], order_by=[f DESC NULLS LAST, i ASC NULLS FIRST]", "ROW_NUMBER() as rn", "LAG(u, 2) as lag_u",
                 "LEAD(b, 0) as lead_b", "FIRST_VALUE(u) as first_u", "LAST_VALUE(d) RANGE_TO_CURRENT as last_d", "SUM(i) RANGE_TO_CURRENT as sum_i",
                 "COUNT(UInt8(1)) RANGE_TO_CURRENT as star", "MAX(d) ROWS_TO_CURRENT as max_d", "MAX(kn) PARTITION as max_kn"):
        assert part in text, (part, text)
    # the DEFAULT frame without an order_by is the whole partition
    text = ba.WindowAggExec([col("k")], [], [W("SUM", "i", "t"), W("LAST_VALUE", "u", "l"), W("RANK", None, "r")], leaf()).display()
    assert "SUM(i) PARTITION as t" in text and "LAST_VALUE(u) PARTITION as l" in text and "RANK() as r" in text
    assert "order_by=[]" in text and "mem://window" in text


def test_with_new_children_and_stacking():
    first = ba.WindowAggExec([col("k")], [asc("i")], [W("ROW_NUMBER", None, "r1")], leaf())
    second = ba.WindowAggExec([col("u")], [asc("r1", True)], [W("SUM", "r1", "s2", frame="ROWS_TO_CURRENT")], first)       # reads the first one's output
    assert second.schema()[-2:] == [("r1", "UInt64", False), ("s2", "UInt64", True)]
    again = second.with_new_children([first])
    assert again.schema() == second.schema() and again.display() == second.display()
    assert [c.as_any() for c in again.children()] == ["WindowAggExec"]
    with pytest.raises(ba.PlanError, match="WindowAggExec wrong number of children"):
        second.with_new_children([first, first])
    # a two-partition input is taken at plan time and refused when it runs (test_window_gpu.py)
    assert ba.WindowAggExec([], [], [W("ROW_NUMBER", None, "r")], leaf(2)).output_partitioning().count == 1


REFUSALS = [
    ("nine partition keys", lambda: ba.WindowAggExec([col("k")] * 9, [], [W("ROW_NUMBER", None, "r")], leaf()), ba.NotImplementedOnGpu,
     "at most 8 partition keys and 8 order keys"),
    ("nine order keys", lambda: ba.WindowAggExec([], [asc("k")] * 9, [W("ROW_NUMBER", None, "r")], leaf()), ba.NotImplementedOnGpu,
     "at most 8 partition keys and 8 order keys"),
    ("MIN over Utf8", lambda: ba.WindowAggExec([], [], [W("MIN", "s", "m")], leaf()), ba.NotImplementedOnGpu, "MIN over Utf8 is not supported as a window function"),
    ("MAX over Boolean", lambda: ba.WindowAggExec([], [], [W("MAX", "b", "m")], leaf()), ba.NotImplementedOnGpu, "MAX over Boolean is not supported"),
    ("SUM over Utf8", lambda: ba.WindowAggExec([], [], [W("SUM", "s", "m")], leaf()), ba.PlanError, "SUM does not support Utf8"),
    ("AVG over Boolean", lambda: ba.WindowAggExec([], [], [W("AVG", "b", "m")], leaf()), ba.PlanError, "AVG does not support Boolean"),
    ("negative k", lambda: ba.WindowAggExec([], [], [W("LAG", "k", "l", -1)], leaf()), ba.PlanError, "LAG offset must not be negative, got -1"),
    ("negative k of LEAD", lambda: ba.WindowAggExec([], [], [W("LEAD", "k", "l", -(2**63))], leaf()), ba.PlanError, "LEAD offset must not be negative"),
    ("unknown function", lambda: ba.WindowAggExec([], [], [raw(13, col("k"), "n")], leaf()), ba.PlanError, "Unknown window function 13"),
    ("function 0", lambda: ba.WindowAggExec([], [], [raw(0, col("k"), "n")], leaf()), ba.PlanError, "Unknown window function 0"),
    ("unknown frame", lambda: ba.WindowAggExec([], [], [raw("SUM", col("k"), "n", frame=4)], leaf()), ba.PlanError, "Unknown window frame 4"),
    ("no argument", lambda: ba.WindowAggExec([], [], [W("SUM", None, "n")], leaf()), ba.PlanError, "SUM needs an argument"),
    ("no function", lambda: ba.WindowAggExec([col("k")], [], [], leaf()), ba.PlanError, "needs at least one window expression"),
    ("unknown key column", lambda: ba.WindowAggExec([col("nope")], [], [W("ROW_NUMBER", None, "r")], leaf()), ba.PlanError, "nope"),
    ("unknown argument column", lambda: ba.WindowAggExec([], [], [W("LAG", "nope", "l")], leaf()), ba.PlanError, "nope"),
]


@pytest.mark.parametrize("what, make, error, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_each_refusal_arrives_when_the_plan_is_made(what, make, error, message):
    with pytest.raises(error, match=message):
        make()


def test_the_python_mirror_refuses_names_it_does_not_know():
    for fun in ("NTILE", "PERCENT_RANK", "CUME_DIST", "NTH_VALUE", "sum"):
        with pytest.raises(NotImplementedError):
            E.WindowExpr(fun, col("k"), "x")
    with pytest.raises(NotImplementedError):
        E.WindowExpr("SUM", col("k"), "x", frame="ROWS_3_PRECEDING")
    assert ba.WindowAggExec._FN == dict(ROW_NUMBER=1, RANK=2, DENSE_RANK=3, LAG=4, LEAD=5, FIRST_VALUE=6, LAST_VALUE=7, SUM=8, AVG=9, COUNT=10, MIN=11, MAX=12)
    assert ba.WindowAggExec._FRAME == dict(DEFAULT=0, PARTITION=1, ROWS_TO_CURRENT=2, RANGE_TO_CURRENT=3)
    header = open(os.path.join(ROOT, "include", "ballista_hip.h")).read()
    for name, v in list(ba.WindowAggExec._FN.items()) + [("FRAME_" + k, v) for k, v in ba.WindowAggExec._FRAME.items()]:
        prefix = "BHIP_" if name.startswith("FRAME_") else "BHIP_WIN_"
        assert re.search(rf"\b{prefix}{name} = {v}\b", header), name


# ---- 4. the tile constants -----------------------------------------------------------------------------------------------------------

def test_tile_constants_match_the_header():
    text = open(os.path.join(ROOT, "ballista_amd", "csrc", "window_kernels.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (WINDOW_[A-Z_]+) = (\d+);", text)}
    assert consts["WINDOW_TILE_ROWS"] == ba.plan.WINDOW_TILE_ROWS == K.T
    assert consts["WINDOW_SUMMARY_STEP"] == K.SUMMARY_STEP
    assert consts["WINDOW_BLOCK"] * consts["WINDOW_ROUNDS"] == consts["WINDOW_TILE_ROWS"]
    # S: the smallest row count with more tile summaries than one step of the second level takes
    assert -(-K.S // K.T) == K.SUMMARY_STEP + 1 and -(-(K.S - 1) // K.T) == K.SUMMARY_STEP
    assert K.SIZES[-1] == K.S + 1 and {1, 2, 63, 64, 65, K.T - 1, K.T, K.T + 1, 3 * K.T + 1} <= set(K.SIZES)
