"""CPU tier of WindowAggExec's sliding ROWS frames: no GPU work.

1. the restatement (tests/window_frame_cases.py) against the standard library's sqlite3: all five aggregates and FIRST_VALUE / LAST_VALUE
   over frames on both sides of the current row, on a table SQLite can hold (integers within Int63, sixteenths: every sum is exact
   whatever the order).  The frame follows the ROW order, so SQLite is given the input row number as the last order key;
2. plan-time behaviour over a leaf with no context: schema and nullability (the empty-frame rule), display, the two frames that are
   named frames, with_new_children, every refusal, and the raw C entry point;
3. the constants and the struct of the Python mirror against the headers."""
import ctypes as C
import os
import re
import sqlite3

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col
from oracle.engine import OCol
from tests import window_cases as K, window_frame_cases as FK
from tests.window_frame_cases import F, W, asc
from tests.test_window_cases_cpu import SPECS, leaf, raw, sqlite_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against SQLite ------------------------------------------------------------------------------------------------

SQLITE_FRAMES = [(-1, 0), (0, 0), (0, 1), (-2, 2), (-3, -1), (1, 2), (-70, -65), (-100, 100), (None, 1), (None, -1), (None, 0), (None, None),
                 (-2, None), (1, None), (0, None)]


def bound_sql(offset, unbounded):
    if offset is None:
        return unbounded
    return "CURRENT ROW" if offset == 0 else f"{-offset} PRECEDING" if offset < 0 else f"{offset} FOLLOWING"


def frame_sql(frame):
    return f"ROWS BETWEEN {bound_sql(frame.start, 'UNBOUNDED PRECEDING')} AND {bound_sql(frame.end, 'UNBOUNDED FOLLOWING')}"


def sql_for(w, partition_by, order_by):
    order_sql = [f"{s.expr.name} {'DESC' if s.descending else 'ASC'} NULLS {'FIRST' if s.nulls_first else 'LAST'}" for s in order_by]
    part_sql = ("PARTITION BY " + ", ".join(partition_by) + " ") if partition_by else ""
    fn = {"SUM": "sum", "AVG": "avg", "COUNT": "count", "MIN": "min", "MAX": "max", "FIRST_VALUE": "first_value", "LAST_VALUE": "last_value"}[w.fun]
    return f"{fn}({w.expr.name}) OVER ({part_sql}ORDER BY {', '.join(order_sql + ['rn'])} {frame_sql(w.frame)})"


def sqlite_exprs():
    ws = []
    for k, (a, b) in enumerate(SQLITE_FRAMES):
        for fun in FK.FRAMED:
            ws += [W(fun, "x", f"{fun}_x_{k}", frame=F(a, b)), W(fun, "f", f"{fun}_f_{k}", frame=F(a, b))]
        ws += [W("COUNT", "s", f"count_s_{k}", frame=F(a, b)), W("LAST_VALUE", "s", f"last_s_{k}", frame=F(a, b))]
    return ws


@pytest.mark.parametrize("spec", list(SPECS))
def test_the_restatement_agrees_with_sqlite(spec):
    assert sqlite3.sqlite_version_info >= (3, 30), sqlite3.sqlite_version
    partition_by, order_by = SPECS[spec]
    batch = sqlite_table()
    ws = sqlite_exprs()
    pb = [col(k) for k in partition_by]
    got = FK.restate(K.sorted_input(batch, pb, order_by), pb, order_by, ws)
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE t (p, q, o, x, f, s, rn)")
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?, ?, ?)", list(zip(*[batch[k].to_pylist() for k in ("p", "q", "o", "x", "f", "s", "rn")])))
    want = {}
    for lo in range(0, len(ws), 40):                     # (SQLite limits the columns of one SELECT)
        for r in db.execute("SELECT rn, " + ", ".join(sql_for(w, partition_by, order_by) for w in ws[lo:lo + 40]) + " FROM t"):
            want.setdefault(r[0], []).extend(r[1:])
    assert len(want) == len(batch["rn"])
    rns = got["rn"].to_pylist()
    for k, w in enumerate(ws):
        mine = got[w.name].to_pylist()
        bad = [(rn, mine[i], want[rn][k]) for i, rn in enumerate(rns) if mine[i] != want[rn][k] or type(mine[i]) is not type(want[rn][k])]
        assert not bad, (w.name, sql_for(w, partition_by, order_by), bad[:5])
    # the table exercises what the frames are there for: empty frames (NULL and 0), frames cut by a partition's end
    k = SQLITE_FRAMES.index((-3, -1))
    assert None in got[f"SUM_x_{k}"].to_pylist() and 0 in got[f"COUNT_x_{k}"].to_pylist() and 3 in got[f"COUNT_x_{k}"].to_pylist()
    assert None in got[f"FIRST_VALUE_x_{SQLITE_FRAMES.index((1, 2))}"].to_pylist()


def test_frame_bounds_and_the_ordered_sum_by_hand():
    """p = a a a a b, the values 1 NULL 4 16 64 in that order: small enough to do by hand"""
    batch = {"p": OCol("Utf8", ["a", "a", "a", "a", "b"]), "v": OCol("Float64", [1.0, 0.0, 4.0, 16.0, 64.0], np.array([True, False, True, True, True])),
             "rn": OCol("Int64", np.arange(5, dtype=np.int64))}
    ps, pe, _, _ = FK.bounds(batch, [col("p")], [])
    assert FK.frame_bounds(ps, pe, F(-1, 1)) == ([0, 0, 1, 2, 4], [1, 2, 3, 3, 4])
    assert FK.frame_bounds(ps, pe, F(1, 2)) == ([1, 2, 3, None, None], [2, 3, 3, None, None])
    assert FK.frame_bounds(ps, pe, F(None, -1)) == ([None, 0, 0, 0, None], [None, 0, 1, 2, None])
    assert FK.frame_bounds(ps, pe, F(-2, None)) == ([0, 0, 0, 1, 4], [3, 3, 3, 3, 4])
    assert FK.frame_bounds(ps, pe, F(2**62, 2**62 + 1)) == ([None] * 5, [None] * 5)
    assert FK.frame_bounds(ps, pe, F(-2**62, 0)) == ([0, 0, 0, 0, 4], [0, 1, 2, 3, 4])
    got = FK.restate(batch, [col("p")], [], [W("SUM", "v", "s", frame=F(-1, 1)), W("AVG", "v", "a", frame=F(1, 2)), W("COUNT", "v", "c", frame=F(1, 2)),
                                            W("MIN", "v", "m", frame=F(None, -1)), W("LAST_VALUE", "v", "l", frame=F(-1, 0)),
                                            W("FIRST_VALUE", "v", "f", frame=F(1, 1)), W("ROW_NUMBER", None, "r", frame=F(1, 1))])
    assert got["s"].to_pylist() == [1.0, 5.0, 20.0, 20.0, 64.0] and got["a"].to_pylist() == [4.0, 10.0, 16.0, None, None]
    assert got["c"].to_pylist() == [1, 2, 1, 0, 0] and got["m"].to_pylist() == [None, 1.0, 1.0, 1.0, None]
    assert got["l"].to_pylist() == [1.0, None, 4.0, 16.0, 64.0] and got["f"].to_pylist() == [None, 4.0, 16.0, None, None]
    assert got["r"].to_pylist() == [1, 2, 3, 4, 1]
    # the order of the additions is the row order: 2^53 + 1 + 1 loses both ones, 1 + 1 + 2^53 keeps them
    big = {"v": OCol("Float64", [2.0**53, 1.0, 1.0, 2.0**53]), "rn": OCol("Int64", np.arange(4, dtype=np.int64))}
    got = FK.restate(big, [], [], [W("SUM", "v", "s", frame=F(-2, 0))])
    assert got["s"].to_pylist() == [2.0**53, 2.0**53, 2.0**53, 2.0**53 + 2.0]


# ---- 2. plan time, with no GPU ----------------------------------------------------------------------------------------------------------

def test_schema_nullability_and_display():
    ws = [W("SUM", "i", "sum_i", frame=F(-2, 0)), W("SUM", "f32", "sum_f32", frame=F(-6, 0)), W("AVG", "i", "avg_i", frame=F(-1, 1)),
          W("COUNT", "s", "count_s", frame=F(1, 2)), E.count_star("star", F(-3, None)), W("MIN", "f32", "min_f32", frame=F(0, 4095)),
          W("MAX", "d", "max_d", frame=F(None, 3)), W("FIRST_VALUE", "u", "first_in", frame=F(-1, 1)), W("FIRST_VALUE", "u", "first_after", frame=F(1, 3)),
          W("LAST_VALUE", "d", "last_before", frame=F(None, -1)), W("LAST_VALUE", "kn", "last_kn", frame=F(0, 0)), W("LAST_VALUE", "d", "last_tail", frame=F(-2, None)),
          W("ROW_NUMBER", None, "rn", frame=F(1, 2)), W("LAG", "u", "lag_u", 2, frame=F(-5, 5)), W("SUM", "k", "far", frame=F(-2**63, 2**63 - 1))]
    plan = ba.WindowAggExec([col("k")], [asc("i")], ws, leaf())
    assert plan.schema() == leaf().schema() + [
        ("sum_i", "Int64", True), ("sum_f32", "Float64", True), ("avg_i", "Float64", True), ("count_s", "UInt64", False), ("star", "UInt64", False),
        ("min_f32", "Float32", True), ("max_d", "Date32", True), ("first_in", "Utf8", False), ("first_after", "Utf8", True), ("last_before", "Date32", True),
        ("last_kn", "Int64", True), ("last_tail", "Date32", False), ("rn", "UInt64", False), ("lag_u", "Utf8", True), ("far", "Int64", True)]
    text = plan.display()
    for part in ("SUM(i) ROWS BETWEEN 2 PRECEDING AND CURRENT ROW as sum_i", "AVG(i) ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING as avg_i",
                 "COUNT(s) ROWS BETWEEN 1 FOLLOWING AND 2 FOLLOWING as count_s", "COUNT(UInt8(1)) ROWS BETWEEN 3 PRECEDING AND UNBOUNDED FOLLOWING as star",
                 "MIN(f32) ROWS BETWEEN CURRENT ROW AND 4095 FOLLOWING as min_f32", "MAX(d) ROWS BETWEEN UNBOUNDED PRECEDING AND 3 FOLLOWING as max_d",
                 "FIRST_VALUE(u) ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING as first_in", "LAST_VALUE(d) ROWS BETWEEN UNBOUNDED PRECEDING AND 1 PRECEDING as last_before",
                 "LAST_VALUE(kn) ROWS BETWEEN CURRENT ROW AND CURRENT ROW as last_kn", "ROW_NUMBER() as rn", "LAG(u, 2) as lag_u",
                 "SUM(k) ROWS BETWEEN 9223372036854775808 PRECEDING AND 9223372036854775807 FOLLOWING as far"):
        assert part in text, (part, text)


def test_the_two_frames_that_are_named_frames_display_as_them():
    ws = [W("SUM", "f", "run", frame=F(None, 0)), W("MIN", "f", "all", frame=F(None, None)), W("LAST_VALUE", "u", "last", frame=F(None, 0)),
          W("FIRST_VALUE", "u", "first", frame=F(None, None)), W("AVG", "f", "kept", frame=F(None, 1))]
    plan = ba.WindowAggExec([col("k")], [asc("i")], ws, leaf())
    text = plan.display()
    for part in ("SUM(f) ROWS_TO_CURRENT as run", "MIN(f) PARTITION as all", "LAST_VALUE(u) ROWS_TO_CURRENT as last", "FIRST_VALUE(u) as first",
                 "AVG(f) ROWS BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING as kept"):
        assert part in text, (part, text)
    named = ba.WindowAggExec([col("k")], [asc("i")], [W("SUM", "f", "run", frame="ROWS_TO_CURRENT"), W("MIN", "f", "all", frame="PARTITION"),
                                                      W("LAST_VALUE", "u", "last", frame="ROWS_TO_CURRENT"), W("FIRST_VALUE", "u", "first"),
                                                      W("AVG", "f", "kept", frame=F(None, 1))], leaf())
    assert named.display() == text and named.schema() == plan.schema()
    # the offset of an unbounded side is not read, however large: handed to the C entry point directly
    h = plan_window_frames([("SUM", "f", 0, L.RowsFrameC(1, 0, 2**62, 0)), ("SUM", "f", 0, L.RowsFrameC(1, 1, 2**62, -2**62))])
    assert "SUM(f) ROWS_TO_CURRENT as w0, SUM(f) PARTITION as w1" in h.display()


def plan_window_frames(items, null_array=False):
    """bhip_plan_window_frames over raw structs: items = (function, column, frame number, RowsFrameC or None)"""
    inp = leaf()
    lw = ba.plan._Lowered()
    fns = (L.WindowExprC * len(items))()
    rows = (C.POINTER(L.RowsFrameC) * len(items))()
    for i, (fun, name, frame, r) in enumerate(items):
        fns[i] = L.WindowExprC(ba.WindowAggExec._FN[fun], lw.expr(col(name)), 1, frame, b"w%d" % i)
        if r is not None:
            rows[i] = C.pointer(r)
    h = C.c_void_p()
    L.check(L.lib().bhip_plan_window_frames(inp._h, 0, None, 0, None, len(items), fns, None if null_array else rows, C.byref(h)))
    plan = object.__new__(ba.ExecutionPlan)
    ba.ExecutionPlan.__init__(plan, h, None, [inp])
    return plan


def test_the_raw_entry_point():
    # a rows frame goes with BHIP_FRAME_DEFAULT only
    for frame in (1, 2, 3):
        with pytest.raises(ba.PlanError, match="a rows frame goes with BHIP_FRAME_DEFAULT"):
            plan_window_frames([("SUM", "k", frame, L.RowsFrameC(0, 0, -1, 0))])
    with pytest.raises(ba.PlanError, match="Unknown window frame 4"):
        plan_window_frames([("SUM", "k", 4, L.RowsFrameC(0, 0, -1, 0))])
    # a null entry: fns[i].frame as it is; a null array: bhip_plan_window
    text = plan_window_frames([("SUM", "k", 2, None), ("SUM", "k", 0, L.RowsFrameC(0, 0, -1, 0)), ("SUM", "k", 0, None)]).display()
    assert "SUM(k) ROWS_TO_CURRENT as w0, SUM(k) ROWS BETWEEN 1 PRECEDING AND CURRENT ROW as w1, SUM(k) PARTITION as w2" in text
    assert "SUM(k) ROWS_TO_CURRENT as w0" in plan_window_frames([("SUM", "k", 2, None)], null_array=True).display()
    with pytest.raises(ba.PlanError, match="Unknown window frame 4"):
        plan_window_frames([("SUM", "k", 4, None)], null_array=True)


def test_with_new_children_keeps_the_frames():
    first = ba.WindowAggExec([col("k")], [asc("i")], [W("SUM", "f", "m", frame=F(-6, 0)), W("LAST_VALUE", "u", "l", frame=F(1, 1))], leaf())
    second = ba.WindowAggExec([col("u")], [], [W("MAX", "m", "mm", frame=F(-1, 1)), W("COUNT", "l", "c", frame=F(2, None))], first)
    assert second.schema()[-4:] == [("m", "Float64", True), ("l", "Utf8", True), ("mm", "Float64", True), ("c", "UInt64", False)]
    again = second.with_new_children([first])
    assert again.schema() == second.schema() and again.display() == second.display()
    assert "MAX(m) ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING as mm" in again.display() and "SUM(f) ROWS BETWEEN 6 PRECEDING AND CURRENT ROW as m" in again.display()
    assert [w.frame for w in again.window_exprs] == [F(-1, 1), F(2, None)]


CAP = ba.plan.WINDOW_SLIDE_MAX_ROWS


def one(fun, name, frame):
    return lambda: ba.WindowAggExec([], [], [W(fun, name, "w", frame=frame)], leaf())


REFUSALS = [
    ("start after end", one("SUM", "k", F(1, 0)), ba.PlanError, "SUM ROWS BETWEEN 1 FOLLOWING AND CURRENT ROW: frame start lies after its end"),
    ("start after end, far", one("COUNT", "k", F(2**63 - 1, -2**63)), ba.PlanError, "frame start lies after its end"),
    ("start after end on a function without a frame", one("LAG", "k", F(3, 2)), ba.PlanError, "frame start lies after its end"),
    ("float SUM wider than the cap", one("SUM", "f", F(-CAP, 0)), ba.NotImplementedOnGpu,
     rf"SUM\(Float64\) over ROWS BETWEEN {CAP} PRECEDING AND CURRENT ROW: a frame wider than {CAP} rows"),
    ("Float32 SUM wider than the cap", one("SUM", "f32", F(-1, CAP - 1)), ba.NotImplementedOnGpu, rf"SUM\(Float32\) over ROWS BETWEEN 1 PRECEDING AND {CAP - 1} FOLLOWING"),
    ("AVG of integers wider than the cap", one("AVG", "i", F(-2**63, 2**63 - 1)), ba.NotImplementedOnGpu, rf"AVG\(Int32\) over ROWS BETWEEN .* a frame wider than {CAP} rows"),
    ("MIN wider than the cap", one("MIN", "k", F(0, CAP)), ba.NotImplementedOnGpu, rf"MIN\(Int64\) over ROWS BETWEEN CURRENT ROW AND {CAP} FOLLOWING: a frame wider"),
    ("MAX wider than the cap", one("MAX", "d", F(-5000, 0)), ba.NotImplementedOnGpu, r"MAX\(Date32\) over ROWS BETWEEN 5000 PRECEDING AND CURRENT ROW: a frame wider"),
    ("float SUM to UNBOUNDED FOLLOWING", one("SUM", "f", F(-2, None)), ba.NotImplementedOnGpu,
     r"SUM\(Float64\) over ROWS BETWEEN 2 PRECEDING AND UNBOUNDED FOLLOWING: a frame from an offset to UNBOUNDED FOLLOWING"),
    ("AVG to UNBOUNDED FOLLOWING", one("AVG", "k", F(0, None)), ba.NotImplementedOnGpu, r"AVG\(Int64\) over ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING"),
    ("MIN to UNBOUNDED FOLLOWING", one("MIN", "i", F(1, None)), ba.NotImplementedOnGpu, r"MIN\(Int32\) over ROWS BETWEEN 1 FOLLOWING AND UNBOUNDED FOLLOWING"),
    ("MAX to UNBOUNDED FOLLOWING", one("MAX", "f32", F(-1, None)), ba.NotImplementedOnGpu, r"MAX\(Float32\) over ROWS BETWEEN 1 PRECEDING AND UNBOUNDED FOLLOWING"),
    ("MIN over Utf8 keeps its own refusal", one("MIN", "s", F(-1, 0)), ba.NotImplementedOnGpu, "MIN over Utf8 is not supported as a window function"),
    ("SUM over Utf8 keeps its own refusal", one("SUM", "s", F(-1, 0)), ba.PlanError, "SUM does not support Utf8"),
    ("unknown frame through bhip_plan_window", lambda: ba.WindowAggExec([], [], [raw("SUM", col("k"), "n", frame=4)], leaf()), ba.PlanError, "Unknown window frame 4"),
    ("unknown function", lambda: ba.WindowAggExec([], [], [raw(13, col("k"), "n", frame=F(-1, 0))], leaf()), ba.PlanError, "Unknown window function 13"),
]


@pytest.mark.parametrize("what, make, error, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_each_refusal_arrives_when_the_plan_is_made(what, make, error, message):
    with pytest.raises(error, match=message):
        make()


def test_what_is_at_the_limits_is_taken():
    """exactly the cap; any width for COUNT, the integer SUM and the gathers; any offsets with an unbounded start"""
    ws = [W("SUM", "f", "a", frame=F(-(CAP - 1), 0)), W("AVG", "k", "b", frame=F(-5000, -5000 + CAP - 1)), W("MIN", "f32", "c", frame=F(2**62, 2**62 + 1)),
          W("SUM", "k", "d", frame=F(-2**62, 0)), W("COUNT", "f", "e", frame=F(-2**63, 2**63 - 1)), W("SUM", "u8", "f_", frame=F(-2, None)),
          W("FIRST_VALUE", "f", "g", frame=F(-2, None)), W("LAST_VALUE", "s", "h", frame=F(-10**6, 10**6)), W("MAX", "f", "i_", frame=F(None, 2**62)),
          W("SUM", "f", "j", frame=F(None, -2**62))]
    plan = ba.WindowAggExec([col("k")], [], ws, leaf())
    assert [f[0] for f in plan.schema()][-len(ws):] == [w.name for w in ws]
    assert f"SUM(f) ROWS BETWEEN {CAP - 1} PRECEDING AND CURRENT ROW as a" in plan.display()


def test_the_python_mirror():
    for bad in ("1", 1.0, True, 2**63, -2**63 - 1):
        with pytest.raises(TypeError):
            F(bad, 0)
        with pytest.raises(TypeError):
            F(None, bad)
    assert F(-2, 0) == F(-2, 0) and F(-2, 0) != F(-2, None) and hash(F(None, 3)) == hash(F(None, 3))
    assert E.WindowExpr("SUM", col("k"), "x", frame=F(-2**63, 2**63 - 1)).frame == F(-2**63, 2**63 - 1)
    for frame in ("ROWS_3_PRECEDING", "ROWS", None, (-3, 0)):
        with pytest.raises(NotImplementedError):
            E.WindowExpr("SUM", col("k"), "x", frame=frame)
    assert E.count_star("c", F(-1, 0)).frame == F(-1, 0)


# ---- 3. the mirror against the headers -----------------------------------------------------------------------------------------------------

def test_the_cap_and_the_struct_match_the_headers():
    text = open(os.path.join(ROOT, "ballista_amd", "csrc", "window_kernels.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (WINDOW_[A-Z_]+) = (\d+);", text)}
    assert consts["WINDOW_SLIDE_MAX_ROWS"] == ba.plan.WINDOW_SLIDE_MAX_ROWS == 4096
    # a tile and the widest frame's neighbourhood, 8 bytes of value and one of flags per row, under 64 KiB of LDS
    assert (consts["WINDOW_TILE_ROWS"] + consts["WINDOW_SLIDE_MAX_ROWS"] - 1) * 9 <= 64 * 1024
    header = open(os.path.join(ROOT, "include", "ballista_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} bhip_rows_frame;", header)
    assert m, "bhip_rows_frame"
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    fields = [(name.strip(), ctype[decl.split()[0]]) for decl in m.group(1).split(";") if decl.strip()
              for name in decl.strip().split(None, 1)[1].split(",")]
    assert fields == L.RowsFrameC._fields_ and C.sizeof(L.RowsFrameC) == 24
    assert re.search(r"bhip_status bhip_plan_window_frames\([^;]*const bhip_window_expr\* fns,\s*const bhip_rows_frame\* const\* rows_frames, bhip_plan\*\* out\);", header)
    assert "bhip_plan_window_frames" in L.SYMBOLS and L.SYMBOLS["bhip_plan_window_frames"][1][:-2] == L.SYMBOLS["bhip_plan_window"][1][:-1]
