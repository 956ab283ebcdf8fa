"""CPU tier of WindowAggExec's RANGE and GROUPS frames: no GPU work.

1. the restatement (tests/window_value_frame_cases.py) against the standard library's sqlite3 (RANGE / GROUPS with offsets since 3.28):
   all five aggregates over twenty-one frames in both units, keys ascending and descending, NULLS FIRST and LAST, integer and float
   keys, two order keys and none, on a table SQLite can hold (integers within Int63, sixteenths: every sum is exact, and compared
   within 1e-6 since SQLite's order of additions is its own).  The row number cannot be an order key here (it would split the peer
   groups), so FIRST_VALUE / LAST_VALUE are pinned through the frame's row count: lo .. hi is contiguous and its length is SQLite's.
   The one corner where the contract and SQLite part is pinned as such (where_sqlite_keeps_the_nulls);
2. what SQLite cannot express, pinned by hand: the two zeros under OFFSET 0 against CURRENT ROW, NaN keys of both signs, infinite keys,
   Int64 keys at both extremes with offsets of +-(2^63 - 1), UInt64 keys above 2^63;
3. plan time over a leaf with no context: every refusal, the canonical forms and display(), with_new_children, nullability, the raw
   C entry point;
4. the Python mirror against the header."""
import ctypes as C
import math
import os
import re
import sqlite3

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col
from oracle.engine import OCol
from tests import window_cases as K, window_value_frame_cases as VK
from tests.window_value_frame_cases import CUR, F, G, R, W, asc
from tests.test_window_cases_cpu import leaf, raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = ba.plan.WINDOW_SLIDE_MAX_ROWS


# ---- 1. the restatement against SQLite ------------------------------------------------------------------------------------------------

def sqlite_table(n=300, seed=11):
    """o: ties and gaps, NULLs; k = o / 2 as a float key; x, f: the arguments"""
    rng = np.random.default_rng(seed)
    o = rng.choice(np.array([-9, -8, -5, -4, -4, 0, 1, 2, 7, 8, 13, 20], np.int64), n)
    o_valid = rng.random(n) > 0.12
    return {"p": OCol("Int64", rng.integers(0, 5, n), rng.random(n) > 0.1),
            "o": OCol("Int64", o, o_valid),
            "k": OCol("Float64", o / 2.0, o_valid.copy()),
            "q": OCol("Int64", rng.integers(0, 3, n), rng.random(n) > 0.1),
            "x": OCol("Int64", rng.integers(-10**9, 10**9, n), rng.random(n) > 0.2),
            "f": OCol("Float64", rng.integers(-2000, 2000, n) / 16.0, rng.random(n) > 0.2),
            "rn": OCol("Int64", np.arange(n, dtype=np.int64))}


# one order key: every frame
ONE_KEY_FRAMES = [R(-2, CUR), R(-3, 3), R(CUR, 4), R(-6, -2), R(1, 5), R(None, -1), R(None, 2), R(-1, None), R(2, None), R(CUR, CUR), R(0, 0),
                  R(CUR, None), G(-1, 1), G(-2, CUR), G(1, 2), G(-3, -1), G(None, 1), G(-1, None), G(CUR, CUR), G(None, -2), G(2, None)]
# two order keys (or none): CURRENT ROW and UNBOUNDED sides under RANGE, anything under GROUPS
ANY_KEYS_FRAMES = [R(CUR, CUR), R(CUR, None), R(None, CUR), G(-1, 1), G(CUR, 2), G(-2, -1), G(None, CUR), G(1, None)]

SPECS = {
    "asc_nulls_first": (["p"], [asc("o")], ONE_KEY_FRAMES),
    "desc_nulls_last": (["p"], [asc("o", True, False)], ONE_KEY_FRAMES),
    "asc_nulls_last": (["p"], [asc("o", False, False)], ONE_KEY_FRAMES),
    "desc_nulls_first_no_partition": ([], [asc("o", True, True)], ONE_KEY_FRAMES),
    "float_key_asc": (["p"], [asc("k")], [R(-1.0, CUR), R(-1.5, 1.5), R(0.5, 2.5), R(-3.0, -1.0), R(None, 0.5), R(-0.5, None), R(0.0, 0.0)]),
    "float_key_desc": (["p"], [asc("k", True, False)], [R(-1.0, CUR), R(-1.5, 1.5), R(0.5, 2.5), R(-3.0, -1.0), R(None, 0.5), R(-0.5, None)]),
    "two_order_keys": (["p"], [asc("o", False, False), asc("q", True, True)], ANY_KEYS_FRAMES),
    "no_order": (["p"], [], ANY_KEYS_FRAMES),
}


def side_sql(side, is_start):
    if side is None:
        return "UNBOUNDED PRECEDING" if is_start else "UNBOUNDED FOLLOWING"
    if side is CUR:
        return "CURRENT ROW"
    return f"{-side} PRECEDING" if side < 0 or (side == 0 and is_start) else f"{side} FOLLOWING"


def frame_sql(frame):
    return f"{'RANGE' if isinstance(frame, R) else 'GROUPS'} BETWEEN {side_sql(frame.start, True)} AND {side_sql(frame.end, False)}"


def sql_for(w, partition_by, order_by):
    """the five aggregates only: the row number cannot be an order key here (it would split the peer groups), and without it SQLite's
    order inside a peer group is its own, so FIRST_VALUE / LAST_VALUE have no SQLite counterpart — the caller pins them through the
    frame's row count instead"""
    order_sql = [f"{s.expr.name} {'DESC' if s.descending else 'ASC'} NULLS {'FIRST' if s.nulls_first else 'LAST'}" for s in order_by]
    part_sql = ("PARTITION BY " + ", ".join(partition_by) + " ") if partition_by else ""
    fn = {"SUM": "sum", "AVG": "avg", "COUNT": "count", "MIN": "min", "MAX": "max"}[w.fun]
    return f"{fn}({w.expr.name}) OVER ({part_sql}{'ORDER BY ' + ', '.join(order_sql) + ' ' if order_sql else ''}{frame_sql(w.frame)})"


def sqlite_exprs(frames):
    ws = []
    for k, fr in enumerate(frames):
        for fun in K.AGGREGATES:
            ws += [W(fun, "x", f"{fun}_x_{k}", frame=fr), W(fun, "f", f"{fun}_f_{k}", frame=fr)]
        ws += [W("COUNT", "rn", f"rows_{k}", frame=fr)]
    return ws


def where_sqlite_keeps_the_nulls(batch, partition_by, order_by, frame, my_rows, sqlite_rows):
    """The ONE place the contract and SQLite part, pinned here instead of compared.  RANGE with an OFFSET on one side and UNBOUNDED on the
    other, a row whose key is a number, and no number that qualifies for the OFFSET side: by the contract that side has no row and the
    frame is empty; SQLite ranks NULL below (NULLS FIRST) or above (NULLS LAST) every number, so its frame is then the NULL rows at
    the partition's unbounded end.  -> the rows where that happens, after checking that SQLite's frame there is exactly those NULLs
    (and that nothing else is let off: everywhere else the caller compares)."""
    if not isinstance(frame, R) or not ((frame.start is None and VK.is_offset(frame.end)) or (VK.is_offset(frame.start) and frame.end is None)):
        return set()
    ps, pe, _, _ = VK.bounds(batch, partition_by, order_by)
    valid = batch[order_by[0].expr.name].is_valid()
    nulls_at_the_open_end = order_by[0].nulls_first == (frame.start is None)
    rows = set()
    for i in range(len(my_rows)):
        if my_rows[i] == 0 and valid[i] and nulls_at_the_open_end:
            n_null = int((~valid[ps[i]:pe[i] + 1]).sum())
            assert sqlite_rows[i] == n_null, (frame, i, sqlite_rows[i], n_null)
            if n_null:
                rows.add(i)
    return rows


def close(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        return math.isclose(a, b, rel_tol=1e-6, abs_tol=1e-9)
    return a == b and type(a) is type(b)


@pytest.mark.parametrize("spec", list(SPECS))
def test_the_restatement_agrees_with_sqlite(spec):
    assert sqlite3.sqlite_version_info >= (3, 30), sqlite3.sqlite_version
    partition_by, order_by, frames = SPECS[spec]
    batch = sqlite_table()
    ws = sqlite_exprs(frames)
    pb = [col(k) for k in partition_by]
    in_order = K.sorted_input(batch, pb, order_by)
    got = VK.restate(in_order, pb, order_by, ws)
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE t (p, o, k, q, x, f, rn)")
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?, ?, ?)", list(zip(*[batch[k].to_pylist() for k in ("p", "o", "k", "q", "x", "f", "rn")])))
    want = {}
    for lo in range(0, len(ws), 40):                     # (SQLite limits the columns of one SELECT)
        for r in db.execute("SELECT rn, " + ", ".join(sql_for(w, partition_by, order_by) for w in ws[lo:lo + 40]) + " FROM t"):
            want.setdefault(r[0], []).extend(r[1:])
    assert len(want) == len(batch["rn"])
    rns = got["rn"].to_pylist()
    per_frame = len(ws) // len(frames)
    apart = {k: where_sqlite_keeps_the_nulls(in_order, pb, order_by, fr, got[f"rows_{k}"].to_pylist(),
                                             [want[rn][(k + 1) * per_frame - 1] for rn in rns]) for k, fr in enumerate(frames)}
    for k, w in enumerate(ws):
        mine = got[w.name].to_pylist()
        bad = [(rn, mine[i], want[rn][k]) for i, rn in enumerate(rns) if i not in apart[k // per_frame] and not close(mine[i], want[rn][k])]
        assert not bad, (w.name, sql_for(w, partition_by, order_by), bad[:5])
    # FIRST_VALUE / LAST_VALUE are rows lo / hi of the same frames: the frame's rows were just counted against SQLite, and lo .. hi is
    # contiguous, so the two gathers are pinned by hi - lo + 1 == the count, lo at a peer group's first row or the partition's, and so on
    for k, fr in enumerate(frames):
        lo, hi = VK.frame_bounds(in_order, pb, order_by, fr) if isinstance(VK.canonical(fr), (R, G)) else (None, None)
        if lo is None:
            continue
        rows = got[f"rows_{k}"].to_pylist()
        assert [0 if a is None else b - a + 1 for a, b in zip(lo, hi)] == rows, fr
        firsts = VK.restate(in_order, pb, order_by, [W("FIRST_VALUE", "rn", "a", frame=fr), W("LAST_VALUE", "rn", "b", frame=fr)])
        assert firsts["a"].to_pylist() == [None if a is None else rns[a] for a in lo] and firsts["b"].to_pylist() == [None if b is None else rns[b] for b in hi]
    # the table exercises what the frames are there for
    if spec == "asc_nulls_first":
        k = frames.index(R(-6, -2))
        assert None in got[f"SUM_x_{k}"].to_pylist() and 0 in got[f"rows_{k}"].to_pylist() and max(got[f"rows_{k}"].to_pylist()) > 3
        assert 0 in got[f"rows_{frames.index(G(1, 2))}"].to_pylist() and 0 in got[f"rows_{frames.index(R(1, 5))}"].to_pylist()


def test_frames_by_hand():
    """one partition, keys 1 1 3 4 4 4 8 NULL NULL (NULLS LAST): small enough to do by hand"""
    o = OCol("Int64", [1, 1, 3, 4, 4, 4, 8, 0, 0], np.array([True] * 7 + [False] * 2))
    batch = {"o": o, "v": OCol("Float64", [1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0]), "rn": OCol("Int64", np.arange(9, dtype=np.int64))}
    order = [asc("o", False, False)]
    fb = lambda fr: VK.frame_bounds(batch, [], order, fr)
    assert fb(R(-1, CUR)) == ([0, 0, 2, 2, 2, 2, 6, 7, 7], [1, 1, 2, 5, 5, 5, 6, 8, 8])
    assert fb(R(-3, -1)) == ([None, None, 0, 0, 0, 0, None, 7, 7], [None, None, 1, 2, 2, 2, None, 8, 8])       # a NULL key: its peers
    assert fb(R(1, 4)) == ([2, 2, 3, 6, 6, 6, None, 7, 7], [5, 5, 5, 6, 6, 6, None, 8, 8])
    assert fb(R(2, None)) == ([2, 2, 6, 6, 6, 6, None, 7, 7], [8, 8, 8, 8, 8, 8, None, 8, 8])       # no number qualifies: empty, NULLs or not
    assert fb(R(None, -4)) == ([None, None, None, None, None, None, 0, 0, 0], [None, None, None, None, None, None, 5, 8, 8])
    assert fb(G(-1, 1)) == ([0, 0, 0, 2, 2, 2, 3, 6, 6], [2, 2, 5, 6, 6, 6, 8, 8, 8])
    assert fb(G(2, 3)) == ([3, 3, 6, 7, 7, 7, None, None, None], [6, 6, 8, 8, 8, 8, None, None, None])
    assert fb(G(-9, -2)) == ([None, None, None, 0, 0, 0, 0, 0, 0], [None, None, None, 1, 1, 1, 2, 5, 5])
    assert fb(G(CUR, None)) == ([0, 0, 2, 3, 3, 3, 6, 7, 7], [8] * 9)
    desc = {k: c.take(np.arange(9)[::-1]) for k, c in batch.items()}      # NULL NULL 8 4 4 4 3 1 1, descending NULLS FIRST
    assert VK.frame_bounds(desc, [], [asc("o", True, True)], R(-1, CUR)) == ([0, 0, 2, 3, 3, 3, 3, 7, 7], [1, 1, 2, 5, 5, 5, 6, 8, 8])
    assert VK.frame_bounds(desc, [], [asc("o", True, True)], R(1, 3)) == ([0, 0, None, 6, 6, 6, 7, None, None], [1, 1, None, 8, 8, 8, 8, None, None])
    got = VK.restate(batch, [], order, [W("SUM", "v", "s", frame=R(-1, CUR)), W("COUNT", "v", "c", frame=R(1, 4)), W("FIRST_VALUE", "v", "f", frame=G(2, 3)),
                                        W("LAST_VALUE", "v", "l", frame=R(-3, -1)), W("AVG", "v", "a", frame=G(-1, 1)), W("MAX", "v", "m", frame=R(None, -4)),
                                        W("RANK", None, "r", frame=R(1, 4))])
    assert got["s"].to_pylist() == [3.0, 3.0, 4.0, 60.0, 60.0, 60.0, 64.0, 384.0, 384.0] and got["c"].to_pylist() == [4, 4, 3, 1, 1, 1, 0, 2, 2]
    assert got["f"].to_pylist() == [8.0, 8.0, 64.0, 128.0, 128.0, 128.0, None, None, None] and got["l"].to_pylist() == [None, None, 2.0, 4.0, 4.0, 4.0, None, 256.0, 256.0]
    assert got["a"].to_pylist()[:3] == [7 / 3, 7 / 3, 63 / 6] and got["m"].to_pylist() == [None] * 6 + [32.0, 256.0, 256.0]
    assert got["r"].to_pylist() == [1, 1, 3, 4, 4, 4, 7, 8, 8]
    # the order of the additions is the row order from +0.0
    big = {"o": OCol("Int64", [0, 0, 0, 5]), "v": OCol("Float64", [2.0**53, 1.0, 1.0, -0.0]), "rn": OCol("Int64", np.arange(4, dtype=np.int64))}
    got = VK.restate(big, [], [asc("o")], [W("SUM", "v", "s", frame=R(CUR, CUR)), W("SUM", "v", "g", frame=G(0, 0))])
    assert got["s"].to_pylist()[:3] == [2.0**53] * 3 and not math.copysign(1.0, got["s"].to_pylist()[3]) < 0 and got["g"].to_pylist() == got["s"].to_pylist()


# ---- 2. what SQLite cannot express ------------------------------------------------------------------------------------------------------

def f64(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


NEG_NAN, POS_NAN = f64(0xFFF8000000000000), f64(0x7FF8000000000000)


def test_the_two_zeros_under_offset_zero_and_current_row():
    """-0.0 and +0.0 are different peers (by bits) but equal numbers: OFFSET 0 takes both, CURRENT ROW one"""
    batch = {"k": OCol("Float64", [-1.0, -0.0, -0.0, 0.0, 1.0]), "rn": OCol("Int64", np.arange(5, dtype=np.int64))}
    order = [asc("k")]
    assert VK.frame_bounds(batch, [], order, R(CUR, CUR)) == ([0, 1, 1, 3, 4], [0, 2, 2, 3, 4])
    assert VK.frame_bounds(batch, [], order, R(0.0, 0.0)) == ([0, 1, 1, 1, 4], [0, 3, 3, 3, 4])
    assert VK.frame_bounds(batch, [], order, R(-0.0, CUR)) == ([0, 1, 1, 1, 4], [0, 2, 2, 3, 4])
    assert VK.frame_bounds(batch, [], order, G(CUR, CUR)) == ([0, 1, 1, 3, 4], [0, 2, 2, 3, 4])


def test_nan_and_infinite_keys():
    """ascending: -NaN, -inf, numbers, +inf, +NaN, then the NULLs.  A NaN never qualifies; a row whose key is one takes its peers"""
    inf = math.inf
    k = OCol("Float64", [NEG_NAN, -inf, -inf, -5.0, 2.0, 3.0, inf, POS_NAN, POS_NAN, 0.0], np.array([True] * 9 + [False]))
    batch = {"k": k, "rn": OCol("Int64", np.arange(10, dtype=np.int64))}
    order = [asc("k", False, False)]
    fb = lambda fr: VK.frame_bounds(batch, [], order, fr)
    assert fb(R(-1.0, 1.0)) == ([0, 1, 1, 3, 4, 4, 6, 7, 7, 9], [0, 2, 2, 3, 5, 5, 6, 8, 8, 9])       # inf - 1 = inf, -inf + 1 = -inf
    assert fb(R(None, 1.0)) == ([0] * 10, [0, 2, 2, 3, 5, 5, 6, 8, 8, 9])
    assert fb(R(1.0, None)) == ([0, 1, 1, 4, 5, 6, 6, 7, 7, 9], [9] * 10)       # -inf + 1 = -inf and inf + 1 = inf: the row itself qualifies
    assert fb(R(-1e308, 1e308)) == ([0, 1, 1, 3, 3, 3, 6, 7, 7, 9], [0, 2, 2, 5, 5, 5, 6, 8, 8, 9])   # a finite t keeps the infinities out


def test_int64_extremes_do_not_wrap():
    lo64, hi64 = -2**63, 2**63 - 1
    batch = {"k": OCol("Int64", [lo64, lo64 + 1, -1, 0, hi64 - 1, hi64]), "rn": OCol("Int64", np.arange(6, dtype=np.int64))}
    order = [asc("k")]
    fb = lambda fr: VK.frame_bounds(batch, [], order, fr)
    assert fb(R(-hi64, hi64)) == ([0, 0, 0, 1, 2, 3], [2, 3, 4, 5, 5, 5])
    assert fb(R(hi64, hi64)) == ([2, 3, 4, 5, None, None], [2, 3, 4, 5, None, None])          # lo64 + hi64 = -1, lo64 + 1 + hi64 = 0, ...
    assert fb(R(1, hi64)) == ([1, 2, 3, 4, 5, None], [2, 3, 4, 5, 5, None])
    assert fb(R(-hi64, -1)) == ([None, 0, 0, 1, 2, 3], [None, 0, 1, 2, 3, 4])
    assert fb(R(lo64, lo64)) == ([None, None, None, 0, None, 2], [None, None, None, 0, None, 2])   # 0 + lo64 = lo64, hi64 + lo64 = -1
    assert fb(R(-2**62, 2**62)) == ([0, 0, 2, 2, 4, 4], [1, 1, 3, 3, 5, 5])
    down = {k: c.take(np.arange(6)[::-1]) for k, c in batch.items()}
    assert VK.frame_bounds(down, [], [asc("k", True)], R(-hi64, hi64)) == ([0, 0, 0, 1, 2, 3], [2, 3, 4, 5, 5, 5])


def test_uint64_keys_above_2_63():
    top = 2**64 - 1
    batch = {"k": OCol("UInt64", np.array([0, 5, 2**63 - 1, 2**63, 2**63 + 7, top], np.uint64)), "rn": OCol("Int64", np.arange(6, dtype=np.int64))}
    fb = lambda fr: VK.frame_bounds(batch, [], [asc("k")], fr)
    assert fb(R(-7, 1)) == ([0, 0, 2, 2, 3, 5], [0, 1, 3, 3, 4, 5])
    assert fb(R(-(2**63 - 1), 2**63 - 1)) == ([0, 0, 0, 1, 2, 3], [2, 3, 4, 5, 5, 5])
    assert fb(R(2**63 - 1, None)) == ([2, 4, 5, 5, None, None], [5, 5, 5, 5, None, None])


# ---- 3. plan time, with no GPU ----------------------------------------------------------------------------------------------------------

def one(fun, name, frame, order=("k",), partition=()):
    return lambda: ba.WindowAggExec([col(p) for p in partition], [asc(o) for o in order], [W(fun, name, "w", frame=frame)], leaf())


def spec_c(units, start, end):
    side = lambda s: L.FrameBoundC(*s)
    return L.FrameSpecC(units, 0, side(start), side(end))


def plan_window_specs(items, null_array=False, order=("k",)):
    """bhip_plan_window_frame_specs over raw structs: items = (function, column, frame number, FrameSpecC or None)"""
    inp = leaf()
    lw = ba.plan._Lowered()
    fns = (L.WindowExprC * len(items))()
    specs = (C.POINTER(L.FrameSpecC) * len(items))()
    for i, (fun, name, frame, s) in enumerate(items):
        fns[i] = L.WindowExprC(ba.WindowAggExec._FN[fun], lw.expr(col(name)), 1, frame, b"w%d" % i)
        if s is not None:
            specs[i] = C.pointer(s)
    order_c = (L.SortExprC * max(1, len(order)))()
    for i, o in enumerate(order):
        order_c[i] = L.SortExprC(lw.expr(col(o)), 0, 1)
    h = C.c_void_p()
    L.check(L.lib().bhip_plan_window_frame_specs(inp._h, 0, None, len(order), order_c, len(items), fns, None if null_array else specs, C.byref(h)))
    plan = object.__new__(ba.ExecutionPlan)
    ba.ExecutionPlan.__init__(plan, h, None, [inp])
    return plan


UNB, CURRENT, OFF = (0, 0, 0, 0.0), (1, 0, 0, 0.0), 2

REFUSALS = [
    ("start after end", one("SUM", "k", R(1, 0)), ba.PlanError, "SUM RANGE BETWEEN 1 FOLLOWING AND 0 FOLLOWING: frame start lies after its end"),
    ("start after CURRENT ROW", one("COUNT", "k", R(2, CUR)), ba.PlanError, "COUNT RANGE BETWEEN 2 FOLLOWING AND CURRENT ROW: frame start lies after its end"),
    ("CURRENT ROW after end", one("SUM", "k", G(CUR, -1)), ba.PlanError, "SUM GROUPS BETWEEN CURRENT ROW AND 1 PRECEDING: frame start lies after its end"),
    ("float start after end", one("SUM", "k", R(0.5, 0.25), order=("f",)), ba.PlanError, "RANGE BETWEEN 0.5 FOLLOWING AND 0.25 FOLLOWING: frame start lies after its end"),
    ("start after end on a function without a frame", one("LAG", "k", G(3, 2)), ba.PlanError, "frame start lies after its end"),
    ("no order key", one("SUM", "k", R(-1, 0), order=()), ba.PlanError, "a RANGE frame with an offset needs exactly one order key, got 0"),
    ("two order keys", one("SUM", "k", R(-1, CUR), order=("k", "i")), ba.PlanError, "a RANGE frame with an offset needs exactly one order key, got 2"),
    ("two order keys on a function without a frame", one("RANK", None, R(None, 1), order=("k", "i")), ba.PlanError, "needs exactly one order key, got 2"),
    ("a Utf8 key", one("SUM", "k", R(-1, 0), order=("s",)), ba.PlanError, "needs an integer, float, date or timestamp order key, not Utf8"),
    ("a Boolean key", one("COUNT", "k", R(None, 1), order=("b",)), ba.PlanError, "needs an integer, float, date or timestamp order key, not Boolean"),
    ("a float offset for an integer key", one("SUM", "k", R(-0.5, CUR)), ba.PlanError, "the Int64 order key takes Int64 offsets, got a Float64"),
    ("a float offset for a date key", one("SUM", "k", R(CUR, 1.0), order=("d",)), ba.PlanError, "the Date32 order key takes Int64 offsets, got a Float64"),
    ("an integer offset no double holds", one("SUM", "k", R(-(2**53 + 1), CUR), order=("f",)), ba.PlanError,
     "the offset -9007199254740993 over the Float64 order key is not exactly a Float64"),
    ("2^63 - 1 over a float key", one("SUM", "k", R(CUR, 2**63 - 1), order=("f32",)), ba.PlanError, "over the Float32 order key is not exactly a Float64"),
    ("float SUM to UNBOUNDED FOLLOWING", one("SUM", "f", R(-2, None)), ba.NotImplementedOnGpu,
     r"SUM\(Float64\) over RANGE BETWEEN 2 PRECEDING AND UNBOUNDED FOLLOWING: a frame from an offset to UNBOUNDED FOLLOWING is supported for COUNT, integer SUM"),
    ("AVG from CURRENT ROW to UNBOUNDED FOLLOWING", one("AVG", "k", R(CUR, None)), ba.NotImplementedOnGpu,
     r"AVG\(Int64\) over RANGE BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING: a frame from an offset to UNBOUNDED FOLLOWING"),
    ("MIN to UNBOUNDED FOLLOWING under GROUPS", one("MIN", "i", G(1, None)), ba.NotImplementedOnGpu, r"MIN\(Int32\) over GROUPS BETWEEN 1 FOLLOWING AND UNBOUNDED FOLLOWING"),
    ("MAX from CURRENT ROW under GROUPS", one("MAX", "f32", G(CUR, None)), ba.NotImplementedOnGpu, r"MAX\(Float32\) over GROUPS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING"),
    ("MIN over Utf8 keeps its own refusal", one("MIN", "s", G(-1, 0)), ba.NotImplementedOnGpu, "MIN over Utf8 is not supported as a window function"),
    ("unknown units", lambda: plan_window_specs([("SUM", "k", 0, spec_c(3, UNB, CURRENT))]), ba.PlanError, "SUM: unknown frame units 3"),
    ("negative units", lambda: plan_window_specs([("SUM", "k", 0, spec_c(-1, UNB, CURRENT))]), ba.PlanError, "unknown frame units -1"),
    ("unknown side kind", lambda: plan_window_specs([("SUM", "k", 0, spec_c(1, (3, 0, 0, 0.0), CURRENT))]), ba.PlanError, "SUM: unknown frame bound kind 3"),
    ("unknown side kind on a function without a frame", lambda: plan_window_specs([("LAG", "k", 0, spec_c(2, UNB, (-1, 0, 0, 0.0)))]), ba.PlanError,
     "LAG: unknown frame bound kind -1"),
    ("a NaN offset", lambda: plan_window_specs([("SUM", "k", 0, spec_c(1, (OFF, 1, 0, math.nan), CURRENT))], order=("f",)), ba.PlanError,
     "a frame offset must be a finite number, got NaN"),
    ("an infinite offset", lambda: plan_window_specs([("COUNT", "k", 0, spec_c(1, CURRENT, (OFF, 1, 0, math.inf)))], order=("f",)), ba.PlanError,
     "a frame offset must be a finite number, got an infinity"),
    ("a float offset under GROUPS", lambda: plan_window_specs([("SUM", "k", 0, spec_c(2, (OFF, 1, 0, -1.0), CURRENT))]), ba.PlanError,
     "a GROUPS frame takes Int64 offsets, got a Float64"),
]


@pytest.mark.parametrize("what, make, error, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_each_refusal_arrives_when_the_plan_is_made(what, make, error, message):
    with pytest.raises(error, match=message):
        make()


def test_schema_nullability_and_display():
    ws = [W("SUM", "f", "m", frame=R(-7, CUR)), W("AVG", "i", "a", frame=G(-1, 1)), W("COUNT", "s", "c", frame=R(1, None)), E.count_star("star", G(-3, None)),
          W("MIN", "f32", "mn", frame=R(0, 0)), W("MAX", "d", "mx", frame=R(None, 3)), W("FIRST_VALUE", "u", "first_in", frame=R(-1, 1)),
          W("FIRST_VALUE", "u", "first_after", frame=R(1, 3)), W("FIRST_VALUE", "u", "first_groups", frame=G(2, None)),
          W("LAST_VALUE", "d", "last_before", frame=G(None, -1)), W("LAST_VALUE", "kn", "last_kn", frame=R(CUR, CUR)), W("LAST_VALUE", "d", "last_tail", frame=R(-2, None)),
          W("LAST_VALUE", "u", "last_zero", frame=R(CUR, 0)), W("ROW_NUMBER", None, "rn", frame=G(1, 2)), W("LAG", "u", "lag_u", 2, frame=R(-5, 5)),
          W("SUM", "k", "far", frame=R(-2**63, 2**63 - 1)), W("SUM", "f", "rows", frame=F(-6, 0))]
    plan = ba.WindowAggExec([col("u")], [asc("k")], ws, leaf())
    assert plan.schema() == leaf().schema() + [
        ("m", "Float64", True), ("a", "Float64", True), ("c", "UInt64", False), ("star", "UInt64", False), ("mn", "Float32", True), ("mx", "Date32", True),
        ("first_in", "Utf8", False), ("first_after", "Utf8", True), ("first_groups", "Utf8", True), ("last_before", "Date32", True), ("last_kn", "Int64", True),
        ("last_tail", "Date32", False), ("last_zero", "Utf8", False), ("rn", "UInt64", False), ("lag_u", "Utf8", True), ("far", "Int64", True), ("rows", "Float64", True)]
    text = plan.display()
    for part in ("SUM(f) RANGE BETWEEN 7 PRECEDING AND CURRENT ROW as m", "AVG(i) GROUPS BETWEEN 1 PRECEDING AND 1 FOLLOWING as a",
                 "COUNT(s) RANGE BETWEEN 1 FOLLOWING AND UNBOUNDED FOLLOWING as c", "COUNT(UInt8(1)) GROUPS BETWEEN 3 PRECEDING AND UNBOUNDED FOLLOWING as star",
                 "MIN(f32) RANGE BETWEEN 0 PRECEDING AND 0 FOLLOWING as mn", "MAX(d) RANGE BETWEEN UNBOUNDED PRECEDING AND 3 FOLLOWING as mx",
                 "LAST_VALUE(d) GROUPS BETWEEN UNBOUNDED PRECEDING AND 1 PRECEDING as last_before", "LAST_VALUE(kn) RANGE BETWEEN CURRENT ROW AND CURRENT ROW as last_kn",
                 "LAST_VALUE(u) RANGE BETWEEN CURRENT ROW AND 0 FOLLOWING as last_zero", "ROW_NUMBER() as rn", "LAG(u, 2) as lag_u",
                 "SUM(k) RANGE BETWEEN 9223372036854775808 PRECEDING AND 9223372036854775807 FOLLOWING as far", "SUM(f) ROWS BETWEEN 6 PRECEDING AND CURRENT ROW as rows"):
        assert part in text, (part, text)
    # float offsets read back to the same double; an Int64 offset over a float key is the double it equals
    text = ba.WindowAggExec([], [asc("f")], [W("SUM", "k", "a", frame=R(-0.5, 0.1)), W("SUM", "k", "b", frame=R(-7, 1e300)), W("COUNT", "k", "c", frame=R(-2**53, 2**62)),
                                             W("COUNT", "k", "d", frame=R(-0.0, 0.0)), W("COUNT", "k", "e", frame=R(5e-324, 1 / 3))], leaf()).display()
    for part in ("RANGE BETWEEN 0.5 PRECEDING AND 0.1 FOLLOWING as a", "RANGE BETWEEN 7.0 PRECEDING AND 1e+300 FOLLOWING as b",
                 "RANGE BETWEEN 9007199254740992.0 PRECEDING AND 4.611686018427388e+18 FOLLOWING as c", "RANGE BETWEEN 0.0 PRECEDING AND 0.0 FOLLOWING as d",
                 "RANGE BETWEEN 5e-324 FOLLOWING AND 0.3333333333333333 FOLLOWING as e"):
        assert part in text, (part, text)
    assert float("0.1") == 0.1 and float("0.3333333333333333") == 1 / 3 and float("4.611686018427388e+18") == 2.0**62 and float("5e-324") == 5e-324


def test_the_canonical_forms():
    ws = [W("SUM", "f", "all_r", frame=R(None, None)), W("MIN", "f", "all_g", frame=G(None, None)), W("SUM", "f", "run_r", frame=R(None, CUR)),
          W("LAST_VALUE", "u", "run_g", frame=G(None, CUR)), W("COUNT", "f", "run_g0", frame=G(None, 0)), W("FIRST_VALUE", "u", "first", frame=G(None, None)),
          W("AVG", "f", "kept", frame=R(None, 0)), W("SUM", "f", "g0", frame=G(CUR, 1)), W("SUM", "f", "g1", frame=G(0, 1)), W("SUM", "f", "rows", frame=F(None, 0)),
          W("SUM", "f", "slide", frame=F(-6, 0))]
    plan = ba.WindowAggExec([col("u")], [asc("k")], ws, leaf())
    text = plan.display()
    for part in ("SUM(f) PARTITION as all_r", "MIN(f) PARTITION as all_g", "SUM(f) RANGE_TO_CURRENT as run_r", "LAST_VALUE(u) RANGE_TO_CURRENT as run_g",
                 "COUNT(f) RANGE_TO_CURRENT as run_g0", "FIRST_VALUE(u) as first", "AVG(f) RANGE BETWEEN UNBOUNDED PRECEDING AND 0 FOLLOWING as kept",
                 "SUM(f) GROUPS BETWEEN CURRENT ROW AND 1 FOLLOWING as g0", "SUM(f) GROUPS BETWEEN CURRENT ROW AND 1 FOLLOWING as g1", "SUM(f) ROWS_TO_CURRENT as rows",
                 "SUM(f) ROWS BETWEEN 6 PRECEDING AND CURRENT ROW as slide"):
        assert part in text, (part, text)
    named = [W("SUM", "f", "all_r", frame="PARTITION"), W("MIN", "f", "all_g", frame="PARTITION"), W("SUM", "f", "run_r", frame="RANGE_TO_CURRENT"),
             W("LAST_VALUE", "u", "run_g", frame="RANGE_TO_CURRENT"), W("COUNT", "f", "run_g0"), W("FIRST_VALUE", "u", "first"), W("AVG", "f", "kept", frame=R(None, 0)),
             W("SUM", "f", "g0", frame=G(0, 1)), W("SUM", "f", "g1", frame=G(CUR, 1)), W("SUM", "f", "rows", frame="ROWS_TO_CURRENT"), W("SUM", "f", "slide", frame=F(-6, 0))]
    again = ba.WindowAggExec([col("u")], [asc("k")], named, leaf())
    assert again.display() == text and again.schema() == plan.schema()
    # without RANGE / GROUPS frames the operator makes the calls it made before: the same plan either way
    rows_only = [W("SUM", "f", "slide", frame=F(-6, 0)), W("COUNT", "f", "c", frame=F(None, 2))]
    assert ba.WindowAggExec([], [asc("k")], rows_only + [W("MAX", "k", "x", frame=G(None, None))], leaf()).display().replace(", MAX(k) PARTITION as x", "") == \
        ba.WindowAggExec([], [asc("k")], rows_only, leaf()).display()
    # a RANGE frame with CURRENT ROW / UNBOUNDED sides takes any order keys, and none
    for order in ([], [asc("s"), asc("b")]):
        t = ba.WindowAggExec([], order, [W("COUNT", "k", "c", frame=R(CUR, None)), W("SUM", "f", "s", frame=R(CUR, CUR)), W("SUM", "f", "g", frame=G(-1, 1))], leaf()).display()
        assert "COUNT(k) RANGE BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING as c" in t and "SUM(f) RANGE BETWEEN CURRENT ROW AND CURRENT ROW as s" in t


def test_with_new_children_keeps_the_frames():
    first = ba.WindowAggExec([col("u")], [asc("f")], [W("SUM", "f", "m", frame=R(-7, 0.5)), W("LAST_VALUE", "u", "l", frame=G(1, 1)), W("COUNT", "k", "r", frame=F(-1, 0))], leaf())
    second = ba.WindowAggExec([col("u")], [asc("k", True, False)], [W("MAX", "m", "mm", frame=R(-1, CUR)), W("COUNT", "l", "c", frame=G(2, None))], first)
    assert second.schema()[-5:] == [("m", "Float64", True), ("l", "Utf8", True), ("r", "UInt64", False), ("mm", "Float64", True), ("c", "UInt64", False)]
    again = second.with_new_children([first])
    assert again.schema() == second.schema() and again.display() == second.display()
    assert "MAX(m) RANGE BETWEEN 1 PRECEDING AND CURRENT ROW as mm" in again.display() and "SUM(f) RANGE BETWEEN 7.0 PRECEDING AND 0.5 FOLLOWING as m" in again.display()
    assert "COUNT(k) ROWS BETWEEN 1 PRECEDING AND CURRENT ROW as r" in again.display()
    assert [w.frame for w in again.window_exprs] == [R(-1, CUR), G(2, None)]


def test_the_raw_entry_point():
    range_1_0 = lambda: spec_c(1, (OFF, 0, -1, 0.0), CURRENT)
    # a spec goes with BHIP_FRAME_DEFAULT only
    for frame in (1, 2, 3):
        with pytest.raises(ba.PlanError, match="a frame spec goes with BHIP_FRAME_DEFAULT, not with"):
            plan_window_specs([("SUM", "k", frame, range_1_0())])
    with pytest.raises(ba.PlanError, match="Unknown window frame 4"):
        plan_window_specs([("SUM", "k", 4, range_1_0())])
    # a null entry: fns[i].frame as it is; a null array: bhip_plan_window
    text = plan_window_specs([("SUM", "k", 2, None), ("SUM", "k", 0, range_1_0()), ("SUM", "k", 0, None)]).display()
    assert "SUM(k) ROWS_TO_CURRENT as w0, SUM(k) RANGE BETWEEN 1 PRECEDING AND CURRENT ROW as w1, SUM(k) RANGE_TO_CURRENT as w2" in text
    assert "SUM(k) ROWS_TO_CURRENT as w0" in plan_window_specs([("SUM", "k", 2, None)], null_array=True).display()
    with pytest.raises(ba.PlanError, match="Unknown window frame 4"):
        plan_window_specs([("SUM", "k", 4, None)], null_array=True)
    # the numbers of a side that is not an OFFSET are not read
    text = plan_window_specs([("SUM", "k", 0, spec_c(1, (0, 1, 2**62, math.nan), (1, 1, -5, math.inf))), ("SUM", "k", 0, spec_c(2, (0, 0, 9, 0.0), (0, 1, 0, math.nan)))]).display()
    assert "SUM(k) RANGE_TO_CURRENT as w0, SUM(k) PARTITION as w1" in text
    # ROWS-unit specs are rows frames: the same display as bhip_plan_window_frames gives
    from tests.test_window_frames_cpu import plan_window_frames
    pairs = [(spec_c(0, (OFF, 0, -6, 0.0), CURRENT), L.RowsFrameC(0, 0, -6, 0)), (spec_c(0, UNB, (OFF, 0, 2, 0.0)), L.RowsFrameC(1, 0, 0, 2)),
             (spec_c(0, UNB, CURRENT), L.RowsFrameC(1, 0, 0, 0)), (spec_c(0, (OFF, 0, 0, 0.0), UNB), L.RowsFrameC(0, 1, 0, 0)), (spec_c(0, UNB, UNB), L.RowsFrameC(1, 1, 0, 0)),
             (spec_c(0, (OFF, 0, -2**63, 0.0), (OFF, 0, 2**63 - 1, 0.0)), L.RowsFrameC(0, 0, -2**63, 2**63 - 1))]
    by_spec = plan_window_specs([("SUM", "k", 0, s) for s, _ in pairs], order=()).display()
    by_rows = plan_window_frames([("SUM", "k", 0, r) for _, r in pairs]).display()
    assert by_spec == by_rows and "ROWS BETWEEN 6 PRECEDING AND CURRENT ROW" in by_spec and "ROWS_TO_CURRENT" in by_spec
    with pytest.raises(ba.PlanError, match="SUM ROWS BETWEEN 1 FOLLOWING AND CURRENT ROW: frame start lies after its end"):
        plan_window_specs([("SUM", "k", 0, spec_c(0, (OFF, 0, 1, 0.0), CURRENT))])
    with pytest.raises(ba.NotImplementedOnGpu, match=rf"SUM\(Float64\) over ROWS BETWEEN {CAP} PRECEDING AND CURRENT ROW: a frame wider than {CAP} rows"):
        plan_window_specs([("SUM", "f", 0, spec_c(0, (OFF, 0, -CAP, 0.0), CURRENT))])


def test_the_python_mirror():
    for cls in (R, G):
        for bad in ("1", True, 2**63, -2**63 - 1, math.nan, math.inf, (1,), F(0, 0)):
            with pytest.raises(TypeError):
                cls(bad, 0)
            with pytest.raises(TypeError):
                cls(None, bad)
    for bad in (1.0, -0.5):
        with pytest.raises(TypeError):
            G(bad, None)
    assert R(-0.5, 2.0).start == -0.5 and R(-2**63, 2**63 - 1).end == 2**63 - 1 and G(CUR, None).start is CUR and R(None, CUR).end is E.CURRENT_ROW
    assert R(-2, 0) == R(-2, 0) and R(-2, 0) != G(-2, 0) and R(-2, CUR) != R(-2, 0) and hash(G(None, 3)) == hash(G(None, 3)) and repr(CUR) == "CURRENT_ROW"
    assert type(CUR)() is CUR
    assert E.WindowExpr("SUM", col("k"), "x", frame=R(-7, CUR)).frame == R(-7, CUR) and E.count_star("c", G(-1, 1)).frame == G(-1, 1)
    # what was there stays as it was
    assert E.WINDOW_FRAMES == ("DEFAULT", "PARTITION", "ROWS_TO_CURRENT", "RANGE_TO_CURRENT") and len(E.WINDOW_FUNCTIONS) == 12
    assert ba.WindowAggExec._FRAME == dict(DEFAULT=0, PARTITION=1, ROWS_TO_CURRENT=2, RANGE_TO_CURRENT=3)
    for frame in ("RANGE", "GROUPS", None, (-3, 0), CUR):
        with pytest.raises(NotImplementedError):
            E.WindowExpr("SUM", col("k"), "x", frame=frame)


# ---- 4. the mirror against the headers -----------------------------------------------------------------------------------------------------

def test_the_structs_the_enums_and_the_symbol_match_the_header():
    header = open(os.path.join(ROOT, "include", "ballista_hip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "bhip_frame_bound": L.FrameBoundC}

    def fields(name):
        m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header)
        assert m, name
        return [(f.strip(), ctype[decl.split()[0]]) for decl in m.group(1).split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]

    assert fields("bhip_frame_bound") == L.FrameBoundC._fields_ and C.sizeof(L.FrameBoundC) == 24
    assert fields("bhip_frame_spec") == L.FrameSpecC._fields_ and C.sizeof(L.FrameSpecC) == 56
    for name, v in (("BHIP_FRAME_UNITS_ROWS", ba.WindowAggExec._UNITS[F]), ("BHIP_FRAME_UNITS_RANGE", ba.WindowAggExec._UNITS[R]),
                    ("BHIP_FRAME_UNITS_GROUPS", ba.WindowAggExec._UNITS[G]), ("BHIP_BOUND_UNBOUNDED", ba.WindowAggExec.BOUND_UNBOUNDED),
                    ("BHIP_BOUND_CURRENT_ROW", ba.WindowAggExec.BOUND_CURRENT_ROW), ("BHIP_BOUND_OFFSET", ba.WindowAggExec.BOUND_OFFSET)):
        assert re.search(rf"\b{name} = {v}\b", header), name
    assert re.search(r"bhip_status bhip_plan_window_frame_specs\([^;]*const bhip_window_expr\* fns,\s*const bhip_frame_spec\* const\* specs, bhip_plan\*\* out\);", header)
    assert "bhip_plan_window_frame_specs" in L.SYMBOLS and L.SYMBOLS["bhip_plan_window_frame_specs"][1][:-2] == L.SYMBOLS["bhip_plan_window"][1][:-1]
    text = open(os.path.join(ROOT, "ballista_amd", "csrc", "window_kernels.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (WINDOW_[A-Z_]+) = (\d+);", text)}
    # the staged-span budget: more than a tile, within 64 KiB of LDS at 9 bytes a row, and reachable by a frame the cap admits (the GPU
    # tests put an interior tile's span one below, at and one above it)
    assert consts["WINDOW_SLIDE_STAGE_ROWS"] == ba.plan.WINDOW_SLIDE_STAGE_ROWS
    assert consts["WINDOW_TILE_ROWS"] < consts["WINDOW_SLIDE_STAGE_ROWS"] <= consts["WINDOW_TILE_ROWS"] + consts["WINDOW_SLIDE_MAX_ROWS"] - 2
    assert consts["WINDOW_SLIDE_STAGE_ROWS"] * 9 <= 64 * 1024
