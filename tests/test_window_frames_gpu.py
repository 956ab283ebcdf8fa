"""WindowAggExec's sliding ROWS frames on the device against the row-by-row restatement (tests/window_frame_cases.py, itself checked
against sqlite3 by test_window_frames_cpu.py).

The expected value is the restatement applied to the oracle's SortExec over the operator's own sort keys, as in test_window_gpu.py;
every batch carries its input row number (rn).  Integers, counts, validity and gathered values compare bit for bit — and so do SUM of
floats and every AVG over a frame with two finite ends, over positive uniform inputs (u) as well as exact ones (f): the order of the
additions is defined (row order, from +0.0), so the bits are.  MIN / MAX over floats may return either zero.  A float sum whose frame
starts UNBOUNDED PRECEDING has the tile-tree order of the running sums: bit for bit on f, within the project's 1e-6 gate on u.

Frames: one row either side, the row itself, symmetric, wholly before and wholly after the row (empty at a partition's ends), 63 / 64
rows back (a wave), T and more than T rows on both sides (T = WINDOW_TILE_ROWS: the staged span covers neighbouring tiles), exactly
the 4096-row cap, narrow and far (-5000 .. -4990), an unbounded side with an offset on the other, and offsets of 2^62 (clamped).
Sizes 1, 2, 65, T - 1, T, T + 1, 3T + 1 against the six partition shapes of window_cases."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle import engine as og, plan_eval
from oracle.engine import OCol

import helpers
import sort_cases
from tests import window_cases as K, window_frame_cases as FK
from tests.window_frame_cases import F, W, asc

pytestmark = pytest.mark.gpu

RTOL = 1e-6                                    # SUM / AVG over Float64
T = K.T
CAP = ba.plan.WINDOW_SLIDE_MAX_ROWS
SIZES = [1, 2, 65, T - 1, T, T + 1, 3 * T + 1]


def expected(m, partition_by, order_by, ws):
    keys = K.sort_keys(partition_by, order_by)
    in_order = plan_eval.collect(ba.SortExec(keys, m)) if keys else plan_eval.collect(m)
    return FK.restate(in_order, partition_by, order_by, ws)


def without(batch, names):
    return OrderedDict((k, c) for k, c in batch.items() if k not in names)


def check(ctx, batches, partition_by, order_by, ws, within_gate=(), any_zero_sign=(), chunk=40):
    """run the operator (a few of them: `chunk` expressions each) over one partition holding `batches` and compare every column"""
    m = helpers.memory_exec(ctx, [batches])
    got = None
    for at in range(0, len(ws), chunk):
        out = helpers.collect_product(ba.WindowAggExec(partition_by, order_by, ws[at:at + chunk], m))
        assert len(out) == 1
        got = out[0] if got is None else OrderedDict(list(got.items()) + [(w.name, out[0][w.name]) for w in ws[at:at + chunk]])
        assert np.array_equal(got["rn"].values, out[0]["rn"].values)
    want = expected(m, partition_by, order_by, ws)
    loose = set(within_gate) | set(any_zero_sign)
    helpers.assert_bit_exact(without(got, loose), without(want, loose))
    pick = lambda b, names: OrderedDict((k, b[k]) for k in ["rn"] + list(names))
    if within_gate:
        helpers.assert_rows_equal(pick(got, within_gate), pick(want, within_gate), ordered=True, float_rtol=RTOL)
    if any_zero_sign:
        helpers.assert_rows_equal(pick(got, any_zero_sign), pick(want, any_zero_sign), ordered=True, zero_sign_cols=tuple(any_zero_sign))
    return got


def split(batch, cuts):
    n = og.batch_len(batch)
    edges = [0] + [c for c in cuts if 0 < c < n] + [n]
    return [helpers.slice_batch(batch, lo, hi) for lo, hi in zip(edges, edges[1:])]


def tag(frame):
    side = lambda v: "u" if v is None else ("m%d" % -v if v < 0 else "p%d" % v)
    return side(frame.start) + "_" + side(frame.end)


# ---- the narrow frames: every size x every partition shape --------------------------------------------------------------------------------

FINITE = [F(-1, 0), F(0, 0), F(0, 1), F(-2, 2), F(-3, -1), F(1, 2), F(-63, 0), F(-64, 0), F(-5000, -4990), F(2**62, 2**62 + 1)]
EVERYTHING = (F(-2, 2), F(-3, -1), F(1, 2))                              # these take every function; the others the routes' core


def narrow_exprs(strings):
    """-> (expressions, names within the gate, names with either zero)"""
    ws, gate, zero = [], [], []
    for fr in FINITE:
        t = tag(fr)
        ws += [W("SUM", "f", "sum_f_" + t, frame=fr), W("SUM", "u", "sum_u_" + t, frame=fr), W("AVG", "u", "avg_u_" + t, frame=fr),
               W("MIN", "g", "min_g_" + t, frame=fr), W("MAX", "f", "max_f_" + t, frame=fr), W("COUNT", "i64", "cnt_" + t, frame=fr),
               W("SUM", "i64", "sum_i_" + t, frame=fr), W("FIRST_VALUE", "i64", "first_" + t, frame=fr), W("LAST_VALUE", "f", "last_" + t, frame=fr)]
        zero += ["max_f_" + t]
        if fr in EVERYTHING:
            ws += [W("AVG", "f", "avg_f_" + t, frame=fr), W("AVG", "i64", "avg_i_" + t, frame=fr), W("MIN", "f", "min_f_" + t, frame=fr),
                   W("MAX", "i64", "max_i_" + t, frame=fr), W("SUM", "g", "sum_g_" + t, frame=fr), E.count_star("star_" + t, fr),
                   W("LAST_VALUE", "g", "last_g_" + t, frame=fr)]
            zero += ["min_f_" + t]
            if strings:
                ws += [W("FIRST_VALUE", "s", "first_s_" + t, frame=fr), W("COUNT", "s", "cnt_s_" + t, frame=fr)]
    # start unbounded, end an offset: the running state at hi (any aggregate)
    for fr in (F(None, 2), F(None, -1), F(None, 2**62)):
        t = tag(fr)
        ws += [W("SUM", "f", "sum_f_" + t, frame=fr), W("SUM", "u", "sum_u_" + t, frame=fr), W("AVG", "u", "avg_u_" + t, frame=fr),
               W("MIN", "g", "min_g_" + t, frame=fr), W("MAX", "f", "max_f_" + t, frame=fr), W("COUNT", "i64", "cnt_" + t, frame=fr),
               W("SUM", "i64", "sum_i_" + t, frame=fr), W("FIRST_VALUE", "i64", "first_" + t, frame=fr), W("LAST_VALUE", "f", "last_" + t, frame=fr)]
        gate += ["sum_u_" + t, "avg_u_" + t]
        zero += ["max_f_" + t]
    # an offset to UNBOUNDED FOLLOWING, and a start 2^62 rows back (clamped): the difference of running states, and the gathers
    for fr in (F(-2, None), F(-2**62, 0)):
        t = tag(fr)
        ws += [W("COUNT", "i64", "cnt_" + t, frame=fr), W("SUM", "i64", "sum_i_" + t, frame=fr), E.count_star("star_" + t, fr)]
        if fr.end is None:
            ws += [W("FIRST_VALUE", "i64", "first_" + t, frame=fr), W("LAST_VALUE", "f", "last_" + t, frame=fr), W("SUM", "g", "sum_g_" + t, frame=fr)]
    return ws + [W("ROW_NUMBER", None, "row_number", frame=F(-1, 1))], gate, zero


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_narrow_frames_at_every_size_and_partition_shape(ctx, n, shape):
    strings = n <= T + 1
    batch = K.table(n, shape, seed=n + len(shape), strings=strings)
    ws, gate, zero = narrow_exprs(strings)
    got = check(ctx, split(batch, [n // 3]), [col("p")], [asc("o")], ws, within_gate=gate, any_zero_sign=zero)
    # the case is what it says: partitions lie where the shape puts them, and the frames before / after the row are empty at their ends
    rows = got["row_number"].values
    heads = rows == 1
    lasts = np.r_[heads[1:], True]
    assert not got["first_p1_p2"].is_valid()[lasts].any()                            # the last row of a partition has nothing after it
    assert not got["last_m3_m1"].is_valid()[heads].any() and not got["sum_f_m3_m1"].is_valid()[heads].any()
    assert (got["star_m2_u"].values[lasts] == np.minimum(rows, 3)[lasts]).all()
    assert not got["sum_f_p4611686018427387904_p4611686018427387905"].is_valid().any() and not got["cnt_p4611686018427387904_p4611686018427387905"].values.any()
    if shape == "one_partition":
        assert list(np.nonzero(heads)[0]) == [0] and not got["cnt_m5000_m4990"].values.any()      # (test_a_narrow_frame_far_away has the rows for it)
    elif shape == "every_row":
        assert heads.all() and not got["cnt_m1_p0"].values[~got["i64"].is_valid()].any()


# ---- frames as wide as a tile and wider: the staged span reaches into the neighbouring tiles ---------------------------------------------

WIDE = [F(-T, 0), F(-(T + 1), T + 1), F(-(CAP - 1), 0)]


@pytest.mark.parametrize("shape", K.SHAPES)
def test_frames_of_a_tile_and_more(ctx, shape):
    n = 3 * T + 1
    batch = K.table(n, shape, seed=31 + len(shape))
    ws, zero = [], []
    for fr in WIDE:
        t = tag(fr)
        ws += [W("SUM", "f", "sum_f_" + t, frame=fr), W("SUM", "u", "sum_u_" + t, frame=fr), W("MIN", "g", "min_g_" + t, frame=fr),
               W("MAX", "f", "max_f_" + t, frame=fr)]
        zero += ["max_f_" + t]
    got = check(ctx, split(batch, [T + 5]), [col("p")], [asc("o")], ws + [W("ROW_NUMBER", None, "row_number")], any_zero_sign=zero)
    if shape == "one_partition":
        # the widest frame holds every row before the current one: on exact inputs that is the running sum
        run = check(ctx, [batch], [col("p")], [asc("o")], [W("SUM", "f", "run", frame="ROWS_TO_CURRENT")])["run"]
        assert np.array_equal(run.is_valid(), got["sum_f_" + tag(WIDE[2])].is_valid())
        v = run.is_valid()
        assert np.array_equal(run.values[v], got["sum_f_" + tag(WIDE[2])].values[v])


def test_a_narrow_frame_far_away(ctx):
    """the staged span lies four tiles before the tile it serves; in rows 0 .. 4989 the frame is empty"""
    n = 5 * T + 1
    fr = F(-5000, -4990)
    ws = [W("SUM", "f", "sum_f", frame=fr), W("SUM", "u", "sum_u", frame=fr), W("MIN", "g", "min_g", frame=fr), W("COUNT", "i64", "cnt", frame=fr),
          W("FIRST_VALUE", "rn", "first", frame=fr)]
    got = check(ctx, [K.table(n, "one_partition", seed=17)], [col("p")], [asc("o")], ws)
    assert not got["first"].is_valid()[:4990].any() and got["first"].is_valid()[4990:].all() and got["cnt"].values[5000:].any()


def test_counts_and_integer_sums_through_the_second_level_of_the_scans(ctx):
    n = K.S + 1
    batch = K.table(n, "three_tiles", seed=13)
    fr = F(-2, 2)
    check(ctx, split(batch, [100000]), [col("p")], [asc("o")], [W("COUNT", "i64", "cnt", frame=fr), W("SUM", "i64", "sum", frame=fr)])


# ---- the same bits whatever the batches, and twice from one plan -------------------------------------------------------------------------

def test_bounded_float_sums_have_the_same_bits_in_every_run(ctx):
    batch = K.table(3 * T + 1, "three_tiles", seed=11)
    ws = [W("SUM", "u", "sum6", frame=F(-6, 0)), W("AVG", "u", "avg5", frame=F(-2, 2)), W("SUM", "u", "sum_tile", frame=F(-T, 0)),
          W("AVG", "f", "avg_far", frame=F(3, 70)), W("ROW_NUMBER", None, "row_number")]
    plan = ba.WindowAggExec([col("p")], [asc("o")], ws, helpers.memory_exec(ctx, [split(batch, [1000, 1700])]))
    a, b = (helpers.concat(helpers.collect_product(plan)) for _ in range(2))
    c = helpers.concat(helpers.collect_product(ba.WindowAggExec([col("p")], [asc("o")], ws, helpers.memory_exec(ctx, [[batch]]))))
    d = helpers.concat(helpers.collect_product(ba.WindowAggExec([col("p")], [asc("o")], ws, helpers.memory_exec(ctx, [split(batch, [1, 64, 65, 2 * T])]))))
    for other in (b, c, d):
        helpers.assert_bit_exact(other, a)
    # ... and they are the bits of the plain loop
    helpers.assert_bit_exact(a, FK.restate(K.sorted_input(batch, [col("p")], [asc("o")]), [col("p")], [asc("o")], ws))


# ---- every argument type, float specials, no order ---------------------------------------------------------------------------------------

def test_every_argument_type(ctx):
    batch = K.every_type_table(700, seed=3)
    fr = F(-3, 1)
    ws, zero = [], []
    for name in batch:
        if not name.startswith("c_"):
            continue
        t = name[2:]
        ws += [W("COUNT", name, "count_" + t, frame=fr), W("FIRST_VALUE", name, "first_" + t, frame=fr), W("LAST_VALUE", name, "last_" + t, frame=fr)]
        if t not in ("Boolean", "Utf8"):
            ws += [W("SUM", name, "sum_" + t, frame=fr), W("AVG", name, "avg_" + t, frame=fr), W("MIN", name, "min_" + t, frame=fr),
                   W("MAX", name, "max_" + t, frame=fr)]
            zero += ["min_" + t, "max_" + t] if t in K.FLOATS else []
    got = check(ctx, split(batch, [256]), [col("p")], [asc("o")], ws, any_zero_sign=zero)
    assert got["sum_UInt64"].dtype == "UInt64" and got["sum_Int8"].dtype == "Int64" and got["sum_Float32"].dtype == "Float64"
    assert got["min_Float32"].dtype == "Float32" and got["avg_UInt64"].dtype == "Float64"


@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_float_specials_under_min_max_and_the_gathers(ctx, dtype):
    """NaN only while nothing else is in the frame, either zero of a -0.0 / +0.0 tie; the gathers copy every bit pattern"""
    n = 400
    rng = np.random.default_rng(n)
    batch = OrderedDict([("f", sort_cases.float_special_column(dtype, n, rng)), ("t", OCol("Int32", rng.integers(0, 4, n).astype(np.int32))),
                         ("x", OCol("Int64", rng.integers(-100, 100, n))), ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])
    ws, zero = [], []
    for fr in (F(0, 0), F(-2, 2), F(1, 3), F(None, 1)):
        t = tag(fr)
        ws += [W("MIN", "f", "min_" + t, frame=fr), W("MAX", "f", "max_" + t, frame=fr), W("FIRST_VALUE", "f", "first_" + t, frame=fr),
               W("LAST_VALUE", "f", "last_" + t, frame=fr), W("COUNT", "f", "cnt_" + t, frame=fr)]
        zero += ["min_" + t, "max_" + t]
    got = check(ctx, [batch], [col("t")], [asc("x")], ws, any_zero_sign=zero)
    assert np.isnan(got["min_p0_p0"].values[got["min_p0_p0"].is_valid()]).any() and np.isnan(got["max_p0_p0"].values[got["max_p0_p0"].is_valid()]).any()


def test_min_max_over_nans_alone_and_all_null_frames(ctx):
    nan = np.nan
    f = OCol("Float64", [nan, 1.0, nan, -2.0, nan, nan, 3.0, 4.0], np.array([True, True, True, True, False, True, False, False]))
    batch = OrderedDict([("p", OCol("Int32", np.array([0, 0, 0, 0, 1, 1, 2, 2], np.int32))), ("f", f), ("rn", OCol("Int64", np.arange(8, dtype=np.int64)))])
    ws = [W(fun, "f", f"{fun}_{tag(fr)}", frame=fr) for fun in K.AGGREGATES for fr in (F(-1, 0), F(1, 1))]
    # (NaN results compare as NaN, not by their bits)
    got = check(ctx, [batch], [col("p")], [asc("rn")], ws, any_zero_sign=[w.name for w in ws if not w.name.startswith("COUNT")])
    mn = got["MIN_m1_p0"].to_pylist()
    assert np.isnan(mn[0]) and mn[1:4] == [1.0, 1.0, -2.0] and mn[4] is None and np.isnan(mn[5]) and mn[6:] == [None, None]
    assert got["COUNT_m1_p0"].to_pylist() == [1, 2, 2, 2, 0, 1, 0, 0] and got["COUNT_p1_p1"].to_pylist() == [1, 1, 1, 0, 1, 0, 0, 0]
    assert np.isnan(got["SUM_m1_p0"].values[:4]).all() and got["AVG_p1_p1"].to_pylist()[3] is None


def test_the_bounded_sum_starts_at_positive_zero_and_adds_in_row_order(ctx):
    """-0.0 alone sums to +0.0 (0.0 + -0.0); 2^53 + 1 + 1 loses both ones where 1 + 1 + 2^53 keeps them"""
    v = OCol("Float64", [-0.0, -0.0, 2.0**53, 1.0, 1.0, 2.0**53, -0.0], np.array([True, True, True, True, True, True, False]))
    batch = OrderedDict([("v", v), ("w", OCol("Float32", v.values.astype(np.float32), v.valid)), ("rn", OCol("Int64", np.arange(7, dtype=np.int64)))])
    got = check(ctx, [batch], [], [asc("rn")], [W("SUM", "v", "one", frame=F(0, 0)), W("SUM", "v", "three", frame=F(-2, 0)), W("AVG", "v", "avg", frame=F(0, 0)),
                                                W("SUM", "w", "three32", frame=F(-2, 0))])
    assert not np.signbit(got["one"].values[:2]).any() and not np.signbit(got["avg"].values[:2]).any() and got["one"].to_pylist()[6] is None
    assert got["three"].to_pylist()[4:6] == [2.0**53, 2.0**53 + 2.0] and got["three32"].to_pylist()[4:6] == [2.0**53, 2.0**53 + 2.0]


def test_without_order_by_the_frame_runs_over_input_order(ctx):
    batch = K.table(2 * T + 9, "tile_ends", seed=2, strings=True)
    ws = [W("SUM", "u", "s", frame=F(-3, 0)), W("LAST_VALUE", "s", "l", frame=F(1, 1)), W("COUNT", "g", "c", frame=F(-1, None)), W("MIN", "i64", "m", frame=F(0, 5))]
    check(ctx, split(batch, [700]), [col("p")], [], ws)
    check(ctx, split(batch, [700]), [], [], ws)


# ---- launches: named, one frame-bounds launch per distinct frame, the old frames as before ---------------------------------------------------

def test_each_launch_is_timed_under_its_own_name():
    mp = pytest.MonkeyPatch()
    mp.setenv("BHIP_KERNEL_TIMING", "2")
    try:
        tctx = ba.Context(0)
    finally:
        mp.undo()
    batch = K.table(3 * T + 1, "three_tiles", seed=9)
    ws = [W("SUM", "f", "a", frame=F(-6, 0)), W("MIN", "f", "b", frame=F(-6, 0)), W("AVG", "i64", "c", frame=F(-6, 0)), W("SUM", "i64", "d", frame=F(-6, 0)),
          W("COUNT", "i64", "e", frame=F(None, 2)), W("LAST_VALUE", "f", "g", frame=F(None, 2)), W("SUM", "f", "h", frame=F(None, 0)),
          W("SUM", "f", "i", frame="ROWS_TO_CURRENT"), W("SUM", "g", "j", frame=F(-10**12, 0))]
    tctx.kernel_stats(reset=True)
    check(tctx, [batch], [col("p")], [asc("o")], ws, any_zero_sign=["b"])
    stats = tctx.kernel_stats(reset=True)
    # three distinct frames: (-6, 0), (unbounded, 2) and (-10^12, 0); F(None, 0) is ROWS_TO_CURRENT
    assert stats["window_frame_bounds"][1] == 3, stats["window_frame_bounds"]
    assert stats["window_slide"][1] == 3 and stats["window_finish_frame"][1] == 3 and stats["window_finish"][1] == 2, stats
    assert stats["window_scan_apply"][1] == 5
