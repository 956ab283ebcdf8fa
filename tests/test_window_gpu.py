"""WindowAggExec on the device against the row-by-row restatement (tests/window_cases.py, itself checked against sqlite3 and pinned
values by test_window_cases_cpu.py).

The expected value is the restatement applied to the oracle's SortExec over the operator's own sort keys (oracle/plan_eval.py): the
order comes from the existing oracle, the functions from the restatement.  Every batch carries its input row number (rn), so a swap
of two tied rows shows.  Integers, ranks, gathered values, validity and strings compare bit for bit; so do Float64 SUM / AVG over
exact-valued inputs (eighths: every partial sum is exact, whatever the order of the additions).  Over positive uniform inputs — no
cancellation — they compare within the project's 1e-6 relative gate.

Sizes (window_cases.SIZES): 1, 2, 63, 64, 65 around a wave; T - 1, T, T + 1 and 3T + 1 around the tile of the scans (T =
WINDOW_TILE_ROWS); S + 1, where S = T * 256 + 1 is the smallest count whose tile summaries need a second step of the scans' second
level.  At every size: one partition over everything, every row its own partition, partitions that end on a tile's last row, a
partition that begins on the very last row, a partition spanning more than three tiles, peer groups that straddle every tile
boundary."""
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
from tests import window_cases as K
from tests.window_cases import W, asc

pytestmark = pytest.mark.gpu

RTOL = 1e-6                                    # SUM / AVG over Float64


def expected(m, partition_by, order_by, ws):
    keys = K.sort_keys(partition_by, order_by)
    in_order = plan_eval.collect(ba.SortExec(keys, m)) if keys else plan_eval.collect(m)
    return K.restate(in_order, partition_by, order_by, ws)


def without(batch, names):
    return OrderedDict((k, c) for k, c in batch.items() if k not in names)


def check(ctx, batches, partition_by, order_by, ws, within_gate=(), any_zero_sign=()):
    """run the operator over one partition holding `batches` and compare every column; returns the device's result"""
    m = helpers.memory_exec(ctx, [batches])
    plan = ba.WindowAggExec(partition_by, order_by, ws, m)
    assert plan.output_partitioning().count == 1
    out = helpers.collect_product(plan)
    assert len(out) == 1                                               # one output partition, one batch
    got, want = out[0], expected(m, partition_by, order_by, ws)
    loose = set(within_gate) | set(any_zero_sign)
    helpers.assert_bit_exact(without(got, loose), without(want, loose))
    if loose:
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


# ---- every size x every partition shape ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("n", K.SIZES)
def test_sizes_and_partition_shapes(ctx, n, shape):
    full = n <= 3 * K.T + 1
    batch = K.table(n, shape, seed=n + len(shape), strings=full)
    got = check(ctx, split(batch, [n // 3]), [col("p")], [asc("o")], K.standard_exprs(strings=full, full=full))
    # the case is what it says: the partitions and peer groups lie where the shape puts them
    rows = got["row_number"].values
    heads = np.nonzero(rows == 1)[0]
    if shape == "one_partition":
        assert list(heads) == [0] and rows[-1] == n
    elif shape == "every_row":
        assert len(heads) == n
    elif shape == "tile_ends" and n > K.T:
        assert set(range(0, n, K.T)) <= set(heads)
    elif shape == "last_row" and n > 1:
        assert heads[-1] == n - 1
    elif shape == "three_tiles" and n > 4 * K.T:
        assert [int(h) for h in heads if h <= 4 * K.T] == [0, K.T // 2, K.T // 2 + 3 * K.T + 7]       # tiles 1 and 2 hold no head
    elif shape == "peer_straddle" and n > K.T:
        dense = got["dense_rank"].values
        assert all(dense[t] == dense[t - 1] and rows[t] != 1 for t in range(K.T, n, K.T))


# ---- float sums: exact inputs bit for bit (above), positive uniform inputs within the gate, and the same bits twice ------------------------

UNIFORM = [W("SUM", "u", "sum_rows", frame="ROWS_TO_CURRENT"), W("SUM", "u", "sum_range"), W("AVG", "u", "avg_part", frame="PARTITION"),
           W("AVG", "u", "avg_rows", frame="ROWS_TO_CURRENT"), W("ROW_NUMBER", None, "row_number")]


@pytest.mark.parametrize("n, shape", [(3 * K.T + 1, "three_tiles"), (3 * K.T + 1, "tile_ends"), (K.S + 1, "one_partition")])
def test_float_sums_of_positive_inputs_within_the_gate(ctx, n, shape):
    batch = K.table(n, shape, seed=5)
    check(ctx, [batch], [col("p")], [asc("o")], UNIFORM, within_gate=["sum_rows", "sum_range", "avg_part", "avg_rows"])


def test_the_same_plan_twice_gives_the_same_bits(ctx):
    batch = K.table(K.S + 1, "three_tiles", seed=11)
    m = helpers.memory_exec(ctx, [split(batch, [1000, 70000])])
    plan = ba.WindowAggExec([col("p")], [asc("o")], UNIFORM, m)
    a, b = (helpers.concat(helpers.collect_product(plan)) for _ in range(2))
    for name in ("sum_rows", "sum_range", "avg_part", "avg_rows"):
        assert np.array_equal(a[name].values.view(np.uint64), b[name].values.view(np.uint64)), name
    # ... and a fresh plan over the rows handed over in other batches: the order of the additions depends on the row positions alone
    c = helpers.concat(helpers.collect_product(ba.WindowAggExec([col("p")], [asc("o")], UNIFORM, helpers.memory_exec(ctx, [[batch]]))))
    assert np.array_equal(a["sum_rows"].values.view(np.uint64), c["sum_rows"].values.view(np.uint64))


# ---- keys: NULLs, strings, expressions, directions ---------------------------------------------------------------------------------------------

def keyed_table(n, seed):
    rng = np.random.default_rng(seed)
    return OrderedDict([("p", OCol("Int64", rng.integers(0, 6, n), rng.random(n) > 0.1)),
                        ("q", OCol("Utf8", [["north", "South", "north-by-northwest", "", "NORTH"][v] for v in rng.integers(0, 5, n)], rng.random(n) > 0.15)),
                        ("o", OCol("Int32", rng.integers(-5, 12, n).astype(np.int32), rng.random(n) > 0.1)),
                        ("x", OCol("Int64", rng.integers(-10**9, 10**9, n), rng.random(n) > 0.2)),
                        ("s", OCol("Utf8", ["t%d" % v for v in rng.integers(0, 40, n)], rng.random(n) > 0.2)),
                        ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])


KEYED = [W("ROW_NUMBER", None, "row_number"), W("RANK", None, "rank"), W("DENSE_RANK", None, "dense_rank"), W("LAG", "s", "lag_s", 1),
         W("LEAD", "s", "lead_s", 2), W("LAG", "x", "lag0", 0), W("LAG", "x", "lag_far", 5000), W("FIRST_VALUE", "s", "first_s"), W("LAST_VALUE", "s", "last_s"),
         W("LAST_VALUE", "q", "last_q", frame="PARTITION"), W("SUM", "x", "sum_x"), W("COUNT", "s", "count_s", frame="ROWS_TO_CURRENT"),
         E.count_star("count_star", "PARTITION"), W("MIN", "x", "min_x", frame="ROWS_TO_CURRENT"), W("AVG", "x", "avg_x", frame="PARTITION")]


@pytest.mark.parametrize("spec", ["utf8_and_int_keys", "desc_nulls_last", "two_order_keys", "no_order", "nothing", "expression_keys"])
@pytest.mark.parametrize("n", [300, 2 * K.T + 5])
def test_null_string_and_expression_keys(ctx, n, spec):
    lower_q = E.ScalarFunctionExpr("lower", [col("q")])
    partition_by, order_by = {
        "utf8_and_int_keys": ([col("q"), col("p")], [asc("o")]),
        "desc_nulls_last": ([col("p")], [asc("o", True, False)]),
        "two_order_keys": ([], [asc("o", False, False), asc("s", True, True)]),
        "no_order": ([col("q")], []),
        "nothing": ([], []),
        "expression_keys": ([lower_q], [asc(col("o") + col("o"))]),
    }[spec]
    ws = KEYED + ([W("LAG", lower_q, "lag_lower", 1)] if spec == "expression_keys" else [])
    got = check(ctx, split(keyed_table(n, seed=n), [n // 2]), partition_by, order_by, ws)
    if not order_by:
        assert set(got["rank"].values) == {1} and set(got["dense_rank"].values) == {1}


# ---- float specials as partition keys, as order keys and as MIN / MAX arguments ---------------------------------------------------------------

def special_table(dtype, n=400):
    rng = np.random.default_rng(n)
    return OrderedDict([("f", sort_cases.float_special_column(dtype, n, rng)), ("t", OCol("Int32", rng.integers(0, 4, n).astype(np.int32))),
                        ("x", OCol("Int64", rng.integers(-100, 100, n))), ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])


@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_float_specials_as_keys_and_arguments(ctx, dtype):
    batch = special_table(dtype)
    # partition keys: every bit pattern its own partition (-0.0 / +0.0, each NaN payload), the NULLs one partition
    got = check(ctx, [batch], [col("f")], [], [E.count_star("rows"), W("ROW_NUMBER", None, "row_number"), W("SUM", "x", "sum_x")])
    ut = np.uint64 if dtype == "Float64" else np.uint32
    bits, valid = got["f"].values.view(ut), got["f"].is_valid()
    seen = 0
    for b in sort_cases.special_bits(dtype):
        here = valid & (bits == b)                        # (two rows each, less what the NULLs took)
        if here.any():
            assert set(got["rows"].values[here]) == {int(here.sum())}, hex(int(b))
            seen += 1
    assert seen >= 20
    assert set(got["rows"].values[~valid]) == {int((~valid).sum())}
    # order keys, both directions: peers by bit pattern
    for desc, nulls_first in [(False, True), (True, False)]:
        check(ctx, [batch], [col("t")], [asc("f", desc, nulls_first)],
              [W("RANK", None, "rank"), W("DENSE_RANK", None, "dense_rank"), W("COUNT", "x", "upto"), W("LAST_VALUE", "rn", "last_peer")])
    # arguments of MIN / MAX: a NaN only while nothing else is there; either zero may come back
    names = ["min_rows", "max_rows", "min_part", "max_range"]
    check(ctx, [batch], [col("t")], [asc("x")],
          [W("MIN", "f", "min_rows", frame="ROWS_TO_CURRENT"), W("MAX", "f", "max_rows", frame="ROWS_TO_CURRENT"), W("MIN", "f", "min_part", frame="PARTITION"),
           W("MAX", "f", "max_range"), W("LAG", "f", "lag_f", 1), W("FIRST_VALUE", "f", "first_f")], any_zero_sign=names)


def test_min_max_over_nans_alone_and_all_null_frames(ctx):
    nan = np.nan
    f = OCol("Float64", [nan, 1.0, nan, -2.0, nan, nan, 3.0, 4.0], np.array([True, True, True, True, False, True, False, False]))
    batch = OrderedDict([("p", OCol("Int32", np.array([0, 0, 0, 0, 1, 1, 2, 2], np.int32))), ("f", f), ("rn", OCol("Int64", np.arange(8, dtype=np.int64)))])
    ws = [W(fun, "f", f"{fun}_{frame}", frame=frame) for fun in K.AGGREGATES for frame in ("ROWS_TO_CURRENT", "PARTITION")]
    got = check(ctx, [batch], [col("p")], [asc("rn")], ws)
    assert got["MIN_ROWS_TO_CURRENT"].to_pylist()[1:4] == [1.0, 1.0, -2.0] and np.isnan(got["MIN_ROWS_TO_CURRENT"].values[0])
    assert got["MAX_PARTITION"].to_pylist()[6:] == [None, None] and got["COUNT_PARTITION"].to_pylist() == [4, 4, 4, 4, 1, 1, 0, 0]
    assert got["SUM_PARTITION"].to_pylist()[6:] == [None, None] and got["AVG_ROWS_TO_CURRENT"].to_pylist()[4] is None


# ---- every argument type in one table -------------------------------------------------------------------------------------------------------

def test_every_argument_type(ctx):
    batch = K.every_type_table(700, seed=3)
    ws = K.every_type_exprs(batch)
    for lo in range(0, len(ws), 40):                      # a few operators rather than one of 150 columns
        check(ctx, split(batch, [256]), [col("p")], [asc("o")], ws[lo:lo + 40], within_gate=[w.name for w in ws[lo:lo + 40] if w.name == "avg_UInt64"])


def test_uint64_above_2_63_and_wrapping_sums(ctx):
    u = OCol("UInt64", np.array([2**63, 2**63, 5, 2**64 - 1], np.uint64))
    i = OCol("Int64", np.array([2**63 - 1, 1, -2**63, -1], np.int64))
    got = check(ctx, [OrderedDict([("u", u), ("i", i), ("rn", OCol("Int64", np.arange(4, dtype=np.int64)))])], [], [asc("rn")],
                [W("SUM", "u", "su", frame="ROWS_TO_CURRENT"), W("MAX", "u", "mu", frame="ROWS_TO_CURRENT"), W("MIN", "u", "nu", frame="ROWS_TO_CURRENT"),
                 W("SUM", "i", "si", frame="ROWS_TO_CURRENT"), W("MIN", "i", "ni", frame="ROWS_TO_CURRENT"), W("MAX", "i", "xi")])
    assert got["su"].to_pylist() == [2**63, 0, 5, 4] and got["mu"].to_pylist() == [2**63, 2**63, 2**63, 2**64 - 1]
    assert got["si"].to_pylist() == [2**63 - 1, -2**63, 0, -1] and got["nu"].to_pylist() == [2**63, 2**63, 5, 5]


# ---- stacked operators, empty input, more than one input partition ---------------------------------------------------------------------------------

def test_two_stacked_operators_with_different_specifications(ctx):
    batch = K.table(2 * K.T + 9, "tile_ends", seed=2, strings=True)
    m = helpers.memory_exec(ctx, [split(batch, [700])])
    spec1 = ([col("p")], [asc("o")], [W("ROW_NUMBER", None, "r1"), W("SUM", "f", "run1", frame="ROWS_TO_CURRENT")])
    spec2 = ([col("s")], [asc("r1", True, False), asc("rn")], [W("SUM", "r1", "sum_r1", frame="ROWS_TO_CURRENT"), W("LAG", "run1", "lag_run1", 1),
                                                              W("RANK", None, "r2"), W("MAX", "run1", "max_run1")])
    plan = ba.WindowAggExec(*spec2, ba.WindowAggExec(*spec1, m))
    got = helpers.concat(helpers.collect_product(plan))
    want = K.restate(K.sorted_input(batch, *spec1[:2]), *spec1)
    want = K.restate(K.sorted_input(want, *spec2[:2]), *spec2)
    helpers.assert_bit_exact(got, want)
    assert "WindowAggExec" in plan.display().split("\n")[1]


def test_empty_input_gives_no_rows(ctx):
    empty = K.table(0, "one_partition", seed=1)
    for batches in ([empty], [empty, empty]):
        plan = ba.WindowAggExec([col("p")], [asc("o")], K.standard_exprs(), helpers.memory_exec(ctx, [batches]))
        assert sum(og.batch_len(b) for b in helpers.collect_product(plan)) == 0
    # a filter that keeps nothing above real rows
    m = helpers.memory_exec(ctx, [[K.table(100, "tile_ends", seed=1)]])
    plan = ba.WindowAggExec([col("p")], [asc("o")], K.standard_exprs(), ba.FilterExec(col("rn") < E.lit(0), m))
    assert sum(og.batch_len(b) for b in helpers.collect_product(plan)) == 0
    assert [f[0] for f in plan.schema()][-3:] == [w.name for w in K.standard_exprs()][-3:]


def test_two_input_partitions_are_refused_until_merged(ctx):
    batch = K.table(500, "tile_ends", seed=4)
    parts = [[helpers.slice_batch(batch, 0, 200)], [helpers.slice_batch(batch, 200, 500)]]
    ws = [W("ROW_NUMBER", None, "row_number"), W("SUM", "f", "run_f", frame="ROWS_TO_CURRENT")]
    m = helpers.memory_exec(ctx, parts)
    with pytest.raises(ba.PlanError, match="WindowAggExec requires a single input partition: put a MergeExec below it"):
        ba.WindowAggExec([col("p")], [asc("o")], ws, m).collect()
    got = helpers.concat(helpers.collect_product(ba.WindowAggExec([col("p")], [asc("o")], ws, ba.MergeExec(m))))
    helpers.assert_bit_exact(got, K.restate(K.sorted_input(batch, [col("p")], [asc("o")]), [col("p")], [asc("o")], ws))


# ---- every launch has its own name under BHIP_KERNEL_TIMING ------------------------------------------------------------------------------------------

def test_each_launch_is_timed_under_its_own_name():
    mp = pytest.MonkeyPatch()
    mp.setenv("BHIP_KERNEL_TIMING", "2")
    try:
        tctx = ba.Context(0)
    finally:
        mp.undo()
    batch = K.table(3 * K.T + 1, "three_tiles", seed=9)
    tctx.kernel_stats(reset=True)
    check(tctx, [batch], [col("p")], [asc("o")], K.standard_exprs())
    names = set(tctx.kernel_stats(reset=True))
    want = {"window_flags", "window_rank", "window_index", "window_finish", "window_scan_tiles", "window_scan_summaries", "window_scan_apply"}
    want |= {f"window_bounds_{d}_{step}" for d in ("forward", "backward") for step in ("tiles", "summaries", "apply")}
    assert want <= names, sorted(want - names)
