"""HashAggregateExec's Single mode and COUNT / SUM / AVG (DISTINCT x) (host/ops_agg_wide.cpp run_single, kernels_hash.hip
distinct_claim_kernel / distinct_mark_kernel) at their edges.  The cases and the expected numbers are distinct_agg_cases.py's — the
definition in plain Python: per group, the set of (type, bits or bytes) of the non-NULL x — and test_distinct_agg_cases_cpu.py proves
that each case is what it says.  Where a second opinion helps, the oracle evaluates the two-level rewrite (GROUP BY k, x; then COUNT(x)
GROUP BY k) of the same input.

Compared unordered by the key columns: counts and integer sums bit for bit, AVG_DISTINCT within 1e-9.  The route is read from the kernel
list (BHIP_KERNEL_TIMING=2): `distinct_claim` / `distinct_mark` once per different DISTINCT argument, `wide_key_assign` where the group
key does not fit the packed key."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L
from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle import engine as og
from oracle import plan_eval
from oracle.engine import OCol

import helpers
import distinct_agg_cases as D
from test_agg_edges_gpu import ctx  # noqa: F401  (the module fixture that records every launch by name)

pytestmark = pytest.mark.gpu
AVG_RTOL = 1e-9                                           # what the existing edge tests give an AVG
P = ba.plan


def single(group, aggs, m):
    return ba.HashAggregateExec(P.SINGLE, group, aggs, m)


def final_over_partial(group, aggs, m):
    names = {"SUM": "[sum]", "COUNT": "[count]", "MIN": "[min]", "MAX": "[max]", "AVG": "[count]"}
    part = ba.HashAggregateExec(P.PARTIAL, group, aggs, m)
    return ba.HashAggregateExec(P.FINAL, [(col(n), n) for _, n in group], [E.AggregateExpr(a.fun, col(a.name + names[a.fun]), a.name) for a in aggs],
                                ba.MergeExec(part))


def collect(ctx, plan):
    ctx.kernel_stats(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    return got, ctx.kernel_stats(reset=True)


def launches(stats, name):
    return stats[name][1] if name in stats else 0


def compare(got, want, keys, aggs):
    """the columns of `want` in `got`: everything but an AVG_DISTINCT bit for bit"""
    if got:
        assert list(got) == keys + [a.name for a in aggs], list(got)
    sub = OrderedDict((k, got[k]) for k in want) if got else got
    helpers.assert_rows_equal(sub, want, ordered=False, float_rtol=AVG_RTOL, key_cols=keys)
    avg = {a.name for a in aggs if a.fun == "AVG_DISTINCT"}
    exact = lambda b: OrderedDict((k, c) for k, c in b.items() if k not in avg)
    helpers.assert_rows_equal(exact(sub), exact(want), ordered=False, float_rtol=0.0, key_cols=keys)


def run_case(ctx, case, want=None, n_args=1):
    m = helpers.memory_exec(ctx, [[case.table]])
    got, stats = collect(ctx, single(case.group, case.aggs, m))
    compare(got, want or D.expected(case), D.keys_of(case), case.aggs)
    assert launches(stats, "distinct_claim") == launches(stats, "distinct_mark") == (n_args if og.batch_len(case.table) else 0), sorted(stats)
    return got, stats, m


# ---- the interface -----------------------------------------------------------------------------------------------------------------------------

def test_schema_display_and_with_new_children(ctx):
    c = D.null_case("some")
    m = helpers.memory_exec(ctx, [[c.table]])
    plan = single(c.group, c.aggs + [E.Count(col("x"), "n"), E.Avg(col("x"), "a")], m)
    assert [(n, t, bool(nullable)) for n, t, nullable in plan.schema()] == [
        ("k", "Int32", False), ("cd", "UInt64", False), ("sd", "Int64", True), ("ad", "Float64", True), ("n", "UInt64", False), ("a", "Float64", True)]
    text = plan.display()
    assert "mode=Single" in text and "COUNT(DISTINCT x)" in text and "SUM(DISTINCT x)" in text and "AVG(DISTINCT x)" in text, text
    assert plan.output_partitioning().partition_count() == 1
    assert (E.CountDistinct(col("x"), "c").fun, E.SumDistinct(col("x"), "c").fun, E.AvgDistinct(col("x"), "c").fun) == D.DISTINCT_FUNS
    again = plan.with_new_children([m])
    assert again.display() == text
    compare(helpers.concat(helpers.collect_product(again)), D.expected(c), ["k"], plan.aggr_expr)


# ---- A / B. ballot words, blocks, table size ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", D.BALLOT_VARIANTS)
@pytest.mark.parametrize("n", D.BALLOT_SIZES)
def test_rows_around_every_validity_word_and_block_edge(ctx, n, variant):
    """duplicates that straddle rows 63 / 64, 127 / 128, 255 / 256; the last row a duplicate or a first occurrence: its bit is in a word
    that is written whole, rows past n contributing 0"""
    run_case(ctx, D.ballot_case(n, variant))


@pytest.mark.parametrize("shape", D.TABLE_SHAPES)
@pytest.mark.parametrize("n", D.TABLE_SIZES)
def test_rows_on_both_sides_of_the_table_capacity_step(ctx, n, shape):
    """512 rows fill half of 1024 slots, 513 take 2048; all distinct (every row claims a slot) and all equal (every row lowers one word)"""
    run_case(ctx, D.table_case(n, shape))


# ---- C. equality ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", list(D.EQUALITY_VALUES))
def test_values_one_step_apart_are_two_values_and_duplicates_one(ctx, dtype):
    """the lowest bit, the sign, -0.0 / +0.0, two NaN payloads; Boolean; "" / a prefix / 40 bytes that differ in the last"""
    c = D.equality_case(dtype)
    got, _, _ = run_case(ctx, c)
    assert dict(zip(got["k"].to_pylist(), got["cd"].to_pylist())) == c.facts["counts"]


# ---- D. the group key in the comparison ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["packed", "wide"])
def test_equal_values_in_two_groups_count_in_both(ctx, route):
    """... the NULL group key is one group; a Utf8 key too long for the packed key sends the inner aggregate down the wide-key route, a
    short integer key does not, and the counts are right on both"""
    c = D.group_key_case(route)
    got, stats, m = run_case(ctx, c)
    assert ("wide_key_assign" in stats) == c.facts["wide"], sorted(stats)
    # the oracle on the two-level rewrite
    want = plan_eval.collect(D.two_level(m, ["k"], "x", "cd"))
    helpers.assert_rows_equal(OrderedDict((k, got[k]) for k in ("k", "cd")), want, ordered=False, key_cols=["k"])


# ---- E. NULL arguments -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["some", "all"])
def test_null_arguments_are_no_values(ctx, shape):
    """a group with only NULL x: COUNT_DISTINCT 0, SUM_DISTINCT / AVG_DISTINCT NULL; a group with one value and NULLs; x entirely NULL"""
    got, _, _ = run_case(ctx, D.null_case(shape))
    if shape == "all":
        assert got["cd"].to_pylist() == [0, 0, 0] and got["sd"].to_pylist() == [None] * 3 and got["ad"].to_pylist() == [None] * 3


# ---- F. several aggregates -------------------------------------------------------------------------------------------------------------------------

def test_distinct_and_plain_aggregates_in_one_operator(ctx):
    """COUNT_DISTINCT(a), COUNT_DISTINCT(b), SUM_DISTINCT(a), AVG_DISTINCT(a), SUM(y), COUNT(y), MIN(y): `a` is marked once — two claim
    and two mark launches — and the plain aggregates are those of Final over Partial on the same input, bit for bit"""
    c = D.mixed_case()
    got, _, m = run_case(ctx, c, n_args=2)
    plain = [a for a in c.aggs if a.fun not in D.DISTINCT_FUNS]
    want = helpers.concat(helpers.collect_product(final_over_partial(c.group, plain, m)))
    names = ["k"] + [a.name for a in plain]
    helpers.assert_rows_equal(OrderedDict((k, got[k]) for k in names), want, ordered=False, float_rtol=0.0, key_cols=["k"])


# ---- G. no GROUP BY --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [100, 0])
def test_no_group_by(ctx, n):
    """one row; on empty input COUNT_DISTINCT 0 and NULL sums, as Final over Partial gives a COUNT there"""
    got, _, m = run_case(ctx, D.no_group_case(n))
    assert og.batch_len(got) == 1
    plain = helpers.concat(helpers.collect_product(final_over_partial([], [E.Count(col("x"), "c")], m)))
    assert og.batch_len(plain) == 1 and plain["c"].dtype == got["cd"].dtype


# ---- Single without DISTINCT -----------------------------------------------------------------------------------------------------------------------

def test_single_without_distinct_is_final_over_partial(ctx):
    c = D.mixed_case()
    m = helpers.memory_exec(ctx, [[c.table]])
    aggs = [E.Sum(col("y"), "s"), E.Avg(col("a"), "av"), E.Count(col("b"), "n"), E.Min(col("y"), "lo"), E.Max(col("b"), "hi")]
    got, stats = collect(ctx, single(c.group, aggs, m))
    assert not [k for k in stats if k.startswith("distinct_")], sorted(stats)
    want = helpers.concat(helpers.collect_product(final_over_partial(c.group, aggs, m)))
    helpers.assert_rows_equal(got, want, ordered=False, float_rtol=0.0, key_cols=["k"])
    assert og.batch_len(got) == 5


# ---- partitions --------------------------------------------------------------------------------------------------------------------------------------

def two_partitions(ctx, case):
    n = og.batch_len(case.table)
    return helpers.memory_exec(ctx, [[b] for b in D.W.cut(case.table, [n // 3, n - n // 3])])


def test_hash_partitioned_input_is_aggregated_partition_by_partition(ctx):
    c = D.mixed_case()
    m2 = two_partitions(ctx, c)
    plan = single(c.group, c.aggs, ba.RepartitionExec(m2, P.Partitioning.Hash([col("k")], 2)))
    assert plan.output_partitioning().partition_count() == 2
    got, stats = collect(ctx, plan)
    compare(got, D.expected(c), ["k"], c.aggs)             # the union of the two outputs is the one-partition answer
    assert launches(stats, "distinct_claim") == 4          # two arguments in each of two partitions
    # ... and without a DISTINCT: a partition's rows alone
    plain = [E.Sum(col("y"), "s"), E.Count(col("y"), "n")]
    got, _ = collect(ctx, single(c.group, plain, ba.RepartitionExec(m2, P.Partitioning.Hash([col("k")], 2))))
    want = helpers.concat(helpers.collect_product(final_over_partial(c.group, plain, helpers.memory_exec(ctx, [[c.table]]))))
    helpers.assert_rows_equal(got, want, ordered=False, float_rtol=0.0, key_cols=["k"])


def test_partitions_that_split_a_group_are_refused(ctx):
    c = D.mixed_case()
    m2 = two_partitions(ctx, c)
    with pytest.raises(L.PlanError) as e:
        single(c.group, c.aggs, m2)
    assert e.value.code == L.EINVAL and "MergeExec" in str(e.value) and "RepartitionExec(Hash" in str(e.value)
    with pytest.raises(L.PlanError) as e:                   # Hash on an expression that is no group expression
        single(c.group, c.aggs, ba.RepartitionExec(m2, P.Partitioning.Hash([col("a")], 2)))
    assert e.value.code == L.EINVAL and "MergeExec" in str(e.value)
    with pytest.raises(L.PlanError):                        # no GROUP BY: the one group lies in both partitions
        single([], c.aggs, ba.RepartitionExec(m2, P.Partitioning.Hash([col("k")], 2)))
    single(c.group, c.aggs, ba.MergeExec(m2))              # what the message names is legal


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------

def ints_table(names, n=4):
    return OrderedDict((name, OCol("Int64", np.arange(n, dtype=np.int64) + i)) for i, name in enumerate(names))


def test_refusals(ctx):
    c = D.null_case("some")
    m = helpers.memory_exec(ctx, [[c.table]])
    for mode in (P.PARTIAL, P.FINAL):
        with pytest.raises(L.NotImplementedOnGpu) as e:
            ba.HashAggregateExec(mode, c.group, [E.CountDistinct(col("x"), "cd")], m)
        assert e.value.code == L.ENOTIMPL and "Single" in str(e.value) and "DISTINCT" in str(e.value)
    # a ninth different argument (eight are taken; the same argument twice counts once)
    cols9 = [f"x{i}" for i in range(9)]
    m9 = helpers.memory_exec(ctx, [[ints_table(["k"] + cols9)]])
    eight = [E.CountDistinct(col(n), "c" + n) for n in cols9[:8]]
    single(D.group_by("k"), eight + [E.SumDistinct(col("x0"), "again")], m9)
    with pytest.raises(L.NotImplementedOnGpu) as e:
        single(D.group_by("k"), eight + [E.CountDistinct(col("x8"), "c8")], m9)
    assert e.value.code == L.ENOTIMPL and "more than 8 different DISTINCT arguments" in str(e.value)
    # a sixteenth group expression beside a DISTINCT (fifteen are taken; sixteen without a DISTINCT too)
    g16 = [f"g{i}" for i in range(16)]
    m16 = helpers.memory_exec(ctx, [[ints_table(g16 + ["x"])]])
    single(D.group_by(*g16[:15]), [E.CountDistinct(col("x"), "cd")], m16)
    single(D.group_by(*g16), [E.Count(col("x"), "n")], m16)
    with pytest.raises(L.NotImplementedOnGpu) as e:
        single(D.group_by(*g16), [E.CountDistinct(col("x"), "cd")], m16)
    assert e.value.code == L.ENOTIMPL and "more than 15 group expressions" in str(e.value)
    # a string function as the argument, or among the group expressions beside a DISTINCT
    ms = helpers.memory_exec(ctx, [[OrderedDict([("s", OCol("Utf8", ["a", "B"])), ("x", OCol("Int64", [1, 2]))])]])
    lower = E.ScalarFunctionExpr("lower", [col("s")])
    with pytest.raises(L.NotImplementedOnGpu) as e:
        single([], [E.CountDistinct(lower, "cd")], ms)
    assert e.value.code == L.ENOTIMPL and "string function" in str(e.value)
    with pytest.raises(L.NotImplementedOnGpu) as e:
        single([(lower, "l")], [E.CountDistinct(col("x"), "cd")], ms)
    assert e.value.code == L.ENOTIMPL and "string function" in str(e.value)
    single([(col("s"), "s")], [E.CountDistinct(col("s"), "cd")], ms)        # plain Utf8 columns stand in both places
    # a reserved column name in the input
    mr = helpers.memory_exec(ctx, [[ints_table(["k", "__distinct_0"])]])
    with pytest.raises(L.PlanError) as e:
        single(D.group_by("k"), [E.CountDistinct(col("k"), "cd")], mr)
    assert e.value.code == L.EINVAL and "reserved" in str(e.value)
    # SUM / AVG (DISTINCT) take what SUM / AVG take
    with pytest.raises(L.PlanError):
        single([], [E.SumDistinct(col("s"), "sd")], ms)


def test_fifteen_group_expressions_and_a_distinct_take_the_second_hash_pass(ctx):
    """16 hashed columns: the row hash of the columns after the eighth is folded in, as on the wide-key route"""
    g15 = [f"g{i}" for i in range(15)]
    n = 200
    rn = np.arange(n, dtype=np.int64)
    t = OrderedDict((g, OCol("Int64", (rn // (i + 1)) % 3)) for i, g in enumerate(g15))
    t["x"] = OCol("Int64", rn % 7, rn % 5 != 0)
    aggs = [E.CountDistinct(col("x"), "cd"), E.SumDistinct(col("x"), "sd")]
    run_case(ctx, D.Case("fifteen_keys", t, D.group_by(*g15), aggs, {}))


# ---- H. more rows than one trip of the grid ----------------------------------------------------------------------------------------------------------

def test_more_rows_than_one_grid_stride_step(ctx):
    """1.2 M rows > 256 CUs x 16 blocks x 256 threads = 1 048 576: both kernels' row loops take a second trip.  1000 groups, values
    drawn from 5000"""
    assert D.GRID_ROWS > D.GRID_LIMIT == 256 * 16 * 256
    c = D.grid_case()
    run_case(ctx, c, want=D.grid_expected())


# ---- I. float sums -------------------------------------------------------------------------------------------------------------------------------------

def test_float_sums_are_the_same_bits_on_every_run(ctx):
    """SUM_DISTINCT(Float64) over multiples of 0.1, every value 2 to 5 times at scattered rows: three runs on fresh plans agree bit for
    bit, and with the set sum in row order within 1e-9 relative.  This cannot force the race it guards against — which of the equal
    rows survives decides the order of the additions; the argument that the survivor is always the smallest row number (the slot word
    only decreases under atomicMin and every equal row takes part) is carried by DESIGN.md §3.4 and the kernel's comment."""
    c = D.float_sum_case()
    want = D.expected(c)
    runs = []
    for _ in range(3):
        got, _, _ = run_case(ctx, c, want=OrderedDict((k, want[k]) for k in ("k", "cd")))
        runs.append(got)
    for other in runs[1:]:
        helpers.assert_rows_equal(other, runs[0], ordered=False, float_rtol=0.0, key_cols=["k"])
    helpers.assert_rows_equal(runs[0], OrderedDict((k, want[k]) for k in ("k", "sd", "cd")), ordered=False, float_rtol=1e-9, key_cols=["k"])


# ---- J. the property ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", ["k_packed", "k_wide"])
def test_count_distinct_is_the_row_count_of_group_by_k_x(ctx, k):
    """on 5000 random rows of mixed types: COUNT_DISTINCT(x) GROUP BY k = per k the rows of this library's own GROUP BY k, x with a
    non-NULL x — for a packed-key k and a wide-key k"""
    t = D.property_table()
    m = helpers.memory_exec(ctx, [[t]])
    aggs = [E.CountDistinct(col(x), "cd_" + x) for x in D.PROPERTY_X]
    got, stats = collect(ctx, single(D.group_by(k), aggs, m))
    assert launches(stats, "distinct_claim") == launches(stats, "distinct_mark") == len(D.PROPERTY_X)
    assert ("wide_key_assign" in stats) == (k == "k_wide"), sorted(stats)
    compare(got, D.expected_table(t, D.group_by(k), aggs), [k], aggs)
    for x in D.PROPERTY_X:
        pairs = helpers.concat(helpers.collect_product(final_over_partial(D.group_by(k, x), [E.Count(col(x), "n")], m)))
        per_k = {}
        for kv, ok in zip(pairs[k].to_pylist(), pairs[x].is_valid()):
            per_k[kv] = per_k.get(kv, 0) + int(ok)
        assert dict(zip(got[k].to_pylist(), got["cd_" + x].to_pylist())) == per_k, x
