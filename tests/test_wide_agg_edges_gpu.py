"""HashAggregateExec's wide-key route (host/ops_agg_wide.cpp run_wide, kernels_hash.hip wide_key_assign_kernel / wide_keys_equal) and
the string route on top of it, at their edges, against the oracle's evaluation of the same plan.  The cases are wide_agg_cases.py's;
test_wide_agg_cases_cpu.py proves that each is what it says (its pairs of nearly equal keys start at one slot, its collision keys
chain across the table's end, its boundary values straddle the packed key's share by one byte).

Compared unordered by the key columns: keys, counts, integer sums, MIN / MAX bit for bit; Float64 SUM bit for bit too (the arguments
are multiples of 1/8 of small magnitude: every partial sum is exact in any order); AVG within 1e-9.  The route is read from the kernel
list (BHIP_KERNEL_TIMING=2): `wide_key_assign` where a case says wide, absent where it says the key fits."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og
from oracle import plan_eval

import helpers
import wide_agg_cases as W
from test_agg_edges_gpu import ctx, partial  # noqa: F401  (ctx: the module fixture that records every launch by name)

pytestmark = pytest.mark.gpu
AVG_RTOL = 1e-9


def mem(ctx, case):
    return helpers.memory_exec(ctx, case.partitions)


def final_over(group, aggs, below):
    return ba.HashAggregateExec(ba.plan.FINAL, [(col(n), n) for _, n in group], aggs, below)


def final(group, aggs, p):
    return final_over(group, aggs, ba.MergeExec(p))


def run(ctx, plan, key_cols, wide=None, oracle_plan=None):
    """-> (rows, kernel stats).  Every column but an AVG's result compares bit for bit"""
    ctx.kernel_stats(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    stats = ctx.kernel_stats(reset=True)
    want = plan_eval.collect(oracle_plan or plan)
    helpers.assert_rows_equal(got, want, ordered=False, float_rtol=AVG_RTOL, key_cols=key_cols)
    avg = {a.name for a in plan.aggr_expr if a.fun == "AVG"}
    exact = lambda b: OrderedDict((k, c) for k, c in b.items() if k not in avg)
    helpers.assert_rows_equal(exact(got), exact(want), ordered=False, float_rtol=0.0, key_cols=key_cols)
    if wide is not None:
        assert ("wide_key_assign" in stats) == wide, sorted(stats)
    return got, stats


def n_rows(batch):
    return og.batch_len(batch) if batch else 0


def same_rows(a, b, key_cols):
    helpers.assert_rows_equal(a, b, ordered=False, float_rtol=0.0, key_cols=key_cols)


# ---- A. equality, column by column ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", W.EQUALITY_CASES, ids=lambda c: c.name)
def test_equal_keys_only_by_every_bit_of_every_column(ctx, case):
    """pairs of keys that differ in one column by one step — the lowest bit, the sign, -0.0 / +0.0, a NaN's payload, NULL / 0, "" / NULL,
    a prefix, the last byte of 40 — and start at ONE slot: each stays its own group, with its own COUNT and SUM of row numbers"""
    keys = W.keys_of(case)
    got, _ = run(ctx, partial(case.group, case.aggs, mem(ctx, case)), keys, wide=True)
    assert n_rows(got) == case.facts["n_groups"]
    # ... and through Final over two partitions that both hold every key
    t = W.table_of(case)
    n = og.batch_len(t)
    p = partial(case.group, case.aggs, helpers.memory_exec(ctx, [[b] for b in W.cut(t, [n // 2, n - n // 2])]))
    got, _ = run(ctx, final(case.group, case.aggs, p), keys, wide=True)
    assert n_rows(got) == case.facts["n_groups"]


def test_equal_keys_in_arrow_slices_at_a_bit_offset(ctx):
    """the key columns imported from Arrow arrays sliced at bit 3 of their bitmaps, nonsense under the NULLs: two NULL keys with different
    bytes under them are one group"""
    rb, case = W.arrow_slice_case()
    m = ba.MemoryExec([[ba.RecordBatch.from_pyarrow(ctx, rb)]], ctx)
    m._oracle_partitions = case.partitions
    assert [t for _, t, _ in m.schema()] == ["Int32", "Boolean", "Utf8", "Utf8", "Int64"]
    got, _ = run(ctx, partial(case.group, case.aggs, m), W.keys_of(case), wide=True)
    assert n_rows(got) == case.facts["n_groups"]


# ---- B. collisions ----------------------------------------------------------------------------------------------------------------------------------

def test_probe_chain_wraps_past_the_end_of_the_table(ctx):
    """72 distinct keys whose chain starts at slot 1022 / 1023 of 1024 and runs on past slot 0"""
    case = W.slot_collision_case()
    got, _ = run(ctx, partial(case.group, case.aggs, mem(ctx, case)), W.keys_of(case), wide=True)
    assert n_rows(got) == W.COLLISION_KEYS
    assert sorted(got["rn_count[count]"].values.tolist()) == sorted(4 + i % 3 for i in range(W.COLLISION_KEYS))


@pytest.mark.parametrize("case", W.equal_hash_cases(), ids=lambda c: c.name)
def test_equal_row_hashes_are_not_equal_keys(ctx, case):
    """(+0.0, b, c) / (-0.0, b, c) and (NULL, b, c) / (0x6E756C6C6E756C6C, b, c) hash alike: each is its own group"""
    got, _ = run(ctx, partial(case.group, case.aggs, mem(ctx, case)), W.keys_of(case), wide=True)
    assert n_rows(got) == 5


# ---- C. sizes and contention ------------------------------------------------------------------------------------------------------------------------

def run_size_case(ctx, case):
    keys = W.keys_of(case)
    got, stats = run(ctx, partial(case.group, case.aggs, mem(ctx, case)), keys, wide=True)
    assert n_rows(got) == case.facts["n_groups"]
    return stats


@pytest.mark.parametrize("n", W.SIZES)
def test_sizes_around_the_capacity_step_and_the_hint_switch(ctx, n):
    """512 / 513 rows: the table doubles; 4096: the inner aggregate starts on the device-wide table.  One group (every lane claims one
    slot), every row its own (the table half full), two alternating, about sqrt(n) shuffled; an empty batch between two others"""
    for shape in W.SHAPES:
        case = W.size_case(shape, n)
        stats = run_size_case(ctx, case)
        if case.facts["hash_inner"]:
            assert "hash_agg_init" in stats, (shape, sorted(stats))
        elif shape in ("one_group", "two_alternating"):                      # at most two groups below the switch: the register path
            assert "hash_agg_init" not in stats, (shape, sorted(stats))


@pytest.mark.parametrize("shape", ["one_group", "all_distinct"])
def test_more_rows_than_one_grid_stride_step(ctx, shape):
    stats = run_size_case(ctx, W.size_case(shape, W.BIG))
    assert "hash_agg_init" in stats


# ---- D. the fall-over ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", W.FALLOVER_WHERE)
@pytest.mark.parametrize("layout", list(W.LAYOUTS))
def test_one_byte_more_than_the_share_falls_over(ctx, layout, where):
    """a value that just fits its share of the packed key stays packed; one byte more — in row 0, in the last row of the last batch, in a
    row a FilterExec removes, in partition 1 only, behind a partition that taught the operator a register-path hint — goes wide.  The same
    operator collected again (wide_keys_ now set) gives the same rows"""
    case = W.fallover_case(layout, where)
    keys = W.keys_of(case)
    src = mem(ctx, case)
    if case.facts["filtered"]:
        src = ba.FilterExec(W.KEEP, src)
    p = partial(case.group, case.aggs, src)
    first, _ = run(ctx, p, keys, wide=case.facts["wide"])
    again, _ = run(ctx, p, keys, wide=case.facts["wide"])
    same_rows(first, again, keys)
    fit = "F" * case.facts["fits"]
    longest = max(len(s) for s in first["s"].values)
    assert longest == len(fit) + (0 if where in ("fits", "filtered") else 1)
    if where == "partition_1":                                               # Partial (a fresh one) -> Merge -> Final
        f = final(case.group, case.aggs, partial(case.group, case.aggs, mem(ctx, case)))
        got, _ = run(ctx, f, keys, wide=True)
        again, _ = run(ctx, f, keys, wide=True)
        same_rows(got, again, keys)


def test_over_long_value_behind_the_head_sample(ctx):
    """2^17 + 1 rows, six accumulators: the ladder reads its 32 768-row head first, and the only over-long key is the last row's"""
    case = W.head_sample_case()
    got, _ = run(ctx, partial(case.group, case.aggs, mem(ctx, case)), ["s"], wide=True)
    assert sorted(got["s"].values.tolist()) == ["A", "B", "C", "F" * 16]


# ---- E. modes ----------------------------------------------------------------------------------------------------------------------------------------------

def null_group_rows(got):
    return np.array([s.endswith("%02d" % W.NULL_GROUP) for s in got["s"].values])


def test_partial_alone_and_final_over_two_partitions(ctx):
    keys = ["s", "i"]
    p1 = partial(W.MODE_KEYS, W.MODE_AGGS, helpers.memory_exec(ctx, W.mode_partitions(1)))
    got, _ = run(ctx, p1, keys, wide=True)
    dead = null_group_rows(got)
    assert dead.any() and not got["az[sum]"].is_valid()[dead].any() and (got["az[count]"].values[dead] == 0).all()
    p2 = partial(W.MODE_KEYS, W.MODE_AGGS, helpers.memory_exec(ctx, W.mode_partitions(2)))
    part, _ = run(ctx, p2, keys, wide=True)
    whole, _ = run(ctx, final(W.MODE_KEYS, W.MODE_AGGS, p2), keys, wide=True)
    assert n_rows(part) > n_rows(whole) == n_rows(got)                       # the same wide keys in both partitions' states


@pytest.mark.parametrize("coalesce", [False, True], ids=["merge", "merge_coalesce"])
def test_final_over_one_wide_partial_projects_its_state_batch(ctx, coalesce):
    """Final over MergeExec over a ONE-partition Partial with wide keys: run_single_partial projects the Partial's state batch and makes
    AVG as [sum] / CAST([count] AS Float64).  `wide_key_assign` is launched once per collect (by the Partial): the Final aggregated
    nothing a second time.  The first collect makes the packed attempt and flips the Partial's flag, the second finds it set.  The group
    whose arguments are all NULL: AVG and SUM NULL (not NaN), COUNT 0"""
    keys = ["s", "i"]
    p = partial(W.MODE_KEYS, W.MODE_AGGS, helpers.memory_exec(ctx, W.mode_partitions(1)))
    below = ba.MergeExec(p)
    if coalesce:
        below = ba.CoalesceBatchesExec(below, 4096)
    f = final_over(W.MODE_KEYS, W.MODE_AGGS, below)
    results = []
    for _ in range(2):
        got, stats = run(ctx, f, keys, wide=True)
        assert stats["wide_key_assign"][1] == 1, stats["wide_key_assign"]
        dead = null_group_rows(got)
        assert dead.any()
        for name in ("ax", "ay", "az", "sz", "sx"):
            assert not got[name].is_valid()[dead].any(), name
            assert got[name].is_valid()[~dead].all(), name
        assert (got["cz"].values[dead] == 0).all() and (got["cz"].values[~dead] > 0).all()
        assert [got[n].dtype for n in ("ax", "ay", "az")] == ["Float64"] * 3
        results.append(got)
    same_rows(results[0], results[1], keys)


def test_final_over_one_wide_partial_with_a_string_minimum(ctx):
    """MIN(Utf8) among the aggregates: the Partial is a string aggregate and the elision is turned down — the Final aggregates the state
    rows itself (a second wide_key_assign) and agrees all the same"""
    keys = ["s", "i"]
    p = partial(W.MODE_KEYS, W.MODE_STRING_AGGS, helpers.memory_exec(ctx, W.mode_partitions(1)))
    f = final(W.MODE_KEYS, W.MODE_STRING_AGGS, p)
    for _ in range(2):
        got, stats = run(ctx, f, keys, wide=True)
        assert stats["wide_key_assign"][1] == 2 and "rank_to_row" in stats, sorted(stats)
    plain, _ = run(ctx, final(W.MODE_KEYS, W.MODE_AGGS, partial(W.MODE_KEYS, W.MODE_AGGS, helpers.memory_exec(ctx, W.mode_partitions(1)))), keys)
    same_rows(OrderedDict((k, got[k]) for k in plain), plain, keys)


# ---- F. strings on top ---------------------------------------------------------------------------------------------------------------------------------------

def test_string_min_max_grouped_by_a_wide_key(ctx):
    """run_strings ranks the strings, its inner aggregate falls over to run_wide: a group with only NULL strings, equal strings in
    several rows, "", bytes >= 0x80 — and the same through Final"""
    t = W.string_minmax_table()
    n = og.batch_len(t)
    keys = ["s", "i"]
    p = partial(W.MODE_KEYS, W.STRING_AGGS, helpers.memory_exec(ctx, [[b] for b in W.cut(t, [n // 3, n - n // 3])]))
    got, stats = run(ctx, p, keys, wide=True)
    assert "rank_to_row" in stats
    got, stats = run(ctx, final(W.MODE_KEYS, W.STRING_AGGS, p), keys, wide=True)
    assert "rank_to_row" in stats and n_rows(got) == len(W.STRING_GROUPS)
    by_group = dict(zip(got["s"].values.tolist(), zip(got["m_min"].to_pylist(), got["m_max"].to_pylist(), got["m_count"].to_pylist())))
    name = lambda g: "the group of strings number %02d" % g
    assert by_group[name(0)] == (None, None, 0) and by_group[name(1)] == ("same", "same", 18) and by_group[name(3)] == ("", "", 12)
    assert by_group[name(2)][:2] == ("", "a") and by_group[name(4)][:2] == ("z", "ÿ")


@pytest.mark.parametrize("name", list(W.STRING_EXPR_KEYS))
def test_string_expression_keys_that_outgrow_the_packed_key(ctx, name):
    """GROUP BY lower(a) / trim(b) / both / concat(a, b): the lowered key column is longer than 15 bytes, the inner aggregate goes wide.
    (The oracle has no concat: it groups by the column the cases module worked out with Python's str)"""
    device_keys, oracle_keys = W.STRING_EXPR_KEYS[name]
    t = W.string_expr_table()
    m = helpers.memory_exec(ctx, [[b] for b in W.cut(t, [100, W.EXPR_ROWS - 100])])
    keys = [n for _, n in device_keys]
    p, po = partial(device_keys, W.VALUE_AGGS, m), partial(oracle_keys, W.VALUE_AGGS, m)
    run(ctx, p, keys, wide=True, oracle_plan=po)
    run(ctx, final(device_keys, W.VALUE_AGGS, p), keys, wide=True, oracle_plan=final(oracle_keys, W.VALUE_AGGS, po))


@pytest.mark.parametrize("grouped", [True, False])
def test_string_aggregate_over_an_empty_input(ctx, grouped):
    """no rows with a group key, one row of NULLs (COUNT 0) without one — Partial and Final"""
    empty = W.cut(W.string_expr_table(), [0, W.EXPR_ROWS])[0]
    group = [(W.fn("lower", col("a")), "k")] if grouped else []
    aggs = [E.Min(col("a"), "mn"), E.Count(col("a"), "c"), E.Sum(col("v"), "s")]
    p = partial(group, aggs, helpers.memory_exec(ctx, [[empty]]))
    for plan in (p, final(group, aggs, p)):
        got, _ = run(ctx, plan, [n for _, n in group] or None)
        if grouped:
            assert n_rows(got) == 0
        else:
            assert [c.to_pylist() for c in got.values()] == [[None], [0], [None]]


# ---- G. limits ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_sixteen_group_expressions(ctx):
    """16 group expressions are the route's limit (WideKeyCols): their row hash is made in two passes of 8 key parts.  Groups that differ
    only in a column past the eighth stay apart"""
    case = W.many_keys_case(16)
    keys = W.keys_of(case)
    p = partial(case.group, case.aggs, mem(ctx, case))
    got, stats = run(ctx, p, keys, wide=True)
    assert stats["scan_keys"][1] >= 2, stats["scan_keys"]
    got, _ = run(ctx, final(case.group, case.aggs, p), keys, wide=True)
    assert n_rows(got) == case.facts["n_groups"]


def test_seventeen_group_expressions_are_refused(ctx):
    case = W.many_keys_case(17)
    with pytest.raises(ba.NotImplementedOnGpu, match=W.MESSAGES["too_many"]):
        partial(case.group, case.aggs, mem(ctx, case)).collect()


def test_reserved_column_name(ctx):
    """the route adds a column __group_rep to its inner aggregate's input: an input that has one already is refused"""
    case = W.size_case("sqrt_groups", 65)
    t = W.table_of(case)
    t["__group_rep"] = t["b"]
    with pytest.raises(ba.PlanError, match=W.MESSAGES["reserved"]):
        partial(case.group, case.aggs, helpers.memory_exec(ctx, [[t]])).collect()


def test_every_row_filtered_away(ctx):
    case = W.size_case("sqrt_groups", 513)
    p = partial(case.group, case.aggs, ba.FilterExec(col("v") > lit(100.0), mem(ctx, case)))
    for plan in (p, final(case.group, case.aggs, p)):
        got, _ = run(ctx, plan, W.keys_of(case))
        assert n_rows(got) == 0
