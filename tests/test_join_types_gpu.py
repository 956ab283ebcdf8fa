"""GPU parity of HashJoinExec's Full / Semi / Anti / RightSemi / RightAnti join types (kernels_hash.hip: join_probe_exists[_wide],
join_exists_flags[_wide]; Full runs on the kernels Left and Right run on, with both flags).

Expected rows: join_types_cases.expected, derived from the CPU oracle's Inner / Left / Right joins of the same sides and checked
against pyarrow in test_join_types_plan.py.  Rows compare as multisets keyed by the row ids li / ri.  Sizes: 900 build rows in two
partitions; 5000 probe rows as batches of 1025 (one past the 1024-row selection tile), 1975 and 2000 rows — two partitions for
RightSemi / RightAnti, one partition (or two under a MergeExec) for the types that answer for the build side."""
import functools
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og
from oracle.engine import OCol

import helpers
import join_types_cases as JT

pytestmark = pytest.mark.gpu
PROBE_SIDE = (JT.RIGHT_SEMI, JT.RIGHT_ANTI)


def build_exec(ctx, left):
    n = og.batch_len(left)
    cut = min(400, n)
    return helpers.memory_exec(ctx, [[helpers.slice_batch(left, 0, cut)], [helpers.slice_batch(left, cut, n)]])


def probe_exec(ctx, right, partitions):
    """the probe rows cut at JT.CUTS: 2: two partitions (two batches, one batch); 1: one partition; "merge": the two under a MergeExec"""
    n = og.batch_len(right)
    b = [helpers.slice_batch(right, lo, hi) for lo, hi in zip(JT.CUTS, JT.CUTS[1:]) if lo < n or lo == 0]
    if partitions == 1:
        return helpers.memory_exec(ctx, [b])
    two = helpers.memory_exec(ctx, [b[:2], b[2:]])
    return ba.MergeExec(two) if partitions == "merge" else two


def join_plan(ctx, left, right, on, jt, merge=False):
    probe = probe_exec(ctx, right, 2 if jt in PROBE_SIDE else "merge" if merge else 1)
    return ba.HashJoinExec(build_exec(ctx, left), probe, on, jt)


def rows(plan):
    return helpers.concat(helpers.collect_product(plan))


def check(ctx, left, right, on, jt, form=None, merge=False):
    plan = join_plan(ctx, left, right, on, jt, merge)
    got = rows(plan)
    JT.assert_same_rows(got, JT.expected(jt, left, right, on))
    if form is not None:
        assert ctx.join_key_form() == form
    return got


# ---- 1. every type against every build form -----------------------------------------------------------------------------------------

def key_form(form, jt):
    if form == "utf8_long":
        return "wide"
    return "narrow" if form == "int64_unique" and jt == JT.FULL else "packed"       # the existence probes read the general table


@pytest.mark.parametrize("jt", JT.TYPES)
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("form", JT.FORMS)
def test_every_type_against_every_build_form(ctx, form, nulls, jt):
    left, right, on = JT.sides(form, nulls)
    got = check(ctx, left, right, on, jt, key_form(form, jt), merge=nulls)
    if jt == JT.ANTI and nulls:                          # NOT EXISTS: a build row with a NULL key has no partner
        null_rows = set(np.nonzero(~left[on[-1][0]].is_valid())[0].tolist())
        assert null_rows and null_rows <= set(got["li"].values.tolist())
    if jt == JT.RIGHT_ANTI and nulls:
        null_rows = set(np.nonzero(~right[on[-1][1]].is_valid())[0].tolist())
        assert null_rows and null_rows <= set(got["ri"].values.tolist())


@pytest.mark.parametrize("jt", JT.TYPES)
def test_duplicate_keys_through_the_forced_wide_table(ctx, jt, monkeypatch):
    monkeypatch.setenv("BHIP_JOIN_WIDE", "1")
    left, right, on = JT.sides("int64_dup", True)
    check(ctx, left, right, on, jt, "wide")


def test_full_on_the_rank_map_and_with_a_dropped_key_column(ctx):
    """dense unique Int32 keys: the rank map, with both outer flags; and a right key column of the left key's name, which is dropped:
    the unmatched probe rows show NULL there, as a Right join's do"""
    rng = np.random.default_rng(21)
    left = JT.with_ids("l", JT.NL, [("k", OCol("Int32", (rng.permutation(JT.NL) + 100).astype(np.int32))), ("lx", OCol("Float64", rng.random(JT.NL)))])
    right = JT.with_ids("r", JT.NR, [("k", OCol("Int32", rng.integers(0, JT.NL + 300, JT.NR).astype(np.int32), rng.random(JT.NR) > 0.1))])
    got = check(ctx, left, right, [("k", "k")], JT.FULL, "narrow")
    assert list(got.keys()) == ["k", "lx", "li", "ri"]
    unmatched_probe = ~got["li"].is_valid()
    assert unmatched_probe.any() and not got["k"].is_valid()[unmatched_probe].any()


def test_more_than_one_right_partition_is_refused_for_the_build_side_answers(ctx):
    left, right, on = JT.sides("int64_dup", False)
    for jt in (JT.FULL, JT.SEMI, JT.ANTI):
        with pytest.raises(ba.NotImplementedOnGpu, match="MergeExec"):
            ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right, 2), on, jt)
    for jt in PROBE_SIDE:
        assert ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right, 2), on, jt).output_partitioning().count == 2


# ---- 2. probe batch sizes around the bitmap word and the selection tile ------------------------------------------------------------

@pytest.mark.parametrize("jt", PROBE_SIDE)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024])
def test_probe_batch_sizes(ctx, n, jt):
    left, right, on = JT.sides("int64_dup", True, 3, JT.NL, n)
    plan = ba.HashJoinExec(build_exec(ctx, left), helpers.memory_exec(ctx, [[right]]), on, jt)
    JT.assert_same_rows(rows(plan), JT.expected(jt, left, right, on))


EDGE_NL = 300


@functools.lru_cache(maxsize=None)
def edge_sides(unique, n):
    """300 build rows with short Utf8 keys (the general table: no narrow structures), unique or 100 values three times over; ONE probe
    batch of n rows whose last row has a NULL key and, from two rows on, whose first row finds no partner"""
    rng = np.random.default_rng(100 * n + unique)
    pool = ["k%03d" % i + "-" * (i % 8) for i in range(400)]                     # 4 .. 11 bytes; the build side knows the first 300 / 100
    lk = [pool[int(i)] for i in (rng.permutation(EDGE_NL) if unique else rng.integers(0, 100, EDGE_NL))]
    rk = [pool[int(i)] for i in rng.integers(0, 400 if unique else 130, n)]
    rk[0] = "no-partner"
    valid = np.ones(n, dtype=bool)
    valid[-1] = False
    left = JT.with_ids("l", EDGE_NL, [("lk", OCol("Utf8", lk)), ("lx", OCol("Float64", rng.integers(0, 1000, EDGE_NL) / 8.0))])
    right = JT.with_ids("r", n, [("rk", OCol("Utf8", rk, valid)), ("ry", OCol("Int64", rng.integers(0, 10 ** 6, n)))])
    return left, right, [("lk", "rk")]


@pytest.mark.parametrize("jt", ["Inner", "Right", JT.FULL, JT.SEMI, JT.RIGHT_SEMI, JT.RIGHT_ANTI])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
@pytest.mark.parametrize("unique", [True, False])
@pytest.mark.parametrize("form", ["packed", "wide"])
def test_probe_batch_sizes_in_both_key_forms(ctx, form, unique, n, jt, monkeypatch):
    """the one walk under join_probe_match and join_probe_exists (kernels_hash.hip join_owner_walk: four rows per lane and pass over
    packed keys, one over wide keys) at the edges of the bitmap word (64), of one four-row pass of a wave (256) and of the selection
    tile (1024): the match tail with and without right_outer (Right, Full / Inner; a duplicated build side enumerates pairs instead),
    the mark tail (Semi) and the select tail with and without anti (RightAnti / RightSemi)"""
    if form == "wide":
        monkeypatch.setenv("BHIP_JOIN_WIDE", "1")
    left, right, on = edge_sides(unique, n)
    plan = ba.HashJoinExec(helpers.memory_exec(ctx, [[left]]), helpers.memory_exec(ctx, [[right]]), on, jt)
    want = JT.oracle_join(left, right, on, jt) if jt in ("Inner", "Right") else JT.expected(jt, left, right, on)
    JT.assert_same_rows(rows(plan), want)
    assert ctx.join_key_form() == form


# ---- 3. degenerate sides ------------------------------------------------------------------------------------------------------------

def degenerate(case):
    left, right, on = JT.sides("int64_dup", False)
    if case == "empty_build":
        left = helpers.slice_batch(left, 0, 0)
    elif case == "empty_probe":
        right = helpers.slice_batch(right, 0, 0)
    elif case == "no_key_in_common":
        right = OrderedDict(right, rk=OCol("Int64", right["rk"].values + 3))
    else:                                                  # every key in common: both sides hold the same 300 values
        right = OrderedDict(right, rk=OCol("Int64", np.resize(np.unique(left["lk"].values), JT.NR)))
    return left, right, on


@pytest.mark.parametrize("jt", JT.TYPES)
@pytest.mark.parametrize("case", ["empty_build", "empty_probe", "no_key_in_common", "every_key_in_common"])
def test_degenerate_sides(ctx, case, jt):
    left, right, on = degenerate(case)
    nl, nr = og.batch_len(left), og.batch_len(right)
    plan = ba.HashJoinExec(helpers.memory_exec(ctx, [[left]]), helpers.memory_exec(ctx, [[right]]), on, jt)
    got = rows(plan)
    JT.assert_same_rows(got, JT.expected(jt, left, right, on))
    # the row counts the semantics prescribe, whatever the expectation builder says
    n_got = og.batch_len(got)
    if case == "every_key_in_common":
        pairs = int(sum(np.count_nonzero(left["lk"].values == v) for v in right["rk"].values))
        want = {JT.FULL: pairs, JT.SEMI: nl, JT.ANTI: 0, JT.RIGHT_SEMI: nr, JT.RIGHT_ANTI: 0}[jt]
    else:                                                  # no pair at all: every row of either side is unmatched
        want = {JT.FULL: nl + nr, JT.SEMI: 0, JT.ANTI: nl, JT.RIGHT_SEMI: 0, JT.RIGHT_ANTI: nr}[jt]
    assert n_got == want


# ---- 4. parents and children --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt,column", [(JT.FULL, "ri"), (JT.SEMI, "lx"), (JT.ANTI, "li"), (JT.RIGHT_SEMI, "ry"), (JT.RIGHT_ANTI, "ri")])
def test_projection_of_one_column(ctx, jt, column):
    left, right, on = JT.sides("int64_dup", True)
    exprs = [(col(column), "c")]
    got = rows(ba.ProjectionExec(exprs, join_plan(ctx, left, right, on, jt)))
    helpers.assert_rows_equal(got, og.project(JT.expected(jt, left, right, on), exprs), ordered=False)


@pytest.mark.parametrize("jt,key,value", [(JT.SEMI, "lk", "li"), (JT.RIGHT_SEMI, "rk", "ry")])
def test_aggregate_over_an_existence_join(ctx, jt, key, value):
    left, right, on = JT.sides("int64_dup", True)
    group = [(col(key), key)]
    aggs = [E.Sum(col(value), "s"), E.Count(lit(1, E.UINT8), "n")]
    partial = ba.HashAggregateExec(ba.plan.PARTIAL, group, aggs, join_plan(ctx, left, right, on, jt))
    fin = ba.HashAggregateExec(ba.plan.FINAL, group, aggs, ba.MergeExec(partial))
    want = og.hash_aggregate(og.hash_aggregate(JT.expected(jt, left, right, on), "Partial", group, aggs), "Final", group, aggs)
    helpers.assert_rows_equal(rows(fin), want, ordered=False, key_cols=[key])


def test_a_semi_and_a_right_semi_under_an_inner_join(ctx):
    """the build child is a Semi join, the probe child a RightSemi join: the columns the join above only passes on leave both as views
    (the Semi's over its compacted build rows, the RightSemi's over its selection of every probe batch)"""
    la, ra, on = JT.sides("int64_dup", True)
    lb, rb, _ = JT.sides("int64_dup", True, 5)
    semi = join_plan(ctx, la, ra, on, JT.SEMI)
    right_semi = join_plan(ctx, lb, rb, on, JT.RIGHT_SEMI)
    top = ba.HashJoinExec(semi, right_semi, on, ba.plan.INNER)
    want = og.hash_join(JT.expected(JT.SEMI, la, ra, on), JT.expected(JT.RIGHT_SEMI, lb, rb, on), on, "Inner")
    assert og.batch_len(want) > 1000
    JT.assert_same_rows(rows(top), want)


@pytest.mark.parametrize("jt", [JT.RIGHT_ANTI, JT.SEMI])
def test_filter_and_projection_under_the_probe_side(ctx, jt):
    """the fused chain: the predicate runs first and only the surviving rows are probed — a row the filter removes is in no output"""
    left, right, _ = JT.sides("int64_dup", True)
    pred = E.coerce(col("ry") > lit(900000), {"rk": "Int64", "ry": "Int64", "ri": "Int64"})
    exprs = [(col("ri"), "ri"), (col("rk"), "key"), (col("ry"), "ry")]
    probe = probe_exec(ctx, right, 2 if jt in PROBE_SIDE else 1)
    chain = ba.ProjectionExec(exprs, ba.CoalesceBatchesExec(ba.FilterExec(pred, probe), 4096))
    plan = ba.HashJoinExec(build_exec(ctx, left), chain, [("lk", "key")], jt)
    kept = og.project(og.filter_batch(right, pred), exprs)
    assert 0 < og.batch_len(kept) < JT.NR
    got = rows(plan)
    JT.assert_same_rows(got, JT.expected(jt, left, kept, [("lk", "key")]))
    if jt == JT.RIGHT_ANTI:
        assert got["ry"].values.min() > 900000
    else:                                                  # some build rows had partners among the removed rows only
        assert og.batch_len(got) < og.batch_len(JT.expected(jt, left, right, [("lk", "rk")]))


# ---- 5. a packed build side and one probe batch that outgrows the packed key -----------------------------------------------------------

@pytest.mark.parametrize("jt", [JT.ANTI, JT.SEMI])
@pytest.mark.parametrize("unique", [True, False])
def test_the_bits_of_the_packed_table_and_its_wide_sibling_meet(ctx, unique, jt):
    """the second probe batch holds one 16-byte value: it goes through the wide table built over the same build rows, the batches
    around it through the packed one.  A build row is matched if EITHER saw a partner; with duplicate keys the two tables pick
    different representatives of a key, so the answers have to be merged per key, not per bit"""
    rng = np.random.default_rng(8)
    nk = JT.NL if unique else 300
    keys = ["b%04d" % i + "-" * (i % 10) for i in range(nk)]                    # 5 .. 14 bytes
    lk = [keys[int(i)] for i in (rng.permutation(nk) if unique else rng.integers(0, nk, JT.NL))]
    # every probe batch knows its own third of the keys only, so each table sees partners the other never does
    third = lambda j: 0 if j < JT.CUTS[1] else 1 if j < JT.CUTS[2] else 2
    rk = [keys[3 * int(rng.integers(0, nk // 4)) + third(j)] if rng.random() < 0.8 else "none-%d" % j for j in range(JT.NR)]
    rk[2000] = "0123456789abcdef"                                                # 16 bytes, in the second batch
    left = JT.with_ids("l", JT.NL, [("lk", OCol("Utf8", lk)), ("lx", OCol("Float64", rng.random(JT.NL)))])
    right = JT.with_ids("r", JT.NR, [("rk", OCol("Utf8", rk)), ("ry", OCol("Int64", rng.integers(0, 10 ** 6, JT.NR)))])
    on = [("lk", "rk")]
    for batch in range(3):                                                       # each batch alone decides some build rows
        part = helpers.slice_batch(right, JT.CUTS[batch], JT.CUTS[batch + 1])
        rest = OrderedDict((k, c.take(np.r_[0:JT.CUTS[batch], JT.CUTS[batch + 1]:JT.NR])) for k, c in right.items())
        assert set(JT.expected(JT.SEMI, left, part, on)["li"].values) - set(JT.expected(JT.SEMI, left, rest, on)["li"].values)
    check(ctx, left, right, on, jt, "wide")
