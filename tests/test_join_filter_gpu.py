"""GPU parity of HashJoinExec with a residual join filter, all eight join types (kernels_hash.hip: join_pairs_resolve, join_hit_select,
over the candidates of join_probe_count / join_probe_emit[_wide]).

Expected rows: join_filter_cases.expected — the CPU oracle's Inner join filtered by the oracle's evaluator, the eight types derived
from the kept pairs; checked against a nested loop in test_join_filter_plan.py.  Rows compare exactly, as multisets keyed by the row
ids li / ri.  Sizes: 900 build rows in two partitions; 5000 probe rows as batches of 1025 (one past the 1024-row selection tile),
1975 and 2000 rows."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og
from oracle import plan_eval
from oracle.engine import OCol

import helpers
import join_filter_cases as JF
import join_types_cases as JT
from join_filter_cases import build_exec, probe_exec, rows

pytestmark = pytest.mark.gpu
ONE_PARTITION = (JF.LEFT, JT.FULL, JT.SEMI, JT.ANTI)          # a build row's fate depends on every probe row


def join_plan(ctx, left, right, on, jt, flt, merge=False):
    probe = probe_exec(ctx, right, ("merge" if merge else 1) if jt in ONE_PARTITION else 2)
    return ba.HashJoinExec(build_exec(ctx, left), probe, on, jt, filter=flt)


def check(ctx, left, right, on, jt, flt, form=None, merge=False):
    got = rows(join_plan(ctx, left, right, on, jt, flt, merge))
    JT.assert_same_rows(got, JF.expected(jt, left, right, on, flt))
    if form is not None:
        assert ctx.join_key_form() == form
    return got


def one_batch_plan(ctx, left, right_batches, on, jt, flt):
    return ba.HashJoinExec(helpers.memory_exec(ctx, [[left]]), helpers.memory_exec(ctx, [right_batches]), on, jt, filter=flt)


# ---- 1. every type against every build form, the two-sided predicate -------------------------------------------------------------------

@pytest.mark.parametrize("jt", JF.ALL_TYPES)
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("form", JF.FORMS)
def test_every_type_against_every_build_form(ctx, form, nulls, jt):
    """int64_unique: a unique build side, forced through count / emit (no narrow structures under a filter); hot_key: ~1.1 M
    candidates, one probe row's spanning many waves; utf8_long: the wide table"""
    left, right, on = JF.sides(form, nulls)
    flt = JF.predicate("two_sided", left, right, on)
    check(ctx, left, right, on, jt, flt, "wide" if form == "utf8_long" else "packed", merge=nulls)


# ---- 2. the other predicates -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", JF.ALL_TYPES)
@pytest.mark.parametrize("name", [n for n in JF.PREDICATES if n != "two_sided"])
def test_the_other_predicates(ctx, name, jt):
    left, right, on = JF.sides("int64_dup", True)
    flt = JF.predicate(name, left, right, on)
    got = check(ctx, left, right, on, jt, flt)
    n_cand, kli, _ = JF.kept_pairs(left, right, on, flt)
    if name == "never":
        assert len(kli) == 0
        want = {JF.INNER: 0, JF.LEFT: JT.NL, JF.RIGHT: JT.NR, JT.FULL: JT.NL + JT.NR, JT.SEMI: 0, JT.ANTI: JT.NL, JT.RIGHT_SEMI: 0, JT.RIGHT_ANTI: JT.NR}[jt]
        assert og.batch_len(got) == want
        if jt == JF.RIGHT:                                 # every probe row, with NULL left columns
            assert not got["li"].is_valid().any() and not got["lx"].is_valid().any() and sorted(got["ri"].values) == list(range(JT.NR))
    elif name == "always":                                 # the unfiltered join of the same type, by the product itself as well
        assert len(kli) == n_cand
        JT.assert_same_rows(got, rows(join_plan(ctx, left, right, on, jt, None)))
    else:
        assert 0 < len(kli) < n_cand


# ---- 3. state that crosses probe batches ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", [JF.LEFT, JT.FULL, JT.SEMI, JT.ANTI])
def test_a_partner_in_the_last_batch_after_failures_in_the_first(ctx, jt):
    """build row 3: candidates that fail in the first batch, none in the second, its only partner in the last;
    build row 5: candidates in every batch, all failing; build row 9: no candidate at all"""
    rng = np.random.default_rng(4)
    left = JT.with_ids("l", 10, [("lk", OCol("Int64", np.arange(10, dtype=np.int64))), ("lx", OCol("Float64", np.full(10, 50.0)))])
    rk = rng.choice([0, 1, 2, 4, 6, 7, 8, 11, 12], 210).astype(np.int64)
    ry = rng.choice([10, 100], 210).astype(np.int64)      # lx > ry: 10 passes, 100 fails
    rk[[5, 20, 41]], ry[[5, 20, 41]] = 3, 100
    rk[200], ry[200] = 3, 10
    rk[[7, 100, 180]], ry[[7, 100, 180]] = 5, 100
    right = JT.with_ids("r", 210, [("rk", OCol("Int64", rk)), ("ry", OCol("Int64", ry))])
    on = [("lk", "rk")]
    flt = E.coerce(col("lx") > col("ry"), dict(JF.inner_schema(left, right, on)))
    batches = [helpers.slice_batch(right, lo, lo + 70) for lo in (0, 70, 140)]
    got = rows(one_batch_plan(ctx, left, batches, on, jt, flt))
    JT.assert_same_rows(got, JF.expected(jt, left, right, on, flt))
    ids = got["li"].values[got["li"].is_valid()].tolist()
    if jt == JT.SEMI:
        assert 3 in ids and 5 not in ids and 9 not in ids
    elif jt == JT.ANTI:
        assert sorted(ids) == [5, 9]
    else:                                                  # rows 5 and 9 once, with NULL right columns; row 3 with its one partner
        lone = got["li"].values[got["li"].is_valid() & ~got["ri"].is_valid()].tolist()
        assert sorted(lone) == [5, 9] and ids.count(3) == 1


# ---- 4. sizes around the wave and the selection tile ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", [JF.INNER, JF.RIGHT])
@pytest.mark.parametrize("n,kept", [(70, 0), (70, 1), (130, 63), (130, 64), (130, 65), (1100, 1024), (1100, 1025),
                                    (1, 0), (1, 1), (64, 10), (64, 64), (65, 64), (65, 65)])
def test_kept_pairs_and_probe_rows_around_the_edges(ctx, n, kept, jt):
    """one probe batch of n rows, two candidates per row (2 n in all), of which exactly `kept` pass — one per row for the first
    `kept` rows.  n == kept: a row's second candidate still fails, so the kept positions are every other one"""
    nb = 40
    lk = np.repeat(np.arange(nb, dtype=np.int64), 2)
    left = JT.with_ids("l", 2 * nb, [("lk", OCol("Int64", lk)), ("lx", OCol("Float64", np.tile([1.0, -1.0], nb)))])
    ry = np.where(np.arange(n) < kept, 0, 5).astype(np.int64)
    right = JT.with_ids("r", n, [("rk", OCol("Int64", (np.arange(n) * 7 % nb).astype(np.int64))), ("ry", OCol("Int64", ry))])
    on = [("lk", "rk")]
    flt = E.coerce(col("lx") > col("ry"), dict(JF.inner_schema(left, right, on)))
    n_cand, kli, _ = JF.kept_pairs(left, right, on, flt)
    assert n_cand == 2 * n and len(kli) == kept
    got = rows(one_batch_plan(ctx, left, [right], on, jt, flt))
    JT.assert_same_rows(got, JF.expected(jt, left, right, on, flt))
    assert og.batch_len(got) == (kept if jt == JF.INNER else n)


@pytest.mark.parametrize("jt", [JF.INNER, JF.RIGHT, JT.RIGHT_SEMI])
@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_every_candidate_kept(ctx, n, jt):
    """the candidates are the pairs: nothing is gathered, only the bits are set"""
    left = JT.with_ids("l", 30, [("lk", OCol("Int64", np.arange(30, dtype=np.int64) % 15)), ("lx", OCol("Float64", np.full(30, 1.0)))])
    right = JT.with_ids("r", n, [("rk", OCol("Int64", (np.arange(n) % 20).astype(np.int64))), ("ry", OCol("Int64", np.zeros(n, np.int64)))])
    on = [("lk", "rk")]
    flt = E.coerce(col("lx") > col("ry"), dict(JF.inner_schema(left, right, on)))
    got = rows(one_batch_plan(ctx, left, [right], on, jt, flt))
    JT.assert_same_rows(got, JF.expected(jt, left, right, on, flt))


# ---- 5. empty sides ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", JF.ALL_TYPES)
@pytest.mark.parametrize("case", ["empty_build", "empty_probe", "a_batch_without_candidates"])
def test_empty_sides(ctx, case, jt):
    left, right, on = JF.sides("int64_dup", False)
    batches = None
    if case == "empty_build":
        left = helpers.slice_batch(left, 0, 0)
    elif case == "empty_probe":
        right = helpers.slice_batch(right, 0, 0)
    else:                                                  # the first batch knows no build key
        right = OrderedDict(right, rk=OCol("Int64", np.where(np.arange(JT.NR) < 1025, right["rk"].values + 3, right["rk"].values)))
        batches = [helpers.slice_batch(right, 0, 1025), helpers.slice_batch(right, 1025, JT.NR)]
    flt = JF.predicate("two_sided", left, right, on)
    got = rows(one_batch_plan(ctx, left, batches or [right], on, jt, flt))
    JT.assert_same_rows(got, JF.expected(jt, left, right, on, flt))
    nl, nr = og.batch_len(left), og.batch_len(right)
    if case != "a_batch_without_candidates":               # no pair at all: every row of either side is unmatched
        want = {JF.INNER: 0, JF.LEFT: nl, JF.RIGHT: nr, JT.FULL: nl + nr, JT.SEMI: 0, JT.ANTI: nl, JT.RIGHT_SEMI: 0, JT.RIGHT_ANTI: nr}[jt]
        assert og.batch_len(got) == want


# ---- 6. a packed build side and one probe batch that outgrows the packed key -----------------------------------------------------------------

@pytest.mark.parametrize("jt", [JT.SEMI, JF.LEFT, JT.ANTI, JT.FULL])
def test_the_bits_of_the_packed_table_and_its_wide_sibling_meet(ctx, jt):
    """the second probe batch holds one 16-byte value and goes through the wide table over the same build rows; under a filter both
    tables mark the build rows themselves, so the bits of the two simply add up"""
    rng = np.random.default_rng(8)
    nk = 300
    keys = ["b%04d" % i + "-" * (i % 10) for i in range(nk)]                    # 5 .. 14 bytes
    lk = [keys[int(i)] for i in rng.integers(0, nk, JT.NL)]
    third = lambda j: 0 if j < JT.CUTS[1] else 1 if j < JT.CUTS[2] else 2       # every batch knows its own third of the keys
    rk = [keys[3 * int(rng.integers(0, nk // 4)) + third(j)] if rng.random() < 0.8 else "none-%d" % j for j in range(JT.NR)]
    rk[2000] = "0123456789abcdef"                                                # 16 bytes, in the second batch
    left = JT.with_ids("l", JT.NL, [("lk", OCol("Utf8", lk)), ("lx", OCol("Float64", rng.random(JT.NL)))])
    right = JT.with_ids("r", JT.NR, [("rk", OCol("Utf8", rk)), ("ry", OCol("Int64", rng.integers(0, 10 ** 6, JT.NR)))])
    on = [("lk", "rk")]
    flt = E.coerce(col("lx") * lit(1000000.0) > col("ry"), dict(JF.inner_schema(left, right, on)))
    n_cand, kli, kri = JF.kept_pairs(left, right, on, flt)
    in_second = (kri >= JT.CUTS[1]) & (kri < JT.CUTS[2])
    assert set(kli[in_second]) - set(kli[~in_second]) and set(kli[~in_second]) - set(kli[in_second])    # each table decides some rows alone
    assert 0.2 < len(kli) / n_cand < 0.8
    check(ctx, left, right, on, jt, flt, "wide")


# ---- 7. parents and children -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", [JF.INNER, JF.LEFT, JF.RIGHT, JT.FULL, JT.SEMI, JT.RIGHT_ANTI])
def test_a_projection_that_reads_neither_filter_column(ctx, jt):
    left, right, on = JF.sides("int64_dup", True)
    flt = JF.predicate("two_sided", left, right, on)
    ids = [c for c in ("li", "ri") if not (c == "ri" and jt in JF.BUILD_SIDE) and not (c == "li" and jt in JF.PROBE_SIDE)]
    exprs = [(col(c), c) for c in ids]
    got = rows(ba.ProjectionExec(exprs, join_plan(ctx, left, right, on, jt, flt)))
    JT.assert_same_rows(got, og.project(JF.expected(jt, left, right, on, flt), exprs))


@pytest.mark.parametrize("jt", [JF.INNER, JF.RIGHT, JT.SEMI, JT.RIGHT_ANTI])
def test_a_fused_probe_chain_that_renames_a_filter_column(ctx, jt):
    """FilterExec + ProjectionExec under the right child: the probe runs on the source's batches, the rows the FilterExec removes are
    in no output, and the join filter's `val` is the source's `ry`"""
    left, right, _ = JF.sides("int64_dup", True)
    pred = E.coerce(col("ry") > lit(200000), {k: c.dtype for k, c in right.items()})
    exprs = [(col("ri"), "ri"), (col("rk"), "key"), (col("ry"), "val")]
    probe = probe_exec(ctx, right, 1 if jt in ONE_PARTITION else 2)
    chain = ba.ProjectionExec(exprs, ba.CoalesceBatchesExec(ba.FilterExec(pred, probe), 4096))
    on = [("lk", "key")]
    kept = og.project(og.filter_batch(right, pred), exprs)
    assert 0 < og.batch_len(kept) < JT.NR
    flt = E.coerce(col("lx") * lit(8000.0) > col("val"), dict(JF.inner_schema(left, kept, on)))
    got = rows(ba.HashJoinExec(build_exec(ctx, left), chain, on, jt, filter=flt))
    JT.assert_same_rows(got, JF.expected(jt, left, kept, on, flt))
    n_cand, kli, _ = JF.kept_pairs(left, kept, on, flt)
    assert 0 < len(kli) < n_cand


@pytest.mark.parametrize("jt", [JF.INNER, JF.LEFT, JT.SEMI, JT.RIGHT_ANTI])
def test_a_filtered_join_above_an_unfiltered_join(ctx, jt):
    """the right child is a projection of plain columns over an Inner join: the filter reads `ry` (the join below's probe side) and
    `w` (its build side), which arrive as views"""
    left, _, on = JF.sides("int64_unique", True)
    lb, rb, _ = JF.sides("int64_unique", True, 5)
    exprs = [(col("rk"), "rk"), (col("ry"), "ry"), (col("ri"), "ri"), (col("lx"), "w")]
    below = ba.ProjectionExec(exprs, ba.HashJoinExec(build_exec(ctx, lb), probe_exec(ctx, rb, 1), on, JF.INNER))
    mid = og.project(og.hash_join(lb, rb, on, "Inner"), exprs)
    assert og.batch_len(mid) > 1000 and len(np.unique(mid["ri"].values)) == og.batch_len(mid)
    flt = E.coerce((col("lx") * lit(8000.0) > col("ry")).and_(col("w") < lit(100.0)), dict(JF.inner_schema(left, mid, on)))
    got = rows(ba.HashJoinExec(build_exec(ctx, left), below, on, jt, filter=flt))
    JT.assert_same_rows(got, JF.expected(jt, left, mid, on, flt))
    n_cand, kli, _ = JF.kept_pairs(left, mid, on, flt)
    assert 100 < len(kli) < n_cand


# ---- 8. a right child of two partitions ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", [JF.INNER, JF.LEFT, JF.RIGHT, JT.RIGHT_SEMI, JT.RIGHT_ANTI])
def test_a_right_child_of_two_partitions(ctx, jt):
    """one stream per right partition against the one build side; Left emits its unmatched build rows once per task, as it does
    without a filter, so every partition is compared with the join of its own probe rows"""
    left, right, on = JF.sides("int64_dup", True)
    flt = JF.predicate("two_sided", left, right, on)
    plan = ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right, 2), on, jt, filter=flt)
    assert plan.output_partitioning().count == 2
    for p, (lo, hi) in enumerate([(JT.CUTS[0], JT.CUTS[2]), (JT.CUTS[2], JT.CUTS[3])]):
        part = helpers.slice_batch(right, lo, hi)
        got = helpers.concat([helpers.from_device(b) for b in plan.execute(p)])
        JT.assert_same_rows(got, JF.expected(jt, left, part, on, flt))


def test_full_semi_and_anti_still_need_one_right_partition(ctx):
    left, right, on = JF.sides("int64_dup", False)
    flt = JF.predicate("two_sided", left, right, on)
    for jt in (JT.FULL, JT.SEMI, JT.ANTI):
        with pytest.raises(ba.NotImplementedOnGpu, match="MergeExec"):
            ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right, 2), on, jt, filter=flt)


# ---- 9. the probe's fused range filter at the Int32 extremes -----------------------------------------------------------------------------------

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.mark.parametrize("jt", [JF.INNER, JF.RIGHT])
@pytest.mark.parametrize("name,pred", [
    ("gt_max", col("ry") > lit(I32_MAX, E.INT32)), ("lt_min", col("ry") < lit(I32_MIN, E.INT32)),
    ("ge_min", col("ry") >= lit(I32_MIN, E.INT32)), ("le_max", col("ry") <= lit(I32_MAX, E.INT32)),
    ("eq_max", col("ry").eq(lit(I32_MAX, E.INT32))), ("max_lt", lit(I32_MAX, E.INT32) < col("ry")),
    ("min_ge", lit(I32_MIN, E.INT32) >= col("ry")),
])
def test_probe_side_int32_predicates_at_the_extremes(ctx, name, pred, jt):
    """a FilterExec over the probe side of a join on a unique Int32 key runs inside the probe kernel as integer ranges
    (ops_join.cpp::int_ranges_of, the integer image of build_sop's double ranges).  Bounds one past either end of Int32 select
    nothing, bounds AT the ends select everything; probe rows at both extremes, on keys with and without a build row"""
    rng = np.random.default_rng(11)
    nl, nr = 200, 1025 + 70
    left = OrderedDict([("lk", OCol("Int32", rng.permutation(400)[:nl].astype(np.int32))), ("lx", OCol("Float64", rng.random(nl)))])
    ry = rng.integers(-5, 5, nr).astype(np.int64)
    ry[rng.random(nr) < 0.25] = I32_MAX
    ry[rng.random(nr) < 0.25] = I32_MIN
    ry[[0, 1, 63, 64, 1023, 1024, nr - 1]] = [I32_MAX, I32_MIN, I32_MAX, I32_MIN, I32_MIN, I32_MAX, I32_MAX]
    rk = rng.integers(0, 400, nr).astype(np.int32)
    rk[[0, 1, 63, 64, 1023, 1024, nr - 1]] = left["lk"].values[:7]              # the rows at the extremes have partners
    right = OrderedDict([("rk", OCol("Int32", rk)), ("ry", OCol("Int32", ry.astype(np.int32))), ("ri", OCol("Int32", np.arange(nr, dtype=np.int32)))])
    flt = ba.FilterExec(pred, helpers.memory_exec(ctx, [[helpers.slice_batch(right, 0, 1025), helpers.slice_batch(right, 1025, nr)]]))
    plan = ba.HashJoinExec(helpers.memory_exec(ctx, [[left]]), flt, [("lk", "rk")], jt)
    got = helpers.concat(helpers.collect_product(plan))
    want = plan_eval.collect(plan)
    helpers.assert_rows_equal(got, want, ordered=False, key_cols=["ri", "lk"])
    assert ctx.join_key_form() == "narrow"
    n_rows = len(helpers.rows_of(got))
    if name in ("gt_max", "lt_min", "max_lt"):
        assert n_rows == 0
    elif name in ("ge_min", "le_max"):
        assert n_rows == (nr if jt == JF.RIGHT else int(np.isin(rk, left["lk"].values).sum()))
    else:
        assert 0 < n_rows < nr
