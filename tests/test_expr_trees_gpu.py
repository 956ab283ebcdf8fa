"""The expression VM — the compiler in host/expr.cpp (ProgramBuilder), the interpreter in vm_device.h and the sink kernels — on
GENERATED expression trees (tests/expr_tree_cases.py) and on hand-built programs at the compiler's limits (vm_isa.h), against the
CPU oracle: bit exact (float_rtol = 0), validity exact, zero signs count, any NaN matches any NaN.

Random families: Projection (up to 16 outputs), Filter, a fused predicate under an ungrouped partial aggregate, aggregate
arguments (ungrouped and by 3, 7 and about 300 groups) and computed group keys.  A mismatch prints the case id (family, seed,
index — enough to regenerate it), the row count, the trees and the first differing row.

Limit cases: for each bound the largest program it allows (must match the oracle) and the smallest that exceeds it (must be
refused as NotImplementedOnGpu with the builder's own message, at plan construction or at execute — never rows, never an
ExecutionError, never a HIP error)."""
import re
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import plan_eval
from oracle.engine import OCol

import expr_tree_cases as X
import helpers

pytestmark = pytest.mark.gpu

_LEAVES = {}


def leaf(ctx, b):
    """one device copy per shared batch (expr_tree_cases caches the batches: the object is the key)"""
    key = id(b)
    if key not in _LEAVES:
        _LEAVES[key] = (helpers.memory_exec(ctx, [[b]]), b)
    return _LEAVES[key][0]


def check(plan, what, ordered=True, key_cols=None, zero_sign_cols=()):
    got = helpers.concat(helpers.collect_product(plan))
    want = plan_eval.collect(plan)
    try:
        helpers.assert_rows_equal(got, want, ordered=ordered, float_rtol=0.0, key_cols=key_cols, zero_sign_cols=zero_sign_cols)
    except AssertionError as e:
        raise AssertionError(f"{what}\n  {e}") from None


def refused(build, message):
    """`build()` makes the plan; constructing or running it must raise NotImplementedOnGpu with `message`"""
    with pytest.raises(ba.NotImplementedOnGpu, match=re.escape(message)):
        build().collect()


# =====================================================================================================================================
# generated trees
# =====================================================================================================================================
@pytest.mark.parametrize("seed", X.SEEDS)
@pytest.mark.parametrize("family", X.FAMILIES)
def test_generated_trees(ctx, family, seed):
    executed, skipped, messages = 0, 0, set()
    for c in X.cases(family, seed):
        keys = X.key_columns(c)
        try:
            plan = X.build_plan(ba, c, leaf(ctx, X.batch(c.n_rows)))
            check(plan, c.describe(), ordered=keys is None, key_cols=keys, zero_sign_cols=X.zero_sign_columns(c))
            executed += 1
        except ba.NotImplementedOnGpu as e:
            # a random in-limit tree may still be refused (Python cannot predict the instruction count exactly): skipped only
            # when it is one of the builder's limit messages
            assert X.is_limit_refusal(str(e)), f"{c.describe()}\n  refused with: {e}"
            skipped += 1
            messages.add(str(e))
    print(f"{family} seed {seed}: executed {executed}, skipped {skipped} {sorted(messages)}")
    assert skipped <= 0.1 * (executed + skipped), (executed, skipped, sorted(messages))


def test_fused_predicate_guards_integer_division(ctx):
    """the rows the fused predicate drops must not raise a division by zero: u8z is 0 in a third of the rows, and the oracle (which
    filters first) never sees them"""
    for n in (513, 1025):
        b = OrderedDict(X.batch(n))
        rng = np.random.default_rng(n)
        b["u8z"] = OCol(E.UINT8, rng.integers(0, 3, n).astype(np.uint8), rng.random(n) > 0.12)
        q = E.BinaryExpr(col("u8"), "Divide", col("u8z"))
        flt = ba.FilterExec(col("u8z").ne(lit(0, E.UINT8)), helpers.memory_exec(ctx, [[b]]))
        plan = ba.HashAggregateExec("Partial", [], [E.Sum(E.CastExpr(q, E.INT16), "s"), E.Max(q, "m"), E.Count(q, "c")], flt)
        check(plan, f"fused division guard, {n} rows", ordered=False, key_cols=[])


# =====================================================================================================================================
# limit cases (hand-built): sixteen-plus Float64 columns f0 .. f16 around 1.0 and an Int32 column k of three values
# =====================================================================================================================================
def f(i):
    return col(f"f{i}")


def fold(items, op):
    e = items[0]
    for x in items[1:]:
        e = E.BinaryExpr(e, op, x)
    return e


@pytest.mark.parametrize("nulls", [True, False])
def test_limit_referenced_columns(ctx, nulls):
    src = leaf(ctx, X.float_batch(513, nulls))
    check(ba.ProjectionExec([(fold([f(i) for i in range(16)], "Plus"), "s")], src), "16 columns")
    check(ba.FilterExec(fold([f(i) for i in range(16)], "Plus") > lit(16.0), src), "16 columns, filter")
    refused(lambda: ba.ProjectionExec([(fold([f(i) for i in range(17)], "Plus"), "s")], src), "expression references more than 16 columns")
    refused(lambda: ba.FilterExec(fold([f(i) for i in range(17)], "Plus") > lit(16.0), src), "expression references more than 16 columns")


def test_limit_distinct_literals(ctx):
    src = leaf(ctx, X.float_batch(513, True))
    chain = lambda n: fold([f(0)] + [lit(0.5 + i) for i in range(n)], "Plus")
    check(ba.ProjectionExec([(chain(32), "s")], src), "32 literals")
    refused(lambda: ba.ProjectionExec([(chain(33), "s")], src), "expression has more than 32 distinct literals")


def test_limit_instructions(ctx):
    """a left-deep chain: every node contains the one before it, so no two subtrees are equal and CSE cannot shorten it"""
    src = leaf(ctx, X.float_batch(1025, True))

    def chain(n):
        e = f(0)
        for k in range(1, n + 1):
            e = E.BinaryExpr(e, ("Plus", "Minus", "Multiply")[k % 3], f(k % 16))
        return e
    check(ba.ProjectionExec([(chain(96), "s")], src), "96 instructions")
    check(ba.FilterExec(chain(95) > lit(1.0), src), "96 instructions, filter")
    refused(lambda: ba.ProjectionExec([(chain(97), "s")], src), "expression needs more than 96 VM instructions")
    refused(lambda: ba.FilterExec(chain(96) > lit(1.0), src), "expression needs more than 96 VM instructions")


@pytest.mark.parametrize("nulls", [True, False])
def test_limit_boolean_slots(ctx, nulls):
    """Boolean outputs stay live to the end of the program: k comparisons and, computed last, an AND of two more hold k + 2
    Boolean slots at once.  A right-nested AND of k comparisons holds k."""
    src = leaf(ctx, X.float_batch(1025, nulls))
    outs = lambda k: [(f(i) > lit(1.0), f"b{i}") for i in range(k)] + [((f(14) < lit(1.0)).and_(f(15) < lit(1.25)), "last")]
    check(ba.ProjectionExec(outs(14), src), "16 Boolean slots live")
    refused(lambda: ba.ProjectionExec(outs(15), src), "expression needs too many VM registers")

    def nested(k):
        e = f((k - 1) % 16) > lit(0.6 + 0.001 * (k - 1))
        for i in range(k - 2, -1, -1):
            e = (f(i) > lit(0.6 + 0.001 * i)).and_(e)
        return e
    check(ba.FilterExec(nested(16), src), "16 Boolean slots live, filter")
    refused(lambda: ba.FilterExec(nested(17), src), "expression needs too many VM registers")


def test_limit_computed_outputs(ctx):
    src = leaf(ctx, X.float_batch(513, True))
    outs = lambda k: [(f(i % 4) + lit(float(i)), f"o{i}") for i in range(k)]
    check(ba.ProjectionExec(outs(16), src), "16 outputs")
    check(ba.ProjectionExec(outs(16) + [(f(5), "plain")], src), "16 outputs and a column passed through")
    refused(lambda: ba.ProjectionExec(outs(17), src), "more than 16 computed output columns")


def _min_max(n_acc):
    """n_acc distinct accumulators: MIN(f0) .. MIN(f7), MAX(f0) .. MAX(f7), MIN(f8)"""
    specs = [("MIN", i) for i in range(8)] + [("MAX", i) for i in range(8)] + [("MIN", 8)]
    return [E.AggregateExpr(fun, f(i), f"{fun.lower()}{i}") for fun, i in specs[:n_acc]]


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("n_rows", [5, 4099])
def test_limit_accumulators(ctx, n_rows, grouped):
    """8 accumulators are the register path's width (AGG_NACC); 9 to 16 run its 16-register variant over a small input (and the
    hash path over a large one); 17 are refused"""
    src = leaf(ctx, X.float_batch(n_rows, True))
    group = [(col("k"), "k")] if grouped else []
    for n_acc in (8, 9, 16):
        aggs = _min_max(n_acc)
        check(ba.HashAggregateExec("Partial", group, aggs, src), f"{n_acc} accumulators, {n_rows} rows", ordered=False,
              key_cols=[n for _, n in group], zero_sign_cols=[f"{a.name}[{a.fun.lower()}]" for a in aggs])
    refused(lambda: ba.HashAggregateExec("Partial", group, _min_max(17), src), "more than 16 distinct accumulators")


def test_limit_key_parts(ctx):
    """8 key parts are the packed key's bound.  An aggregate with 9 to 16 group expressions answers it the way it answers a layout wider
    than 16 bytes, on its wide-key route (representative rows); 17 are refused.  Every other consumer of key parts refuses the ninth"""
    src = leaf(ctx, X.float_batch(1025, True))
    keys = lambda k: [(f(i) > lit(1.0), f"g{i}") for i in range(k)]
    aggs = [E.Count(f(0), "c"), E.Min(f(9), "m")]
    for k in (8, 9, 16):
        check(ba.HashAggregateExec("Partial", keys(k), aggs, src), f"{k} key parts", ordered=False, key_cols=[f"g{i}" for i in range(k)],
              zero_sign_cols=["m[min]"])
    refused(lambda: ba.HashAggregateExec("Partial", keys(17), aggs, src), "more than 16 group expressions")
    nine = [f(i) > lit(1.0) for i in range(9)]
    refused(lambda: ba.RepartitionExec(src, ba.Partitioning.Hash(nine, 3)), "more than 8 key columns")


# ---- the value-slot sweep -------------------------------------------------------------------------------------------------------
# Sixteen loaded Float64 columns are live from the start of a tile to their last use.  A(w) = s1 * (s2 * (.. * sw)), si = f(2i-2) +
# f(2i-1), leaves w sums pending while every column is still waiting for P = f0 * f1 * .. * f15, which comes after it: 16 + w value
# slots at the peak, w = 1 .. 8 -> 17 .. 24 (VM_MAX_VSLOTS); w = 9 is refused.  "Mirrored" swaps the operands of every sum and
# multiplies P from f15 down: the same pressure with the columns freed in the opposite order.
#
# Which R (rows per thread; a tile is 256 * R rows) a sink takes — launch_common.h: bytes(R) = n_vslots * 256R * (9 with NULLs, else
# 8) + n_bslots * 256R, LDS = 160 KiB:
#   projection / keys / hash-aggregate sinks (choose_r): R = 4 while 2 * bytes(4) <= 160 KiB, i.e. up to 8 value slots with NULLs (9
#     without), else R = 2 — every width of the sweep runs their R = 2 kernels (24 slots: 24 * 512 * 9 + 16 * 512 = 116 KiB);
#   predicate sink (1024-row selection tiles): R = 4 while bytes(4) <= 160 KiB: up to 17 value slots with NULLs (17 * 9216 + 1024 =
#     154 KiB; 18 do not fit) and 19 without (19 * 8192 + 1024 = 153 KiB; 20 do not) — w = 1 with NULLs and w <= 3 without run
#     R = 4, every wider one the two-pass R = 2 kernel.  Before that kernel existed those widths failed with a HIP error;
#   register-path aggregate: R = 2 always.
_PAIRS = [(2 * i, 2 * i + 1) for i in range(8)] + [(0, 2)]


def pending(w, mirrored):
    s = [(f(b) + f(a)) if mirrored else (f(a) + f(b)) for a, b in _PAIRS[:w]]
    e = s[-1]
    for x in reversed(s[:-1]):
        e = x * e
    return e


def product(mirrored):
    return fold([f(i) for i in (range(15, -1, -1) if mirrored else range(16))], "Multiply")


def sweep_plan(sink, w, mirrored, src):
    """(the aggregates are ungrouped or grouped by the predicate itself: the sixteen columns are all a program may reference, so a
    plain group column would be a seventeenth)"""
    value = pending(w, mirrored) - product(mirrored)
    pred = pending(w, mirrored) * lit(0.5 ** w) > product(mirrored)          # (scaled: about half of the non-NULL rows pass)
    if sink == "projection":
        return ba.ProjectionExec([(value, "v")], src), None, ()
    if sink == "filter":
        return ba.FilterExec(pred, src), None, ()
    if sink == "fused":
        return ba.HashAggregateExec("Partial", [], [E.Count(f(0), "c"), E.Min(f(1), "m")], ba.FilterExec(pred, src)), [], ("m[min]",)
    if sink == "aggarg":
        return ba.HashAggregateExec("Partial", [], [E.Count(value, "c"), E.Min(value, "mn"), E.Max(value, "mx")], src), [], ("mn[min]", "mx[max]")
    if sink == "groupkey":
        return ba.HashAggregateExec("Partial", [(pred, "g")], [E.Count(f(0), "c"), E.Min(f(1), "m")], src), ["g"], ("m[min]",)
    raise ValueError(sink)


@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("sink", ["projection", "filter", "fused", "aggarg", "groupkey"])
def test_value_slot_sweep(ctx, sink, nulls):
    for n in (513, 1025):
        src = leaf(ctx, X.float_batch(n, nulls))
        for mirrored in (False, True):
            for w in range(1, 9):
                plan, keys, loose = sweep_plan(sink, w, mirrored, src)
                check(plan, f"sweep {sink}, w = {w} ({16 + w} value slots), nulls = {nulls}, mirrored = {mirrored}, {n} rows",
                      ordered=keys is None, key_cols=keys, zero_sign_cols=loose)
            refused(lambda: sweep_plan(sink, 9, mirrored, src)[0], "expression needs too many VM registers")


@pytest.mark.parametrize("nulls", [True, False])
def test_wide_predicate_selection_tiles(ctx, nulls):
    """the predicate sink's two-pass kernel (24 value slots) where a 1024-row selection tile is full, ends in its first half, at the
    half, or in its second half, over one and several tiles"""
    for n in (1, 511, 512, 513, 1023, 1024, 1025, 1536, 1537, 2560, 3073):
        src = leaf(ctx, X.float_batch(n, nulls))
        check(ba.FilterExec(pending(8, False) * lit(0.5 ** 8) > product(False), src), f"24-slot predicate, {n} rows, nulls = {nulls}")


# ---- CSE keys -------------------------------------------------------------------------------------------------------------------
def _named(names, n=513, seed=3):
    rng = np.random.default_rng(seed)
    return OrderedDict((name, OCol(E.FLOAT64, np.round(rng.uniform(-4, 4, n) * 8) / 8, rng.random(n) > 0.12)) for name in names)


CSE_COLLISIONS = {
    # a Float64 literal prints without its type: the column named "1" and lit(1.0) both print "1"
    "column_named_like_a_literal": (["1", "x"], col("1") + lit(1.0)),
    # the load of schema position 0 used to be cached as "#col0"
    "column_named_like_a_load": (["a", "#col0"], col("a") + col("#col0")),
    # a column named like the display string of another expression: an unaliased upstream output
    "column_named_like_an_expression": (["a", "b", "(a Plus b)"], (col("a") + col("b")) * col("(a Plus b)")),
}


@pytest.mark.parametrize("name", sorted(CSE_COLLISIONS))
def test_cse_keys_are_injective(ctx, name):
    names, e = CSE_COLLISIONS[name]
    src = helpers.memory_exec(ctx, [[_named(names)]])
    check(ba.ProjectionExec([(e, "v")], src), f"{name}: projection")
    check(ba.FilterExec(e > lit(1.0), src), f"{name}: filter")


def test_cse_still_shares_equal_subtrees(ctx):
    """the other direction: 48 copies of one subtree are one computation (97 instructions if each were compiled again)"""
    src = leaf(ctx, X.float_batch(513, True))
    shared = lambda: (f(0) * f(1)) + f(2)
    check(ba.ProjectionExec([(fold([shared() for _ in range(48)], "Plus"), "v")], src), "48 equal subtrees")
