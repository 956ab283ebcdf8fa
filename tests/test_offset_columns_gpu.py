"""Operators over columns that are not what the allocator hands out: borrowed device buffers (bhip_batch_from_device) that start at
any boundary their type allows, in exactly their Arrow size with poison around them (offset_columns.py), and the slices a hash
repartition's scatter pass gives its partitions.

Every case asserts
  (a) the plan over the borrowed batch equals the oracle's evaluation of the same plan: bit for bit (rows, order, validity,
      integers, strings, gathered floats, sorted output), Float64 SUM / AVG within the project's 1e-6 relative gate;
  (b) the run over the 0x00 arena and the run over the 0xFF arena agree bit for bit on everything (a) compares bit for bit: no byte
      beyond a column's end reaches a result;
  (c) where the library reports a route, the expected one ran: the wide-load kernels only over 16-byte aligned columns.
Sizes are the smallest at which each mechanism can go wrong; the margins of the arena make an over-read of a few bytes harmless."""
import os
from collections import OrderedDict

os.environ.setdefault("BHIP_KERNEL_TIMING", "1")

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og, plan_eval
from oracle.engine import OCol

import helpers
import join_types_cases as JT
import offset_columns as oc
import sort_cases
import window_cases as K
from test_lean_gpu import AGGS_Q1, SCHEMA as Q1_SCHEMA, batch as q1_batch, on_expected_kernel

pytestmark = pytest.mark.gpu

GATE = 1e-6                    # SUM / AVG over Float64
POISONS = (0x00, 0xFF)


def switched(*names):
    """an A/B switch forces a route below the expected one: only the answer is checked"""
    return any(os.environ.get(v, "0") not in ("", "0") for v in names)


@pytest.fixture(scope="module")
def tctx():
    """a context that names every launch, however small (BHIP_KERNEL_TIMING is read when a context is created)"""
    old = os.environ.get("BHIP_KERNEL_TIMING")
    os.environ["BHIP_KERNEL_TIMING"] = "2"
    try:
        return ba.Context(0)
    finally:
        if old is None:
            del os.environ["BHIP_KERNEL_TIMING"]
        else:
            os.environ["BHIP_KERNEL_TIMING"] = old


def S(name, desc=False, nulls_first=True):
    return E.PhysicalSortExpr(col(name), descending=desc, nulls_first=nulls_first)


def run(plan):
    return helpers.concat(helpers.collect_product(plan))


def both(ctx, inputs, make_plan, tail_bits=0, route=None):
    """make_plan(*sources) over each input (batch, shifts) borrowed from a 0x00 and from a 0xFF arena -> ([got00, gotFF], the last
    plan); route(): asserts what the library reports, after each run"""
    got = []
    for poison in POISONS:
        plan = make_plan(*[oc.borrow(ctx, b, s, poison, tail_bits) for b, s in inputs])
        got.append(run(plan))
        if route is not None:
            route()
    return got, plan


def exact(ctx, inputs, make_plan, tail_bits=0, route=None, want=None):
    """(a) and (b) for a plan whose whole output compares bit for bit, in order"""
    got, plan = both(ctx, inputs, make_plan, tail_bits, route)
    want = plan_eval.collect(plan) if want is None else want
    for g in got:
        helpers.assert_bit_exact(g, want)
    helpers.assert_bit_exact(got[0], got[1])
    return got[0]


def without_floats(batch):
    return OrderedDict((k, c) for k, c in batch.items() if c.dtype not in og.FLOAT_TYPES)


def gated(ctx, inputs, make_plan, keys, tail_bits=0, route=None, want=None):
    """(a) and (b) for an aggregate: groups in any order, SUM / AVG over Float64 within the gate, everything else exact"""
    got, plan = both(ctx, inputs, make_plan, tail_bits, route)
    want = plan_eval.collect(plan) if want is None else want
    for g in got:
        helpers.assert_rows_equal(g, want, ordered=False, float_rtol=GATE, key_cols=keys)
    helpers.assert_rows_equal(without_floats(got[0]), without_floats(got[1]), ordered=False, key_cols=keys)
    return got[0]


# ---- the import edge ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,role,shift", [("Int64", "data", 4), ("Float64", "data", 12), ("Int32", "data", 2), ("Float32", "data", 6),
                                              ("Int16", "data", 1), ("UInt16", "data", 15), ("Boolean", "data", 4), ("Utf8", "offsets", 2),
                                              ("Int8", "validity", 4), ("Utf8", "validity", 1), ("Timestamp(Nanosecond)", "data", 4)])
def test_a_pointer_off_its_alignment_is_refused(ctx, dtype, role, shift):
    """a value's own width, 4 bytes for offsets, 8 bytes for bitmaps (include/ballista_hip.h): BHIP_EINVAL, on the host"""
    n = 70
    values = ["ab"] * n if dtype == "Utf8" else np.arange(n) % 2 == 0 if dtype == "Boolean" else np.arange(n)
    valid = np.arange(n) % 5 != 0 if role == "validity" else None
    b = OrderedDict([("ok", OCol("Int32", np.arange(n))), ("x", OCol(dtype, values, valid))])
    with pytest.raises(L.PlanError) as err:
        oc.borrow_batch(ctx, b, {("x", role): shift}, 0x00)
    assert err.value.code == L.EINVAL and "device column x: " + role in str(err.value)
    # the same column on its own alignment, off 16 bytes, is taken and read back as it is
    ok = {"data": 8, "offsets": 4, "validity": 8}
    helpers.assert_bit_exact(helpers.from_device(oc.borrow_batch(ctx, b, ok, 0xFF)), b)


def test_from_device_pointers_and_from_device_columns_read_back(ctx):
    """a fixed-width NULL-free batch goes through RecordBatch.from_device_pointers, any other through the column descriptors: both
    give the caller's values back, whatever lies around them"""
    n = 1025
    rng = np.random.default_rng(1)
    fixed = OrderedDict([("a", OCol("Int64", rng.integers(-2 ** 62, 2 ** 62, n))), ("b", OCol("Int8", rng.integers(-128, 128, n))),
                         ("c", OCol("Float32", rng.normal(0, 1, n).astype(np.float32))), ("d", OCol("UInt16", rng.integers(0, 2 ** 16, n)))])
    other = OrderedDict(fixed)
    other["s"] = OCol("Utf8", ["v%d" % i * (i % 3) for i in range(n)], rng.random(n) > 0.2)
    other["t"] = OCol("Boolean", rng.random(n) > 0.5, rng.random(n) > 0.2)
    shifts = {"a": 8, "b": 15, "c": 12, "d": 14, "s": 1, "offsets": 12, "validity": 8, "t": 8}
    for poison in POISONS:
        rb = oc.borrow_batch(ctx, fixed, shifts, poison)
        assert [rb.column_device(i)[0] % 16 for i in range(4)] == [8, 15, 12, 14]
        helpers.assert_bit_exact(helpers.from_device(rb), fixed)
        helpers.assert_bit_exact(helpers.from_device(oc.borrow_batch(ctx, other, shifts, poison)), other)


# ---- FilterExec: the range route ---------------------------------------------------------------------------------------------------------

RANGE_SIZES = [1023, 1024, 1025, 4 * 1024 + 1]          # a full tile, the ragged tail, the four-tile pack of the one-column form


def q6_batch(n, nullable=False):
    rng = np.random.default_rng(n)
    v = lambda share: (rng.random(n) > share) if nullable else None
    return OrderedDict([("d", OCol("Date32", rng.integers(8700, 9500, n), v(0.2))),
                        ("y", OCol("Float64", rng.integers(0, 11, n) / 100.0, v(0.3))),
                        ("q", OCol("Float64", rng.integers(1, 51, n).astype(np.float64))),
                        ("p", OCol("Int32", np.arange(n)))])


Q6_PRED = ((col("d") >= E.date32("1994-01-01")).and_(col("d") < E.date32("1995-01-01")).and_(col("y") >= lit(0.05))
           .and_(col("y") <= lit(0.07)).and_(col("q") < lit(24.0)))


def filter_route(tctx, name):
    other = {"range_bitmap": "scan_pred_bitmap", "scan_pred_bitmap": "range_bitmap"}[name]

    def check():
        ks = tctx.kernel_stats(reset=True)
        assert switched("BHIP_NO_RANGE_FILTER") or (name in ks and other not in ks), sorted(ks)
    return check


# the unconstrained column `p` is off 16 bytes in every case: only the columns the predicate reads decide the route
@pytest.mark.parametrize("shifts,route", [({}, "range_bitmap"), ({"y": 8}, "scan_pred_bitmap"), ({"q": 8}, "scan_pred_bitmap"),
                                          ({"d": 4}, "scan_pred_bitmap"), ({"d": 8}, "scan_pred_bitmap"), ({"d": 12}, "scan_pred_bitmap")])
def test_filter_q6_range(tctx, shifts, route):
    for n in RANGE_SIZES:
        b = q6_batch(n)
        tctx.kernel_stats(reset=True)
        got = exact(tctx, [(b, dict(shifts, p=4))], lambda src: ba.FilterExec(Q6_PRED, src), route=filter_route(tctx, route))
        assert 0 < og.batch_len(got) < n


@pytest.mark.parametrize("shift", oc.SHIFTS_4)
def test_filter_one_int32_range(tctx, shift):
    """range_bitmap32: one range over one Int32 column, eight rows per lane"""
    for n in RANGE_SIZES:
        rng = np.random.default_rng(n)
        b = OrderedDict([("i", OCol("Int32", np.concatenate([rng.integers(-100, 100, n - 2), [2 ** 31 - 1, -2 ** 31]]))),
                         ("p", OCol("Int64", np.arange(n)))])
        for pred in ((col("i") >= lit(10, E.INT32)).and_(col("i") < lit(60, E.INT32)), col("i") > lit(-2 ** 31, E.INT32)):
            tctx.kernel_stats(reset=True)
            exact(tctx, [(b, {"i": shift, "p": 8})], lambda src: ba.FilterExec(pred, src),
                  route=filter_route(tctx, "range_bitmap" if shift == 0 else "scan_pred_bitmap"))


@pytest.mark.parametrize("shifts,route", [({"validity": 8}, "range_bitmap"), ({"validity": 8, "y": 8}, "scan_pred_bitmap"),
                                          ({"validity": 8, "d": 4}, "scan_pred_bitmap"), ({"validity": 0, "d": 12}, "scan_pred_bitmap")])
def test_filter_range_over_nullable_columns(tctx, shifts, route):
    """the columns the predicate constrains may hold NULLs on the range route: their bitmaps are read as 64-bit words, 8 bytes past
    a 16-byte boundary as well"""
    for n in RANGE_SIZES:
        b = q6_batch(n, nullable=True)
        tctx.kernel_stats(reset=True)
        exact(tctx, [(b, shifts)], lambda src: ba.FilterExec(Q6_PRED, src), route=filter_route(tctx, route))
        i = OrderedDict([("i", OCol("Int32", b["d"].values - 9000, b["d"].valid)), ("p", b["p"])])
        tctx.kernel_stats(reset=True)
        exact(tctx, [(i, {"validity": 8, "i": shifts.get("d", 0)})], lambda src: ba.FilterExec(col("i") >= lit(10, E.INT32), src),
              route=filter_route(tctx, "range_bitmap" if "d" not in shifts else "scan_pred_bitmap"))


# ---- the Q1-shaped partial aggregate over a filter ------------------------------------------------------------------------------------------

Q1_ROWS = 65_536 + 1025        # the library names the kernel of launches from 65 536 rows up
_q1 = {}


def q1_case(group):
    """the input, its plan and the oracle's answer: computed once, shared by every placement"""
    if group not in _q1:
        b = q1_batch(Q1_ROWS, 5, vocab=("A", "N", "R"))
        pred, g = E.coerce(col("d") <= E.date32("1998-09-02"), Q1_SCHEMA), [(col(group), group)]
        make = lambda src: ba.HashAggregateExec(ba.plan.PARTIAL, g, AGGS_Q1, ba.FilterExec(pred, src))
        want = og.hash_aggregate(og.filter_batch(b, pred), ba.plan.PARTIAL, g, AGGS_Q1)
        _q1[group] = (b, make, want)
    return _q1[group]


def agg_route(ctx, lean):
    def check():
        ms, launches = ctx.kernel_time(reset=True)
        if lean:
            assert launches == 1 and on_expected_kernel(ctx.kernel_name())
        else:               # every scan + aggregate launch of 65 536 rows or more is timed under the name of the kernel that ran
            assert launches == 1 and ctx.kernel_name() in ("scan_agg_sop_kernel", "scan_agg_lowcard_kernel"), (launches, ctx.kernel_name())
    return check


@pytest.mark.parametrize("shifts,lean", [({}, True), ({"ks": 1, ("ks", "offsets"): 4, "kt": 15}, True), ({"x": 8}, False), ({"y": 8}, False),
                                         ({"z": 8}, False), ({"q": 8}, False), ({"d": 4}, False), ({"d": 12}, False), ({"ki": 4}, False),
                                         ({"ki": 8}, False)])
def test_q1_partial_aggregate_int_key(ctx, shifts, lean):
    """grouped by the Int32 column: every column the plan reads on 16 bytes -> the wide-load kernel (the Utf8 columns it does not read
    may lie anywhere); any one of them off 16 bytes -> another kernel, the same answer"""
    b, make, want = q1_case("ki")
    ctx.kernel_time(reset=True)
    got = gated(ctx, [(b, shifts)], make, ["ki"], route=agg_route(ctx, lean), want=want)
    assert og.batch_len(got) == 3


@pytest.mark.parametrize("shifts", [{}, {("ks", "offsets"): 4}, {("ks", "offsets"): 12, "ks": 15}, {"ks": 1}])
def test_q1_partial_aggregate_utf8_key(ctx, shifts):
    """borrowed string bytes have no slack behind them: never the wide-load kernel, wherever the offsets lie.  It is the ownership
    test of lean_bindable that turns these batches away, at every placement: this case checks the answers of the other kernels over
    offsets at 4 and 12 bytes past a 16-byte boundary, NOT the dispatch's own condition on the offsets' alignment, which no borrowed
    column can reach."""
    b, make, want = q1_case("ks")
    ctx.kernel_time(reset=True)
    gated(ctx, [(b, shifts)], make, ["ks"], route=agg_route(ctx, False), want=want)


# ---- Top-K: a limit over a sort -------------------------------------------------------------------------------------------------------------------

TOPK_SIZES = [1031, 4099]      # above SMALL_SORT_MAX (1024); not multiples of 4
TOPK_KS = [1, 37]
KEYS_4 = ["Int32", "Date32", "UInt32", "Float32"]
KEYS_8 = ["Int64", "UInt64", "Float64", "Date64", "Timestamp(Nanosecond)"]


def topk_key(dtype, n, rng):
    if dtype in og.FLOAT_TYPES:
        return sort_cases.float_special_column(dtype, n, rng)
    info = np.iinfo(og.NP_TYPES[dtype])
    v = rng.integers(info.min, info.max, n, dtype=np.int64 if info.min < 0 else np.uint64, endpoint=True).astype(og.NP_TYPES[dtype])
    v[rng.choice(n, 4, replace=False)] = [info.min, info.max, 0, info.max - 1]
    return OCol(dtype, v)


def topk_batch(dtype, n):
    rng = np.random.default_rng(n + len(dtype))
    return OrderedDict([("key", topk_key(dtype, n, rng)), ("t", OCol("Int32", rng.integers(0, 4, n))), ("p", OCol("Int32", np.arange(n)))])


def topk_passes(ctx, by_row):
    """the selection's passes over the key column ran in the expected form: 16-byte loads (topk_diff, topk_hist) or one row per
    thread (topk_diff_row, topk_hist_row); ctx names every launch"""
    ks = ctx.kernel_stats(reset=True)
    ran, other = (("topk_diff_row", "topk_hist_row"), ("topk_diff", "topk_hist"))[::1 if by_row else -1]
    assert switched("BHIP_NO_TOPK") or (ran[0] in ks and not set(other) & set(ks)), sorted(ks)


def check_topk(ctx, b, shifts, keys, ks, form, tail_bits=0, by_row=None):
    """one borrowed batch per poison serves every k; each result equals the oracle's first k rows of the stable sort"""
    srcs = [oc.borrow(ctx, b, shifts, poison, tail_bits) for poison in POISONS]
    for k in ks:
        got = []
        for src in srcs:
            plan = ba.GlobalLimitExec(ba.SortExec(keys, src), k)
            ctx.kernel_stats(reset=True)
            out = plan.collect()
            assert len(out) == 1
            got.append(helpers.from_device(out[0]))
            assert ctx.sort_limit_form() == form or switched("BHIP_NO_TOPK")
            if by_row is not None:
                topk_passes(ctx, by_row)
        want = plan_eval.collect(plan)
        assert og.batch_len(want) == k
        for g in got:
            helpers.assert_bit_exact(g, want)
        helpers.assert_bit_exact(got[0], got[1])


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype,shift", [(t, s) for t in KEYS_4 for s in oc.SHIFTS_4] + [(t, s) for t in KEYS_8 for s in oc.SHIFTS_8])
def test_topk_first_key_types(tctx, dtype, shift, desc):
    """16-byte loads on a 16-byte boundary, one row per thread off it: the same k rows"""
    for n in TOPK_SIZES:
        check_topk(tctx, topk_batch(dtype, n), {"key": shift, "validity": 8 if shift >= 8 else 0, "t": 12, "p": 4},
                   [S("key", desc=desc), S("t", desc=True)], TOPK_KS, "topk", by_row=shift != 0)


@pytest.mark.parametrize("shift", oc.SHIFTS_8)
@pytest.mark.parametrize("end", ["bin_255", "bin_0"])
def test_topk_kth_row_in_the_last_and_the_first_bin(ctx, end, shift):
    """ascending Int64 keys that differ in bytes 0..2: in the pass over byte 2 the k-th row lies in bin 255 (all but 20 rows
    carry 0xFF there) or in bin 0 (k + 60 rows carry 0x00); bytes 0 and 1 are distinct, so the candidates stay few"""
    for n in TOPK_SIZES:
        rng = np.random.default_rng(n)
        k = 37
        top = np.full(n, 0xFF) if end == "bin_255" else rng.integers(1, 256, n)
        few = rng.choice(n, 20 if end == "bin_255" else k + 60, replace=False)
        top[few] = rng.integers(0, 0xFF, len(few)) if end == "bin_255" else 0
        assert (top == 0xFF).sum() >= n - k + 1 if end == "bin_255" else (top == 0).sum() >= k
        b = OrderedDict([("key", OCol("Int64", (top.astype(np.int64) << 16) + rng.permutation(n))), ("p", OCol("Int32", np.arange(n)))])
        check_topk(ctx, b, {"key": shift, "p": 12}, [S("key")], [k], "topk")


@pytest.mark.parametrize("dtype,shift", [("Int16", 2), ("Int16", 14), ("Boolean", 8), ("Int8", 1), ("Int8", 15)])
def test_topk_unsupported_first_key_falls_back(ctx, dtype, shift):
    for n in TOPK_SIZES:
        rng = np.random.default_rng(n)
        key = OCol("Boolean", rng.random(n) > 0.5) if dtype == "Boolean" else topk_key(dtype, n, rng)
        b = OrderedDict([("key", key), ("f", OCol("Float32", rng.normal(0, 1, n).astype(np.float32))), ("p", OCol("Int32", np.arange(n)))])
        check_topk(ctx, b, {"key": shift, "f": 12, "p": 4}, [S("key"), S("f", desc=True)], TOPK_KS, "topk_fallback")


@pytest.mark.parametrize("nulls_first", [True, False])
@pytest.mark.parametrize("dtype,shift", [("Int32", 12), ("Int64", 8), ("Float64", 0)])
def test_topk_nullable_first_key(ctx, dtype, shift, nulls_first):
    """the key's validity 8 bytes past a 16-byte boundary; 20 NULLs: fewer than k = 37, more than k = 1"""
    for n in TOPK_SIZES:
        rng = np.random.default_rng(n)
        valid = np.ones(n, bool)
        valid[rng.choice(n, 20, replace=False)] = False
        key = topk_key(dtype, n, rng)
        b = OrderedDict([("key", OCol(dtype, key.values, valid)), ("t", OCol("Int32", rng.integers(0, 4, n))), ("p", OCol("Int32", np.arange(n)))])
        for desc in (False, True):
            check_topk(ctx, b, {"key": shift, "validity": 8, "t": 4, "p": 8}, [S("key", desc=desc, nulls_first=nulls_first), S("t", desc=True)],
                       TOPK_KS, "topk")


# ---- SortExec alone ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1025, 5000])
def test_sort_three_keys(ctx, n):
    """Float32 12 bytes past a 16-byte boundary, then Int64 at 8, then Utf8 with its offsets at 4 and its bytes at 1: few values
    per key, so that every key decides"""
    rng = np.random.default_rng(n)
    f = sort_cases.special_bits("Float32")[[0, 4, 10, 11, 17, 21]].view(np.float32)
    i = np.array([-2 ** 63, -1, 0, 2 ** 63 - 1, 1 << 32])
    s = ["", "a", "ab", "ab\0", "commonprefix-x", "commonprefix-y", "commonpr", "é"]
    b = OrderedDict([("f", OCol("Float32", f[rng.integers(0, len(f), n)], rng.random(n) > 0.05)),
                     ("i", OCol("Int64", i[rng.integers(0, len(i), n)])),
                     ("s", OCol("Utf8", [s[j] for j in rng.integers(0, len(s), n)], rng.random(n) > 0.05)),
                     ("p", OCol("Int32", np.arange(n)))])
    shifts = {"f": 12, "i": 8, "s": 1, ("s", "offsets"): 4, "validity": 8, "p": 4}
    for keys in ([S("f"), S("i", desc=True), S("s")], [S("f", desc=True, nulls_first=False), S("i"), S("s", desc=True, nulls_first=False)],
                 [S("s"), S("f")], [S("i"), S("f")]):
        exact(ctx, [(b, shifts)], lambda src: ba.SortExec(keys, src))


# ---- HashJoinExec ----------------------------------------------------------------------------------------------------------------------------------------

JOIN_BUILD, JOIN_PROBE = 300, 1025


def join_side(prefix, n, rng, k32, k64):
    words = ["", "a", "BUILDING", "seventeen-bytes-ky", "é日本"]
    return OrderedDict([(prefix + "k", OCol("Int32", k32)), (prefix + "w", OCol("Int64", k64)),
                        (prefix + "8", OCol("Int8", rng.integers(-128, 128, n))), (prefix + "16", OCol("Int16", rng.integers(-2 ** 15, 2 ** 15, n))),
                        (prefix + "f", OCol("Float64", rng.normal(0, 1, n), rng.random(n) > 0.1)),
                        (prefix + "s", OCol("Utf8", [words[j] for j in rng.integers(0, len(words), n)], rng.random(n) > 0.1)),
                        (prefix + "i", OCol("Int64", np.arange(n)))])


def join_shifts(prefix):
    return {prefix + "k": 4, prefix + "w": 8, prefix + "8": 1, prefix + "16": 2, prefix + "f": 8, prefix + "s": 15, (prefix + "s", "offsets"): 12,
            "validity": 8, prefix + "i": 8}


@pytest.mark.parametrize("on", [[("lk", "rk")], [("lw", "rw")], [("lk", "rk"), ("lw", "rw")]])
def test_inner_join_of_two_borrowed_sides(ctx, on):
    rng = np.random.default_rng(len(on))
    k32 = lambda n: rng.integers(-10, 10, n)
    k64 = lambda n: rng.integers(0, 5, n) * 10 ** 10 - 7
    left = join_side("l", JOIN_BUILD, rng, k32(JOIN_BUILD), k64(JOIN_BUILD))
    right = join_side("r", JOIN_PROBE, rng, k32(JOIN_PROBE), k64(JOIN_PROBE))
    got, plan = both(ctx, [(left, join_shifts("l")), (right, join_shifts("r"))], lambda l, r: ba.HashJoinExec(l, r, on, ba.plan.INNER))
    want = og.hash_join(left, right, on, "Inner")
    assert og.batch_len(want) > 1000
    for g in got:
        JT.assert_same_rows(g, want)
    JT.assert_same_rows(got[0], got[1])


def test_inner_join_on_a_unique_key(ctx):
    """a unique Int64 build key (the narrow table) 8 bytes past a 16-byte boundary on both sides"""
    rng = np.random.default_rng(9)
    left = join_side("l", JOIN_BUILD, rng, rng.integers(-60, 60, JOIN_BUILD), rng.permutation(3 * JOIN_BUILD)[:JOIN_BUILD] * 10 ** 10 - 5)
    right = join_side("r", JOIN_PROBE, rng, rng.integers(-60, 60, JOIN_PROBE), rng.integers(0, 3 * JOIN_BUILD, JOIN_PROBE) * 10 ** 10 - 5)
    on = [("lw", "rw")]
    got, plan = both(ctx, [(left, join_shifts("l")), (right, join_shifts("r"))], lambda l, r: ba.HashJoinExec(l, r, on, ba.plan.INNER))
    want = og.hash_join(left, right, on, "Inner")
    assert 100 < og.batch_len(want) < JOIN_PROBE
    for g in got:
        JT.assert_same_rows(g, want)
    JT.assert_same_rows(got[0], got[1])


# ---- the expression VM's narrow loads: the 4-byte word around a value reaches into poison -----------------------------------------------------------------

VM_SIZES = [1, 3, 4, 5, 63, 64, 65, 257]
VM_CASES = ([(t, s) for t in ("Int8", "UInt8") for s in (0, 1, 2, 3)] + [(t, s) for t in ("Int16", "UInt16") for s in (0, 2)] +
            [(t, s) for t in ("Int32", "Float32") for s in (0, 4, 12)] + [("Boolean", 0), ("Boolean", 8)])


def vm_batch(dtype, n):
    """x: NULL-free, the type's maximum in the last row; xn: nullable, the minimum in the last row"""
    rng = np.random.default_rng(n)
    if dtype == "Boolean":
        x, xn = rng.random(n) > 0.5, rng.random(n) > 0.5
        x[-1], xn[-1] = True, False
    else:
        t = og.NP_TYPES[dtype]
        info = np.finfo(t) if dtype == "Float32" else np.iinfo(t)
        draw = lambda: (rng.normal(0, 50, n).astype(t) if dtype == "Float32" else rng.integers(info.min, info.max, n, endpoint=True).astype(t))
        x, xn = draw(), draw()
        x[-1], xn[-1] = info.max, info.min
    valid = rng.random(n) > 0.2
    valid[-1] = True
    return OrderedDict([("x", OCol(dtype, x)), ("xn", OCol(dtype, xn, valid)), ("p", OCol("Int64", np.arange(n)))])


@pytest.mark.parametrize("dtype,shift", VM_CASES)
def test_vm_narrow_loads(ctx, dtype, shift):
    for n in VM_SIZES:
        b = vm_batch(dtype, n)
        shifts = {"x": shift, "xn": shift, "validity": 8, "p": 8}
        if dtype == "Boolean":
            exprs = [(E.NotExpr(col("x")), "not"), (col("x").and_(col("xn")), "and"), (col("xn"), "xn"), (col("x").eq(col("xn")), "eq")]
            pred = col("x")
        else:
            one = lit(1.0 if dtype == "Float32" else 1, dtype)
            exprs = [(col("x") + one, "plus"), (col("xn") - one, "minus"), (col("x") < col("xn"), "lt"), (col("xn").eq(lit(b["xn"].values[-1].item(), dtype)), "eq"),
                     (E.CastExpr(col("x"), "Int64"), "x64"), (E.CastExpr(col("xn"), "Int64"), "xn64"), (col("x"), "x"), (col("xn"), "xn")]
            pred = col("x") >= col("xn")
        got = exact(ctx, [(b, shifts)], lambda src: ba.ProjectionExec(exprs, src))
        if dtype not in ("Boolean", "Float32"):
            assert got["x64"].values[-1] == b["x"].values[-1] and got["xn64"].values[-1] == b["xn"].values[-1]
        exact(ctx, [(b, shifts)], lambda src: ba.FilterExec(pred, src))


# ---- Utf8 with no slack behind its bytes --------------------------------------------------------------------------------------------------------------

UTF8_SIZES = [64, 65, 1025]
UTF8_PLACES = [{"s": 1, ("s", "offsets"): 4, "validity": 8, "v": 8}, {"s": 15, ("s", "offsets"): 12, "validity": 0, "v": 0}]
LONG_KEY = "seventeen-bytes-k"


def utf8_batch(n, long_key=True):
    """NULL rows lie over values of their own (garbage offsets that are still monotone), one of them the literal the filters look
    for; the last row's string is shorter than 8 bytes and ends on the buffer's last byte"""
    assert len(LONG_KEY) == 17
    rng = np.random.default_rng(n)
    words = ["BUILDING", "BUILDINH", "BUILDIN", "MACHINERY", "AUTO", "AUT", "", "é日"] + ([LONG_KEY] if long_key else [])
    if not long_key:
        words = [w[:7] for w in words if len(w.encode()) <= 8]
    s = [words[j] for j in rng.integers(0, len(words), n)]
    valid = rng.random(n) > 0.15
    s[-1], valid[-1] = "AUTO", True
    for i in np.nonzero(~valid)[0]:
        s[i] = ("BUILDING", "AUTO")[i % 2]
    return OrderedDict([("s", OCol("Utf8", s, valid)), ("v", OCol("Int64", rng.integers(-1000, 1000, n))), ("p", OCol("Int32", np.arange(n)))])


@pytest.mark.parametrize("place", range(len(UTF8_PLACES)))
@pytest.mark.parametrize("n", UTF8_SIZES)
def test_utf8_equality_filters_and_the_gather_behind_them(tctx, n, place):
    """utf8_eq_bitmap reads 8 bytes per row where the buffer has them; the rows it keeps are gathered (take_utf8_copy)"""
    b = utf8_batch(n)

    def route():
        ks = tctx.kernel_stats(reset=True)
        assert "utf8_eq_bitmap" in ks or switched("BHIP_NO_UTF8_EQ_FILTER"), sorted(ks)
    for literal in ("BUILDING", "AUTO", "MACHINERY", ""):
        for pred in (col("s").eq(lit(literal)), col("s").ne(lit(literal))):
            tctx.kernel_stats(reset=True)
            exact(tctx, [(b, UTF8_PLACES[place])], lambda src: ba.FilterExec(pred, src), route=route)


@pytest.mark.parametrize("place", range(len(UTF8_PLACES)))
@pytest.mark.parametrize("n", UTF8_SIZES)
def test_utf8_substr_and_concat(ctx, n, place):
    b = utf8_batch(n)
    fn = lambda name, *args: E.ScalarFunctionExpr(name, list(args))
    exprs = [(fn("substr", col("s"), lit(2), lit(3)), "sub"), (fn("concat", col("s"), lit("|"), col("s")), "cat"), (col("s"), "s")]
    ok = b["s"].is_valid()
    want = OrderedDict([("sub", OCol("Utf8", [s[1:4] if k else "" for s, k in zip(b["s"].values, ok)], ok)),
                        ("cat", OCol("Utf8", [s + "|" + s if k else "" for s, k in zip(b["s"].values, ok)], ok)),
                        ("s", OCol("Utf8", [s if k else "" for s, k in zip(b["s"].values, ok)], ok))])
    exact(ctx, [(b, UTF8_PLACES[place])], lambda src: ba.ProjectionExec(exprs, src), want=want)


@pytest.mark.parametrize("long_key", [False, True])
@pytest.mark.parametrize("place", range(len(UTF8_PLACES)))
@pytest.mark.parametrize("n", UTF8_SIZES)
def test_utf8_group_by(ctx, n, place, long_key):
    """keys of at most 7 bytes (the packed key), and with one of 17 bytes among them; Int64 sums and counts: exact"""
    b = utf8_batch(n, long_key)
    g = [(col("s"), "s")]
    aggs = [E.Sum(col("v"), "sv"), E.Count(col("v"), "n"), E.Min(col("v"), "lo")]
    make = lambda src: ba.HashAggregateExec(ba.plan.FINAL, g, aggs, ba.MergeExec(ba.HashAggregateExec(ba.plan.PARTIAL, g, aggs, src)))
    got = gated(ctx, [(b, UTF8_PLACES[place])], make, ["s"])
    assert og.batch_len(got) >= 5


# ---- the bits past the last row in a bitmap's last word ------------------------------------------------------------------------------------------------------

TAIL_SIZES = [1, 63, 65, 1000]


def tail_batch(n):
    rng = np.random.default_rng(n)
    valid, bvalid = rng.random(n) > 0.3, rng.random(n) > 0.3
    valid[-1], bvalid[-1] = False, False                      # the last real bit is 0 right below the set tail bits
    if n > 1:
        valid[0] = True
    return OrderedDict([("a", OCol("Int64", rng.integers(-10 ** 6, 10 ** 6, n), valid)), ("b", OCol("Boolean", rng.random(n) > 0.5, bvalid)),
                        ("c", OCol("Boolean", np.arange(n) % 3 == 0)), ("g", OCol("Int32", rng.integers(0, 3, n))), ("o", OCol("Int32", rng.permutation(n)))])


def tail_runs(ctx, b, make_plan, compare, want=None):
    """the plan over tail_bits = 0 and tail_bits = 1, each over both poisons: four runs, one expectation"""
    got = []
    for tail_bits in (0, 1):
        runs, plan = both(ctx, [(b, {"validity": 8, "b": 8, "c": 0, "a": 8})], make_plan, tail_bits)
        got += runs
    want = plan_eval.collect(plan) if want is None else want
    for g in got:
        compare(g, want)
        compare(g, got[0])


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_bitmap_tail_bits_filter_aggregate_sort(ctx, n):
    b = tail_batch(n)
    unordered = lambda keys: lambda g, w: helpers.assert_rows_equal(g, w, ordered=False, key_cols=keys)
    for pred in (col("b"), col("c"), E.NotExpr(col("b")), E.IsNullExpr(col("a")), col("a") > lit(0), E.IsNotNullExpr(col("b")).and_(col("c"))):
        tail_runs(ctx, b, lambda src: ba.FilterExec(pred, src), helpers.assert_bit_exact)
    aggs = [E.Sum(col("a"), "s"), E.Count(col("a"), "n"), E.Count(col("b"), "nb"), E.Count(lit(1, E.UINT8), "rows")]
    for g in ([], [(col("g"), "g")]):
        make = lambda src: ba.HashAggregateExec(ba.plan.FINAL, g, aggs, ba.MergeExec(ba.HashAggregateExec(ba.plan.PARTIAL, g, aggs, src)))
        tail_runs(ctx, b, make, unordered([name for _, name in g] or None))
    for keys in ([S("a"), S("o")], [S("a", desc=True, nulls_first=False), S("o")], [S("b"), S("c", desc=True), S("o")]):
        tail_runs(ctx, b, lambda src: ba.SortExec(keys, src), helpers.assert_bit_exact)


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_bitmap_tail_bits_window(ctx, n):
    b = tail_batch(n)
    part, order = [col("g")], [K.asc("o")]
    ws = [K.W("COUNT", "a", "cnt"), K.W("COUNT", "b", "cnt_b"), K.W("LAG", "a", "lag"), K.W("LAG", "b", "lag_b", offset=2), K.W("LEAD", "c", "lead_c")]
    want = K.restate(K.sorted_input(b, part, order), part, order, ws)
    tail_runs(ctx, b, lambda src: ba.WindowAggExec(part, order, ws, src), helpers.assert_bit_exact, want=want)


# ---- partition slices as the next operator's input ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def slices(ctx):
    table = oc.slice_table(oc.slice_seed())
    m = helpers.memory_exec(ctx, [[table]])
    return table, lambda: ba.MergeExec(ba.RepartitionExec(m, ba.Partitioning.Hash([col("k")], oc.SLICE_PARTS)))


def test_the_slices_start_off_alignment(ctx, slices):
    table, merged = slices
    rep = merged().children()[0]
    names = list(table)
    first = oc.slice_first(table)
    residues = {name: [] for name in names}
    for p in range(oc.SLICE_PARTS):
        batches = list(rep.execute(p))
        assert sum(x.num_rows for x in batches) == first[p + 1] - first[p]
        for x in batches:
            for i, name in enumerate(names):
                residues[name].append(x.column_device(i)[0] % 16)
    assert any(r % 2 == 1 for r in residues["i8"]), residues
    assert 8 in residues["f64"] and any(r in (4, 12) for r in residues["d"]) and any(r % 4 == 2 for r in residues["i16"]), residues


def test_operators_over_the_slices(ctx, slices):
    table, merged = slices
    pred = ((col("d") >= E.date32("1994-01-01")).and_(col("d") < E.date32("1997-01-01")).and_(col("f64") >= lit(0.02)).and_(col("f64") <= lit(0.07)))
    plan = ba.FilterExec(pred, merged())
    got = run(plan)
    helpers.assert_bit_exact(got, plan_eval.collect(plan))
    assert 100 < og.batch_len(got) < oc.SLICE_ROWS
    for keys in ([S("f32", desc=True), S("p")], [S("d"), S("p")], [S("f64"), S("p", desc=True)]):
        plan = ba.GlobalLimitExec(ba.SortExec(keys, merged()), 37)
        out = plan.collect()
        assert len(out) == 1 and (ctx.sort_limit_form() == "topk" or switched("BHIP_NO_TOPK"))
        helpers.assert_bit_exact(helpers.from_device(out[0]), plan_eval.collect(plan))
    exprs = [(col("i8") + lit(1, "Int8"), "a"), (E.CastExpr(col("i16"), "Int64"), "b"), (E.CastExpr(col("i8"), "Int16") < col("i16"), "c"),
             (col("i8"), "i8"), (col("i16"), "i16"), (col("f32") * lit(2.0, "Float32"), "f")]
    plan = ba.ProjectionExec(exprs, merged())
    helpers.assert_bit_exact(run(plan), plan_eval.collect(plan))
    for g in ([], [(col("i8"), "i8")]):
        aggs = [E.Sum(col("f64") * (lit(1.0) - col("f64")), "s"), E.Avg(col("f64"), "a"), E.Count(lit(1, E.UINT8), "n"), E.Sum(col("i16"), "si")]
        plan = ba.HashAggregateExec(ba.plan.FINAL, g, aggs, ba.MergeExec(ba.HashAggregateExec(ba.plan.PARTIAL, g, aggs, ba.FilterExec(pred, merged()))))
        helpers.assert_rows_equal(run(plan), plan_eval.collect(plan), ordered=False, float_rtol=GATE, key_cols=[name for _, name in g] or None)


def test_routes_over_the_slices(tctx):
    """in a context that names every launch: the slices that start off 16 bytes do not take range_bitmap, nor the 16-byte loads of
    the selection"""
    table = oc.slice_table(oc.slice_seed())
    m = helpers.memory_exec(tctx, [[table]])
    plan = ba.FilterExec(col("d") >= E.date32("1995-01-01"), ba.MergeExec(ba.RepartitionExec(m, ba.Partitioning.Hash([col("k")], oc.SLICE_PARTS))))
    tctx.kernel_stats(reset=True)
    got = run(plan)
    ks = tctx.kernel_stats(reset=True)
    helpers.assert_bit_exact(got, plan_eval.collect(plan))
    # ... and the limit over a sort reads partition 2, the one batch large enough to select from, one row per thread
    for key in ("d", "f64"):
        plan = ba.GlobalLimitExec(ba.SortExec([S(key), S("p")], ba.MergeExec(ba.RepartitionExec(m, ba.Partitioning.Hash([col("k")], oc.SLICE_PARTS)))), 37)
        tctx.kernel_stats(reset=True)
        out = plan.collect()
        helpers.assert_bit_exact(helpers.from_device(out[0]), plan_eval.collect(plan))
        if not switched("BHIP_NO_PARTITION_SCATTER"):
            topk_passes(tctx, True)
    if not switched("BHIP_NO_RANGE_FILTER", "BHIP_NO_PARTITION_SCATTER"):
        assert ks.get("range_bitmap", (0, 0))[1] == 1 and ks.get("scan_pred_bitmap", (0, 0))[1] == 2, ks       # partition 0 starts the buffer; 1 and 2 at odd rows
