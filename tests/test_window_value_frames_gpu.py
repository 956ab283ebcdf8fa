"""WindowAggExec's RANGE and GROUPS frames on the device against the row-by-row restatement (tests/window_value_frame_cases.py, itself
checked against sqlite3 and by hand in test_window_value_frames_cpu.py).

The expected value is the restatement applied to the oracle's SortExec over the operator's own sort keys, as in
test_window_frames_gpu.py; every batch carries its input row number (rn).  Integers, counts, validity and gathered values compare bit
for bit, and so do SUM of floats and every AVG over a frame without an unbounded side, over positive uniform inputs (u) as well as
exact ones (f): the additions run in row order from +0.0.  MIN / MAX over floats may return either zero.  A float sum whose frame
starts UNBOUNDED PRECEDING has the tile-tree order of the running sums: within the project's 1e-6 gate on u.

Sizes 1, 2, 65, T - 1, T, T + 1, 3T + 1 against the six partition shapes of window_cases (last_row: a one-row partition on the last
row), the frame list of the CPU test under the four orderings; every key type; keys at the ends of Int64 and UInt64; float specials as
keys; equivalence with ROWS frames over a consecutive key, from the device; narrow frames far apart (the global-memory walk of
window_slide_value); the limit found when the query runs; reproducibility; launch accounting."""
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
from tests import window_cases as K, window_value_frame_cases as VK
from tests.window_value_frame_cases import CUR, F, G, R, W, asc

pytestmark = pytest.mark.gpu

RTOL = 1e-6                                    # SUM / AVG over Float64
T = K.T
CAP = ba.plan.WINDOW_SLIDE_MAX_ROWS
STAGE = ba.plan.WINDOW_SLIDE_STAGE_ROWS
SIZES = [1, 2, 65, T - 1, T, T + 1, 3 * T + 1]
SLIDING = (("SUM", "f"), ("SUM", "u"), ("AVG", "u"), ("MIN", "g"), ("MAX", "f"))                 # what window_slide_value serves
ANY_WIDTH = (("COUNT", "i64"), ("SUM", "i64"), ("FIRST_VALUE", "i64"), ("LAST_VALUE", "f"))


def expected(m, partition_by, order_by, ws):
    keys = K.sort_keys(partition_by, order_by)
    in_order = plan_eval.collect(ba.SortExec(keys, m)) if keys else plan_eval.collect(m)
    return VK.restate(in_order, partition_by, order_by, ws)


def without(batch, names):
    return OrderedDict((k, c) for k, c in batch.items() if k not in names)


def run(ctx, batches, partition_by, order_by, ws, chunk=40):
    """the operator (a few of them: `chunk` expressions each) over one partition holding `batches` -> (its input plan, one batch)"""
    m = helpers.memory_exec(ctx, [batches])
    got = None
    for at in range(0, len(ws), chunk):
        out = helpers.collect_product(ba.WindowAggExec(partition_by, order_by, ws[at:at + chunk], m))
        assert len(out) == 1
        got = out[0] if got is None else OrderedDict(list(got.items()) + [(w.name, out[0][w.name]) for w in ws[at:at + chunk]])
        assert np.array_equal(got["rn"].values, out[0]["rn"].values)
    return m, got


def check(ctx, batches, partition_by, order_by, ws, within_gate=(), any_zero_sign=(), chunk=40):
    m, got = run(ctx, batches, partition_by, order_by, ws, chunk)
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
    def side(v):
        if v is None:
            return "u"
        if v is CUR:
            return "c"
        return ("m%s" % -v if v < 0 else "p%s" % v).replace(".", "d").replace("+", "")
    return ("r" if isinstance(frame, R) else "g" if isinstance(frame, G) else "w") + side(frame.start) + "_" + side(frame.end)


def exprs_over(frames, sliding=SLIDING, any_width=ANY_WIDTH):
    """-> (expressions, names within the gate, names with either zero): every function a frame takes"""
    ws, gate, zero = [], [], []
    for fr in frames:
        t = tag(fr)
        funs = list(any_width) + ([] if fr.end is None and fr.start is not None else list(sliding))       # (the four from an offset to UNBOUNDED FOLLOWING are refused)
        for fun, arg in funs:
            name = f"{fun}_{arg}_{t}"
            ws.append(W(fun, arg, name, frame=fr))
            if fun in ("MIN", "MAX") and arg == "f":
                zero.append(name)
            elif fr.start is None and arg == "u":
                gate.append(name)
    return ws, gate, zero


# ---- every size x every partition shape, the CPU test's frames, the four orderings --------------------------------------------------------

from tests.test_window_value_frames_cpu import ONE_KEY_FRAMES                 # noqa: E402  (R and G, both sides of the row, unbounded sides)

ORDERINGS = [(False, True), (True, False), (False, False), (True, True)]      # (descending, nulls_first)


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_value_frames_at_every_size_and_partition_shape(ctx, n, shape):
    """the ordering rotates with (size, shape): each of the four meets every size and every shape"""
    descending, nulls_first = ORDERINGS[(SIZES.index(n) + K.SHAPES.index(shape)) % 4]
    batch = VK.table(n, shape, seed=n + len(shape))
    ws, gate, zero = exprs_over(ONE_KEY_FRAMES)
    got = check(ctx, split(batch, [n // 3]), [col("p")], [asc("o", descending, nulls_first)], ws + [W("ROW_NUMBER", None, "row_number", frame=G(-1, 1))],
                within_gate=gate, any_zero_sign=zero)
    rows = got["row_number"].values
    heads = rows == 1
    lasts = np.r_[heads[1:], True]
    # the case is what it says: partitions lie where the shape puts them, frames before / after the row are empty at a partition's ends
    assert not got["FIRST_VALUE_i64_gp1_p2"].is_valid()[lasts].any() and not got["COUNT_i64_gm3_m1"].values[heads].any()
    assert (got["COUNT_i64_rc_c"].values <= got["COUNT_i64_gm1_p1"].values).all()
    if shape == "one_partition":
        assert list(np.nonzero(heads)[0]) == [0]
    elif shape == "every_row":
        assert heads.all() and not got["COUNT_i64_rp1_p5"].values[got["o"].is_valid()].any()          # (a NULL key: the row's peers, itself)
    elif shape == "last_row" and n > 1:
        assert heads[-1] and rows[-2] == n - 1


# ---- key types and extremes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(VK.KEY_TYPES))
def test_every_key_type(ctx, key):
    n = T + 1
    batch = VK.table(n, "tile_ends", seed=5 + len(key), key=key)
    s = lambda m: VK.step(key, m)
    frames = [R(s(-2), CUR), R(s(-3), s(3)), R(s(1), s(5)), R(s(-6), s(-2)), R(None, s(-1)), R(s(-1), None), R(s(0), s(0)), G(-1, 1)]
    ws, gate, zero = exprs_over(frames)
    for descending, nulls_first in ((False, True), (True, False)):
        got = check(ctx, split(batch, [400]), [col("p")], [asc("o", descending, nulls_first)], ws, within_gate=gate, any_zero_sign=zero)
        assert got["o"].dtype == key and got[f"COUNT_i64_{tag(frames[1])}"].values.max() > 4 and not got[f"COUNT_i64_{tag(frames[2])}"].values.all()


@pytest.mark.parametrize("key", ["Int64", "UInt64"])
def test_keys_at_the_ends_of_the_type_do_not_wrap(ctx, key):
    """offsets of +-2^62 and +-(2^63 - 1) over keys at both ends of the type: the comparison is exact"""
    n = 300
    rng = np.random.default_rng(3)
    lo64, hi64 = -2**63, 2**63 - 1
    if key == "Int64":
        pool = np.array([lo64, lo64 + 1, -2**62 - 1, -2**62, -1, 0, 1, 2**62, hi64 - 1, hi64], np.int64)
    else:
        pool = np.array([0, 1, 2**62, 2**63 - 1, 2**63, 2**63 + 1, 2**63 + 2**62, 2**64 - 2, 2**64 - 1], np.uint64)
    batch = OrderedDict([("p", OCol("Int32", rng.integers(0, 2, n).astype(np.int32))), ("o", OCol(key, rng.choice(pool, n), rng.random(n) > 0.05)),
                         ("i64", OCol("Int64", rng.integers(-100, 100, n))), ("f", OCol("Float64", rng.integers(-64, 64, n) / 8.0)),
                         ("u", OCol("Float64", rng.uniform(0.5, 2.0, n))), ("g", OCol("Int32", rng.integers(-9, 9, n).astype(np.int32))),
                         ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])
    frames = [R(-hi64, hi64), R(-2**62, 2**62), R(2**62, hi64), R(-hi64, -2**62), R(lo64, CUR), R(1, hi64), R(hi64, hi64), R(lo64, lo64), R(None, -2**62), R(2**62, None)]
    ws, gate, zero = exprs_over(frames)
    for descending, nulls_first in ((False, True), (True, False)):
        got = check(ctx, [batch], [col("p")], [asc("o", descending, nulls_first)], ws, within_gate=gate, any_zero_sign=zero)
        counts = got[f"COUNT_i64_{tag(R(-hi64, hi64))}"].values
        assert counts.min() >= 1 and len(set(counts.tolist())) > 2                     # neither everything nor nothing: nothing wrapped into place


@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_float_specials_as_the_order_key(ctx, dtype):
    """NaNs of both signs, infinities, both zeros, denormals and NULLs in the key: a NaN never qualifies and takes its peers; OFFSET 0
    takes the two zeros together where CURRENT ROW keeps them apart"""
    n = 400
    rng = np.random.default_rng(n)
    batch = OrderedDict([("o", sort_cases.float_special_column(dtype, n, rng)), ("p", OCol("Int32", rng.integers(0, 2, n).astype(np.int32))),
                         ("i64", OCol("Int64", rng.integers(-100, 100, n))), ("f", OCol("Float64", rng.integers(-64, 64, n) / 8.0)),
                         ("u", OCol("Float64", rng.uniform(0.5, 2.0, n))), ("g", OCol("Int32", rng.integers(-9, 9, n).astype(np.int32))),
                         ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])
    frames = [R(0.0, 0.0), R(CUR, CUR), R(-1.0, 1.0), R(-1e300, 1e300), R(1.0, 1e30), R(-1e30, -1e-30), R(None, 0.5), R(-0.5, None), R(-0.0, CUR), R(5e-324, None)]
    ws, gate, zero = exprs_over(frames)
    for descending, nulls_first in ((False, True), (True, False)):
        got = check(ctx, [batch], [], [asc("o", descending, nulls_first)], ws, within_gate=gate, any_zero_sign=zero)
        zero_rows = got["o"].is_valid() & (got["o"].values == 0)
        assert len(set(np.signbit(got["o"].values[zero_rows]).tolist())) == 2         # both zeros are there, in one partition
        assert (got[f"COUNT_i64_{tag(R(0.0, 0.0))}"].values[zero_rows] > got[f"COUNT_i64_{tag(R(CUR, CUR))}"].values[zero_rows]).all()
        nans = got["o"].values[got["o"].is_valid() & np.isnan(got["o"].values)]
        assert len(set(np.signbit(nans).tolist())) == 2                               # and NaNs of both signs


def test_an_all_equal_key_makes_the_partition_one_peer_group(ctx):
    n = T + 1
    batch = VK.table(n, "tile_ends", seed=8)
    batch["o"] = OCol("Int64", np.full(n, 7, np.int64))
    frames = [R(CUR, CUR), R(-1, 1), R(0, 0), G(-1, 1), G(CUR, CUR), G(1, 2), R(1, 2), R(None, 0), G(-2, -1)]
    ws, gate, zero = exprs_over(frames)
    got = check(ctx, split(batch, [500]), [col("p")], [asc("o")], ws + [E.count_star("part", "PARTITION")], within_gate=gate, any_zero_sign=zero)
    for fr in frames[:5]:
        assert np.array_equal(got[f"COUNT_i64_{tag(fr)}"].values, got["COUNT_i64_rc_c"].values)
    assert not got["COUNT_i64_gp1_p2"].values.any() and not got["COUNT_i64_rp1_p2"].values.any() and got["part"].values.max() > 300


# ---- over a consecutive key RANGE and GROUPS are ROWS: from the device, bit for bit ---------------------------------------------------

def consecutive_key_table(n, shape, seed):
    """window_cases.table with o = the row's number inside its partition, in the order the table leaves it in (unique, consecutive)"""
    t = K.table(n, shape, seed)
    rng = np.random.default_rng(seed + 1)
    p = np.asarray(t["p"].values)
    o = np.zeros(n, np.int64)
    for v in np.unique(p):
        at = np.nonzero(p == v)[0]
        o[at] = rng.permutation(len(at))
    t["o"] = OCol("Int64", o)
    return t


EQUIVALENT = [("three_tiles", 3 * T + 1, (1, 0)), ("tile_ends", 3 * T + 1, (2, 2)), ("three_tiles", 3 * T + 1, (63, 0)), ("one_partition", 5 * T + 1, (T, 0)),
              ("one_partition", 5 * T + 1, (CAP - 1, 0)), ("one_partition", 5 * T + 1, (STAGE - T - 1, 0)), ("one_partition", 5 * T + 1, ((STAGE - T) // 2, (STAGE - T) // 2)),
              ("three_tiles", 5 * T + 1, (3, STAGE - T - 2))]


@pytest.mark.parametrize("shape, n, ab", EQUIVALENT, ids=["%s-%d-%d" % (s, ab[0], ab[1]) for s, _, ab in EQUIVALENT])
def test_over_a_consecutive_key_range_and_groups_are_rows(ctx, shape, n, ab):
    """a + b + T rows is an interior tile's span: the last three cases put it one below, at and one above the staged-span budget"""
    a, b = ab
    batch = consecutive_key_table(n, shape, seed=a + b)
    funs = [("SUM", "f"), ("SUM", "u"), ("AVG", "u"), ("AVG", "i64"), ("MIN", "g"), ("MAX", "f"), ("MIN", "i64"), ("MAX", "u"), ("COUNT", "i64"), ("SUM", "i64"),
            ("COUNT", "g"), ("FIRST_VALUE", "i64"), ("LAST_VALUE", "f")]
    ws = [W(fun, arg, f"{kind}_{fun}_{arg}", frame=fr) for kind, fr in (("rows", F(-a, b)), ("range", R(-a, b)), ("groups", G(-a, b))) for fun, arg in funs]
    ws.append(W("ROW_NUMBER", None, "row_number"))
    _, got = run(ctx, split(batch, [n // 2]), [col("p")], [asc("o")], ws)
    assert np.array_equal(got["o"].values + 1, got["row_number"].values.astype(np.int64))          # the key is what the case says
    rows = OrderedDict((f"{fun}_{arg}", got[f"rows_{fun}_{arg}"]) for fun, arg in funs)
    for kind in ("range", "groups"):
        helpers.assert_bit_exact(OrderedDict((f"{fun}_{arg}", got[f"{kind}_{fun}_{arg}"]) for fun, arg in funs), rows)
    star = helpers.collect_product(ba.WindowAggExec([col("p")], [asc("o")], [E.count_star("w", R(-a, b))], helpers.memory_exec(ctx, [[batch]])))[0]["w"].values
    assert star.max() == min(a + b + 1, int(np.bincount(np.asarray(batch["p"].values)).max()))        # the frame reaches its full width somewhere


# ---- narrow frames far apart: the global-memory walk -------------------------------------------------------------------------------------

def test_narrow_frames_that_lie_far_apart(ctx):
    """Tile 0 holds two clusters of keys, 0 .. 511 and 1000 .. 1511.  Under (+5000 FOLLOWING, +5005 FOLLOWING) the first cluster's
    frames land on the rows with keys 5000 .. 5516, the second's on 6000 .. 6516, and about 8T rows of key 5700 lie between that no
    frame covers: every frame holds at most 6 rows, the tile's span more than nine tiles"""
    half, c = T // 2, 5000
    keys = np.concatenate([np.arange(half), 1000 + np.arange(half), c + np.arange(half + 5), np.full(8 * T, c + 700), 1000 + c + np.arange(half + 5)]).astype(np.int64)
    n = len(keys)
    assert n <= 12 * T
    rng = np.random.default_rng(21)
    perm = rng.permutation(n)
    batch = OrderedDict([("o", OCol("Int64", keys[perm])), ("f", OCol("Float64", rng.integers(-1024, 1025, n) / 8.0, rng.random(n) > 0.1)),
                         ("u", OCol("Float64", rng.uniform(0.5, 2.0, n))), ("g", OCol("Int32", rng.integers(-100, 100, n).astype(np.int32), rng.random(n) > 0.1)),
                         ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])
    fr = R(c, c + 5)
    ws = [W("SUM", "f", "sum_f", frame=fr), W("SUM", "u", "sum_u", frame=fr), W("AVG", "u", "avg_u", frame=fr), W("AVG", "g", "avg_g", frame=fr),
          W("MIN", "g", "min_g", frame=fr), W("MAX", "f", "max_f", frame=fr), W("MIN", "u", "min_u", frame=fr), W("MAX", "g", "max_g", frame=fr),
          W("COUNT", "rn", "rows", frame=fr), W("FIRST_VALUE", "o", "first", frame=fr), W("LAST_VALUE", "o", "last", frame=fr)]
    got = check(ctx, split(batch, [3000]), [], [asc("o")], ws, any_zero_sign=["max_f"])
    # from the data: tile 0's frames are narrow and its span exceeds what is staged
    in_order = K.sorted_input(batch, [], [asc("o")])
    lo, hi = VK.frame_bounds(in_order, [], [asc("o")], fr)
    assert all(lo[i] is not None and hi[i] - lo[i] + 1 == 6 for i in range(T))
    assert max(hi[:T]) - min(lo[:T]) + 1 > STAGE and max(hi[:T]) - min(lo[:T]) + 1 > 9 * T
    assert got["rows"].values[:T].tolist() == [6] * T and not got["rows"].values[T:].any()
    assert np.array_equal(got["first"].values[:T], np.asarray(got["o"].values[:T]) + c) and np.array_equal(got["last"].values[:T], np.asarray(got["o"].values[:T]) + c + 5)


# ---- the limit that only the data knows -------------------------------------------------------------------------------------------------

def equal_keys(n):
    rng = np.random.default_rng(n)
    return OrderedDict([("o", OCol("Int64", np.full(n, 3, np.int64))), ("f", OCol("Float64", rng.integers(-1024, 1025, n) / 8.0)),
                        ("i64", OCol("Int64", rng.integers(-10**6, 10**6, n))), ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])


def test_the_widest_frame_is_found_when_the_query_runs(ctx):
    fr = R(CUR, CUR)
    got = check(ctx, [equal_keys(CAP)], [], [asc("o")], [W("SUM", "f", "s", frame=fr)])
    assert got["s"].is_valid().all() and len(set(got["s"].values.tolist())) == 1
    batch = equal_keys(CAP + 1)
    for fun in ("SUM", "AVG", "MIN", "MAX"):
        plan = ba.WindowAggExec([], [asc("o")], [W("COUNT", "i64", "c", frame=fr), W(fun, "f", "s", frame=fr)], helpers.memory_exec(ctx, [[batch]]))   # the plan is made
        with pytest.raises(ba.NotImplementedOnGpu, match=rf"{fun}\(Float64\) over RANGE BETWEEN CURRENT ROW AND CURRENT ROW: the widest frame holds {CAP + 1} rows"):
            helpers.collect_product(plan)
    with pytest.raises(ba.NotImplementedOnGpu, match=rf"AVG\(Int64\) over GROUPS BETWEEN 1 PRECEDING AND CURRENT ROW: the widest frame holds {CAP + 1} rows; a frame wider than {CAP} rows"):
        helpers.collect_product(ba.WindowAggExec([], [asc("o")], [W("AVG", "i64", "a", frame=G(-1, CUR))], helpers.memory_exec(ctx, [[batch]])))
    # what takes every width does, over the same rows and the same frame
    got = check(ctx, [batch], [], [asc("o")], [W("COUNT", "i64", "c", frame=fr), W("SUM", "i64", "s", frame=fr), W("LAST_VALUE", "f", "l", frame=fr),
                                               W("FIRST_VALUE", "i64", "first", frame=G(CUR, 1))])
    assert (got["c"].values == CAP + 1).all()
    # ... and the context goes on: an ordinary query, correct
    again = check(ctx, split(K.table(T + 1, "tile_ends", seed=4), [300]), [col("p")], [asc("o")], K.standard_exprs())
    assert og.batch_len(again) == T + 1


# ---- the same bits whatever the batches, and twice from one plan; no order keys ------------------------------------------------------------

def test_float_sums_over_value_frames_have_the_same_bits_in_every_run(ctx):
    batch = VK.table(3 * T + 1, "three_tiles", seed=11)
    ws = [W("SUM", "u", "range6", frame=R(-6, CUR)), W("AVG", "u", "groups3", frame=G(-1, 1)), W("SUM", "u", "wide", frame=R(-300, 0)),
          W("AVG", "f", "after", frame=R(3, 70)), W("MIN", "u", "min", frame=G(-2, 0)), W("ROW_NUMBER", None, "row_number")]
    order = [asc("o", True, False)]
    plan = ba.WindowAggExec([col("p")], order, ws, helpers.memory_exec(ctx, [split(batch, [1000, 1700])]))
    a, b = (helpers.concat(helpers.collect_product(plan)) for _ in range(2))
    c = helpers.concat(helpers.collect_product(ba.WindowAggExec([col("p")], order, ws, helpers.memory_exec(ctx, [[batch]]))))
    d = helpers.concat(helpers.collect_product(ba.WindowAggExec([col("p")], order, ws, helpers.memory_exec(ctx, [split(batch, [1, 64, 65, 2 * T])]))))
    for other in (b, c, d):
        helpers.assert_bit_exact(other, a)
    # ... and they are the bits of the plain loop
    helpers.assert_bit_exact(a, VK.restate(K.sorted_input(batch, [col("p")], order), [col("p")], order, ws))


def test_without_order_by_the_partition_is_one_peer_group(ctx):
    batch = K.table(2 * T + 9, "tile_ends", seed=2, strings=True)
    ws = [W("SUM", "u", "s", frame=R(CUR, CUR)), W("LAST_VALUE", "s", "l", frame=G(CUR, CUR)), W("COUNT", "g", "c", frame=G(-1, 1)), W("MIN", "i64", "m", frame=G(0, 5)),
          W("COUNT", "g", "none", frame=G(1, 2)), W("FIRST_VALUE", "s", "first", frame=R(CUR, None)), E.count_star("part", "PARTITION")]
    got = check(ctx, split(batch, [700]), [col("p")], [], ws)
    assert np.array_equal(got["c"].values, check(ctx, [batch], [col("p")], [], [W("COUNT", "g", "c", frame="PARTITION")])["c"].values) and not got["none"].values.any()
    check(ctx, split(batch, [700]), [], [], ws)


# ---- launches ---------------------------------------------------------------------------------------------------------------------------------

def test_each_launch_is_timed_under_its_own_name():
    mp = pytest.MonkeyPatch()
    mp.setenv("BHIP_KERNEL_TIMING", "2")
    try:
        tctx = ba.Context(0)
    finally:
        mp.undo()
    batch = VK.table(3 * T + 1, "three_tiles", seed=9)
    ws = [W("SUM", "f", "w_a", frame=R(-6, CUR)), W("MIN", "f", "w_b", frame=R(-6, CUR)), W("AVG", "i64", "w_c", frame=R(-6, CUR)), W("SUM", "i64", "w_d", frame=R(-6, CUR)),
          W("COUNT", "i64", "w_e", frame=G(None, 2)), W("LAST_VALUE", "f", "w_g", frame=G(None, 2)), W("MAX", "f", "w_h", frame=G(None, 2)),
          W("SUM", "f", "w_i", frame=R(None, CUR)), W("SUM", "f", "w_j", frame=G(None, None)), W("COUNT", "f", "w_k", frame=G(None, 0)),
          W("SUM", "f", "w_l", frame=F(-6, 0)), W("SUM", "i64", "w_m", frame=F(-6, 0)), W("COUNT", "g", "w_n", frame=F(None, 2)), W("FIRST_VALUE", "g", "w_o", frame=G(-1, 1))]
    tctx.kernel_stats(reset=True)
    check(tctx, [batch], [col("p")], [asc("o")], ws, any_zero_sign=["w_b", "w_h"])
    stats = tctx.kernel_stats(reset=True)
    # three distinct value frames: RANGE (-6, CURRENT), GROUPS (unbounded, 2), GROUPS (-1, 1); the canonical forms launch none
    assert stats["window_value_bounds"][1] == 3, stats["window_value_bounds"]
    assert stats["window_slide_value"][1] == 3, stats["window_slide_value"]                  # a, b, c: the sliding functions over a frame with two ends
    # the ROWS frames of the same operator as before: two distinct frames, one window_slide, and the finishes over (lo, hi): d, e, h, m, n
    assert stats["window_frame_bounds"][1] == 2 and stats["window_slide"][1] == 1 and stats["window_finish_frame"][1] == 5, stats
    assert stats["window_finish"][1] == 3                                                    # i, j, k: named frames
    # without a RANGE / GROUPS frame nothing of the new path runs
    check(tctx, [batch], [col("p")], [asc("o")], [W("SUM", "f", "w_l", frame=F(-6, 0)), W("SUM", "f", "w_i", frame=R(None, CUR)), W("MIN", "g", "w_j", frame=G(None, None))])
    stats = tctx.kernel_stats(reset=True)
    none = (0.0, 0)
    assert stats.get("window_value_bounds", none)[1] == 0 and stats.get("window_slide_value", none)[1] == 0
    assert stats["window_slide"][1] == 1 and stats["window_frame_bounds"][1] == 1
