"""CAST to and from Utf8 on the device (kernels_cast.hip, host/utf8_exprs.cpp): every direction of the table in DESIGN.md §3.2,
declined float strings, compositions with the other string nodes, and every operator that takes the lowering — against the Python
restatement of the table (tests/cast_text_cases.py) and, for the operators, the oracle run over the same plan with the cast columns
computed in Python.

Row counts: 63 / 64 / 65 sit around one validity ballot word, 257 around a workgroup, 5000 spans several workgroups."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og, plan_eval
from oracle.engine import OCol
from tests import cast_text_cases as K, helpers

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 5000]


@pytest.fixture(scope="module")
def ctx():
    return ba.Context(0)


def fn(name, e):
    return E.ScalarFunctionExpr(name, [e])


def cast(e, t):
    return E.CastExpr(e, t)


def some_nulls(n, seed, nulls):
    return (np.random.default_rng(seed).random(n) > 0.1) if nulls else None


def parsed(c: OCol, to):
    """CAST(c AS to) by the restatement; a declined value must not be in a batch that is expected to run"""
    vals = [K.parse(s, to) if ok else None for s, ok in zip(c.values, c.is_valid())]
    assert not any(v is K.DECLINED for v in vals)
    return OCol(to, [0 if v is None else v for v in vals], np.array([v is not None for v in vals], np.bool_))


def formatted(c: OCol):
    vals = [K.format_value(v.item() if hasattr(v, "item") else v, c.dtype) if ok else None for v, ok in zip(c.values, c.is_valid())]
    return OCol("Utf8", ["" if v is None else v for v in vals], np.array([v is not None for v in vals], np.bool_))


def assert_column(got: OCol, want: OCol, what):
    """bit-exact: result type, validity, and the value of every valid row (floats by bit pattern)"""
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert len(got) == len(want), what
    gv, wv = got.is_valid(), want.is_valid()
    assert np.array_equal(gv, wv), (what, [(i, got.values[i], want.values[i]) for i in np.nonzero(gv != wv)[0][:5]])
    g = [K.bits(v, got.dtype) for v, ok in zip(got.values, gv) if ok]
    w = [K.bits(v, want.dtype) for v, ok in zip(want.values, wv) if ok]
    assert g == w, (what, [(a, b) for a, b in zip(g, w) if a != b][:5])


def run(plan):
    return helpers.concat(helpers.collect_product(plan))


# ---- every direction ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_utf8_to_every_type(ctx, n, nulls):
    b = OrderedDict((t, OCol("Utf8", K.random_strings(t, n, seed=n + i), some_nulls(n, n + 100 + i, nulls))) for i, t in enumerate(K.PARSE_TYPES))
    if not nulls:
        assert all(c.valid is None for c in b.values())               # no validity buffer at all
    plan = ba.ProjectionExec([(cast(col(t), t), "to_" + t) for t in K.PARSE_TYPES], helpers.memory_exec(ctx, [[b]]))
    assert [(t, u) for _, t, u in plan.schema()] == [(t, True) for t in K.PARSE_TYPES]
    got = run(plan)
    for t in K.PARSE_TYPES:
        assert_column(got["to_" + t], parsed(b[t], t), t)


def utf8_layout(rb, i):
    """(offsets, value bytes of the column) as the device holds them"""
    _, dtype, _, nbytes, has_valid = rb.column_info(i)
    assert dtype == "Utf8"
    n = rb.num_rows
    off, data, vbuf = np.zeros(n + 1, np.int32), np.zeros(max(1, nbytes), np.uint8), np.zeros((n + 7) // 8 + 8, np.uint8)
    L.check(L.lib().bhip_batch_column_to_host(rb._h, i, data.ctypes.data, off.ctypes.data, vbuf.ctypes.data if has_valid else None))
    return off, nbytes


@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_every_type_to_utf8(ctx, n, nulls):
    b = OrderedDict((t, OCol(t, K.random_values(t, n, seed=n + i), some_nulls(n, n + 200 + i, nulls))) for i, t in enumerate(K.FORMAT_TYPES))
    plan = ba.ProjectionExec([(cast(col(t), "Utf8"), "s_" + t) for t in K.FORMAT_TYPES], helpers.memory_exec(ctx, [[b]]))
    assert [t for _, t, _ in plan.schema()] == ["Utf8"] * len(K.FORMAT_TYPES)
    batches = plan.collect()
    got = helpers.concat([helpers.from_device(x) for x in batches])
    for i, t in enumerate(K.FORMAT_TYPES):
        want = formatted(b[t])
        assert_column(got["s_" + t], want, t)
        off, nbytes = utf8_layout(batches[0], i)
        total = sum(len(s) for s, ok in zip(want.values, want.is_valid()) if ok)
        assert off[0] == 0 and off[-1] == nbytes == total and np.all(np.diff(off) >= 0), (t, off[0], off[-1], nbytes, total)


# ---- declined float strings ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("to", ["Float64", "Float32"])
@pytest.mark.parametrize("row", [0, 256, 96])                   # the first row, the last, the middle of the second wave
def test_a_declined_float_string_fails_the_batch(ctx, to, row):
    n = 257
    bad = {"Float64": "0.1234567890123456789", "Float32": "16777217"}[to]
    vals = K.random_strings(to, n, seed=3)
    vals[row] = bad
    plan = lambda c: ba.ProjectionExec([(cast(col("s"), to), "v")], helpers.memory_exec(ctx, [[OrderedDict([("s", c)])]]))
    with pytest.raises(ba.NotImplementedOnGpu, match="cast Utf8 -> " + to):
        plan(OCol("Utf8", vals)).collect()
    # the same batch with that row NULL runs, and the context goes on to run an accepted batch correctly
    masked = OCol("Utf8", vals, np.arange(n) != row)
    assert_column(run(plan(masked))["v"], parsed(masked, to), "masked")
    vals[row] = "2.5"
    assert_column(run(plan(OCol("Utf8", vals)))["v"], parsed(OCol("Utf8", vals), to), "accepted")


# ---- composition -----------------------------------------------------------------------------------------------------------------

def mixed_batch(n, seed=1):
    rng = np.random.default_rng(seed)
    words = ["12", " 12 ", "\t-7\n", "007", "+5", "x", "", " ", "2147483647", "2147483648", "-2147483648", "11", "9", "10", "3.5", "　42　"]
    return OrderedDict([("s", OCol("Utf8", [words[k] for k in rng.integers(0, len(words), n)], rng.random(n) > 0.1)),
                        ("k", OCol("Int64", rng.integers(-15, 40, n), rng.random(n) > 0.1)),
                        ("r", OCol("Int32", np.arange(n, dtype=np.int32)))])


def test_casts_nest_with_each_other_and_with_the_string_nodes(ctx):
    b = mixed_batch(1500, seed=2)
    m = helpers.memory_exec(ctx, [[b]])
    text_case = E.CaseExpr(None, [(col("k") < lit(0, "Int64"), cast(col("k"), "Utf8"))], col("s"))
    int_case = E.CaseExpr(None, [(col("k") > lit(20, "Int64"), cast(col("s"), "Int32"))], lit(0, "Int32"))
    exprs = [(cast(fn("trim", col("s")), "Int32"), "trimmed"), (fn("upper", cast(col("k"), "Utf8")), "upper"),
             (cast(cast(col("k"), "Utf8"), "Int64").eq(col("k")), "round_trip"), (text_case, "text_case"), (int_case, "int_case"),
             (cast(lit("42"), "Int64"), "fortytwo"), (cast(lit("x"), "Int32"), "no_number"), (cast(lit(7, "Int32"), "Utf8"), "seven"),
             (cast(lit("1994-01-01"), "Date32"), "day"), (col("r"), "r")]
    plan = ba.ProjectionExec(exprs, m)
    assert [t for _, t, _ in plan.schema()] == ["Int32", "Utf8", "Boolean", "Utf8", "Int32", "Int64", "Int32", "Utf8", "Date32", "Int32"]
    got = run(plan)
    n = len(b["r"])
    ks, si = formatted(b["k"]), parsed(b["s"], "Int32")
    assert_column(got["trimmed"], parsed(og.evaluate(fn("trim", col("s")), b), "Int32"), "CAST(trim(s) AS Int32)")
    assert_column(got["upper"], ks, "upper(CAST(k AS Utf8))")
    kv = b["k"].is_valid()
    assert np.array_equal(got["round_trip"].is_valid(), kv) and bool(np.all(got["round_trip"].values[kv]))
    neg = kv & (b["k"].values < 0)
    assert_column(got["text_case"], OCol("Utf8", np.where(neg, ks.values, b["s"].values), np.where(neg, True, b["s"].is_valid())), "CASE .. THEN CAST(k AS Utf8)")
    big = kv & (b["k"].values > 20)
    assert_column(got["int_case"], OCol("Int32", np.where(big, si.values, 0), np.where(big, si.is_valid(), True)), "CASE .. THEN CAST(s AS Int32)")
    assert_column(got["fortytwo"], OCol("Int64", [42] * n), "CAST('42' AS Int64)")
    assert_column(got["no_number"], OCol("Int32", [0] * n, np.zeros(n, np.bool_)), "CAST('x' AS Int32)")
    assert_column(got["seven"], OCol("Utf8", ["7"] * n), "CAST(7 AS Utf8)")
    assert_column(got["day"], OCol("Date32", [8766] * n), "CAST('1994-01-01' AS Date32)")


# ---- in every operator that takes the lowering -----------------------------------------------------------------------------------

def with_cast_columns(b):
    out = OrderedDict(b)
    out["ks"], out["si"], out["sf"] = formatted(b["k"]), parsed(b["s"], "Int32"), parsed(b["s"], "Float64")
    return out


def drop(batch, *names):
    return OrderedDict((k, c) for k, c in batch.items() if k not in names)


def test_filter_on_a_parsed_string(ctx):
    b = mixed_batch(3000, seed=4)
    got = run(ba.FilterExec(cast(col("s"), "Int32") > lit(10, "Int32"), helpers.memory_exec(ctx, [[b]])))
    want = plan_eval.collect(ba.FilterExec(col("si") > lit(10, "Int32"), helpers.memory_exec(ctx, [[with_cast_columns(b)]])))
    assert 0 < len(want["r"]) < 3000
    helpers.assert_rows_equal(got, drop(want, "ks", "si", "sf"), ordered=True)


def test_sort_on_a_formatted_integer(ctx):
    b = mixed_batch(1200, seed=5)
    got = run(ba.SortExec([E.PhysicalSortExpr(cast(col("k"), "Utf8")), E.PhysicalSortExpr(col("r"))], helpers.memory_exec(ctx, [[b]])))
    want = plan_eval.collect(ba.SortExec([E.PhysicalSortExpr(col("ks")), E.PhysicalSortExpr(col("r"))], helpers.memory_exec(ctx, [[with_cast_columns(b)]])))
    helpers.assert_rows_equal(got, drop(want, "ks", "si", "sf"), ordered=True)
    order = [k for k in got["k"].to_pylist() if k is not None]
    assert order.index(10) < order.index(9) and order != sorted(order)              # string order, not numeric order


def test_aggregate_grouped_by_a_formatted_key_over_parsed_arguments(ctx):
    b = mixed_batch(6000, seed=6)
    b["s"] = OCol("Utf8", [s if s != "3.5" else "35" for s in b["s"].values], b["s"].valid)      # integer-valued: SUM is exact in any order
    parts = lambda bb: [[helpers.slice_batch(bb, 0, 2500)], [helpers.slice_batch(bb, 2500, 6000)]]

    def plan(m, key, fsum, icount):
        aggs = [E.Sum(fsum, "sx"), E.Count(icount, "n")]
        partial = ba.HashAggregateExec(ba.plan.PARTIAL, [(key, "ks")], aggs, m)
        return ba.HashAggregateExec(ba.plan.FINAL, [(col("ks"), "ks")], aggs, ba.MergeExec(partial))

    got = run(plan(helpers.memory_exec(ctx, parts(b)), cast(col("k"), "Utf8"), cast(col("s"), "Float64"), cast(col("s"), "Int32")))
    c = with_cast_columns(b)
    want = plan_eval.collect(plan(helpers.memory_exec(ctx, parts(c)), col("ks"), col("sf"), col("si")))
    helpers.assert_rows_equal(got, want, ordered=False, key_cols=["ks"])
    # COUNT skipped the rows the cast made NULL: fewer than the rows with a string, more than none
    counted = sum(got["n"].to_pylist())
    assert counted == int(c["si"].is_valid().sum()) and 0 < counted < int(b["s"].is_valid().sum())


# ---- empty input, empty strings -------------------------------------------------------------------------------------------------

def test_zero_rows_and_empty_strings(ctx):
    exprs = [(cast(col("s"), "Int32"), "i"), (cast(col("s"), "Float64"), "f"), (cast(col("s"), "Boolean"), "b"), (cast(col("k"), "Utf8"), "ks")]
    empty = OrderedDict([("s", OCol("Utf8", [])), ("k", OCol("Int64", np.zeros(0, np.int64)))])
    got = ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[empty]])).collect()
    assert sum(x.num_rows for x in got) == 0
    for x in got:
        assert [t for _, t in x.schema()] == ["Int32", "Float64", "Boolean", "Utf8"]
    n = 130
    blank = OrderedDict([("s", OCol("Utf8", [""] * n)), ("k", OCol("Int64", np.arange(n)))])
    got = run(ba.ProjectionExec(exprs[:3], helpers.memory_exec(ctx, [[blank]])))
    for name, t in (("i", "Int32"), ("f", "Float64"), ("b", "Boolean")):
        assert_column(got[name], OCol(t, [0] * n, np.zeros(n, np.bool_)), name)


# ---- the wire plan -----------------------------------------------------------------------------------------------------------

def test_casts_through_the_wire_plan(ctx):
    """the plan of tests/test_cast_text_cpu.py, with a memory leaf: decoded and ctypes-built plans give the same result"""
    from tests import plan_nodes as N, proto_encode as pe
    b = drop(mixed_batch(700, seed=8), "r")
    m = helpers.memory_exec(ctx, [[b]])
    exprs = [(cast(col("s"), "Int32"), "si"), (cast(col("k"), "Utf8"), "ks"), (cast(lit("42"), "Int64"), "fortytwo")]
    stand_in = N.MemoryExec([[b]])
    stand_in.name = "mem://casts"
    decoded = ba.ExecutionPlan.from_proto(ctx, pe.plan(N.ProjectionExec(exprs, stand_in)), lambda leaf: m)
    direct = ba.ProjectionExec(exprs, m)
    assert decoded.display() == direct.display()
    got, same = run(decoded), run(direct)
    for name, want in (("si", parsed(b["s"], "Int32")), ("ks", formatted(b["k"])), ("fortytwo", OCol("Int64", [42] * 700))):
        assert_column(got[name], want, name)
        assert_column(same[name], want, name)
