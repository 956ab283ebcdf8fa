"""concat / nullif / date_trunc / to_timestamp on the device (kernels_str.hip, kernels_cast.hip, host/utf8_exprs.cpp, host/expr.cpp),
through the C ABI, against the contract of DESIGN.md §3.2: Python str for concat, numpy for nullif, the restatement
(tests/temporal_cases.py) for the two temporal functions.  oracle/engine.py does not know these functions: where an operator is
checked against it, the function's result is computed here and handed to the oracle plan as a plain column.

Row counts: 63 / 64 / 65 sit around one validity ballot word, 257 around a workgroup, 4099 spans several workgroups and ends
mid-word.  WAVE_BYTES is STR_CONCAT_WAVE_BYTES (str_kernels.h): a concat row whose result is longer is copied by its whole wave,
a shorter one by its own lane — the 1000-byte and the 70 000-byte row sit on either side of it."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col, lit
from oracle import plan_eval
from oracle.engine import OCol
from tests import helpers, temporal_cases as K

pytestmark = pytest.mark.gpu

WAVE_BYTES = 1024
SIZES = [0, 1, 63, 64, 65, 257, 4099]
LENGTHS = [0, 1, 7, 8, 9, 255, 256, 257]


@pytest.fixture(scope="module")
def ctx():
    return ba.Context(0)


def fn(name, *args):
    return E.ScalarFunctionExpr(name, list(args))


def run(plan):
    return helpers.concat(helpers.collect_product(plan))


def bits(c: OCol):
    """the valid rows' values as comparable bit patterns (floats: NaN payload and zero sign included)"""
    v = c.values
    if c.dtype == "Float64":
        v = v.view(np.uint64)
    elif c.dtype == "Float32":
        v = v.view(np.uint32)
    return [x.item() if hasattr(x, "item") else x for x, ok in zip(v, c.is_valid()) if ok]


def assert_column(got: OCol, want: OCol, what):
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert len(got) == len(want), (what, len(got), len(want))
    gv, wv = got.is_valid(), want.is_valid()
    assert np.array_equal(gv, wv), (what, [(i, got.values[i], want.values[i]) for i in np.nonzero(gv != wv)[0][:5]])
    g, w = bits(got), bits(want)
    assert g == w, (what, [(i, a if not isinstance(a, str) else a[:40], b if not isinstance(b, str) else b[:40]) for i, (a, b) in enumerate(zip(g, w)) if a != b][:5])


# ---- concat ---------------------------------------------------------------------------------------------------------------------

def text_of(nbytes, rng):
    """a string of exactly nbytes UTF-8 bytes: ASCII, or 2-, 3- and 4-byte characters with an ASCII tail"""
    kind = int(rng.integers(0, 3))
    if kind == 0 or nbytes < 4:
        return "".join("xy#ab"[k] for k in rng.integers(0, 5, nbytes))
    ch = ("é", "€", "𝄞")[int(rng.integers(0, 3))]
    w = len(ch.encode())
    return ch * (nbytes // w) + "z" * (nbytes % w)


def concat_batch(n, seed):
    rng = np.random.default_rng(seed)
    cols = OrderedDict()
    for name in ("a", "b", "c", "p"):
        cols[name] = [text_of(LENGTHS[k], rng) for k in rng.integers(0, len(LENGTHS), n)]
    valid = {name: rng.random(n) > 0.15 for name in ("a", "b", "c")}
    if n >= 257:
        cols["b"][5], cols["b"][200] = text_of(1000, rng), "L" + text_of(69998, rng) + "R"
        cols["a"][5], cols["c"][5], cols["p"][5] = "é", "", ""                 # row 5 of concat(a, b, c): 1002 bytes
        for name in valid:
            valid[name][[5, 200]] = True
    b = OrderedDict((name, OCol("Utf8", cols[name], valid.get(name))) for name in cols)
    b["z"] = OCol("Utf8", [""] * n, np.zeros(n, np.bool_))
    b["k"] = OCol("Int64", rng.integers(-50, 50, n))
    return b


def py_concat(b, *args):
    """SQL ||: NULL where any argument is; a str argument is a literal"""
    n = len(b["a"])
    valid = np.ones(n, np.bool_)
    parts = []
    for a in args:
        if isinstance(a, str):
            parts.append([a] * n)
        else:
            valid &= a.is_valid()
            parts.append(list(a.values))
    return OCol("Utf8", ["".join(p) if ok else "" for ok, *p in zip(valid, *parts)] if parts else [], valid)


def utf8_raw(rb, i):
    """(offsets, value bytes) of column i as the device holds them"""
    _, dtype, _, nbytes, has_valid = rb.column_info(i)
    assert dtype == "Utf8"
    n = rb.num_rows
    off, data, vbuf = np.zeros(n + 1, np.int32), np.zeros(max(1, nbytes), np.uint8), np.zeros((n + 7) // 8 + 8, np.uint8)
    L.check(L.lib().bhip_batch_column_to_host(rb._h, i, data.ctypes.data, off.ctypes.data, vbuf.ctypes.data if has_valid else None))
    return off, data[:nbytes].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_concat_to_the_byte_and_to_the_offset(ctx, n):
    b = concat_batch(n, seed=n + 1)
    A, B, C, P, Z = (col(x) for x in "abcpz")
    exprs = [(fn("concat", A, B, C), "abc"), (fn("concat", A, lit("#"), C, lit("")), "lits"), (fn("concat", A), "k1"),
             (fn("concat", A, B, C, A, lit("-é-"), B, C, P), "k8"), (fn("concat", A, Z), "all_null"), (fn("concat", P, lit("|"), P), "no_null"),
             (fn("concat", lit("x"), lit("y")), "two_lits")]
    want = [py_concat(b, b["a"], b["b"], b["c"]), py_concat(b, b["a"], "#", b["c"], ""), py_concat(b, b["a"]),
            py_concat(b, b["a"], b["b"], b["c"], b["a"], "-é-", b["b"], b["c"], b["p"]), py_concat(b, b["a"], b["z"]),
            py_concat(b, b["p"], "|", b["p"]), py_concat(b, "x", "y")]
    plan = ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]]))
    nullable = lambda *names: any(b[x].valid is not None for x in names)            # (a short column may happen to hold no NULL)
    assert plan.schema() == [("abc", "Utf8", nullable("a", "b", "c")), ("lits", "Utf8", nullable("a", "c")), ("k1", "Utf8", nullable("a")),
                             ("k8", "Utf8", nullable("a", "b", "c")), ("all_null", "Utf8", nullable("a", "z")), ("no_null", "Utf8", False),
                             ("two_lits", "Utf8", False)]
    assert n < 63 or nullable("a") and nullable("b") and nullable("c") and nullable("z")
    batches = plan.collect()
    assert sum(x.num_rows for x in batches) == n
    if n == 0:
        return
    got = helpers.concat([helpers.from_device(x) for x in batches])
    if n >= 257:
        lens = [len(s.encode()) for s in want[0].values]
        assert lens[5] <= WAVE_BYTES < 70000 <= lens[200]                   # both sides of the long-row threshold
        lens8 = [len(s.encode()) for s in want[3].values]                  # eight arguments: many rows beyond the threshold
        assert any(0 < x <= WAVE_BYTES for x in lens8) and sum(x > WAVE_BYTES for x in lens8) > n // 20
    for i, ((_, name), w) in enumerate(zip(exprs, want)):
        assert_column(got[name], w, name)
        off, data = utf8_raw(batches[0], i)
        encoded = [s.encode() if ok else b"" for s, ok in zip(w.values, w.is_valid())]
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(x) for x in encoded])]).astype(np.int32)), name
        assert data == b"".join(encoded), name
    assert got["no_null"].valid is None and not got["all_null"].is_valid().any()


def test_concat_nests_with_the_other_string_nodes(ctx):
    n = 1500
    rng = np.random.default_rng(9)
    words = ["Alpha", "BETA", "", "gamma Delta", "x"]
    b = OrderedDict([("a", OCol("Utf8", [words[k] for k in rng.integers(0, 5, n)], rng.random(n) > 0.1)),
                     ("b", OCol("Utf8", [words[k] for k in rng.integers(0, 5, n)], rng.random(n) > 0.1)),
                     ("k", OCol("Int64", rng.integers(-99, 99, n), rng.random(n) > 0.1))])
    e = fn("concat", fn("lower", col("a")), fn("concat", col("b"), lit("-")), E.CastExpr(col("k"), "Utf8"))
    got = run(ba.ProjectionExec([(e, "v"), (fn("octet_length", e), "len")], helpers.memory_exec(ctx, [[b]])))
    lower = OCol("Utf8", [s.lower() for s in b["a"].values], b["a"].valid)
    ks = OCol("Utf8", [str(int(v)) for v in b["k"].values], b["k"].valid)
    want = py_concat(b, lower, b["b"], "-", ks)
    assert_column(got["v"], want, "nested concat")
    assert_column(got["len"], OCol("Int32", [len(s.encode()) for s in want.values], want.valid), "octet_length(concat)")
    assert 0.5 < want.is_valid().mean() < 0.8


def operator_batch(n, seed):
    rng = np.random.default_rng(seed)
    b = OrderedDict([("a", OCol("Utf8", [["x", "xy", "", "é"][k] for k in rng.integers(0, 4, n)], rng.random(n) > 0.1)),
                     ("c", OCol("Utf8", [["y", "#y", "ab"][k] for k in rng.integers(0, 3, n)], rng.random(n) > 0.1)),
                     ("r", OCol("Int32", np.arange(n, dtype=np.int32)))])
    return b, py_concat(b, b["a"], "#", b["c"])


KEY = fn("concat", col("a"), lit("#"), col("c"))


def with_key(b, key):
    out = OrderedDict(b)
    out["key"] = key
    return out


def drop(batch, *names):
    return OrderedDict((k, c) for k, c in batch.items() if k not in names)


def test_concat_as_a_filter_operand(ctx):
    b, key = operator_batch(3000, seed=3)
    pred = lambda x: E.BinaryExpr(x, "Like", lit("x%#y"))
    got = run(ba.FilterExec(pred(KEY), helpers.memory_exec(ctx, [[b]])))
    want = plan_eval.collect(ba.FilterExec(pred(col("key")), helpers.memory_exec(ctx, [[with_key(b, key)]])))
    assert 0 < len(want["r"]) < 3000
    helpers.assert_rows_equal(got, drop(want, "key"), ordered=True)


def test_concat_as_a_group_key(ctx):
    b, key = operator_batch(6000, seed=4)
    parts = lambda bb: [[helpers.slice_batch(bb, 0, 2500)], [helpers.slice_batch(bb, 2500, 6000)]]

    def plan(m, k):
        aggs = [E.Count(col("r"), "n"), E.Sum(col("r"), "sr")]
        partial = ba.HashAggregateExec(ba.plan.PARTIAL, [(k, "key")], aggs, m)
        return ba.HashAggregateExec(ba.plan.FINAL, [(col("key"), "key")], aggs, ba.MergeExec(partial))

    got = run(plan(helpers.memory_exec(ctx, parts(b)), KEY))
    want = plan_eval.collect(plan(helpers.memory_exec(ctx, parts(with_key(b, key))), col("key")))
    helpers.assert_rows_equal(got, want, ordered=False, key_cols=["key"])
    assert len(got["key"]) >= 12 and sum(got["n"].to_pylist()) == 6000          # 4 x 3 keys, and the rows of the NULL key


def test_concat_as_a_sort_key(ctx):
    b, key = operator_batch(1200, seed=5)
    order = lambda k: [E.PhysicalSortExpr(k, descending=True), E.PhysicalSortExpr(col("r"))]
    got = run(ba.SortExec(order(KEY), helpers.memory_exec(ctx, [[b]])))
    want = plan_eval.collect(ba.SortExec(order(col("key")), helpers.memory_exec(ctx, [[with_key(b, key)]])))
    helpers.assert_rows_equal(got, drop(want, "key"), ordered=True)


# ---- nullif ---------------------------------------------------------------------------------------------------------------------

FIXED_TYPES = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64", "Float32", "Float64", "Date32", "Date64",
               "Timestamp(Second)", "Timestamp(Millisecond)", "Timestamp(Microsecond)", "Timestamp(Nanosecond)", "Boolean"]


def case_of(a, b, t):
    return E.CaseExpr(None, [(E.BinaryExpr(a, "Eq", b), E.Literal(None, t))], a)


def small_values(t, n, rng):
    if t == "Boolean":
        return rng.random(n) > 0.5
    lo = 0 if t.startswith("U") else -2
    return rng.integers(lo, lo + 5, n).astype(np.float64 if t.startswith("Float") else np.int64)


@pytest.mark.parametrize("t", FIXED_TYPES)
def test_nullif_on_every_fixed_width_type(ctx, t):
    n = 4099
    rng = np.random.default_rng(len(t) * 7 + sum(map(ord, t)))
    b = OrderedDict([("a", OCol(t, small_values(t, n, rng), rng.random(n) > 0.1)), ("b", OCol(t, small_values(t, n, rng), rng.random(n) > 0.1))])
    one = E.Literal(True if t == "Boolean" else 1, t)
    pairs = [("col", col("b")), ("lit", one), ("null", E.Literal(None, t))]
    exprs = [(fn("nullif", col("a"), y), "nullif_" + k) for k, y in pairs] + [(case_of(col("a"), y, t), "case_" + k) for k, y in pairs]
    plan = ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]]))
    assert plan.schema()[:3] == [("nullif_" + k, t, True) for k, _ in pairs]
    got = run(plan)
    av, bv = b["a"].is_valid(), b["b"].is_valid()
    eq_col = bv & (b["a"].values == b["b"].values)
    eq_lit = b["a"].values == (True if t == "Boolean" else 1)
    for k, equal in (("col", eq_col), ("lit", eq_lit), ("null", np.zeros(n, np.bool_))):
        want = OCol(t, b["a"].values, av & ~equal)
        assert_column(got["nullif_" + k], want, (t, k))
        assert_column(got["nullif_" + k], got["case_" + k], (t, k, "against CASE"))
    assert 0.1 < (av & eq_col).mean() < 0.9


def test_nullif_float64_with_nan_and_signed_zeros_is_the_librarys_eq(ctx):
    specials = np.array([0.0, -0.0, np.nan, -np.nan, 1.5, np.inf, -np.inf, 5e-324])
    a, b = (x.ravel() for x in np.meshgrid(specials, specials))
    batch = OrderedDict([("a", OCol("Float64", a)), ("b", OCol("Float64", b))])
    exprs = [(fn("nullif", col("a"), col("b")), "nullif"), (case_of(col("a"), col("b"), "Float64"), "case"), (col("a").eq(col("b")), "eq"),
             (fn("nullif", col("a"), lit(0.0)), "nz"), (case_of(col("a"), lit(0.0), "Float64"), "case_nz")]
    got = run(ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[batch]])))
    assert_column(got["nullif"], got["case"], "CASE")
    assert_column(got["nz"], got["case_nz"], "CASE against 0.0")
    eq = got["eq"].values.astype(np.bool_) & got["eq"].is_valid()
    assert_column(got["nullif"], OCol("Float64", a, ~eq), "whatever Eq says")
    plain = ~np.isnan(a) & ~np.isnan(b) & (a != 0) & (b != 0)              # numpy and IEEE agree beyond doubt here
    assert np.array_equal(got["nullif"].is_valid()[plain], (a != b)[plain])


def test_nullif_coerces_like_the_two_sides_of_eq(ctx):
    n = 300
    rng = np.random.default_rng(2)
    b = OrderedDict([("i", OCol("Int32", rng.integers(-2, 3, n), rng.random(n) > 0.1)), ("f", OCol("Float32", rng.integers(-2, 3, n).astype(np.float32)))])
    schema = {"i": "Int32", "f": "Float32"}
    exprs = [(E.coerce(fn("nullif", col("i"), lit(0)), schema), "vs_int64"), (E.coerce(fn("nullif", col("f"), col("i")), schema), "float_vs_int")]
    plan = ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]]))
    assert plan.schema() == [("vs_int64", "Int64", True), ("float_vs_int", "Float32", True)]
    got = run(plan)
    iv = b["i"].is_valid()
    assert_column(got["vs_int64"], OCol("Int64", b["i"].values, iv & (b["i"].values != 0)), "Int32 against an Int64 literal")
    assert_column(got["float_vs_int"], OCol("Float32", b["f"].values, ~(iv & (b["f"].values == b["i"].values))), "Float32 against Int32")
    with pytest.raises(ba.PlanError, match="nullif arguments have different types"):
        ba.ProjectionExec([(fn("nullif", col("i"), lit(0)), "x")], helpers.memory_exec(ctx, [[b]]))


def test_division_by_nullif_does_not_raise_divide_by_zero(ctx):
    n = 1000
    rng = np.random.default_rng(3)
    x, y = rng.integers(-1000, 1000, n), rng.integers(-3, 4, n)
    y_valid = rng.random(n) > 0.1
    m = helpers.memory_exec(ctx, [[OrderedDict([("x", OCol("Int64", x)), ("y", OCol("Int64", y, y_valid))])]])
    with pytest.raises(ba.ExecutionError, match="Divide by zero"):
        ba.ProjectionExec([(col("x") / col("y"), "q")], m).collect()
    got = run(ba.ProjectionExec([(col("x") / fn("nullif", col("y"), lit(0)), "q")], m))
    ok = y_valid & (y != 0)
    q = np.where(ok, np.trunc(x / np.where(y == 0, 1, y)), 0).astype(np.int64)
    assert_column(got["q"], OCol("Int64", q, ok), "x / nullif(y, 0)")
    assert (y == 0).sum() > 50


# ---- date_trunc -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 4099])
@pytest.mark.parametrize("unit", list(K.UNITS))
def test_date_trunc_every_unit_and_granularity(ctx, unit, n):
    ups = K.UNITS[unit][1]
    v = K.random_values(unit, n, seed=n + ups % 97)
    pinned = [x * ups // 10**9 for x in (-500000000, 3 * 86400 * 10**9, 4 * 86400 * 10**9 + 10**9, 1609632000 * 10**9, 1709164800 * 10**9)]
    if unit == K.NS:
        pinned += [K.I64_MIN, K.I64_MIN + 1, K.I64_MAX, -1, 0]
    v[:len(pinned)] = pinned
    valid = np.random.default_rng(n).random(n) > 0.1
    valid[:len(pinned)] = True
    b = OrderedDict([("t", OCol(unit, v, valid))])
    exprs = [(fn("date_trunc", lit(g), col("t")), g) for g in K.GRANULARITIES]
    plan = ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]]))
    assert plan.schema() == [(g, unit, True) for g in K.GRANULARITIES]
    got = run(plan)
    for g in K.GRANULARITIES:
        want = K.date_trunc(g, v, unit)
        ok = valid & np.array([w is not None for w in want])
        assert_column(got[g], OCol(unit, [0 if w is None else w for w in want], ok), (unit, g))
    if unit == K.NS:
        assert got["year"].to_pylist()[5] is None and got["second"].to_pylist()[0] == -10**9 and got["week"].to_pylist()[0] == -259200 * 10**9


def test_date_trunc_over_an_expression_and_over_literals(ctx):
    n = 300
    s = np.random.default_rng(1).integers(-10**9, 2 * 10**9, n)
    b = OrderedDict([("s", OCol("Timestamp(Second)", s)), ("u", OCol("Utf8", ["x"] * n))])
    exprs = [(fn("date_trunc", lit("hour"), E.CastExpr(col("s"), "Timestamp(Millisecond)")), "cast_then_hour"),
             (fn("date_trunc", lit("year"), fn("date_trunc", lit("week"), col("s"))), "nested"),
             (fn("date_trunc", lit("month"), fn("to_timestamp", lit("2024-02-29T12:00:00+01:00"))), "folded"),
             (fn("date_trunc", lit("day"), E.Literal(None, "Timestamp(Second)")), "null_literal"),
             (fn("to_timestamp", E.Literal(None, "Utf8")), "null_text")]
    got = run(ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]])))
    assert_column(got["cast_then_hour"], OCol("Timestamp(Millisecond)", K.date_trunc("hour", s * 1000, "Timestamp(Millisecond)")), "cast")
    weeks = K.date_trunc("week", s, "Timestamp(Second)")
    assert_column(got["nested"], OCol("Timestamp(Second)", K.date_trunc("year", weeks, "Timestamp(Second)")), "nested")
    assert_column(got["folded"], OCol(K.NS, [1706745600 * 10**9] * n), "folded")
    assert_column(got["null_literal"], OCol("Timestamp(Second)", [0] * n, np.zeros(n, np.bool_)), "NULL literal")
    assert_column(got["null_text"], OCol(K.NS, [0] * n, np.zeros(n, np.bool_)), "to_timestamp(NULL)")


# ---- to_timestamp ------------------------------------------------------------------------------------------------------------------

def test_to_timestamp_pinned_and_random_texts(ctx):
    cases = K.PINNED_TEXTS + K.random_texts(4099, seed=7)
    n = len(cases)
    valid = np.random.default_rng(8).random(n) > 0.1
    valid[:len(K.PINNED_TEXTS)] = True
    texts = [t if ok else "not a timestamp" for (t, _), ok in zip(cases, valid)]          # a NULL row's bytes are never parsed
    b = OrderedDict([("s", OCol("Utf8", texts, valid)), ("u", OCol("Utf8", [t for t, _ in cases]))])
    plan = ba.ProjectionExec([(fn("to_timestamp", col("s")), "ts"), (fn("to_timestamp", col("u")), "tu")], helpers.memory_exec(ctx, [[b]]))
    assert plan.schema() == [("ts", K.NS, True), ("tu", K.NS, False)]
    got = run(plan)
    want = [ns for _, ns in cases]
    assert_column(got["ts"], OCol(K.NS, want, valid), "with NULLs")
    assert_column(got["tu"], OCol(K.NS, want), "without")
    assert got["tu"].valid is None


@pytest.mark.parametrize("bad", ["2021-02-29T00:00:00", "2262-04-11T23:47:16.854775808", "", "2021-03-01"])
def test_one_bad_text_fails_the_query_and_the_context_goes_on(ctx, bad):
    n, row = 257, 130
    texts = [t for t, _ in K.random_texts(n, seed=9)]
    want = [K.to_timestamp(t) for t in texts]
    plan = lambda c: ba.ProjectionExec([(fn("to_timestamp", col("s")), "ts")], helpers.memory_exec(ctx, [[OrderedDict([("s", c)])]]))
    broken = list(texts)
    broken[row] = bad
    with pytest.raises(ba.ExecutionError, match="to_timestamp"):
        plan(OCol("Utf8", broken)).collect()
    masked = np.arange(n) != row
    assert_column(run(plan(OCol("Utf8", broken, masked)))["ts"], OCol(K.NS, want, masked), "the bad row NULL")
    assert_column(run(plan(OCol("Utf8", texts)))["ts"], OCol(K.NS, want), "the next, valid batch")


def test_a_bad_literal_fails_when_the_plan_is_made(ctx):
    b = OrderedDict([("k", OCol("Int64", [1]))])
    with pytest.raises(ba.ExecutionError, match="to_timestamp"):
        ba.ProjectionExec([(fn("to_timestamp", lit("yesterday")), "ts")], helpers.memory_exec(ctx, [[b]]))


# ---- composed ---------------------------------------------------------------------------------------------------------------------

MONTH_KEY = fn("date_trunc", lit("month"), fn("to_timestamp", fn("concat", col("d"), lit("T00:00:00"))))


def date_table(n=700, seed=6):
    days = np.random.default_rng(seed).integers(0, 730, n) + np.datetime64("2019-06-01", "D").astype(np.int64)
    d = days.astype("datetime64[D]")
    return OrderedDict([("d", OCol("Utf8", [str(x) for x in d]))]), d


def month_counts(d):
    months, counts = np.unique(d.astype("datetime64[M]"), return_counts=True)
    return {int(m.astype("datetime64[ns]").astype(np.int64)): int(c) for m, c in zip(months, counts)}


def aggregate(node, m):
    partial = node.HashAggregateExec(ba.plan.PARTIAL, [(MONTH_KEY, "month")], [E.Count(col("d"), "n")], m)
    # (Final reads the state columns by position; its argument is a placeholder that names a column of its input)
    return node.HashAggregateExec(ba.plan.FINAL, [(col("month"), "month")], [E.Count(col("month"), "n")], node.MergeExec(partial))


def test_count_by_month_of_parsed_date_strings(ctx):
    b, d = date_table()
    got = run(aggregate(ba, helpers.memory_exec(ctx, [[b]])))
    assert got["month"].dtype == K.NS and got["month"].is_valid().all()
    want = month_counts(d)
    assert len(want) == 24 and dict(zip(got["month"].to_pylist(), got["n"].to_pylist())) == want


def test_count_by_month_through_the_wire_plan(ctx):
    from tests import plan_nodes as N, proto_encode as pe
    b, d = date_table(seed=16)
    m = helpers.memory_exec(ctx, [[b]])
    stand_in = N.MemoryExec([[b]])
    stand_in.name = "mem://dates"
    decoded = ba.ExecutionPlan.from_proto(ctx, pe.plan(aggregate(N, stand_in)), lambda leaf: m)
    assert "date_trunc('month', to_timestamp(concat(d, 'T00:00:00')))" in decoded.display()
    got = run(decoded)
    assert dict(zip(got["month"].to_pylist(), got["n"].to_pylist())) == month_counts(d)
