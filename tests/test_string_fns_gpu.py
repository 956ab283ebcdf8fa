"""substr / left / right / char_length / strpos / starts_with / date_part on the device (kernels_str.hip, kernels_cast.hip,
host/utf8_exprs.cpp, host/expr.cpp), through the C ABI, against the restatement of DESIGN.md §3.2 (tests/string_fn_cases.py):
bytes, offsets, data_bytes and validity all exact.

Row counts: 1, 63 / 64 / 65 around one validity ballot word, 256 / 257 around a workgroup, 513 two workgroups and one row.
WAVE_BYTES is STR_CONCAT_WAVE_BYTES (str_kernels.h): a row whose RESULT is longer is copied by its whole wave, a shorter one by its
own lane — rows 5 .. 8 put results of exactly WAVE_BYTES and WAVE_BYTES + 1 bytes on either side of it."""
import math
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col, lit
from oracle.engine import OCol
from tests import helpers, string_fn_cases as K

pytestmark = pytest.mark.gpu

WAVE = K.WAVE_BYTES
SIZES = [1, 63, 64, 65, 256, 257, 513]


@pytest.fixture(scope="module")
def ctx():
    return ba.Context(0)


def fn(name, *args):
    return E.ScalarFunctionExpr(name, list(args))


def i64(v):
    return E.Literal(v, "Int64")


def run(plan):
    return helpers.concat(helpers.collect_product(plan))


def assert_column(got: OCol, want: OCol, what):
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert len(got) == len(want), (what, len(got), len(want))
    gv, wv = got.is_valid(), want.is_valid()
    assert np.array_equal(gv, wv), (what, [(i, got.values[i], want.values[i]) for i in np.nonzero(gv != wv)[0][:5]])
    g = [x.item() if hasattr(x, "item") else x for x, ok in zip(got.values, gv) if ok]
    w = [x.item() if hasattr(x, "item") else x for x, ok in zip(want.values, wv) if ok]
    assert g == w, (what, [(i, str(a)[:40], str(b)[:40]) for i, (a, b) in enumerate(zip(g, w)) if a != b][:5])


def utf8_raw(rb, i):
    """(offsets, value bytes) of column i as the device holds them; the byte count is the column's data_bytes"""
    _, dtype, _, nbytes, has_valid = rb.column_info(i)
    assert dtype == "Utf8"
    n = rb.num_rows
    off, data, vbuf = np.zeros(n + 1, np.int32), np.zeros(max(1, nbytes), np.uint8), np.zeros((n + 7) // 8 + 8, np.uint8)
    L.check(L.lib().bhip_batch_column_to_host(rb._h, i, data.ctypes.data, off.ctypes.data, vbuf.ctypes.data if has_valid else None))
    return off, data[:nbytes].tobytes()


def edge_rows(n):
    """the first and the last row of every wave"""
    return sorted({r for r in (0, 63, 64, 127, 128, n - 1) if 0 <= r < n})


def string_batch(n, seed):
    rng = np.random.default_rng(seed)
    s = [K.random_string(rng) if rng.random() > 0.15 else "" for _ in range(n)]
    u = []
    for x in s:                                         # a piece of s, its prefix half the time, else an unrelated string
        if len(x) and rng.random() < 0.7:
            a = 0 if rng.random() < 0.5 else int(rng.integers(0, len(x)))
            u.append(x[a:a + int(rng.integers(0, 4))])
        else:
            u.append(K.random_string(rng, 3))
    if n >= 256:
        s[5], s[6], s[7], s[8] = "x" * 2000, "y" * WAVE, "€" * 400, "z" * (WAVE + 1)
    st = np.array([K.random_int(rng, len(x)) for x in s], np.int64)
    cnt = np.array([K.I64_MAX if c in (K.I64_MIN, K.I64_MAX) else abs(c) for c in (K.random_int(rng, len(x)) for x in s)], np.int64)
    nn = np.array([K.random_int(rng, len(x)) for x in s], np.int64)
    if n >= 256:
        st[5:9], cnt[5:9], nn[5:9] = 2, WAVE + 1, WAVE + 1
    valid = {}
    for name in ("s", "st", "cnt", "nn", "v"):
        v = rng.random(n) > 0.1
        if name == "s":
            v[edge_rows(n)] = False
        if n >= 256:
            v[5:9] = True
        valid[name] = v if n >= 63 else None            # (one row: valid, and its columns without a validity buffer)
    return OrderedDict([("s", OCol("Utf8", s, valid["s"])), ("u", OCol("Utf8", u)), ("v", OCol("Utf8", list(reversed(u)), valid["v"])),
                        ("st", OCol("Int64", st, valid["st"])), ("cnt", OCol("Int64", cnt, valid["cnt"])), ("nn", OCol("Int64", nn, valid["nn"])),
                        ("one", OCol("Int64", np.ones(n, np.int64)))])


def expected(b, name, *args):
    """args: OCol (a column) or a Python value (a literal); NULL where any column argument is"""
    n = len(b["s"])
    valid = np.ones(n, np.bool_)
    for a in args:
        if isinstance(a, OCol):
            valid &= a.is_valid()
    rows = zip(*[a.values if isinstance(a, OCol) else [a] * n for a in args])
    vals = [K.STRING_FUNCTIONS[name](*(x.item() if hasattr(x, "item") else x for x in r)) if ok else None for r, ok in zip(rows, valid)]
    dtype = {"char_length": "Int32", "strpos": "Int32", "starts_with": "Boolean"}.get(name, "Utf8")
    zero = "" if dtype == "Utf8" else False if dtype == "Boolean" else 0
    nullable = any(isinstance(a, OCol) and a.valid is not None for a in args)
    return OCol(dtype, [zero if v is None else v for v in vals] if dtype == "Utf8" else np.array([zero if v is None else v for v in vals]),
                valid if nullable else None)


def calls(b):
    """(expression, expected column) of every function, integer and string arguments as literals and as columns"""
    S, U, V, ST, CNT, NN = (col(x) for x in ("s", "u", "v", "st", "cnt", "nn"))
    s, u, v, st, cnt, nn = (b[x] for x in ("s", "u", "v", "st", "cnt", "nn"))
    out = [(fn("substr", S, i64(1), i64(2)), expected(b, "substr", s, 1, 2)),
           (fn("substr", S, i64(0), i64(3)), expected(b, "substr", s, 0, 3)),
           (fn("substring", S, i64(3)), expected(b, "substr", s, 3)),
           (fn("substr", S, i64(2), i64(WAVE + 1)), expected(b, "substr", s, 2, WAVE + 1)),
           (fn("substr", S, i64(K.I64_MAX), i64(K.I64_MAX)), expected(b, "substr", s, K.I64_MAX, K.I64_MAX)),
           (fn("substr", S, i64(K.I64_MIN), i64(K.I64_MAX)), expected(b, "substr", s, K.I64_MIN, K.I64_MAX)),
           (fn("substr", S, i64(-2), i64(K.I64_MAX)), expected(b, "substr", s, -2, K.I64_MAX)),
           (fn("left", S, i64(WAVE + 1)), expected(b, "left", s, WAVE + 1)),
           (fn("left", S, i64(WAVE)), expected(b, "left", s, WAVE)),
           (fn("left", S, i64(-2)), expected(b, "left", s, -2)),
           (fn("right", S, i64(3)), expected(b, "right", s, 3)),
           (fn("right", S, i64(-1)), expected(b, "right", s, -1)),
           (fn("right", S, i64(WAVE + 1)), expected(b, "right", s, WAVE + 1)),
           (fn("right", U, i64(K.I64_MIN)), expected(b, "right", u, K.I64_MIN)),
           (fn("substr", S, ST, CNT), expected(b, "substr", s, st, cnt)),
           (fn("substr", S, ST), expected(b, "substr", s, st)),
           (fn("substr", U, i64(2), CNT), expected(b, "substr", u, 2, cnt)),
           (fn("substr", U, ST, i64(2)), expected(b, "substr", u, st, 2)),
           (fn("left", S, NN), expected(b, "left", s, nn)),
           (fn("right", S, NN), expected(b, "right", s, nn)),
           (fn("left", U, NN), expected(b, "left", u, nn)),
           (fn("substr", U, col("one") + col("one")), expected(b, "substr", u, 2)),
           (fn("char_length", S), expected(b, "char_length", s)),
           (fn("length", U), expected(b, "char_length", u)),
           (fn("strpos", S, U), expected(b, "strpos", s, u)),
           (fn("strpos", S, V), expected(b, "strpos", s, v)),
           (fn("strpos", S, lit("é")), expected(b, "strpos", s, "é")),
           (fn("strpos", U, lit("")), expected(b, "strpos", u, "")),
           (fn("starts_with", S, U), expected(b, "starts_with", s, u)),
           (fn("starts_with", U, S), expected(b, "starts_with", u, s)),
           (fn("starts_with", S, lit("a")), expected(b, "starts_with", s, "a")),
           (fn("starts_with", U, lit("")), expected(b, "starts_with", u, ""))]
    return out


@pytest.mark.parametrize("n", SIZES)
def test_every_string_function_to_the_byte_and_to_the_offset(ctx, n):
    b = string_batch(n, seed=n)
    cs = calls(b)
    exprs = [(e, f"c{i}") for i, (e, _) in enumerate(cs)]
    plan = ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]]))
    assert plan.schema() == [(f"c{i}", w.dtype, w.valid is not None) for i, (_, w) in enumerate(cs)]
    batches = plan.collect()
    assert len(batches) == 1 and batches[0].num_rows == n
    got = helpers.from_device(batches[0])
    if n >= 256:
        lens = lambda i: [len(x.encode()) for x in cs[i][1].values]
        assert lens(3)[5] == WAVE + 1 and lens(3)[8] == WAVE and lens(7)[5] == WAVE + 1 and lens(7)[6] == WAVE and lens(7)[7] == 1200
        assert lens(12)[8] == WAVE + 1 and lens(12)[6] == WAVE and lens(14)[5] == WAVE + 1 and lens(18)[5] == WAVE + 1
    for i, (_, w) in enumerate(cs):
        assert_column(got[f"c{i}"], w, (i, exprs[i][0].fun))
        assert (got[f"c{i}"].valid is None) == (w.valid is None), i
        if w.dtype == "Utf8":
            off, data = utf8_raw(batches[0], i)
            encoded = [x.encode() if ok else b"" for x, ok in zip(w.values, w.is_valid())]
            assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(x) for x in encoded])]).astype(np.int32)), i
            assert data == b"".join(encoded), i
    if n >= 63:
        nulls = ~b["s"].is_valid()
        assert nulls[0] and nulls[n - 1] and (n < 65 or (nulls[63] and nulls[64]))


def test_null_literals_and_folded_calls(ctx):
    n = 65
    b = string_batch(n, seed=3)
    null_i, null_s = E.Literal(None, "Int64"), E.Literal(None, "Utf8")
    exprs = [(fn("substr", col("u"), null_i), "a"), (fn("substr", col("u"), i64(1), null_i), "b"), (fn("left", null_s, i64(1)), "c"),
             (fn("strpos", col("u"), null_s), "d"), (fn("starts_with", null_s, col("u")), "e"), (fn("char_length", null_s), "f"),
             (fn("substr", lit("naïve€𝄞x"), i64(3), i64(4)), "g"), (fn("right", lit("abcde"), i64(-2)), "h"), (fn("char_length", lit("€𝄞")), "i"),
             (fn("strpos", lit("€𝄞x"), lit("x")), "j"), (fn("starts_with", lit("abc"), lit("")), "k"),
             (fn("date_part", lit("doy"), E.date32("2000-12-31")), "l"), (fn("date_part", lit("year"), E.Literal(K.I64_MIN, "Timestamp(Second)")), "m"),
             (fn("date_part", lit("second"), E.Literal(-1, "Timestamp(Nanosecond)")), "o")]
    got = run(ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]])))
    none = np.zeros(n, np.bool_)
    for name, t, z in (("a", "Utf8", ""), ("b", "Utf8", ""), ("c", "Utf8", ""), ("d", "Int32", 0), ("e", "Boolean", False), ("f", "Int32", 0), ("m", "Int32", 0)):
        assert_column(got[name], OCol(t, [z] * n if t == "Utf8" else np.array([z] * n), none), name)
    for name, t, v in (("g", "Utf8", "ïve€"), ("h", "Utf8", "cde"), ("i", "Int32", 2), ("j", "Int32", 3), ("k", "Boolean", True), ("l", "Int32", 366), ("o", "Int32", 59)):
        assert_column(got[name], OCol(t, [v] * n if t == "Utf8" else np.array([v] * n)), name)


def test_a_negative_count_in_one_row_fails_the_batch_and_the_context_goes_on(ctx):
    n, row = 257, 130
    b = string_batch(n, seed=11)
    s = OCol("Utf8", b["s"].values)
    good = np.abs(np.random.default_rng(1).integers(0, 6, n)).astype(np.int64)
    bad = good.copy()
    bad[row] = -1
    plan = lambda c: ba.ProjectionExec([(fn("substr", col("s"), i64(2), col("cnt")), "x")], helpers.memory_exec(ctx, [[OrderedDict([("s", s), ("cnt", c)])]]))
    want = [K.substr(x, 2, int(c)) for x, c in zip(s.values, good)]
    with pytest.raises(ba.ExecutionError, match=K.NEGATIVE):
        plan(OCol("Int64", bad)).collect()
    masked = np.arange(n) != row
    assert_column(run(plan(OCol("Int64", bad, masked)))["x"], OCol("Utf8", [w if ok else "" for w, ok in zip(want, masked)], masked), "the bad row NULL")
    assert_column(run(plan(OCol("Int64", good)))["x"], OCol("Utf8", want), "the next, valid batch")
    last = good.copy()
    last[n - 1] = K.I64_MIN                                           # ... in the last row of the last, partial wave
    with pytest.raises(ba.ExecutionError, match=K.NEGATIVE):
        plan(OCol("Int64", last)).collect()


# ---- date_part ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_date_part_every_type_and_part(ctx, n):
    for dtype in K.TEMPORAL:
        edges = K.edge_values(dtype)
        values = np.array((edges[-4:] + edges[:9] + edges[9:])[:n] + [int(x) for x in K.random_temporal(dtype, max(0, n - len(edges)), seed=n)])[:n]
        valid = np.random.default_rng(n).random(n) > 0.1
        valid[:min(n, 13)] = True
        if n >= 63:
            valid[edge_rows(n)[1:]] = False
        col_valid = valid if n >= 63 else None
        np_t = np.int32 if dtype == "Date32" else np.int64
        b = OrderedDict([("x", OCol(dtype, values.astype(np_t), col_valid))])
        plan = ba.ProjectionExec([(fn("date_part", lit(p), col("x")), p) for p in K.PARTS], helpers.memory_exec(ctx, [[b]]))
        assert plan.schema() == [(p, "Int32", True) for p in K.PARTS]
        got = run(plan)
        for p in K.PARTS:
            want = [K.date_part(p, int(x), dtype) for x in values]
            ok = (valid if col_valid is not None else np.ones(n, np.bool_)) & np.array([w is not None for w in want])
            assert_column(got[p], OCol("Int32", np.array([0 if w is None else w for w in want], np.int32), ok), (dtype, p))
        if dtype == "Timestamp(Second)":
            assert got["year"].to_pylist()[0] is None                   # the int64 minimum: the year does not fit Int32


# ---- composed -------------------------------------------------------------------------------------------------------------------------

def phone_batch(n, seed):
    rng = np.random.default_rng(seed)
    phones = [f"{rng.integers(10, 35)}-{rng.integers(100, 1000)}-{rng.integers(100, 1000)}-{rng.integers(1000, 10000)}" for _ in range(n)]
    return OrderedDict([("c_phone", OCol("Utf8", phones, rng.random(n) > 0.05)), ("c_acctbal", OCol("Float64", np.round(rng.random(n) * 1000, 2))),
                        ("r", OCol("Int32", np.arange(n, dtype=np.int32)))])


CODE = fn("substr", col("c_phone"), i64(1), i64(2))


def test_substr_in_list_in_a_filter(ctx):
    b = phone_batch(257, seed=1)
    got = run(ba.FilterExec(E.InListExpr(CODE, [lit("13"), lit("31")]), helpers.memory_exec(ctx, [[b]])))
    want = [r for r, p, ok in zip(b["r"].values, b["c_phone"].values, b["c_phone"].is_valid()) if ok and p[:2] in ("13", "31")]
    assert 0 < len(want) < 100 and got["r"].to_pylist() == want


def test_substr_of_concat_lower_of_left_and_cast_of_substr(ctx):
    n = 257
    b = phone_batch(n, seed=2)
    rng = np.random.default_rng(2)
    b["w"] = OCol("Utf8", [["Alpha", "BETA", "", "gAmma Delta", "xY"][k] for k in rng.integers(0, 5, n)], rng.random(n) > 0.1)
    exprs = [(fn("substr", fn("concat", col("w"), lit("#"), col("c_phone")), i64(4), i64(5)), "sc"),
             (fn("lower", fn("left", col("w"), i64(3))), "ll"), (E.CastExpr(CODE, "Int32"), "code"),
             (fn("char_length", fn("concat", col("w"), col("w"))), "n2"), (fn("strpos", fn("upper", col("w")), lit("A")), "pa"),
             (fn("substr", col("c_phone"), E.CastExpr(fn("strpos", col("c_phone"), lit("-")), "Int64") + i64(1), i64(3)), "after_dash")]
    got = run(ba.ProjectionExec(exprs, helpers.memory_exec(ctx, [[b]])))
    w, p = b["w"], b["c_phone"]
    both = w.is_valid() & p.is_valid()
    assert_column(got["sc"], OCol("Utf8", [K.substr(a + "#" + c, 4, 5) if ok else "" for a, c, ok in zip(w.values, p.values, both)], both), "substr of concat")
    assert_column(got["ll"], OCol("Utf8", [a[:3].lower() if ok else "" for a, ok in zip(w.values, w.is_valid())], w.is_valid()), "lower of left")
    assert_column(got["code"], OCol("Int32", np.array([int(c[:2]) for c in p.values], np.int32), p.is_valid()), "CAST of substr")
    assert_column(got["n2"], OCol("Int32", np.array([2 * len(a) for a in w.values], np.int32), w.is_valid()), "char_length of concat")
    assert_column(got["pa"], OCol("Int32", np.array([a.upper().find("A") + 1 for a in w.values], np.int32), w.is_valid()), "strpos of upper")
    assert_column(got["after_dash"], OCol("Utf8", [c[3:6] if ok else "" for c, ok in zip(p.values, p.is_valid())], p.is_valid()), "substr from strpos")


def two_phase(keys, aggs, finals, m):
    partial = ba.HashAggregateExec(ba.plan.PARTIAL, keys, aggs, m)
    return ba.HashAggregateExec(ba.plan.FINAL, [(col(name), name) for _, name in keys], finals, ba.MergeExec(partial))


def test_substr_as_a_group_key_with_count_and_sum(ctx):
    """the shape of TPC-H Q22's first stage: customers by the country code of the phone number"""
    n = 1024
    b = phone_batch(n, seed=3)
    parts = [[helpers.slice_batch(b, 0, 400)], [helpers.slice_batch(b, 400, n)]]
    aggs = [E.Count(col("c_acctbal"), "numcust"), E.Sum(col("c_acctbal"), "totacctbal")]
    got = run(two_phase([(CODE, "cntrycode")], aggs, aggs, helpers.memory_exec(ctx, parts)))
    groups = {}
    for p, ok, bal in zip(b["c_phone"].values, b["c_phone"].is_valid(), b["c_acctbal"].values):
        groups.setdefault(p[:2] if ok else None, []).append(float(bal))
    want = {k: (len(v), math.fsum(v)) for k, v in groups.items()}          # fsum: the exact sum, rounded once
    assert len(want) == 26 and None in want
    rows = {k: (c, t) for k, c, t in zip(got["cntrycode"].to_pylist(), got["numcust"].to_pylist(), got["totacctbal"].to_pylist())}
    assert rows.keys() == want.keys() and len(got["cntrycode"]) == 26
    for k in want:
        # c positive values summed in whatever order: each of the c - 1 additions rounds once, (c - 1) * 2^-53 relative to the exact
        # sum, and the reference is that sum rounded once more
        assert rows[k][0] == want[k][0] and abs(rows[k][1] - want[k][1]) <= want[k][0] * 2.0**-53 * want[k][1], k


def date_batch(n, seed):
    rng = np.random.default_rng(seed)
    days = rng.integers(K.days_of(1992, 1, 1), K.days_of(1998, 12, 31) + 1, n).astype(np.int32)
    return OrderedDict([("d", OCol("Date32", days, rng.random(n) > 0.05)), ("amount", OCol("Int64", rng.integers(-1000, 1000, n))),
                        ("r", OCol("Int32", np.arange(n, dtype=np.int32)))])


def test_date_part_year_as_a_group_key_with_sum(ctx):
    """the shape of TPC-H Q9's grouping: extract(year from o_orderdate)"""
    n = 1024
    b = date_batch(n, seed=4)
    parts = [[helpers.slice_batch(b, 0, 500)], [helpers.slice_batch(b, 500, n)]]
    aggs = [E.Sum(col("amount"), "sum_profit")]
    got = run(two_phase([(fn("date_part", lit("year"), col("d")), "o_year")], aggs, aggs, helpers.memory_exec(ctx, parts)))
    want = {}
    for d, ok, a in zip(b["d"].values, b["d"].is_valid(), b["amount"].values):
        k = K.date_part("year", int(d), "Date32") if ok else None
        want[k] = want.get(k, 0) + int(a)
    assert sorted(k for k in want if k is not None) == list(range(1992, 1999)) and None in want
    assert got["o_year"].dtype == "Int32" and dict(zip(got["o_year"].to_pylist(), got["sum_profit"].to_pylist())) == want


def test_date_part_as_a_sort_key(ctx):
    n = 300
    b = date_batch(n, seed=5)
    order = [E.PhysicalSortExpr(fn("date_part", lit("month"), col("d")), descending=True), E.PhysicalSortExpr(fn("date_part", lit("dow"), col("d"))),
             E.PhysicalSortExpr(col("r"))]
    got = run(ba.SortExec(order, helpers.memory_exec(ctx, [[b]])))
    part = lambda p, i: K.date_part(p, int(b["d"].values[i]), "Date32") if b["d"].is_valid()[i] else None
    # descending with NULLs first, then ascending with NULLs first, then the row number
    want = sorted(range(n), key=lambda i: ((0, 0) if part("month", i) is None else (1, -part("month", i)), (0, 0) if part("dow", i) is None else (1, part("dow", i)), i))
    assert got["r"].to_pylist() == want and list(got) == ["d", "amount", "r"]


def test_starts_with_in_a_joins_residual_filter(ctx):
    rng = np.random.default_rng(6)
    nl, nr = 40, 300
    left = OrderedDict([("lk", OCol("Int64", rng.integers(0, 20, nl))), ("prefix", OCol("Utf8", [["1", "2", "13", ""][k] for k in rng.integers(0, 4, nl)], rng.random(nl) > 0.1))])
    phones = phone_batch(nr, seed=7)
    right = OrderedDict([("rk", OCol("Int64", rng.integers(0, 20, nr))), ("c_phone", phones["c_phone"]), ("r", phones["r"])])
    plan = ba.HashJoinExec(helpers.memory_exec(ctx, [[left]]), helpers.memory_exec(ctx, [[right]]), [("lk", "rk")], ba.plan.INNER,
                           filter=fn("starts_with", col("c_phone"), col("prefix")))
    got = run(plan)
    want = sorted((int(a), int(r)) for a, (lk, pf, pok) in enumerate(zip(left["lk"].values, left["prefix"].values, left["prefix"].is_valid()))
                  for rk, ph, hok, r in zip(right["rk"].values, right["c_phone"].values, right["c_phone"].is_valid(), right["r"].values)
                  if lk == rk and pok and hok and ph.startswith(pf))
    pairs = sorted(zip(got["lk"].to_pylist(), got["prefix"].to_pylist(), got["r"].to_pylist()))
    assert 50 < len(want) < nl * nr // 20
    assert pairs == sorted((int(left["lk"].values[a]), left["prefix"].values[a], r) for a, r in want)


def test_a_large_utf8_input_gives_a_large_result(ctx):
    import pyarrow as pa
    rng = np.random.default_rng(8)
    n = 257
    words = [None if rng.random() < 0.1 else K.random_string(rng) for _ in range(n)]
    t = pa.table([pa.array(words, pa.large_string()), pa.array(["ab"] * n, pa.string())],
                 schema=pa.schema([pa.field("s", pa.large_string()), pa.field("u", pa.string(), nullable=False)]))
    leaf = ba.ArrowStreamExec(pa.RecordBatchReader.from_batches(t.schema, t.to_batches()), ctx)
    exprs = [(fn("substr", col("s"), i64(2), i64(3)), "sub"), (fn("left", col("s"), i64(-1)), "l"), (fn("right", col("u"), i64(1)), "r"),
             (fn("char_length", col("s")), "n"), (fn("starts_with", col("s"), col("u")), "sw")]
    plan = ba.ProjectionExec(exprs, leaf)
    assert plan.schema() == [("sub", "LargeUtf8", True), ("l", "LargeUtf8", True), ("r", "Utf8", False), ("n", "Int32", True), ("sw", "Boolean", True)]
    got = pa.Table.from_batches([x.to_pyarrow() for x in plan.collect()])
    assert got.schema.field("sub").type == pa.large_string() and got.schema.field("r").type == pa.string()
    assert got["sub"].to_pylist() == [None if w is None else K.substr(w, 2, 3) for w in words]
    assert got["l"].to_pylist() == [None if w is None else K.left(w, -1) for w in words]
    assert got["r"].to_pylist() == ["b"] * n and got["n"].to_pylist() == [None if w is None else len(w) for w in words]
    assert got["sw"].to_pylist() == [None if w is None else w.startswith("ab") for w in words]
