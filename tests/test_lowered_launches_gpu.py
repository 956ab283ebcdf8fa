"""Every kind of lowered node (host/utf8_exprs.cpp: an expression evaluated as an extra column of the batch) alone in a
ProjectionExec: the kernel launches behind it, pinned by name and count; the same 14 expressions over an empty and over a one-row
batch; and the three evaluators that size their data buffer from a bound, with the bound above 64 MiB, where they read the true total
before they allocate.

The expected values come from the Python restatements the other suites use (tests/string_fn_cases.py, tests/cast_text_cases.py,
tests/temporal_cases.py), hashlib and str; Utf8 results are compared to the byte and to the offset as the device holds them.

LAUNCHES was recorded from Context.kernel_stats() at BHIP_KERNEL_TIMING=2 (every launch is named, however small) before the scalar
functions moved into one table: launch counts have no noise, so equality is exact."""
import hashlib
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col, lit
from oracle.engine import OCol
from tests import cast_text_cases as CK, helpers, string_fn_cases as K, temporal_cases as TK

pytestmark = pytest.mark.gpu

NS = "Timestamp(Nanosecond)"


def fn(name, *args):
    return E.ScalarFunctionExpr(name, list(args))


def i64(v):
    return E.Literal(v, "Int64")


def batch(n, seed=1):
    """s: timestamp texts (what to_timestamp accepts: any other value fails the batch), NULL in row 3 when there is one"""
    rng = np.random.default_rng(seed)
    s = [t for t, _ in TK.random_texts(n, seed)]
    valid = np.arange(n) != 3
    return OrderedDict([("s", OCol("Utf8", s, valid)), ("i", OCol("Int64", rng.integers(-5, 40, n))), ("f", OCol("Float64", rng.random(n))),
                        ("d", OCol("Date32", rng.integers(-30000, 30000, n).astype(np.int32))),
                        ("t", OCol(NS, TK.random_values(NS, n, seed)))])


def rows(b, *names):
    return zip(*[b[x].to_pylist() for x in names])


def cases(b):
    """[(name, expression, result type, expected values with None for NULL)]: each lowered node kind once"""
    S = col("s")
    null_in = lambda f: [None if any(x is None for x in r) else f(*r) for r in rows(b, "s", "i", "f", "d", "t")]
    return [
        ("lower", fn("lower", S), "Utf8", null_in(lambda s, i, f, d, t: s.lower())),
        ("sha256", fn("sha256", S), "Binary", null_in(lambda s, i, f, d, t: hashlib.sha256(s.encode()).digest())),
        ("concat", fn("concat", S, lit("-"), S), "Utf8", null_in(lambda s, i, f, d, t: s + "-" + s)),
        ("substr", fn("substr", S, i64(2), i64(3)), "Utf8", null_in(lambda s, i, f, d, t: K.substr(s, 2, 3))),
        ("left", fn("left", S, col("i")), "Utf8", null_in(lambda s, i, f, d, t: K.left(s, i))),
        ("case", E.CaseExpr(None, [(col("f") > lit(0.5), S)], lit("none")), "Utf8",
         [s if f > 0.5 else "none" for s, f in rows(b, "s", "f")]),
        ("cast_to_utf8", E.CastExpr(col("i"), "Utf8"), "Utf8", [CK.format_value(i, "Int64") for i, in rows(b, "i")]),
        ("cast_from_utf8", E.CastExpr(S, "Int64"), "Int64", null_in(lambda s, i, f, d, t: CK.parse(s, "Int64"))),
        ("to_timestamp", fn("to_timestamp", S), NS, null_in(lambda s, i, f, d, t: TK.to_timestamp(s))),
        ("date_trunc", fn("date_trunc", lit("month"), col("t")), NS, [TK.date_trunc_one("month", t, NS) for t, in rows(b, "t")]),
        ("date_part", fn("date_part", lit("year"), col("d")), "Int32", [K.date_part("year", d, "Date32") for d, in rows(b, "d")]),
        ("char_length", fn("char_length", S), "Int32", null_in(lambda s, i, f, d, t: K.char_length(s))),
        ("strpos", fn("strpos", S, lit("a")), "Int32", null_in(lambda s, i, f, d, t: K.strpos(s, "a"))),
        ("starts_with", fn("starts_with", S, S), "Boolean", null_in(lambda s, i, f, d, t: K.starts_with(s, s))),
    ]


CASE_NAMES = ["lower", "sha256", "concat", "substr", "left", "case", "cast_to_utf8", "cast_from_utf8", "to_timestamp", "date_trunc",
              "date_part", "char_length", "strpos", "starts_with"]

# {case: {kernel name: launches}} of one 1000-row batch through ProjectionExec([(expression, "x")])
LAUNCHES = {
    "lower": {"str_transform_lengths": 1, "str_transform_write": 1},
    "sha256": {"sha2": 1},
    "concat": {"concat_lengths": 1, "concat_write": 1},
    "substr": {"str_range_lengths": 1, "str_range_write": 1},
    "left": {"str_range_lengths": 1, "str_range_write": 1},
    # (scan_project: the WHEN condition as a Boolean column; str_broadcast: the ELSE literal as a column)
    "case": {"scan_project": 1, "str_broadcast": 1, "str_select_lengths": 1, "str_select_write": 1},
    "cast_to_utf8": {"cast_format_lengths": 1, "cast_format_write": 1},
    "cast_from_utf8": {"cast_parse": 1},
    "to_timestamp": {"to_timestamp_parse": 1},
    "date_trunc": {"date_trunc": 1},
    "date_part": {"date_part": 1},
    "char_length": {"char_length": 1},
    "strpos": {"strpos": 1},
    "starts_with": {"starts_with": 1},
}


# ---- launch pinning --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def timed():
    """a context that names every launch, however small (BHIP_KERNEL_TIMING is read when a context is created), and the 1000-row
    batch on it"""
    mp = pytest.MonkeyPatch()
    mp.setenv("BHIP_KERNEL_TIMING", "2")
    try:
        c = ba.Context(0)
    finally:
        mp.undo()
    b = batch(1000)
    return c, b, helpers.memory_exec(c, [[b]])


def launches_of(tctx, plan):
    tctx.kernel_stats(reset=True)
    batches = plan.collect()
    return {k: v[1] for k, v in tctx.kernel_stats(reset=True).items()}, batches


@pytest.mark.parametrize("name", CASE_NAMES)
def test_launches_of_each_lowered_node_kind(timed, name):
    tctx, b, leaf = timed
    assert not b["s"].is_valid()[3] and [c[0] for c in cases(b)] == CASE_NAMES
    _, e, dtype, want = next(c for c in cases(b) if c[0] == name)
    plan = ba.ProjectionExec([(e, "x")], leaf)
    assert [t for _, t, _ in plan.schema()] == [dtype]
    got, batches = launches_of(tctx, plan)
    assert values_of(batches, 0, dtype) == want
    assert got == LAUNCHES[name]


# ---- empty and single-row batches ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    return ba.Context(0)


def utf8_raw(rb, i):
    """(offsets, value bytes, validity or None) of column i as the device holds them; the byte count is the column's data_bytes"""
    _, dtype, _, nbytes, has_valid = rb.column_info(i)
    assert dtype in ("Utf8", "Binary")
    n = rb.num_rows
    off, data, vbuf = np.zeros(n + 1, np.int32), np.zeros(max(1, nbytes), np.uint8), np.zeros((n + 7) // 8 + 8, np.uint8)
    L.check(L.lib().bhip_batch_column_to_host(rb._h, i, data.ctypes.data, off.ctypes.data, vbuf.ctypes.data if has_valid else None))
    return off, data[:nbytes].tobytes(), np.unpackbits(vbuf, bitorder="little")[:n].astype(np.bool_) if has_valid else None


def values_of(batches, i, dtype):
    """column i of the batches as Python values, None for NULL (a Binary column: bytes)"""
    out = []
    for rb in batches:
        if dtype == "Binary":
            off, data, valid = utf8_raw(rb, i)
            out += [data[off[k]:off[k + 1]] if valid is None or valid[k] else None for k in range(rb.num_rows)]
        else:
            got = OCol(*rb.column(i))
            assert got.dtype == dtype
            out += got.to_pylist()
    return out


def assert_layout(rb, i, encoded, what):
    """column i holds exactly these values' bytes, back to back, under offsets that are their running sum"""
    off, data, _ = utf8_raw(rb, i)
    lens = np.fromiter((len(x) for x in encoded), np.int64, len(encoded))
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)), what
    assert data == b"".join(encoded), what


@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single_row_batches(ctx, n):
    b = batch(n)
    cs = cases(b)
    plan = ba.ProjectionExec([(e, name) for name, e, _, _ in cs], helpers.memory_exec(ctx, [[b]]))
    assert [(name, t) for name, t, _ in plan.schema()] == [(name, t) for name, _, t, _ in cs]
    batches = plan.collect()
    assert sum(x.num_rows for x in batches) == n
    for i, (name, _, dtype, want) in enumerate(cs):
        assert len(want) == n and values_of(batches, i, dtype) == want, name
        if n and dtype in ("Utf8", "Binary"):
            assert_layout(batches[0], i, [b"" if w is None else w if dtype == "Binary" else w.encode() for w in want], name)


# ---- the bound above 64 MiB: the true total is read before the data buffer is sized ---------------------------------------------------

BOUND = 64 << 20
N_BIG = 40000
LIT_BYTES = 240                             # STR_LITERAL_MAX (str_kernels.h): the longest literal a CASE branch or concat carries


def test_case_of_eight_long_literals_over_the_bound(ctx):
    """8 WHEN branches of 240-byte literals over 40 000 rows: the branches' byte counts sum to 8 * 240 * 40 000 = 76.8 MB, above the
    64 MiB bound, and a row takes one of them: 9.6 MB in all"""
    rng = np.random.default_rng(5)
    k = rng.integers(0, 8, N_BIG)
    lits = [chr(ord("a") + j) * LIT_BYTES for j in range(8)]
    assert 8 * LIT_BYTES * N_BIG > BOUND
    e = E.CaseExpr(None, [(col("k").eq(i64(j)), lit(lits[j])) for j in range(8)], None)
    plan = ba.ProjectionExec([(e, "x")], helpers.memory_exec(ctx, [[OrderedDict([("k", OCol("Int64", k))])]]))
    batches = plan.collect()
    assert len(batches) == 1 and batches[0].num_rows == N_BIG and batches[0].column_info(0)[3] == LIT_BYTES * N_BIG
    assert_layout(batches[0], 0, [lits[j].encode() for j in k], "CASE")


def test_concat_of_a_column_with_itself_eight_times_over_the_bound(ctx):
    """one 240-byte-per-row Utf8 column, 8 times, over 40 000 rows: bound and total are both 76.8 MB"""
    rng = np.random.default_rng(6)
    s = [chr(ord("a") + int(j)) * LIT_BYTES for j in rng.integers(0, 26, N_BIG)]
    assert 8 * LIT_BYTES * N_BIG > BOUND
    plan = ba.ProjectionExec([(fn("concat", *[col("s")] * 8), "x")], helpers.memory_exec(ctx, [[OrderedDict([("s", OCol("Utf8", s))])]]))
    batches = plan.collect()
    assert len(batches) == 1 and batches[0].num_rows == N_BIG and batches[0].column_info(0)[3] == 8 * LIT_BYTES * N_BIG
    assert_layout(batches[0], 0, [(x * 8).encode() for x in s], "concat")


CAST_TEXT_MAX = 20                          # cast_format_max(Int64) (cast_text.h): "-9223372036854775808"
N_CAST = BOUND // CAST_TEXT_MAX + 1


def test_cast_int64_to_utf8_over_the_bound(ctx):
    """CAST(x AS Utf8) of Int64, whose cast_format_max of 20 bytes is the largest of the fixed-width types (UInt64 shares it), at
    n = 3 355 444 rows: the smallest n with n * 20 > 64 MiB (3 355 443 * 20 = 67 108 860 <= 67 108 864 < 3 355 444 * 20)"""
    assert (N_CAST - 1) * CAST_TEXT_MAX <= BOUND < N_CAST * CAST_TEXT_MAX and N_CAST == 3355444
    rng = np.random.default_rng(7)
    x = rng.integers(-10**6, 10**6, N_CAST)
    x[:4] = [CK.INT_RANGE["Int64"][0], CK.INT_RANGE["Int64"][1], 0, -1]
    valid = np.ones(N_CAST, np.bool_)
    valid[[5, N_CAST - 1]] = False
    plan = ba.ProjectionExec([(E.CastExpr(col("x"), "Utf8"), "s")], helpers.memory_exec(ctx, [[OrderedDict([("x", OCol("Int64", x, valid))])]]))
    batches = plan.collect()
    assert len(batches) == 1 and batches[0].num_rows == N_CAST
    assert CK.format_value(int(x[0]), "Int64") == str(int(x[0])) and len(str(int(x[0]))) == CAST_TEXT_MAX
    texts = [str(v).encode() for v in x.tolist()]
    texts[5] = texts[N_CAST - 1] = b""
    assert_layout(batches[0], 0, texts, "CAST")
    assert np.array_equal(utf8_raw(batches[0], 0)[2], valid)
