"""CPU tier of concat / nullif / date_trunc / to_timestamp: the one grammar and calendar header (ballista_amd/csrc/temporal_text.h)
against the Python restatement (tests/temporal_cases.py), and the plan-time behaviour of the four functions with no GPU.

tests/c/temporal_text_check.cpp is a stand-alone program over that header — its own main, no HIP, no GPU — built here with
-fsanitize=address,undefined by the ROCm clang.  It reads one case per line and prints the int64, INVALID or NULL; every line is
compared.  The kernels (kernels_cast.hip) and the host's folding of literals run the same functions, so what holds here holds for
them (tests/test_scalar_fns_gpu.py checks that they do)."""
import os
import subprocess

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle.engine import OCol
from tests import plan_nodes as N, proto_encode as pe, temporal_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CLANGXX):
        pytest.skip("no ROCm clang for the sanitizer build")
    exe = str(tmp_path_factory.mktemp("temporal_text") / "temporal_text_check")
    r = subprocess.run([CLANGXX, "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ballista_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "temporal_text_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return exe


def run_checker(exe, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_bytes("".join(f"{d}\t{t}\t{a}\n" for d, t, a in lines).encode("utf-8"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-6000:]
    out = r.stdout.decode("utf-8").split("\n")
    assert out[-1] == "" and len(out) == len(lines) + 1, (len(out), len(lines))
    return out[:-1]


def parse_line(text):
    return ("P", "-", text)


def trunc_line(unit, g, v):
    return ("D", f"{K.UNITS[unit][0]}/{g}", str(int(v)))


def answer(v, none):
    return none if v is None else str(int(v))


# ---- the restatement first ----------------------------------------------------------------------------------------------------

def test_the_restatement_gives_the_pinned_values():
    """the expectations below come from the restatement: pin the literals of the contract, so that a slip in the restatement
    cannot pass as agreement"""
    for text, ns in K.PINNED_TEXTS:
        assert K.to_timestamp(text) == ns, text
    for text in K.INVALID_TEXTS:
        assert K.to_timestamp(text) is None, text
    for g, v, want in K.PINNED_TRUNC:
        assert K.date_trunc_one(g, v, K.NS) == want, (g, v)
        assert K.date_trunc(g, [v, 86400 * 10**9], K.NS) == [want, 86400 * 10**9 if g in ("second", "minute", "hour", "day") else K.date_trunc_one(g, 0, K.NS)], (g, v)
    # the scalar and the numpy restatement agree on every unit
    for unit, g, v in K.pinned_every_unit():
        assert K.date_trunc(g, [v], unit) == [K.date_trunc_one(g, v, unit)], (unit, g, v)
    assert K.date_trunc_one("week", -500, "Timestamp(Millisecond)") == -259200000 and K.date_trunc_one("month", -1, "Timestamp(Second)") == -2678400


def test_the_restatement_alone_keeps_nulls_under_one_percent():
    """inputs whose floor is unrepresentable give NULL: only within a year of the int64 minimum, so a NULL cannot hide a wrong floor"""
    v = K.random_values(K.NS, 20000, seed=4)
    nulls = sum(r is None for g in K.GRANULARITIES for r in K.date_trunc(g, v, K.NS))
    print("NULL floors among the nanosecond draws:", nulls, "of", 7 * len(v))
    assert nulls < 0.01 * len(v)
    for unit in K.UNITS:
        if unit != K.NS:
            assert all(r is not None for g in K.GRANULARITIES for r in K.date_trunc(g, K.random_values(unit, 2000, seed=5), unit))


# ---- the header, through the sanitized program ------------------------------------------------------------------------------------

def test_pinned_and_invalid_texts_through_the_sanitized_program(checker, tmp_path):
    texts = [t for t, _ in K.PINNED_TEXTS] + K.INVALID_TEXTS
    got = run_checker(checker, tmp_path, [parse_line(t) for t in texts])
    assert got[:len(K.PINNED_TEXTS)] == [str(ns) for _, ns in K.PINNED_TEXTS]
    assert got[len(K.PINNED_TEXTS):] == ["INVALID"] * len(K.INVALID_TEXTS), [t for t, g in zip(texts, got) if g != "INVALID"][len(K.PINNED_TEXTS):]


def test_pinned_truncations_through_the_sanitized_program(checker, tmp_path):
    lines = [trunc_line(K.NS, g, v) for g, v, _ in K.PINNED_TRUNC]
    want = [answer(w, "NULL") for _, _, w in K.PINNED_TRUNC]
    every = K.pinned_every_unit()
    lines += [trunc_line(u, g, v) for u, g, v in every]
    want += [answer(K.date_trunc_one(g, v, u), "NULL") for u, g, v in every]
    lines += [("D", "ns/Month", "0"), ("D", "ns/", "0"), ("D", "ns/months", "0"), ("D", "ns/mont", "0"), ("D", "ns/quarter", "0")]
    want += ["UNKNOWN"] * 5
    got = run_checker(checker, tmp_path, lines)
    assert got == want, [(l, g, w) for l, g, w in zip(lines, got, want) if g != w][:10]


def test_random_texts_parse_to_the_bit(checker, tmp_path):
    """20 000 random instants of the whole int64 range, formatted with random fraction widths, separators and offsets"""
    cases = K.random_texts(20000, seed=1)
    assert all(K.to_timestamp(t) == ns for t, ns in cases)
    got = run_checker(checker, tmp_path, [parse_line(t) for t, _ in cases])
    bad = [(t, g, ns) for (t, ns), g in zip(cases, got) if g != str(ns)]
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("unit", list(K.UNITS))
def test_random_values_through_every_granularity(checker, tmp_path, unit):
    """20 000 random values of the unit: the floor by numpy's datetime64 conversion, NULL where it does not fit int64"""
    v = K.random_values(unit, 20000, seed=11 + len(unit))
    lines, want = [], []
    for g in K.GRANULARITIES:
        lines += [trunc_line(unit, g, x) for x in v]
        want += [answer(r, "NULL") for r in K.date_trunc(g, v, unit)]
    nulls = want.count("NULL")
    assert nulls < 0.01 * len(v) if unit == K.NS else nulls == 0, nulls
    got = run_checker(checker, tmp_path, lines)
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])


# ---- plan time, with no GPU ---------------------------------------------------------------------------------------------------------

def fn(name, *args):
    return E.ScalarFunctionExpr(name, list(args))


def wire_fn(name, *args):
    e = object.__new__(E.ScalarFunctionExpr)          # past the host mirror's own checks: the wire can carry any call
    e.fun, e.args = name, list(args)
    return e


def leaf():
    b = {"s": OCol("Utf8", ["a", ""], np.array([True, False])), "u": OCol("Utf8", ["b", "c"]), "k": OCol("Int64", [1, 2]),
         "i": OCol("Int32", [1, 2]), "t": OCol("Timestamp(Millisecond)", np.array([1, 2], np.int64)),
         "d": OCol("Date32", np.array([1, 2], np.int32)), "g": OCol("Utf8", ["day", "day"])}
    m = N.MemoryExec([[b]])
    m.name = "mem://fns"
    return m


def decode(exprs):
    return ba.ExecutionPlan.from_proto(None, pe.plan(N.ProjectionExec(exprs, leaf())))


def test_wire_plan_with_the_four_functions_decodes():
    """on the commit before this feature the decode itself raised NotImplementedOnGpu "scalar function 'concat' is not supported\""""
    exprs = [(fn("concat", col("s"), lit("#"), col("u")), "c3"), (fn("concat", col("u"), lit("x")), "c2"), (fn("nullif", col("i"), lit(0)), "nz"),
             (fn("nullif", col("k"), col("k")), "nk"), (fn("date_trunc", lit("month"), col("t")), "month"), (fn("to_timestamp", col("s")), "ts"),
             (fn("to_timestamp", col("u")), "tu"), (fn("to_timestamp", lit("1969-12-31T23:59:59.5Z")), "folded"),
             (fn("date_trunc", lit("day"), fn("to_timestamp", lit("1969-12-31T23:59:59.5Z"))), "folded_day")]
    plan = decode(exprs)
    assert plan.schema() == [("c3", "Utf8", True), ("c2", "Utf8", False), ("nz", "Int64", True), ("nk", "Int64", True),
                             ("month", "Timestamp(Millisecond)", True), ("ts", "Timestamp(Nanosecond)", True),
                             ("tu", "Timestamp(Nanosecond)", False), ("folded", "Timestamp(Nanosecond)", False),
                             ("folded_day", "Timestamp(Nanosecond)", True)]
    text = plan.display()
    for part in ("concat(s, '#', u)", "concat(u, 'x')", "nullif(CAST(i AS Int64), Int64(0))", "nullif(k, k)", "date_trunc('month', t)",
                 "to_timestamp(s)"):
        assert part in text, (part, text)


def test_the_python_mirror_types_and_coerces_like_the_library():
    s = {"s": E.UTF8, "i": E.INT32, "k": E.INT64, "t": E.TIMESTAMP_US, "f": E.FLOAT64}
    assert E.expr_type(fn("concat", col("s"), lit("x")), s) == E.UTF8 and E.expr_type(fn("to_timestamp", col("s")), s) == E.TIMESTAMP_NS
    assert E.expr_type(fn("date_trunc", lit("week"), col("t")), s) == E.TIMESTAMP_US and E.expr_type(fn("nullif", col("f"), lit(0.0)), s) == E.FLOAT64
    c = E.coerce(fn("nullif", col("i"), lit(0)), s)
    assert isinstance(c.args[0], E.CastExpr) and c.args[0].dtype == E.INT64 and E.expr_type(c, s) == E.INT64
    c = E.coerce(fn("nullif", col("f"), lit(0)), s)
    assert isinstance(c.args[1], E.Literal) and c.args[1].dtype == E.FLOAT64 and c.args[1].value == 0.0
    with pytest.raises(NotImplementedError):
        fn("md5", col("s"))
    with pytest.raises(NotImplementedError, match="more than 8"):
        fn("concat", *[col("s")] * 9)
    with pytest.raises(ValueError):
        fn("nullif", col("i"))


def test_two_concats_that_differ_in_their_second_argument_are_two_columns():
    """Utf8Lowering::rewrite de-duplicates nodes by their text: a call printed by its first argument alone would merge these"""
    both = decode([(fn("octet_length", fn("concat", col("s"), lit("x"))), "a"), (fn("octet_length", fn("concat", col("s"), lit("yy"))), "b")])
    text = both.display()
    assert "concat(s, 'x')" in text and "concat(s, 'yy')" in text
    one = decode([(fn("concat", col("s"), lit("x")), "a"), (fn("concat", col("s"), lit("yy")), "b")])
    assert one.schema() == [("a", "Utf8", True), ("b", "Utf8", True)]


REFUSALS = [
    (wire_fn("concat", *[col("s")] * 9), ba.NotImplementedOnGpu, "concat with more than 8 arguments"),
    (wire_fn("nullif", col("s"), lit("a")), ba.NotImplementedOnGpu, "nullif over Utf8"),
    (wire_fn("date_trunc", lit("quarter"), col("t")), ba.PlanError, "Unsupported date_trunc granularity 'quarter'"),
    (wire_fn("date_trunc", lit("Month"), col("t")), ba.PlanError, "Unsupported date_trunc granularity 'Month'"),
    (wire_fn("date_trunc", col("g"), col("t")), ba.NotImplementedOnGpu, "date_trunc granularity must be a non-NULL Utf8 literal"),
    (wire_fn("date_trunc", lit("day"), col("d")), ba.PlanError, "date_trunc requires a Timestamp argument, not Date32"),
    (wire_fn("concat", col("s"), col("k")), ba.PlanError, "concat requires Utf8 arguments, not Int64"),
    (wire_fn("to_timestamp", col("k")), ba.PlanError, "to_timestamp requires a Utf8 argument"),
    (wire_fn("md5", col("s")), ba.NotImplementedOnGpu, "md5"),
    (wire_fn("array", col("k"), col("k")), ba.NotImplementedOnGpu, "array"),
    (wire_fn("nullif", col("k")), ba.PlanError, "takes two arguments"),
]


@pytest.mark.parametrize("e, error, message", REFUSALS, ids=[m for _, _, m in REFUSALS])
def test_each_refusal_arrives_with_its_status_and_message(e, error, message):
    with pytest.raises(error, match=message):
        decode([(e, "x")])
    # ... in a filter as well as in a projection, where the result type allows one
    if E.expr_type(e, {"s": "Utf8", "k": "Int64", "t": "Timestamp(Millisecond)", "d": "Date32", "g": "Utf8"}) != "Utf8" and e.fun not in ("md5", "array"):
        with pytest.raises(error, match=message):
            ba.ExecutionPlan.from_proto(None, pe.plan(N.FilterExec(E.IsNotNullExpr(e), leaf())))
