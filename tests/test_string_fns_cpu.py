"""CPU tier of substr / left / right / char_length / strpos / starts_with / date_part: the headers that hold their rules
(ballista_amd/csrc/str_text.h, and date_part in temporal_text.h) against the Python restatement (tests/string_fn_cases.py), and the
plan-time behaviour of the seven functions with no GPU.

tests/c/scalar_text_check.cpp is a stand-alone program over the two headers — its own main, no HIP, no GPU — built here with
-fsanitize=address,undefined by the ROCm clang.  It reads one case per line and prints the answer; every line is compared.  The
kernels (kernels_str.hip, kernels_cast.hip) and the host's folding of literals run the same functions, so what holds here holds
for them (tests/test_string_fns_gpu.py checks that they do).

The functions have no wire form: the plans below are made through the C ABI over a leaf decoded from a wire plan with no context,
which can be inspected and not executed."""
import os
import subprocess

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle.engine import OCol
from tests import plan_nodes as N, proto_encode as pe, string_fn_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CLANGXX):
        pytest.skip("no ROCm clang for the sanitizer build")
    exe = str(tmp_path_factory.mktemp("scalar_text") / "scalar_text_check")
    r = subprocess.run([CLANGXX, "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ballista_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "scalar_text_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return exe


def run_checker(exe, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_bytes("".join("\t".join(fields) + "\n" for fields in lines).encode("utf-8"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-6000:]
    out = r.stdout.decode("utf-8").split("\n")
    assert out[-1] == "" and len(out) == len(lines) + 1, (len(out), len(lines))
    return out[:-1]


def string_line(fn, args):
    return [fn] + [a if isinstance(a, str) else str(int(a)) for a in args]


def part_line(part, v, dtype):
    return ["date_part", f"{K.TEMPORAL[dtype][0]}/{part}", str(int(v))]


def text_of(answer):
    if answer is None:
        return "NULL"
    if isinstance(answer, bool):
        return "true" if answer else "false"
    return answer if isinstance(answer, str) else str(int(answer))


# ---- the restatement first ----------------------------------------------------------------------------------------------------

def test_the_restatement_gives_the_pinned_values():
    """the expectations below come from the restatement: pin the literals of the contract, so that a slip in the restatement
    cannot pass as agreement"""
    for fn, args, want in K.PINNED_STRINGS:
        got = K.evaluate(fn, args)
        assert got == want and type(got) is type(want), (fn, args, got)
    assert K.evaluate("substr", ("abc", 1, -1)) == K.NEGATIVE
    for part, v, dtype, want in K.PINNED_PARTS:
        assert K.date_part(part, v, dtype) == want, (part, v, dtype)
    # 2024-02-29T13:14:15.987654321Z, a Thursday, in every unit
    ns = (K.days_of(2024, 2, 29) * 86400 + 13 * 3600 + 14 * 60 + 15) * 10**9 + 987654321
    want = dict(year=2024, quarter=1, month=2, day=29, dow=4, doy=60, hour=13, minute=14, second=15)
    for dtype in ("Timestamp(Second)", "Timestamp(Millisecond)", "Timestamp(Microsecond)", "Timestamp(Nanosecond)", "Date64"):
        v = ns // (86400 * 10**9 // K.TEMPORAL[dtype][1])
        assert {p: K.date_part(p, v, dtype) for p in K.PARTS} == want, dtype
    assert {p: K.date_part(p, K.days_of(2024, 2, 29), "Date32") for p in K.PARTS} == dict(want, hour=0, minute=0, second=0)


# ---- the headers, through the sanitized program -----------------------------------------------------------------------------------

def test_pinned_calls_through_the_sanitized_program(checker, tmp_path):
    lines = [string_line(fn, args) for fn, args, _ in K.PINNED_STRINGS] + [["substr", "abc", "1", "-1"], ["substr", "", str(K.I64_MIN), str(K.I64_MIN)]]
    want = [text_of(w) for _, _, w in K.PINNED_STRINGS] + [K.NEGATIVE] * 2
    lines += [part_line(p, v, t) for p, v, t, _ in K.PINNED_PARTS]
    want += [text_of(w) for _, _, _, w in K.PINNED_PARTS]
    lines += [["date_part", "ns/" + p, "0"] for p in ("Year", "", "years", "yea", "week", "epoch")]
    want += ["UNKNOWN"] * 6
    got = run_checker(checker, tmp_path, lines)
    assert got == want, [(l, g, w) for l, g, w in zip(lines, got, want) if g != w][:10]


def test_random_string_calls_agree_to_the_byte(checker, tmp_path):
    """7 000 calls over strings of 0 .. 40 code points of 1 to 4 bytes; start, count and n from {int64 min, -3 .. len + 3, int64 max}"""
    calls = K.random_string_calls(7000, seed=1)
    want = [text_of(K.evaluate(fn, args)) for fn, args in calls]
    assert 100 < want.count(K.NEGATIVE) < 700 and want.count("") > 300 and want.count("true") > 200 and want.count("false") > 200
    got = run_checker(checker, tmp_path, [string_line(fn, args) for fn, args in calls])
    bad = [(c, g, w) for c, g, w in zip(calls, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("dtype", list(K.TEMPORAL))
def test_date_part_every_part_at_the_edges_and_at_random(checker, tmp_path, dtype):
    """the days around every month end of two leap and two ordinary years, +-1 unit around 0 and the midnights, the extremes of the
    storage type, and 2 000 random values"""
    values = K.edge_values(dtype) + [int(v) for v in K.random_temporal(dtype, 2000, seed=len(dtype))]
    lines = [part_line(p, v, dtype) for p in K.PARTS for v in values]
    want = [text_of(K.date_part(p, v, dtype)) for p in K.PARTS for v in values]
    nulls = want.count("NULL")
    # only a year can be NULL, and only of seconds: int64 milliseconds end in the year 292 278 994, inside Int32
    assert (nulls > 0) == (dtype == "Timestamp(Second)") and nulls < 0.05 * len(want), nulls
    got = run_checker(checker, tmp_path, lines)
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])


# ---- plan time, with no GPU ---------------------------------------------------------------------------------------------------------

def fn(name, *args):
    return E.ScalarFunctionExpr(name, list(args))


def c_fn(name, *args):
    e = object.__new__(E.ScalarFunctionExpr)          # past the host mirror's own checks: the C ABI can be handed any call
    e.fun, e.args = name, list(args)
    return e


def leaf():
    """a plan to build on, made with no context"""
    b = {"s": OCol("Utf8", ["a", ""], np.array([True, False])), "u": OCol("Utf8", ["b", "c"]), "k": OCol("Int64", [1, 2]),
         "kn": OCol("Int64", [1, 2], np.array([True, False])), "i": OCol("Int32", [1, 2]), "f": OCol("Float64", [1.0, 2.0]),
         "t": OCol("Timestamp(Millisecond)", np.array([1, 2], np.int64)), "d": OCol("Date32", np.array([1, 2], np.int32)),
         "d64": OCol("Date64", np.array([1, 2], np.int64), np.array([True, False])), "g": OCol("Utf8", ["day", "day"])}
    m = N.MemoryExec([[b]])
    m.name = "mem://fns"
    return ba.ExecutionPlan.from_proto(None, pe.plan(m))


SCHEMA = {"s": "Utf8", "u": "Utf8", "k": "Int64", "kn": "Int64", "i": "Int32", "f": "Float64", "t": "Timestamp(Millisecond)", "d": "Date32",
          "d64": "Date64", "g": "Utf8"}


def project(exprs):
    return ba.ProjectionExec(exprs, leaf())


def test_result_types_nullability_and_display():
    """on the commit before this feature E.ScalarFunctionExpr("substr", ...) raised NotImplementedError and the C ABI answered
    BHIP_ENOTIMPL"""
    exprs = [(fn("substr", col("s"), lit(1), lit(2)), "sub3"), (fn("substring", col("u"), lit(2)), "sub2"), (fn("substr", col("u"), col("kn")), "sub_col"),
             (fn("left", col("u"), lit(3)), "l"), (fn("right", col("s"), col("k")), "r"),
             (fn("char_length", col("s")), "n"), (fn("length", col("u")), "n_alias"), (fn("character_length", col("u")), "n_alias2"),
             (fn("strpos", col("u"), lit("b")), "p"), (fn("strpos", col("u"), col("s")), "p_col"),
             (fn("starts_with", col("u"), lit("")), "sw"), (fn("starts_with", col("s"), col("u")), "sw_col"),
             (fn("date_part", lit("year"), col("d")), "y"), (fn("date_part", lit("dow"), col("t")), "dow"), (fn("date_part", lit("hour"), col("d64")), "h"),
             (fn("substr", lit("alphabet"), lit(0), lit(3)), "folded"), (fn("strpos", lit("€𝄞x"), lit("x")), "folded_pos"),
             (fn("date_part", lit("doy"), E.date32("2000-12-31")), "folded_doy"), (fn("left", col("u"), E.Literal(None, "Int64")), "null_n")]
    plan = project(exprs)
    assert plan.schema() == [("sub3", "Utf8", True), ("sub2", "Utf8", False), ("sub_col", "Utf8", True), ("l", "Utf8", False), ("r", "Utf8", True),
                             ("n", "Int32", True), ("n_alias", "Int32", False), ("n_alias2", "Int32", False), ("p", "Int32", False),
                             ("p_col", "Int32", True), ("sw", "Boolean", False), ("sw_col", "Boolean", True), ("y", "Int32", True),
                             ("dow", "Int32", True), ("h", "Int32", True), ("folded", "Utf8", False), ("folded_pos", "Int32", False),
                             ("folded_doy", "Int32", True), ("null_n", "Utf8", True)]
    text = plan.display()
    for part in ("substr(s, Int64(1), Int64(2)) as sub3", "substr(u, Int64(2)) as sub2", "left(u, Int64(3))", "right(s, k)", "char_length(s) as n",
                 "char_length(u) as n_alias,", "char_length(u) as n_alias2", "strpos(u, 'b')", "starts_with(s, u)", "date_part('year', d)",
                 "date_part('dow', t)"):
        assert part in text, (part, text)
    # the same functions in a filter and below the VM's own operators
    f = ba.FilterExec(E.InListExpr(fn("substr", col("u"), lit(1), lit(2)), [lit("13"), lit("31")]), leaf())
    assert "substr(u, Int64(1), Int64(2)) IN ('13', '31')" in f.display()
    ba.FilterExec(fn("starts_with", fn("lower", fn("left", col("u"), lit(3))), lit("ab")).and_(fn("date_part", lit("year"), col("d")).eq(lit(1995, "Int32"))), leaf())
    ba.ProjectionExec([(E.CastExpr(fn("substr", col("u"), lit(1), lit(2)), "Int32"), "code"),
                       (fn("substr", col("u"), E.CastExpr(fn("strpos", col("u"), lit("-")), "Int64") + lit(1)), "after_dash")], leaf())


def test_the_python_mirror_types_and_coerces_like_the_library():
    assert E.expr_type(fn("substr", col("s"), lit(1)), SCHEMA) == E.UTF8 and E.expr_type(fn("left", col("s"), lit(1)), SCHEMA) == E.UTF8
    assert E.expr_type(fn("right", col("s"), lit(1)), SCHEMA) == E.UTF8 and E.expr_type(fn("length", col("s")), SCHEMA) == E.INT32
    assert E.expr_type(fn("strpos", col("s"), lit("a")), SCHEMA) == E.INT32 and E.expr_type(fn("starts_with", col("s"), lit("a")), SCHEMA) == E.BOOLEAN
    assert E.expr_type(fn("date_part", lit("year"), col("d")), SCHEMA) == E.INT32
    assert fn("substring", col("s"), lit(1)).fun == "substr" and fn("length", col("s")).fun == fn("character_length", col("s")).fun == "char_length"
    c = E.coerce(fn("substr", col("s"), col("i"), lit(2, "Int32")), SCHEMA)
    assert isinstance(c.args[1], E.CastExpr) and c.args[1].dtype == E.INT64
    assert isinstance(c.args[2], E.Literal) and c.args[2].dtype == E.INT64 and c.args[2].value == 2
    assert project([(c, "x")]).schema() == [("x", "Utf8", True)]
    with pytest.raises(ba.PlanError, match="left requires Int64 arguments after the first, not Int32"):
        project([(fn("left", col("s"), col("i")), "x")])
    for name, args in (("substr", [col("s")]), ("substr", [col("s")] + [lit(1)] * 3), ("left", [col("s")]), ("right", [col("s"), lit(1), lit(1)]),
                       ("char_length", [col("s"), col("s")]), ("strpos", [col("s")]), ("starts_with", [col("s")]), ("date_part", [col("d")])):
        with pytest.raises(ValueError):
            fn(name, *args)
    for name in ("replace", "lpad", "rpad", "split_part", "btrim", "md5", "array"):
        with pytest.raises(NotImplementedError):
            fn(name, col("s"), col("s"))


REFUSALS = [
    (c_fn("substr", col("s")), ba.PlanError, "takes two or three arguments"),
    (c_fn("substr", col("s"), lit(1), lit(1), lit(1)), ba.PlanError, "takes two or three arguments"),
    (c_fn("left", col("s")), ba.PlanError, "'left' takes two arguments"),
    (c_fn("char_length", col("s"), col("s")), ba.PlanError, "takes one argument"),
    (c_fn("strpos", col("s")), ba.PlanError, "'strpos' takes two arguments"),
    (c_fn("date_part", col("d")), ba.PlanError, "'date_part' takes two arguments"),
    (c_fn("substr", col("s"), lit(1), lit(-1)), ba.PlanError, "negative substring length not allowed"),
    (c_fn("substring", col("s"), lit(1), lit(-(2**63))), ba.PlanError, "negative substring length not allowed"),
    (c_fn("substr", col("k"), lit(1)), ba.PlanError, "substr requires a Utf8 first argument, not Int64"),
    (c_fn("right", col("s"), col("f")), ba.PlanError, "right requires Int64 arguments after the first, not Float64"),
    (c_fn("substr", col("s"), lit("1")), ba.PlanError, "substr requires Int64 arguments after the first, not Utf8"),
    (c_fn("length", col("k")), ba.PlanError, "char_length requires a Utf8 first argument, not Int64"),
    (c_fn("strpos", col("s"), col("k")), ba.PlanError, "strpos requires Utf8 arguments, not Int64"),
    (c_fn("starts_with", col("s"), lit("x" * 241)), ba.NotImplementedOnGpu, "starts_with with a literal longer than 240 bytes"),
    (c_fn("date_part", col("g"), col("t")), ba.NotImplementedOnGpu, "date_part part must be a non-NULL Utf8 literal"),
    (c_fn("date_part", E.Literal(None, "Utf8"), col("t")), ba.NotImplementedOnGpu, "date_part part must be a non-NULL Utf8 literal"),
    (c_fn("date_part", lit("week"), col("t")), ba.PlanError, "Unsupported date_part part 'week'"),
    (c_fn("date_part", lit("epoch"), col("t")), ba.PlanError, "Unsupported date_part part 'epoch'"),
    (c_fn("date_part", lit("Year"), col("d")), ba.PlanError, "Unsupported date_part part 'Year'"),
    (c_fn("date_part", lit("year"), col("k")), ba.PlanError, "date_part requires a Date32, Date64 or Timestamp argument, not Int64"),
    (c_fn("date_part", lit("year"), col("s")), ba.PlanError, "date_part requires a Date32, Date64 or Timestamp argument, not Utf8"),
    (c_fn("replace", col("s"), col("s"), col("s")), ba.NotImplementedOnGpu, "scalar function 'replace' is not supported"),
    (c_fn("split_part", col("s"), lit("-"), lit(1)), ba.NotImplementedOnGpu, "scalar function 'split_part' is not supported"),
]


@pytest.mark.parametrize("e, error, message", REFUSALS, ids=[f"{e.fun}-{m}" for e, _, m in REFUSALS])
def test_each_refusal_arrives_when_the_plan_is_made(e, error, message):
    with pytest.raises(error, match=message):
        project([(e, "x")])
    with pytest.raises(error, match=message):
        ba.FilterExec(E.IsNotNullExpr(e), leaf())
    with pytest.raises(error, match=message):                       # ... nested in another lowered node and in the VM's part
        project([(E.CaseExpr(None, [(E.IsNullExpr(e), lit(1))], lit(2)), "x")])
