"""CPU tier of CAST to and from Utf8: the one value grammar (ballista_amd/csrc/cast_text.h) against the Python restatement of the
cast table (tests/cast_text_cases.py), and the wire plan that carries such casts.

tests/c/cast_text_check.cpp is a stand-alone program over that header — its own main, no HIP, no GPU — built here with
-fsanitize=address,undefined by the ROCm clang (the compiler `make host-asan` uses).  It reads one case per line and prints NULL,
DECLINED or the value, floats as bit patterns; every line is compared.  The kernels (kernels_cast.hip) and the host's folding of
literals run the same functions, so what holds here holds for them (tests/test_cast_utf8_gpu.py checks that they do)."""
import os
import subprocess

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle.engine import OCol
from tests import cast_text_cases as K, plan_nodes as N, proto_encode as pe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CLANGXX):
        pytest.skip("no ROCm clang for the sanitizer build")
    exe = str(tmp_path_factory.mktemp("cast_text") / "cast_text_check")
    r = subprocess.run([CLANGXX, "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ballista_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "cast_text_check.cpp"), "-o", exe], capture_output=True, text=True)
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


def expected_line(direction, t, arg):
    if direction == "F":
        text = K.format_value(int(arg), t)
        return "NULL" if text is None else text
    v = K.parse(arg, t)
    if v is None:
        return "NULL"
    if v is K.DECLINED:
        return "DECLINED"
    if t == "Float64":
        return "0x%016x" % K.bits(v, t)
    if t == "Float32":
        return "0x%08x" % K.bits(v, t)
    if t == "Boolean":
        return "true" if v else "false"
    return str(int(v))


def test_the_restatement_classifies_the_named_cases_as_the_table_says():
    """the expectations of the lists below come from the restatement: pin the classes the table names, so that a slip in the
    restatement cannot pass as agreement"""
    for s in K.FLOAT_ACCEPTED:
        assert K.parse(s, "Float64") not in (None, K.DECLINED), s
    for s in K.FLOAT_DECLINED:
        assert K.parse(s, "Float64") is K.DECLINED and K.parse(s, "Float32") is K.DECLINED, s
    for s in K.FLOAT_NULL:
        assert K.parse(s, "Float64") is None and K.parse(s, "Float32") is None, s
    for s in K.FLOAT32_DECLINED:
        assert K.parse(s, "Float32") is K.DECLINED, s
    assert K.bits(K.parse("16777218", "Float32"), "Float32") == 0x4B800001 and K.bits(K.parse("1.0000001", "Float32"), "Float32") == 0x3F800001
    assert K.bits(K.parse("-0.0", "Float64"), "Float64") == 1 << 63 and K.bits(K.parse("1e22", "Float64"), "Float64") == 0x4480F0CF064DD592
    assert K.parse("1000000000000000000000", "Float64") == 1e21 and K.parse("0e999999999999", "Float64") == 0.0
    for t, (lo, hi) in K.INT_RANGE.items():
        assert [K.parse(str(v), t) for v in (lo, hi, lo - 1, hi + 1)] == [lo, hi, None, None], t
        assert K.parse("0" * 40 + "7", t) == 7 and K.parse("+7", t) == 7 and K.parse("007", t) == 7
        assert [K.parse(s, t) for s in ("", " 1", "1 ", "1.0", "٣", "12" * 150)] == [None] * 6
        assert K.parse("-0", t) == (None if t.startswith("U") else 0) and K.parse("-1", t) == (None if t.startswith("U") else -1)
    assert [K.parse(s, "Boolean") for s in ("tRuE", "T", "YeS", "y", "oN", "1", "fAlSe", "F", "No", "n", "OfF", "0", "2", "tr")] == [True] * 6 + [False] * 6 + [None] * 2
    assert [K.parse(s, "Date32") for s in ("2000-02-29", "1900-02-29", "0000-01-01", "9999-12-31", "2001-13-01", "2001-1-01", "2001-01-1", "1970-01-01")] == \
        [11016, None, K.DATE_MIN, K.DATE_MAX, None, None, None, 0]
    assert [K.format_value(d, "Date32") for d in (K.DATE_MIN, K.DATE_MAX, K.DATE_MIN - 1, K.DATE_MAX + 1, 0, -1)] == \
        ["0000-01-01", "9999-12-31", None, None, "1970-01-01", "1969-12-31"]
    assert K.format_value(True, "Boolean") == "1" and K.format_value(-128, "Int8") == "-128" and K.format_value(2**64 - 1, "UInt64") == "18446744073709551615"


def test_every_case_of_the_list_through_the_sanitized_program(checker, tmp_path):
    lines = [("P", t, s) for t, s in K.parse_cases()] + [("F", t, str(v)) for t, v in K.format_cases()]
    got = run_checker(checker, tmp_path, lines)
    bad = [(l, g, expected_line(*l)) for l, g in zip(lines, got) if g != expected_line(*l)]
    assert not bad, bad[:10]


def test_random_float_strings_class_and_bits(checker, tmp_path):
    """20 000 strings: repr() of random doubles, %.*f and %.*e with 1-17 digits.  The restatement says accept or decline; the
    program must agree on the class and, where accepted, on every bit — to Float64 and to Float32"""
    strings = K.random_float_strings(20000)
    classes = [K.parse(s, "Float64") for s in strings]
    assert all(c is not None for c in classes)
    share = sum(c is not K.DECLINED for c in classes) / len(classes)
    print(f"accepted share of the random float strings: {share:.3f}")
    assert share >= 0.60, share                    # declines must not hide failures
    assert share <= 0.95, share                    # ... and the decline side is exercised too
    lines = [("P", "Float64", s) for s in strings] + [("P", "Float32", s) for s in strings]
    got = run_checker(checker, tmp_path, lines)
    bad = [(l, g, expected_line(*l)) for l, g in zip(lines, got) if g != expected_line(*l)]
    assert not bad, (len(bad), bad[:10])


def cast_projection_plan():
    b = {"s": OCol("Utf8", ["1"], np.array([True])), "k": OCol("Int64", [1])}
    leaf = N.MemoryExec([[b]])
    leaf.name = "mem://casts"
    exprs = [(E.CastExpr(col("s"), E.INT32), "si"), (E.CastExpr(col("k"), E.UTF8), "ks"), (E.CastExpr(lit("42"), E.INT64), "fortytwo")]
    return N.ProjectionExec(exprs, leaf), exprs


def test_wire_plan_with_utf8_casts_decodes(tmp_path):
    """a CastNode to and from Utf8 is accepted when the plan is decoded, with the types and nullability of the table
    (on the commit before this feature the decode itself raised NotImplementedOnGpu "cast Utf8 -> Int32")"""
    described, _ = cast_projection_plan()
    plan = ba.ExecutionPlan.from_proto(None, pe.plan(described))
    sch = plan.schema()
    assert [(n, t) for n, t, _ in sch] == [("si", "Int32"), ("ks", "Utf8"), ("fortytwo", "Int64")]
    assert sch[0][2] is True                       # a string that is no Int32 is NULL
    assert "CAST(s AS Int32)" in plan.display() and "CAST(k AS Utf8)" in plan.display()
    # what stays out is still refused when the plan is made, not when it runs
    for e, what in [(E.CastExpr(col("s"), E.DATE64), "Date64"), (E.CastExpr(E.CastExpr(col("k"), E.FLOAT64), E.UTF8), "Float64 -> Utf8")]:
        leaf = described.input
        with pytest.raises(ba.NotImplementedOnGpu, match=what):
            ba.ExecutionPlan.from_proto(None, pe.plan(N.ProjectionExec([(e, "x")], leaf)))
