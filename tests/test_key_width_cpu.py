"""CPU tier: "the keys do not fit the 16-byte packed key" is a type, KeyWidthError (host/core.hpp) — what HashAggregateExec and
HashJoinExec answer with their wide-key forms — and only the three places that mean it raise it: ProgramBuilder::add_key (more than 8
key parts), ProgramBuilder::finish (the layout) and check_scan_flags (a Utf8 value longer than its share).  Another BHIP_ENOTIMPL of
the same compiler is a plain Error, and a divide by zero beside a long key value stays the divide by zero.

`make -C ballista_amd/csrc key-width-check` links tests/c/key_width_check.cpp with the -fsanitize=address,undefined objects of the
host sources; the program (its own main, no HIP call, nothing is loaded into Python) prints `ok <case>` per case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ballista_amd", "csrc")
EXE = os.path.join(CSRC, "build_asan", "key_width_check")

CASES = ["eight_int32_keys", "nine_int32_keys", "two_int64_keys", "three_int64_keys_before_finish", "three_int64_keys", "seventeen_accumulators",
         "no_flag", "divide_by_zero", "key_too_long", "both_flags"]


def test_key_width_error_is_raised_by_its_three_origins_only():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang for the sanitizer build")
    r = subprocess.run(["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1)), "key-width-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    assert r.stdout.split("\n") == ["ok " + c for c in CASES] + [""]
