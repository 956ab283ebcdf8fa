"""CPU tier: the host half of ParquetExec (host/parquet_host.cpp: footer, page headers, Snappy, levels, run tables, string walks,
stage_chunk) against pyarrow, on the files of tests/parquet_files.py — pages that end inside a validity word, one-row and
all-NULL pages, REQUIRED fields, a 0-entry dictionary, index widths up to 32 bits, the legacy PLAIN_DICTIONARY id, hand-written
run mixes and clipped runs, uncompressed V2 pages in a Snappy chunk, bit-packed definition levels.

`make -C ballista_amd/csrc parquet-check` links tests/c/parquet_decode_check.cpp with the -fsanitize=address,undefined objects
of the host sources; the program (its own main, nothing is loaded into Python) finishes parse_chunk's output in plain
sequential C++ and prints every value.  The whole text must equal pyarrow's read of the same files, with the chunks staged
(BHIP_PARQUET_PER_PAGE unset) and as page lists (BHIP_PARQUET_PER_PAGE=1): the two forms the device half is handed."""
import os
import subprocess

import pytest

import parquet_files as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ballista_amd", "csrc")
EXE = os.path.join(CSRC, "build_asan", "parquet_decode_check")


@pytest.fixture(scope="module")
def program():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang for the sanitizer build")
    r = subprocess.run(["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1)), "parquet-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EXE


def first_difference(got, want):
    g, w = got.split("\n"), want.split("\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            head = next((x for x in reversed(w[:i + 1]) if x.startswith("#")), "")
            return f"line {i}: got {a!r}, pyarrow has {b!r} ({head})"
    return f"{len(g)} lines, pyarrow has {len(w)}"


@pytest.mark.parametrize("per_page", ["", "1"], ids=["staged", "per_page"])
@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_host_decode_equals_pyarrow(program, tmp_path, case, per_page):
    _, write, _ = case
    paths = write(str(tmp_path))                                  # asserts the case's structural precondition
    want = P.canonical_text(paths)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("BHIP_PARQUET_PER_PAGE", None)
    if per_page:
        env["BHIP_PARQUET_PER_PAGE"] = per_page
    r = subprocess.run([program] + paths, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    assert r.stdout == want, first_difference(r.stdout, want)
