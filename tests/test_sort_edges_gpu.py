"""SortExec on each of its device routes at the inputs and sizes where a route can go wrong without the other tests noticing.

Routes (kernels_sort.hip, ops_sort.cpp): `rowsort` up to 256 rows; the small sort (one LDS rank sort per key image) up to 1024;
`bucket_sort` from 1025 to 2^22 rows under fixed-width keys of at most four words, falling back to the LSD passes when a bin holds
more than 512 rows; the LSD radix passes for everything else, with 4 sub-tiles per workgroup up to 2^21 rows and 16 above.  All of
them must give ONE stable order, and for floats the total order of DESIGN.md "Sort order of floating-point keys".

Expected values come from oracle/plan_eval.py on the same plan (its float order is pinned by test_sort_order_cpu.py against a
third statement); the comparison is bit exact (a NaN's payload and a zero's sign count) and every batch carries its row numbers,
so a swap of two equal keys shows.  The context times every launch: the kernel names say which route ran, and a case that names a
route fails when another one ran."""
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
from test_types_gpu import FIXED

pytestmark = pytest.mark.gpu

PLACEMENTS = [(False, False), (False, True), (True, False), (True, True)]          # (descending, nulls_first)
# launch names that must / must not appear in kernel_stats() on each route ("small" and "lsd" run the same key kernels: the row
# count tells them apart, 1024 being the small sort's last size)
ROUTES = {
    "rowsort": ({"rowsort"}, {"sort_key_fixed", "bucket_sort"}),
    "small": ({"sort_key_fixed"}, {"rowsort", "bucket_sort"}),
    "lsd": ({"sort_key_fixed"}, {"rowsort", "bucket_sort"}),
    "bucket": ({"bucket_sort"}, {"rowsort", "sort_key_fixed"}),
    "bucket_fell_back": ({"bucket_sort", "sort_key_fixed"}, {"rowsort"}),
}


def S(name, desc=False, nulls_first=True):
    return E.PhysicalSortExpr(col(name), descending=desc, nulls_first=nulls_first)


@pytest.fixture(scope="module")
def tctx():
    """a context that times every launch, however small (BHIP_KERNEL_TIMING is read when a context is created)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("BHIP_KERNEL_TIMING", "2")
    try:
        return ba.Context(0)
    finally:
        mp.undo()


def sort_and_check(ctx, m, keys, route):
    plan = ba.SortExec(keys, m)
    ctx.kernel_stats(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    ks = ctx.kernel_stats(reset=True)
    helpers.assert_bit_exact(got, plan_eval.collect(plan))
    present, absent = ROUTES[route]
    assert present <= set(ks) and not (absent & set(ks)), (route, sorted(ks))
    return got


def route_of(n):
    return "rowsort" if n <= 256 else "small" if n <= 1024 else "bucket"


# ---- float specials on every route ---------------------------------------------------------------------------------------------

def special_batch(dtype, n):
    rng = np.random.default_rng(n)
    return OrderedDict([("f", sort_cases.float_special_column(dtype, n, rng)), ("t", OCol("Int32", rng.integers(0, 4, n))),
                        ("s", OCol("Utf8", [f"v{v}" for v in rng.integers(0, 3, n)])), ("row", OCol("Int64", np.arange(n)))])


@pytest.mark.parametrize("n", [40, 256, 257, 1024, 1025, 3000])
@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_float_specials(tctx, dtype, n):
    """signed NaNs with payloads, infinities, the largest and smallest normals, subnormals and both zeros, each twice, with NULLs
    (whose stored values differ): the last size of rowsort, the first and last of the small sort, the first of the bucket path.  The
    fillers are spread over the octaves, so no bucket bin comes near its limit: from 1025 rows the bucket path must not fall back."""
    m = helpers.memory_exec(tctx, [[special_batch(dtype, n)]])
    for desc, nf in PLACEMENTS:
        sort_and_check(tctx, m, [S("f", desc, nf)], route_of(n))
        sort_and_check(tctx, m, [S("f", desc, nf), S("t", desc=True)], route_of(n))


@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_float_specials_lsd(tctx, dtype):
    """a trailing Utf8 key keeps the list off the bucket path: the float key goes through the LSD radix passes"""
    m = helpers.memory_exec(tctx, [[special_batch(dtype, 3000)]])
    for desc, nf in PLACEMENTS:
        sort_and_check(tctx, m, [S("f", desc, nf), S("s")], "lsd")


# ---- integer and temporal extremes on the small sort and the LSD passes ------------------------------------------------------------

def extremes_batch(dtype, n):
    rng = np.random.default_rng(n)
    nt = og.NP_TYPES[dtype]
    if dtype in og.FLOAT_TYPES:
        info = np.finfo(nt)
        v = rng.normal(0, 1e3, n).astype(nt)
    else:
        info = np.iinfo(nt)
        v = rng.integers(info.min, info.max, n, dtype=np.int64 if info.min < 0 else np.uint64, endpoint=True).astype(nt)
    edge = np.array([info.min, info.max, 0, -1 if info.min < 0 else info.max - 1], dtype=nt)
    v[rng.choice(n, 8, replace=False)] = np.concatenate([edge, edge])
    return OrderedDict([("k", OCol(dtype, v, rng.random(n) > 0.1)), ("s", OCol("Utf8", [f"v{x}" for x in rng.integers(0, 3, n)])),
                        ("row", OCol("Int64", np.arange(n)))])


@pytest.mark.parametrize("dtype", FIXED)
def test_extremes_off_the_rowsort_and_bucket_routes(tctx, dtype):
    """the type's minimum, maximum, 0 and -1 (twice each, NULLs beside them) as a key of 600 rows (the small sort) and, in front of a
    Utf8 key, of 3000 rows (the LSD passes); test_types_gpu.py sorts the same types at 200 and 3000 rows: rowsort and the bucket path"""
    small = helpers.memory_exec(tctx, [[extremes_batch(dtype, 600)]])
    lsd = helpers.memory_exec(tctx, [[extremes_batch(dtype, 3000)]])
    for desc in (False, True):
        sort_and_check(tctx, small, [S("k", desc, not desc)], "small")
        sort_and_check(tctx, lsd, [S("k", desc, not desc), S("s")], "lsd")


# ---- the bucket path's bin limit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("copies", [511, 512])
def test_bucket_bin_limit(tctx, copies):
    """keys j << 40 for j < 4488 plus `copies` more of 17 << 40: 4999 or 5000 rows, so the split digit is the 13 differing bits and
    equals j.  Bin 17 holds 512 rows (the most a bin may: ranked inside the bucket path) or 513 (the sort falls back to the LSD
    passes); either way the equal keys come out in row order."""
    rng = np.random.default_rng(copies)
    k = np.concatenate([np.arange(4488, dtype=np.int64), np.full(copies, 17, np.int64)]) << 40
    k = k[rng.permutation(len(k))]
    b = OrderedDict([("k", OCol("Int64", k)), ("row", OCol("Int64", np.arange(len(k))))])
    m = helpers.memory_exec(tctx, [[b]])
    for desc in (False, True):
        got = sort_and_check(tctx, m, [S("k", desc)], "bucket" if copies == 511 else "bucket_fell_back")
        rows = got["row"].values[got["k"].values == 17 << 40]
        assert len(rows) == copies + 1 and np.all(rows[1:] > rows[:-1])
        assert np.array_equal(rows, np.nonzero(k == 17 << 40)[0])


# ---- a split digit that draws on three and four key words ------------------------------------------------------------------------------

@pytest.mark.parametrize("nullable", [False, True])
def test_bucket_digit_across_words(tctx, nullable):
    """5000 rows, keys (Int32 of 2 values, Int32 of 4 values DESC, Float64): the 13-bit digit takes one bit of the first word, two of
    the second and the rest from the third; with a nullable first key its NULL rank is one more word in front"""
    n = 5000
    rng = np.random.default_rng(5 + nullable)
    b = OrderedDict([("a", OCol("Int32", rng.integers(0, 2, n), (rng.random(n) > 0.05) if nullable else None)),
                     ("t", OCol("Int32", rng.integers(0, 4, n))), ("u", OCol("Float64", rng.random(n))),
                     ("row", OCol("Int64", np.arange(n)))])
    m = helpers.memory_exec(tctx, [[b]])
    for nf in (True, False):
        sort_and_check(tctx, m, [S("a", nulls_first=nf), S("t", desc=True), S("u")], "bucket")


# ---- the sizes at which the large routes switch ------------------------------------------------------------------------------------

def large_batch(n):
    rng = np.random.default_rng(n % 1000)
    return OrderedDict([("f", sort_cases.float_special_column("Float64", n, rng)),
                        ("d", OCol("Date32", rng.integers(8000, 10400, n), rng.random(n) > 0.02)),
                        ("t", OCol("Int32", rng.integers(0, 4, n), rng.random(n) > 0.02)),
                        ("e", OCol("Int32", rng.integers(0, 2**31, n))),
                        ("row", OCol("Int64", np.arange(n)))])


@pytest.mark.parametrize("n", [1 << 21, (1 << 21) + 1, 1 << 22, (1 << 22) + 1])
def test_large_route_limits(tctx, n):
    """2^21 is the last size of the radix passes with 4 sub-tiles per workgroup and 2^21 + 1 the first with 16 (one row in the
    last workgroup): three nullable keys are six words, more than the bucket path takes.  2^22 is the bucket path's last size (2^20
    bins) and 2^22 + 1 goes to the 16-sub-tile passes whatever the keys.  BHIP_SORT_ITEMS and BHIP_NO_BUCKET_SORT are read once per
    process, so these are the smallest sizes at which the switches show; most of a case's time is the numpy reference."""
    m = helpers.memory_exec(tctx, [[large_batch(n)]])
    if n <= (1 << 21) + 1:
        sort_and_check(tctx, m, [S("t", True, False), S("f", nulls_first=True), S("d", True, True)], "lsd")
        return
    # the Q3 shape.  The NULL rows of `f` share one bin (200 K rows), so at 2^22 the bucket path runs all its kernels over 2^20 bins and
    # hands over to the LSD passes; (e, row DESC) without NULLs has about four rows per bin and stays on the bucket path
    # (e >= 0: an Int32's image is sign-extended, so under both signs the 20 leading differing bits all repeat the sign: two bins)
    sort_and_check(tctx, m, [S("f", True, False), S("d")], "bucket_fell_back" if n == 1 << 22 else "lsd")
    if n == 1 << 22:
        sort_and_check(tctx, m, [S("e"), S("row", desc=True)], "bucket")
