"""TEST INFRASTRUCTURE shared by test_distinct_agg_cases_cpu.py (no GPU) and test_distinct_agg_gpu.py: the inputs of the tests of
HashAggregateExec's Single mode with COUNT / SUM / AVG (DISTINCT x) (host/ops_agg_wide.cpp run_single, kernels_hash.hip
distinct_claim_kernel / distinct_mark_kernel) and a statement of what they compute, in plain Python from the definition
(DESIGN.md §3.4): per group, the SET of (type, bits or bytes) of the non-NULL values of x.

Nothing here touches a device.  A case is (name, table, group expressions, aggregates, facts); `facts` holds what the case claims of
itself and test_distinct_agg_cases_cpu.py proves each claim.  `expected(case)` is the answer; `expected(case, mistake=...)` is the
answer of an implementation that makes one of MISTAKES — a case discriminates when a mistake changes one of its numbers.

Floats are written by their BIT PATTERN, so that a NaN's payload and a zero's sign arrive as written.  The NaNs are quiet ones: the
device compares a Float32 by the bits of the double it equals, and that widening is one-to-one on everything but signalling NaNs."""
import functools
from collections import OrderedDict, namedtuple

import numpy as np

from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle import engine as og
from oracle.engine import OCol

import wide_agg_cases as W

Case = namedtuple("Case", "name table group aggs facts")
column = W.column
LONG = W.LONG                                              # 40 bytes: no share of the packed key holds it
DISTINCT_FUNS = ("COUNT_DISTINCT", "SUM_DISTINCT", "AVG_DISTINCT")
MISTAKES = ("null_is_a_value", "zeros_merged", "nans_merged", "empty_is_null", "prefix_is_equal", "group_key_ignored")


def keys_of(case):
    return [n for _, n in case.group]


def group_by(*names):
    return [(col(n), n) for n in names]


# ---- the definition ----------------------------------------------------------------------------------------------------------------------

def identities(c):
    """per row None for a NULL, else (type, bits or bytes): two rows hold the same value exactly when these are equal"""
    ok = c.is_valid().tolist()
    if c.dtype == "Utf8":
        vals = [s.encode("utf-8") for s in c.values]
    elif c.dtype == "Boolean":
        vals = [bool(v) for v in c.values]
    else:
        bits = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[c.values.dtype.itemsize]
        vals = np.ascontiguousarray(c.values).view(bits).tolist()
    return [(c.dtype, v) if o else None for v, o in zip(vals, ok)]


def _mistaken(ident, c, mistake):
    """the identities an implementation with `mistake` would compare"""
    if mistake == "null_is_a_value":
        return [(c.dtype, "NULL") if i is None else i for i in ident]
    if mistake == "empty_is_null" and c.dtype == "Utf8":
        return [None if i is not None and i[1] == b"" else i for i in ident]
    if mistake in ("zeros_merged", "nans_merged") and c.dtype in og.FLOAT_TYPES:
        out = []
        for i, v in zip(ident, c.values.tolist()):
            if i is not None and mistake == "zeros_merged" and v == 0:
                i = (c.dtype, 0)
            if i is not None and mistake == "nans_merged" and v != v:
                i = (c.dtype, "NaN")
            out.append(i)
        return out
    return ident


def _same(a, b, mistake):
    if mistake == "prefix_is_equal" and isinstance(a[-1], bytes):
        return a[:-1] == b[:-1] and (a[-1].startswith(b[-1]) or b[-1].startswith(a[-1]))
    return a == b


def first_rows(table, keys, x, mistake=None):
    """-> (group id per row, number of groups, per row: x is non-NULL and no earlier row of the group holds the same value).  The
    walk is in row order, so the survivor of equal rows is the one with the smallest row number"""
    n = og.batch_len(table)
    kcells = [identities(table[k]) for k in keys]
    xi = _mistaken(identities(table[x]), table[x], mistake)
    gid, groups, first = [], {}, np.zeros(n, np.bool_)
    seen_sets, seen_lists = {}, {}
    for r in range(n):
        g = groups.setdefault(tuple(kc[r] for kc in kcells), len(groups))
        gid.append(g)
        if xi[r] is None:
            continue
        scope = 0 if mistake == "group_key_ignored" else g
        if mistake == "prefix_is_equal":
            members = seen_lists.setdefault(scope, [])
            if not any(_same(m, xi[r], mistake) for m in members):
                members.append(xi[r])
                first[r] = True
        else:
            members = seen_sets.setdefault(scope, set())
            if xi[r] not in members:
                members.add(xi[r])
                first[r] = True
    return np.array(gid, np.int64), len(groups), first


def expected_table(table, group, aggs, mistake=None):
    """the output of the Single aggregate: the groups in order of first appearance; the key columns, then one column per DISTINCT
    aggregate (others are not computed here: the tests compare them with Final over Partial).  SUM_DISTINCT adds the survivors in row
    order (integers: exact; floats: the tests use values whose sums are exact, or compare within a stated tolerance)"""
    keys = [n for _, n in group]
    n = og.batch_len(table)
    out = OrderedDict()
    cache = {}
    for a in aggs:
        if a.fun not in DISTINCT_FUNS:
            continue
        assert isinstance(a.expr, E.Column), "the cases take DISTINCT over plain columns"
        x = a.expr.name
        if x not in cache:
            cache[x] = first_rows(table, keys, x, mistake)
        gid, ng, first = cache[x]
        if not keys:
            ng = 1                                          # no GROUP BY: one row, on empty input too
            gid = np.zeros(n, np.int64)
        if not out:
            head = [int(np.nonzero(gid == g)[0][0]) for g in range(ng)] if keys else []
            for k in keys:
                out[k] = table[k].take(np.array(head, np.int64))
        count = np.bincount(gid[first], minlength=ng).astype(np.uint64)
        c = table[x]
        if a.fun == "COUNT_DISTINCT":
            out[a.name] = OCol("UInt64", count)
            continue
        is_float = c.dtype in og.FLOAT_TYPES
        sums = np.zeros(ng, np.float64 if is_float or a.fun == "AVG_DISTINCT" else np.uint64 if c.dtype in og.UNSIGNED_TYPES else np.int64)
        for r in np.nonzero(first)[0]:
            sums[gid[r]] += c.values[r]
        if a.fun == "SUM_DISTINCT":
            out[a.name] = OCol("Float64" if is_float else "UInt64" if c.dtype in og.UNSIGNED_TYPES else "Int64", sums, count > 0)
        else:
            out[a.name] = OCol("Float64", sums / np.maximum(count, 1), count > 0)
    return out


def expected(case, mistake=None):
    return expected_table(case.table, case.group, case.aggs, mistake)


def numbers(batch, names):
    """the DISTINCT results as comparable rows (NULL = None)"""
    return sorted(zip(*[batch[n].to_pylist() for n in names]), key=repr)


def two_level(m, keys, x, name):
    """the rewrite a caller could do by hand, from the operators that know no DISTINCT: GROUP BY keys, x; then COUNT(x) GROUP BY keys.
    Its output is the Single aggregate's for one COUNT_DISTINCT(x)"""
    import ballista_amd as ba
    g1 = group_by(*keys, x)
    p1 = ba.HashAggregateExec(ba.plan.PARTIAL, g1, [E.Count(col(x), "__n")], m)
    f1 = ba.HashAggregateExec(ba.plan.FINAL, g1, [E.AggregateExpr("COUNT", col("__n[count]"), "__n")], ba.MergeExec(p1))
    g2 = group_by(*keys)
    p2 = ba.HashAggregateExec(ba.plan.PARTIAL, g2, [E.Count(col(x), name)], f1)
    return ba.HashAggregateExec(ba.plan.FINAL, g2, [E.AggregateExpr("COUNT", col(name + "[count]"), name)], ba.MergeExec(p2))


# ---- A. ballot words and blocks ------------------------------------------------------------------------------------------------------------

BALLOT_SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257]     # one validity word = 64 rows, one block = 256
BALLOT_VARIANTS = ("last_is_duplicate", "last_is_first")


@functools.lru_cache(maxsize=None)
def ballot_case(n, variant):
    """rows 2j-1 and 2j hold the same (k, x): every pair (63, 64), (127, 128), (255, 256) straddles a word or block edge.  The last row
    repeats row 0 in one variant and holds a value of its own in the other (n = 1: it is the only row either way)"""
    rn = np.arange(n, dtype=np.int64)
    pair = (rn + 1) // 2
    k, x = (pair % 3).astype(np.int32), pair * 10
    x_valid = pair % 7 != 5                                # some pairs NULL: two rows of zero bits across an edge
    if variant == "last_is_duplicate":
        k[n - 1], x[n - 1], x_valid[n - 1] = k[0], x[0], x_valid[0]
    else:
        k[n - 1], x[n - 1], x_valid[n - 1] = 1, 10 ** 9, True
    t = OrderedDict([("k", OCol("Int32", k)), ("x", OCol("Int64", x, x_valid))])
    aggs = [E.CountDistinct(col("x"), "cd"), E.SumDistinct(col("x"), "sd")]
    return Case(f"ballot_{n}_{variant}", t, group_by("k"), aggs, {"rows": n, "last_is_first": variant == "last_is_first" or n == 1,
                                                                  "straddling": [(e - 1, e) for e in (64, 128, 256) if e < n]})


# ---- B. table size -----------------------------------------------------------------------------------------------------------------------------

TABLE_SIZES = [512, 513]                                   # table_capacity: 1024 slots hold 512 rows, 513 take 2048
TABLE_SHAPES = ("all_distinct", "all_equal")


@functools.lru_cache(maxsize=None)
def table_case(n, shape):
    rn = np.arange(n, dtype=np.int64)
    x = rn * 3 - 700 if shape == "all_distinct" else np.full(n, 42, np.int64)
    t = OrderedDict([("k", OCol("Int32", np.zeros(n, np.int32))), ("x", OCol("Int64", x))])
    return Case(f"table_{n}_{shape}", t, group_by("k"), [E.CountDistinct(col("x"), "cd"), E.SumDistinct(col("x"), "sd")],
                {"rows": n, "distinct": n if shape == "all_distinct" else 1})


# ---- C. equality, type by type -------------------------------------------------------------------------------------------------------------

F64 = {"zero": 0x0000000000000000, "neg_zero": 0x8000000000000000, "one": 0x3FF0000000000000, "one_ulp": 0x3FF0000000000001,
       "neg_one": 0xBFF0000000000000, "nan_a": 0x7FF8000000000001, "nan_b": 0x7FF8000000000002}
F32 = {"zero": 0x00000000, "neg_zero": 0x80000000, "one": 0x3F800000, "one_ulp": 0x3F800001, "neg_one": 0xBF800000,
       "nan_a": 0x7FC00001, "nan_b": 0x7FC00002}
INT_VALUES = [0, 1, -1, 2, 3, -2]                          # lowest bit: 0 / 1, 2 / 3; sign: 1 / -1, 2 / -2
EQUALITY_VALUES = {
    "Int32": INT_VALUES + [2 ** 31 - 1, -2 ** 31],
    "Int64": INT_VALUES + [2 ** 63 - 1, -2 ** 63, 2 ** 32, 2 ** 32 + 1],      # (a difference above bit 31 too)
    "Date32": INT_VALUES + [2 ** 31 - 1, -2 ** 31],
    "Float32": list(F32.values()),
    "Float64": list(F64.values()),
    "Boolean": [True, False],
    "Utf8": ["", "a", "ab", LONG, LONG[:-1] + "!", LONG[:-1]],                    # "", a prefix, 40 bytes differing in the last
}


@functools.lru_cache(maxsize=None)
def equality_case(dtype):
    """group 0: every value twice (true duplicates, apart) with NULLs between; group 1: every second value once.  All of them are
    different values, so COUNT_DISTINCT is their number"""
    vals = EQUALITY_VALUES[dtype]
    x = vals + [None] + list(reversed(vals)) + [None] + vals[::2]
    k = [0] * (2 * len(vals) + 2) + [1] * len(vals[::2])
    t = OrderedDict([("k", OCol("Int32", np.array(k, np.int32))), ("x", column(dtype, x))])
    return Case(f"equality_{dtype}", t, group_by("k"), [E.CountDistinct(col("x"), "cd")],
                {"counts": {0: len(vals), 1: len(vals[::2])}, "rows": len(x)})


# ---- D. the group key in the comparison ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def group_key_case(route):
    """the same x in several groups counts in each; the NULL group key is one group.  packed: a short integer key; wide: a Utf8 key too
    long for the packed key, so that the inner aggregate takes the wide-key route"""
    gk = [0, 1, None, 0, 1, None, 2, None, 2, 0]
    x = [7, 7, 7, 7, 8, 9, 7, 7, None, 8]
    if route == "packed":
        kc = column("Int32", gk)
    else:
        kc = column("Utf8", [None if g is None else LONG + str(g) for g in gk])
    t = OrderedDict([("k", kc), ("x", column("Int64", x))])
    return Case(f"group_key_{route}", t, group_by("k"), [E.CountDistinct(col("x"), "cd"), E.SumDistinct(col("x"), "sd")],
                {"wide": route == "wide", "counts": {0: 2, 1: 2, None: 2, 2: 1}, "rows": len(x)})


# ---- E. NULL arguments -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def null_case(shape):
    if shape == "some":
        k = [0, 0, 0, 1, 1, 1, 1, 2]
        x = [None, None, None, None, 5, None, 5, 6]         # group 0: only NULLs; group 1: one value and NULLs
    else:
        k = [0, 1, 0, 1, 2] * 30                          # 150 rows: more than two validity words of NULLs
        x = [None] * 150
    t = OrderedDict([("k", OCol("Int32", np.array(k, np.int32))), ("x", column("Int64", x))])
    aggs = [E.CountDistinct(col("x"), "cd"), E.SumDistinct(col("x"), "sd"), E.AvgDistinct(col("x"), "ad")]
    return Case(f"nulls_{shape}", t, group_by("k"), aggs, {"rows": len(x), "all_null": shape == "all"})


# ---- F. several aggregates ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mixed_case():
    n = 300
    rn = np.arange(n, dtype=np.int64)
    t = OrderedDict([("k", OCol("Int32", (rn % 5).astype(np.int32))),
                     ("a", OCol("Int64", ((rn // 5) ** 2 + (rn % 5) * 3) % 29 - 9, rn % 9 != 4)),
                     ("b", column("Utf8", [None if i % 11 == 3 else "s" * (i % 4) + str(i % 6) for i in range(n)])),
                     ("y", OCol("Int64", rn * 13 - 1000, rn % 6 != 1))])
    aggs = [E.CountDistinct(col("a"), "cd_a"), E.CountDistinct(col("b"), "cd_b"), E.SumDistinct(col("a"), "sd_a"), E.AvgDistinct(col("a"), "ad_a"),
            E.Sum(col("y"), "sum_y"), E.Count(col("y"), "count_y"), E.Min(col("y"), "min_y")]
    return Case("mixed", t, group_by("k"), aggs, {"rows": n, "distinct_args": 2})


# ---- G. no GROUP BY ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def no_group_case(n):
    rn = np.arange(n, dtype=np.int64)
    t = OrderedDict([("x", OCol("Int64", rn % 17, rn % 4 != 2 if n else None))])
    return Case(f"no_group_{n}", t, [], [E.CountDistinct(col("x"), "cd"), E.SumDistinct(col("x"), "sd"), E.AvgDistinct(col("x"), "ad")], {"rows": n})


# ---- H. more rows than one trip of the grid ----------------------------------------------------------------------------------------------------

GRID_ROWS = 1_200_000
GRID_LIMIT = 256 * 16 * 256                                # CUs x blocks per CU x threads: one trip of the kernels' row loops


@functools.lru_cache(maxsize=None)
def grid_case():
    rng = np.random.default_rng(20)
    t = OrderedDict([("k", OCol("Int32", rng.integers(0, 1000, GRID_ROWS).astype(np.int32))),
                     ("x", OCol("Int64", rng.integers(0, 5000, GRID_ROWS)))])
    return Case("grid", t, group_by("k"), [E.CountDistinct(col("x"), "cd"), E.SumDistinct(col("x"), "sd")], {"rows": GRID_ROWS})


def grid_expected():
    """the definition on integers without NULLs, by numpy: the distinct (k, x) pairs"""
    c = grid_case()
    k, x = c.table["k"].values.astype(np.int64), c.table["x"].values
    pairs = np.unique(k * 5000 + x)
    pk, px = pairs // 5000, pairs % 5000
    ks = np.unique(pk)
    return OrderedDict([("k", OCol("Int32", ks.astype(np.int32))), ("cd", OCol("UInt64", np.bincount(pk, minlength=1000)[ks].astype(np.uint64))),
                        ("sd", OCol("Int64", np.bincount(pk, weights=px, minlength=1000)[ks].astype(np.int64)))])


# ---- I. float sums ----------------------------------------------------------------------------------------------------------------------------

FLOAT_ROWS = 20_000


@functools.lru_cache(maxsize=None)
def float_sum_case():
    """multiples of 0.1 (their sum depends on the order of the additions), every value 2 to 5 times at scattered rows, 8 groups"""
    rng = np.random.default_rng(7)
    vals, reps = [], []
    v = 0
    while sum(reps) < FLOAT_ROWS:
        vals.append(v)
        reps.append(min(int(rng.integers(2, 6)), FLOAT_ROWS - sum(reps)))
        v += 1
    if reps[-1] < 2:                                       # the last value must occur twice as well: take a row from a value with 3 or more
        reps[next(i for i, r in enumerate(reps) if r >= 3)] -= 1
        reps[-1] += 1
    ids = np.repeat(np.array(vals, np.int64), reps)
    rng.shuffle(ids)
    t = OrderedDict([("k", OCol("Int32", (ids % 8).astype(np.int32))), ("x", OCol("Float64", ids * 0.1))])
    return Case("float_sum", t, group_by("k"), [E.SumDistinct(col("x"), "sd"), E.CountDistinct(col("x"), "cd")],
                {"rows": FLOAT_ROWS, "min_reps": min(reps), "max_reps": max(reps)})


# ---- J. the property: COUNT_DISTINCT(x) GROUP BY k = the rows of GROUP BY k, x with a non-NULL x, per k ----------------------------------------

PROPERTY_ROWS = 5000


@functools.lru_cache(maxsize=None)
def property_table():
    rng = np.random.default_rng(99)
    n = PROPERTY_ROWS
    ki = rng.integers(0, 40, n)
    t = OrderedDict([("k_packed", OCol("Int32", ki.astype(np.int32), rng.random(n) > 0.05)),
                     ("k_wide", column("Utf8", [None if r < 0.05 else LONG + str(v) for v, r in zip(ki.tolist(), rng.random(n).tolist())])),
                     ("x_i64", OCol("Int64", rng.integers(-30, 30, n), rng.random(n) > 0.1)),
                     ("x_f64", OCol("Float64", rng.integers(-8, 8, n) / 8.0, rng.random(n) > 0.1)),
                     ("x_utf8", column("Utf8", [None if r < 0.1 else "v" * (v % 5) + str(v % 7) for v, r in zip(rng.integers(0, 50, n).tolist(), rng.random(n).tolist())])),
                     ("x_bool", OCol("Boolean", rng.random(n) > 0.5, rng.random(n) > 0.3)),
                     ("x_date", OCol("Date32", rng.integers(0, 20, n).astype(np.int32), rng.random(n) > 0.1))])
    return t


PROPERTY_X = ["x_i64", "x_f64", "x_utf8", "x_bool", "x_date"]
