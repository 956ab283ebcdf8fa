"""Inputs shared by the fast-path edge tests (test_fastpath_edge_cases_cpu.py checks the tables themselves on the CPU,
test_fastpath_edges_gpu.py runs them through every device route).

host/sop.cpp re-derives expression semantics outside the expression VM: an AND of `column <op> literal` comparisons becomes one
closed [lo, hi] range per column (strict bounds move to the neighbouring double, or by 1 for Int32 / Date32), and SUM arguments
become chain steps f = sgn * x + add; t = t_prev * f.  The tables here put rows AT those bounds and operands at the edges of the
double format, built so that every expected result is exact:

* predicate cases: a column that holds the literal L, both neighbours, -L, both zeros, both smallest subnormals, both infinities,
  three NaN bit patterns and ordinary values; the special values sit at the rows where the kernels' row mappings change (BOUNDARY)
  and at random rows in between;
* conjunction cases: several comparisons on one column and on up to five columns, with and without NULLs;
* chain cases: every group has ONE designated row whose product may be non-zero; every other row of the group either fails the
  predicate or has finite factors and an exact +-0.0 product.  The group's SUM is then that one product bit for bit in any order
  of addition (x + 0.0 == x for every non-zero or NaN x); only where the product itself is +-0.0 is the sign of the sum open.
  chain_expected() asserts this in plain Python floats for every case it is asked about.

`fold` restates which predicates build_sop folds into ranges (the others run on the expression VM): the expected route of a
case, never its expected rows — those come from the oracle, and in the CPU test from a row-by-row comparison in Python."""
import math
import sys
from collections import OrderedDict

import numpy as np

from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle.engine import OCol

INF = math.inf
DBL_MAX = sys.float_info.max
DBL_MIN = 2.2250738585072014e-308           # the smallest normal double
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NAN_BITS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123)
OPS = ("Eq", "Lt", "LtEq", "Gt", "GtEq")
F64_LITERALS = (0.0, -0.0, 5e-324, -5e-324, DBL_MIN, 0.1, 1.0, DBL_MAX, -DBL_MAX, INF, -INF)
I32_LITERALS = (INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX)
# rows at which a kernel's mapping changes: the row pair of a lane, the 64-row ballot word, the 512-row sub-tile, the 1024-row
# tile, the pack of four tiles; the last row is added per size
BOUNDARY = (0, 1, 63, 64, 511, 512, 1023, 1024, 4095, 4096)


def boundary_rows(n):
    return sorted({i for i in BOUNDARY if i < n} | {n - 1})


def f64(bits):
    return float(np.array([bits], np.uint64).view(np.float64)[0])


def bits_of(v):
    return int(np.array([v], np.float64).view(np.uint64)[0])


def next_up(v):
    return math.nextafter(v, INF)


def next_down(v):
    return math.nextafter(v, -INF)


def compare(op, a, b):
    """`a <op> b` over Python floats or ints (a NaN fails everything)"""
    return {"Eq": a == b, "Lt": a < b, "LtEq": a <= b, "Gt": a > b, "GtEq": a >= b}[op]


# ---- predicates as terms: (column, op, literal value, literal on the left) ------------------------------------------------------

def literal_expr(value, dtype):
    return E.Literal(value, dtype)


def term_expr(term, schema):
    name, op, value, lit_left = term
    l, r = col(name), literal_expr(value, schema[name])
    return E.BinaryExpr(r, op, l) if lit_left else E.BinaryExpr(l, op, r)


def conj_expr(terms, schema):
    e = term_expr(terms[0], schema)
    for t in terms[1:]:
        e = e.and_(term_expr(t, schema))
    return e


def twice(p):
    """`p OR p`: the truth table of p (Kleene: NULL OR NULL is NULL, dropped like NULL), but no AND of comparisons any more"""
    return E.BinaryExpr(p, "Or", p)


def term_holds(term, value):
    """the term over one valid Python value"""
    _, op, literal, lit_left = term
    return compare(op, literal, value) if lit_left else compare(op, value, literal)


FLIPPED = {"Eq": "Eq", "Lt": "Gt", "LtEq": "GtEq", "Gt": "Lt", "GtEq": "LtEq"}


def fold(terms, schema):
    """the ranges build_sop folds the AND of `terms` into, column -> (lo, hi) as doubles, or None where it declines and the
    expression VM runs the predicate: a NaN literal, an empty range (x > +inf, x < -inf, an empty intersection), more than four
    columns"""
    ranges = OrderedDict()
    for name, op, value, lit_left in terms:
        if lit_left:
            op = FLIPPED[op]
        is_int = schema[name] in ("Int32", "Date32")
        v = float(value)
        if v != v:
            return None
        lo, hi = -INF, INF
        if op == "Eq":
            lo = hi = v
        elif op == "Lt":
            hi = v - 1.0 if is_int else next_down(v)
        elif op == "LtEq":
            hi = v
        elif op == "Gt":
            lo = v + 1.0 if is_int else next_up(v)
        else:
            lo = v
        if not is_int and ((op == "Lt" and v == -INF) or (op == "Gt" and v == INF)):
            lo, hi = INF, -INF
        if name in ranges:
            lo, hi = max(lo, ranges[name][0]), min(hi, ranges[name][1])
        elif len(ranges) == 4:
            return None
        ranges[name] = (lo, hi)
    if any(lo > hi for lo, hi in ranges.values()):
        return None
    return ranges


# ---- one-comparison predicate cases ---------------------------------------------------------------------------------------------

def float_specials(L):
    """what a Float64 predicate column holds for the literal L, as bit patterns; the first eleven go to the BOUNDARY rows"""
    b = bits_of
    return np.array([b(L), b(next_up(L)), b(next_down(L)), b(-L), NAN_BITS[0], b(0.0), b(-0.0), b(INF), b(-INF), b(5e-324), b(-5e-324),
                     NAN_BITS[1], NAN_BITS[2], b(0.1), b(1.0), b(-1.0), b(123.456), b(-DBL_MAX), b(DBL_MAX)], np.uint64)


def int_specials(L):
    return np.array([v for v in (L, L - 1, L + 1, INT32_MIN, INT32_MAX, 0, -1, 1, 7) if INT32_MIN <= v <= INT32_MAX], np.int64)


def _sprinkle(n, specials, ordinary, rng, shift):
    """n values: half ordinary, half drawn from `specials`, and the specials in turn at the boundary rows"""
    out = np.where(rng.random(n) < 0.5, rng.choice(specials, n), ordinary)
    for j, row in enumerate(boundary_rows(n)):
        out[row] = specials[(j + shift) % len(specials)]
    return out


def float_pred_batch(L, n, shift=0, seed=0):
    """(id, x): x as described in the module docstring for the literal L; shift rotates which special sits at which boundary row
    (0: L itself at row 0)"""
    rng = np.random.default_rng(1000 + seed + n)
    ordinary = (rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-30, 30, n))).view(np.uint64)
    bits = _sprinkle(n, float_specials(L), ordinary, rng, shift).astype(np.uint64)
    return OrderedDict([("id", OCol("Int32", np.arange(n, dtype=np.int32))), ("x", OCol("Float64", bits.view(np.float64)))])


def int_pred_batch(dtype, L, n, shift=0, seed=0, nulls=False):
    """(id, x): an Int32 / Date32 column with rows at L and L +- 1 (where that does not wrap) and at both extremes"""
    rng = np.random.default_rng(2000 + seed + n)
    ordinary = np.where(rng.random(n) < 0.5, rng.integers(-1000, 1000, n), rng.integers(INT32_MIN, INT32_MAX, n, endpoint=True))
    vals = _sprinkle(n, int_specials(L), ordinary, rng, shift).astype(np.int32)
    valid = rng.random(n) > 0.2 if nulls and n > 1 else None
    return OrderedDict([("id", OCol("Int32", np.arange(n, dtype=np.int32))), ("x", OCol(dtype, vals, valid))])


PRED_SCHEMA = {"Float64": {"id": "Int32", "x": "Float64"}, "Int32": {"id": "Int32", "x": "Int32"}, "Date32": {"id": "Int32", "x": "Date32"}}


def single_terms(L):
    """every operator with the literal on the right and on the left"""
    return [("x", op, L, left) for op in OPS for left in (False, True)]


def kept_rows(batch, terms):
    """the row numbers a filter on the AND of `terms` keeps, row by row in plain Python: every term TRUE over a valid value"""
    n = len(next(iter(batch.values())))
    cols = {name: batch[name].to_pylist() for name in {t[0] for t in terms}}
    return [i for i in range(n) if all(cols[t[0]][i] is not None and term_holds(t, cols[t[0]][i]) for t in terms)]


# ---- conjunctions ---------------------------------------------------------------------------------------------------------------

CONJ_SCHEMA = OrderedDict([("id", "Int32"), ("a", "Float64"), ("b", "Float64"), ("c", "Float64"), ("i", "Int32"), ("d", "Date32"),
                           ("j", "Int32")])
D0 = 9000                                    # the Date32 bound of the cases
CONJ_CASES = OrderedDict([
    # two comparisons on one column
    ("intersection", [("a", "Gt", 1.0, False), ("a", "LtEq", 5.0, False)]),
    ("redundant", [("a", "Gt", 1.0, False), ("a", "Gt", 0.5, False)]),
    ("eq_and_range", [("a", "Eq", 3.0, False), ("a", "GtEq", 1.0, False), ("a", "Gt", 5.0, True)]),
    ("int_intersection", [("i", "Gt", 6, False), ("i", "Lt", 9, False)]),
    # intersections that come out empty: the VM, no rows
    ("empty_5_3", [("a", "Gt", 5.0, False), ("a", "Lt", 3.0, False)]),
    ("empty_eq_gt", [("a", "Eq", 3.0, False), ("a", "Gt", 3.0, False)]),
    ("empty_int", [("i", "Gt", 7, False), ("i", "Lt", 8, False)]),
    # two, three and four distinct columns
    ("two_columns", [("a", "GtEq", 1.0, False), ("i", "Lt", 8, False)]),
    ("three_columns", [("d", "LtEq", D0, False), ("a", "Gt", 1.0, True), ("b", "Lt", 0.5, False)]),
    ("four_columns", [("a", "LtEq", 5.0, False), ("i", "GtEq", 7, False), ("d", "Gt", D0 - 1, False), ("b", "GtEq", -0.0, False),
                      ("a", "Gt", 0.5, False)]),
    # five: build_sop holds four ranges
    ("five_columns", [("a", "LtEq", 5.0, False), ("i", "GtEq", 7, False), ("d", "Gt", D0 - 1, False), ("b", "GtEq", -0.0, False),
                      ("c", "Lt", INF, False)]),
])
CONJ_EMPTY = ("empty_5_3", "empty_eq_gt", "empty_int")


def conj_batch(n, nulls="none", seed=0):
    """rows around every bound of CONJ_CASES.  nulls: "none", "one" (column a) or "all" (every range column), about 25 % each"""
    rng = np.random.default_rng(3000 + seed + n)
    pick = lambda vals: np.array(vals)[rng.integers(0, len(vals), n)]
    fa = [0.5, next_up(0.5), next_down(0.5), 1.0, next_up(1.0), next_down(1.0), 3.0, next_up(3.0), next_down(3.0), 5.0, next_up(5.0),
          next_down(5.0), 2.0, 4.0, math.nan, INF, -INF, 0.0]
    fb = [0.5, next_down(0.5), next_up(0.5), 0.0, -0.0, -5e-324, 5e-324, 0.25, math.nan, -INF]
    fc = [INF, DBL_MAX, 1.0, math.nan, -INF]
    ints = [6, 7, 8, 9, 5, INT32_MIN, INT32_MAX, 0]
    days = [D0 - 1, D0, D0 + 1, D0 - 2, INT32_MIN, INT32_MAX]
    # most rows pass most terms, so that every combination of "which term fails" occurs and the conjunctions keep rows
    a = np.where(rng.random(n) < 0.6, pick([2.0, 3.0, 4.0, 5.0, next_up(1.0)]), pick(fa))
    b = np.where(rng.random(n) < 0.6, pick([0.0, -0.0, 0.25, next_down(0.5)]), pick(fb))
    c = np.where(rng.random(n) < 0.7, pick([DBL_MAX, 1.0]), pick(fc))
    i = np.where(rng.random(n) < 0.6, pick([7, 8]), pick(ints))
    d = np.where(rng.random(n) < 0.6, pick([D0]), pick(days))
    valid = lambda k: rng.random(n) > 0.25 if nulls == "all" or (nulls == "one" and k == "a") else None
    return OrderedDict([("id", OCol("Int32", np.arange(n, dtype=np.int32))), ("a", OCol("Float64", a, valid("a"))),
                        ("b", OCol("Float64", b, valid("b"))), ("c", OCol("Float64", c, valid("c"))),
                        ("i", OCol("Int32", i.astype(np.int32), valid("i"))), ("d", OCol("Date32", d.astype(np.int32), valid("d"))),
                        ("j", OCol("Int32", rng.integers(0, 100, n).astype(np.int32)))])


def null_rows_that_would_pass(batch, terms):
    """rows the predicate drops only because a value is NULL"""
    n = len(next(iter(batch.values())))
    names = {t[0] for t in terms}
    values = {k: batch[k].values.tolist() for k in names}
    valid = {k: batch[k].is_valid() for k in names}
    return [r for r in range(n) if not all(valid[k][r] for k in names) and all(term_holds(t, values[t[0]][r]) for t in terms)]


# ---- chain cases ----------------------------------------------------------------------------------------------------------------

CHAIN_SCHEMA = OrderedDict([("ki", "Int32"), ("kl", "Int64"), ("k1", "Utf8"), ("ks", "Utf8"), ("kt", "Utf8"), ("d", "Date32"),
                            ("p", "Float64"), ("x", "Float64"), ("y", "Float64"), ("z", "Float64"), ("q", "Float64"), ("i", "Int32")])
X, Y, Z, Q = col("x"), col("y"), col("z"), col("q")
ONE = lit(1.0)
# alias -> (expression, the same product over one row's Python floats, in the expression's own order of operations)
CHAINS = OrderedDict([
    ("x", (X, lambda r: r["x"])),
    ("y", (Y, lambda r: r["y"])),
    ("z", (Z, lambda r: r["z"])),
    ("q", (Q, lambda r: r["q"])),
    ("xy", (X * Y, lambda r: r["x"] * r["y"])),
    ("xz", (X * Z, lambda r: r["x"] * r["z"])),
    ("x_1my", (X * (ONE - Y), lambda r: r["x"] * (1.0 - r["y"]))),
    ("x_1py", (X * (ONE + Y), lambda r: r["x"] * (1.0 + r["y"]))),
    ("xm25_y", ((X - lit(2.5)) * Y, lambda r: (r["x"] - 2.5) * r["y"])),
    ("1pz_1my_x", ((ONE + Z) * (ONE - Y) * X, lambda r: (1.0 + r["z"]) * (1.0 - r["y"]) * r["x"])),
    ("x_plus_negzero", (X + lit(-0.0), lambda r: r["x"] + (-0.0))),
    ("zero_minus_x", (lit(0.0) - X, lambda r: 0.0 - r["x"])),
    ("x_minus_zero", (X - lit(0.0), lambda r: r["x"] - 0.0)),
    ("x_3", (X * lit(3.0), lambda r: r["x"] * 3.0)),
    ("casti_x", (E.CastExpr(col("i"), "Float64") * X, lambda r: float(r["i"]) * r["x"])),
    ("x_1my_1pz", (X * (ONE - Y) * (ONE + Z), lambda r: r["x"] * (1.0 - r["y"]) * (1.0 + r["z"]))),
])
# case -> (the SUMs in order, chain steps build_sop makes of them, columns only: the wide-load kernels take it)
CHAIN_CASES = OrderedDict([
    ("x", (["x"], 1, True)),
    ("xy", (["xy"], 2, True)),
    ("x_1my", (["x_1my"], 2, True)),
    ("x_1py", (["x_1py"], 2, True)),
    ("xm25_y", (["xm25_y"], 2, True)),
    ("three_factors", (["1pz_1my_x"], 3, True)),
    ("x_plus_negzero", (["x_plus_negzero"], 1, True)),
    ("zero_minus_x", (["zero_minus_x"], 1, True)),
    ("x_minus_zero", (["x_minus_zero"], 1, True)),
    ("literal_factor", (["x_3"], 2, False)),
    ("cast_factor", (["casti_x"], 2, False)),
    ("q1_prefixes", (["x", "x_1my", "x_1my_1pz"], 3, True)),                       # each sum continues the one before it
    ("prefix_not_of_previous", (["x_1my", "z", "x_1my_1pz"], 6, True)),            # the third extends the first, not the second
    ("same_length_last_differs", (["xy", "xz"], 4, True)),
    ("q1_five", (["q", "x", "x_1my", "x_1my_1pz", "y"], 5, True)),                 # the specialised kernels' step count
    ("eight_steps", (["xy", "xz", "xm25_y", "q", "z"], 8, True)),                  # SOP_NSTEP
    ("nine_steps", (["xy", "xz", "xm25_y", "q", "z", "y"], 9, True)),              # one more: the VM
])
SOP_NSTEP = 8

# the designated rows' operands (x, y, z, q, i)
HOT = [
    (3.0, 0.9999999999999999, 0.25, 7.0, 3),              # 1.0 - y cancels to 2^-53
    (DBL_MAX, -1.0, 1.0, DBL_MAX, 2),                     # x * (1 - y) overflows to +inf
    (5e-324, 0.5, 0.0, 1.0, 1),                           # 5e-324 * 0.5 is a tie that rounds to zero
    (DBL_MIN, 0.9999999999999999, -0.5, 3.0, -1),         # x * y: a tie at the subnormals' edge, x * z a subnormal, x * (1 - y) zero
    (INF, 0.0, 0.0, 1.0, 0),                              # inf * 0 is NaN
    (-DBL_MAX, -0.5, 0.5, 2.0, INT32_MAX),                # -inf by overflow
    (math.nan, 0.5, 0.5, 1.0, 5),                         # a NaN operand
    (-INF, 2.0, -1.0, -1.0, INT32_MIN),                   # (1 + z) is zero against an infinity
    (1234.5, 0.07, 0.02, 17.0, -7),                       # ordinary
]
KEYS = {   # group number -> key value; the last group of a batch only ever holds rows that fail the predicate
    "ki": lambda g: [INT32_MIN, INT32_MAX, 0, -1][g] if g < 4 else 1000003 * g,
    "kl": lambda g: [-2 ** 63, 2 ** 63 - 1, 2 ** 40, -1][g] if g < 4 else 2 ** 33 * g,
    "k1": lambda g: "ANRXBCDEFGHIJKLM"[g],
    "ks": lambda g: "AN"[(g // 2) % 2] + ("" if g < 4 else str(g)),
    "kt": lambda g: "FO"[g % 2],
}


def chain_aggs(case):
    return [E.Sum(CHAINS[a][0], "s_" + a) for a in CHAIN_CASES[case][0]] + [E.Count(lit(1, E.UINT8), "n")]


def pred_values(term, dtype):
    """(values that pass the term, values that fail it) among the special values of its literal"""
    L = term[2]
    if dtype == "Float64":
        cand = [f64(int(b)) for b in float_specials(L)]
    else:
        cand = [int(v) for v in int_specials(L)] + [-1000, 1000]
    ok = [v for v in cand if term_holds(term, v)]
    return ok, [v for v in cand if not term_holds(term, v)]


def chain_batch(n, term, n_live_groups, hot_groups, operand_set, zero_yz, seed=0):
    """n rows over the groups 0 .. n_live_groups (the last one dead rows only, n permitting).  term: the predicate, over column p
    (Float64) or d (Date32).  Every group of hot_groups gets its designated row at a boundary row; the other rows are "zero rows"
    (pass the predicate; x and q are +-0.0; y and z too where zero_yz, else finite) or "dead rows" (fail the predicate; operands
    of any kind: infinities, NaN, large values)."""
    rng = np.random.default_rng(4000 + seed + 7 * n + operand_set)
    pcol = term[0]
    ok, bad = pred_values(term, CHAIN_SCHEMA[pcol])
    group = rng.integers(0, n_live_groups, n)
    kind = rng.choice(["zero", "dead"], n, p=[0.6, 0.4])
    if not ok:
        kind[:] = "dead"                                   # x > +inf: nothing passes
    else:
        rows = boundary_rows(n)
        spots = rng.permutation(len(rows))[:len(hot_groups)]
        for g, s in zip(hot_groups, spots):
            group[rows[s]] = g
            kind[rows[s]] = "hot"
    if n > n_live_groups + 8 and bad:
        lone = rng.choice(np.flatnonzero(kind != "hot"), 3, replace=False)
        group[lone] = n_live_groups                        # a key value no live row has
        kind[lone] = "dead"
    if not bad:
        kind[kind == "dead"] = "zero"                      # x <= +inf over non-NaN specials etc.: nothing fails
    choose = lambda vals: np.asarray(vals)[rng.integers(0, len(vals), n)]
    zero = lambda: choose([0.0, -0.0])
    finite = lambda: rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-40, 40, n))
    wild = [INF, -INF, math.nan, DBL_MAX, 1e300, -7.25, 5e-324]
    is_zero, is_dead = kind == "zero", kind == "dead"
    cols = {"x": np.where(is_zero, zero(), choose(wild)), "q": np.where(is_zero, zero(), choose(wild)),
            "y": np.where(is_zero, zero() if zero_yz else finite(), choose(wild)),
            "z": np.where(is_zero, zero() if zero_yz else finite(), choose(wild)),
            "i": np.where(is_zero, rng.integers(-5, 5, n), rng.integers(1, 100, n))}
    hot_of = {g: HOT[(len(hot_groups) * operand_set + k) % len(HOT)] for k, g in enumerate(hot_groups)}
    for r in np.flatnonzero(kind == "hot"):
        for k, v in zip("xyzqi", hot_of[int(group[r])]):
            cols[k][r] = v
    as_col = (lambda vals: np.array([bits_of(v) for v in vals], np.uint64)) if pcol == "p" else (lambda vals: np.array(vals, np.int64))
    pv = np.where(is_dead, choose(as_col(bad or ok)), choose(as_col(ok or bad)))
    out = OrderedDict((k, OCol(CHAIN_SCHEMA[k], [f(int(g)) for g in group])) for k, f in KEYS.items())
    out["p"] = OCol("Float64", pv.astype(np.uint64).view(np.float64) if pcol == "p" else rng.integers(-3, 3, n).astype(np.float64))
    out["d"] = OCol("Date32", (pv if pcol == "d" else rng.integers(8000, 10000, n)).astype(np.int32))
    for k in "xyzq":
        out[k] = OCol("Float64", cols[k])
    out["i"] = OCol("Int32", cols["i"].astype(np.int32))
    return OrderedDict((k, out[k]) for k in CHAIN_SCHEMA)


def chain_batches(n, term, case, grouped=True, operand_set=0, n_groups=3, seed=0):
    """the batches of one chain case of n rows in all (n == 2 * 1024 + 513: two batches of unequal size, each group's designated
    row in one of them)"""
    zero_yz = any(a in ("y", "z", "xm25_y") for a in CHAIN_CASES[case][0])     # a zero x alone does not make these zero
    g = min(n_groups if grouped else 1, n)
    if n == 2 * 1024 + 513:
        hot = list(range(g))
        return [chain_batch(1024 + 513, term, g, hot[0::2], operand_set, zero_yz, seed),
                chain_batch(1024, term, g, hot[1::2], operand_set + 1, zero_yz, seed + 1)]
    return [chain_batch(n, term, g, list(range(g)), operand_set, zero_yz, seed)]


def chain_expected(batches, term, case, key_cols):
    """group key tuple -> (row count, [the SUMs]) over all batches, after asserting the condition that makes them exact: among a
    group's rows that pass the predicate at most ONE has a non-zero (or NaN) product in any SUM of the case or an operand that is
    not finite; every other one has finite operands and an exact +-0.0 product in every SUM.  Also returns the SUM columns in
    which some group's result is a zero (its sign is open)."""
    aliases = CHAIN_CASES[case][0]
    groups = OrderedDict()
    for b in batches:
        lists = {k: b[k].to_pylist() for k in list(key_cols) + [term[0], "x", "y", "z", "q", "i"]}
        for r in range(len(lists["x"])):
            pv = lists[term[0]][r]
            if pv is None or not term_holds(term, pv):
                continue
            row = {k: lists[k][r] for k in ("x", "y", "z", "q", "i")}
            groups.setdefault(tuple(lists[k][r] for k in key_cols), []).append(row)
    expected, open_sign = OrderedDict(), set()
    for key, rows in groups.items():
        products = [[CHAINS[a][1](row) for a in aliases] for row in rows]
        designated = [k for k, (row, ps) in enumerate(zip(rows, products))
                      if any(v != 0.0 for v in ps) or not all(math.isfinite(row[c]) for c in "xyzq")]      # NaN != 0.0 is true
        assert len(designated) <= 1, (case, key, [rows[k] for k in designated])
        sums = list(products[designated[0]]) if designated else [0.0] * len(aliases)
        open_sign.update("s_" + a for a, v in zip(aliases, sums) if v == 0.0)
        expected[key] = (len(rows), sums)
    return expected, sorted(open_sign)
