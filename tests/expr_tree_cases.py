"""TEST INFRASTRUCTURE shared by test_expr_trees_cpu.py and test_expr_trees_gpu.py: a seeded, deterministic generator of TYPED
expression trees over `ballista_amd.expr`, the batches they run on, and the plans ("sinks") that carry them through the
expression VM (host/expr.cpp ProgramBuilder -> vm_device.h -> the sink kernels).

Everything here is a pure function of (family, seed): the same call gives the same trees, so a mismatch is reproducible from the
seed and the sink alone.  The oracle's `_binary` wants equal operand types, so every mixed-type step is an explicit CastExpr and
nothing goes through `coerce`.

What is deliberately NOT generated (the oracle cannot be the judge there):
  * transcendental functions (not bit exact), nullif (the oracle lacks it), temporal arithmetic;
  * integer division on SIGNED types (the oracle's |a| // |b| restatement is wrong at the type's minimum) and by anything that
    could be zero: unsigned `/` only, by a non-zero literal or by a column built without zeros (`u8nz` .. `u64nz`) — the oracle
    raises on any live zero divisor and which rows are live under a CASE is not specified;
  * Float -> Boolean casts (refused by the compiler) and float group keys (a computed NaN's sign and payload are not specified).
"""
from __future__ import annotations

import functools
import math
import random
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from ballista_amd import expr as E
from oracle.engine import NP_TYPES, OCol

SIGNED = (E.INT8, E.INT16, E.INT32, E.INT64)
UNSIGNED = (E.UINT8, E.UINT16, E.UINT32, E.UINT64)
INTS = SIGNED + UNSIGNED
FLOATS = (E.FLOAT32, E.FLOAT64)
NUMERIC = INTS + FLOATS
NARROW = (E.INT8, E.INT16, E.INT32, E.UINT8, E.UINT16, E.UINT32, E.FLOAT32)      # arithmetic takes a second (wrap / round) instruction
ROW_COUNTS = (1, 511, 512, 513, 1023, 1025, 1537)        # both sides of the 512-row (R=2) and 1024-row (R=4) tiles
FAMILIES = ("projection", "filter", "fused", "aggarg", "groupkey")
SEEDS = (11, 12)
TREES_PER_FAMILY = 40
MATH_FNS = ("sqrt", "abs", "floor", "ceil", "round", "trunc", "signum")      # the bit-exact ones
COMPARES = E.COMPARE_OPS

# every source -> target pair the generator draws casts from, and test_expr_trees_cpu.py demands at least once
CAST_PAIRS = tuple([(s, t) for s in NUMERIC for t in NUMERIC if s != t] +
                   [(E.BOOLEAN, t) for t in INTS] + [(s, E.BOOLEAN) for s in INTS] +
                   [(E.DATE32, E.INT32), (E.DATE32, E.INT64), (E.INT32, E.DATE32), (E.INT64, E.DATE32)])
# the node kinds (`kinds_of`) the generator must produce at least once
NODE_KINDS = tuple(["Column", "Literal", "NullLiteral", "Plus", "Minus", "Multiply", "DivideFloat", "DivideUnsigned", "And", "Or", "Not",
                    "IsNull", "IsNotNull", "Negative", "Cast", "CaseWhen", "CaseWhenElse", "CaseBase", "CaseBaseElse", "CaseNullBase",
                    "CaseNullCondition", "In", "NotIn", "InNullItem"] + list(COMPARES) + list(MATH_FNS))

# the builder's refusals that count as a SKIPPED random tree (host/expr.cpp; anything else is a failure)
LIMIT_MESSAGES = ("expression references more than 16 columns", "expression loads more than 16 columns",
                  "expression has more than 32 distinct literals", "expression needs more than 96 VM instructions",
                  "expression needs too many VM registers", "more than 8 key columns", "more than 16 distinct accumulators",
                  "more than 16 computed output columns")


def is_limit_refusal(message: str) -> bool:
    return any(m in message for m in LIMIT_MESSAGES)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
_F64_EDGES = [math.nan, math.inf, -math.inf, 0.0, -0.0, 5e-324, 1.7976931348623157e308, -1.7976931348623157e308,
              9007199254740993.0, 9223372036854775808.0, 2147483647.5, 0.49999999999999994, 4503599627370496.5, 255.9, -128.9]
_F32_EDGES = [math.nan, math.inf, -math.inf, 0.0, -0.0, 1e-45, 3.4028234663852886e38, -3.4028234663852886e38,
              9007199254740993.0, 9223372036854775808.0, 2147483647.5, 0.49999999999999994, 4503599627370496.5, 255.9, -128.9]


def _int_edges(t):
    lo, hi = E._INT_RANGE[t]
    return [lo, hi, 0, 1] + ([-1] if lo < 0 else [])


def _column(rng, dtype, n, body, edges, null_share, nonzero=False):
    """`body` values with every edge value planted twice where there is room — once in a valid row, once in a NULL row — and
    about `null_share` of the rows NULL"""
    vals = np.array(body, dtype=NP_TYPES[dtype])
    valid = rng.random(n) >= null_share if null_share > 0 else np.ones(n, np.bool_)
    spots = rng.permutation(n)
    for k, v in enumerate(list(edges) + list(edges)):
        if k >= n:
            break
        vals[spots[k]] = v
        if null_share > 0:
            valid[spots[k]] = k < len(edges)
    if nonzero:
        vals[vals == 0] = 3
    return OCol(dtype, vals, None if null_share == 0 else valid)


@functools.lru_cache(maxsize=None)
def batch(n: int, seed: int = 5) -> "OrderedDict[str, OCol]":
    """the batch every family runs on.  One object per (n, seed): the tests share it and never modify it"""
    rng = np.random.default_rng(1000 * seed + n)
    out = OrderedDict()

    def ints(t, small=0.75, nonzero=False):
        lo, hi = E._INT_RANGE[t]
        wide = rng.integers(lo, hi, n, dtype=np.int64 if lo < 0 else np.uint64, endpoint=True).astype(NP_TYPES[t])
        near = rng.integers(max(lo, -12), min(hi, 12), n, endpoint=True).astype(NP_TYPES[t])
        return _column(rng, t, n, np.where(rng.random(n) < small, near, wide), _int_edges(t), 0.12, nonzero)

    for t, name in zip(INTS, ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64")):
        out[name] = ints(t)
    for t, name in zip(UNSIGNED, ("u8nz", "u16nz", "u32nz", "u64nz")):       # divisors: no zero, not even under a NULL
        out[name] = ints(t, small=0.9, nonzero=True)
    body = np.where(rng.random(n) < 0.7, np.round(rng.normal(0, 6, n) * 2) / 2, rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 18, n))
    out["f64"] = _column(rng, E.FLOAT64, n, body, _F64_EDGES, 0.12)
    out["g64"] = _column(rng, E.FLOAT64, n, np.round(rng.normal(0, 4, n) * 4) / 4, _F64_EDGES[:6], 0.12)
    body = np.where(rng.random(n) < 0.7, np.round(rng.normal(0, 6, n) * 2) / 2, rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 12, n))
    with np.errstate(all="ignore"):
        out["f32"] = _column(rng, E.FLOAT32, n, body.astype(np.float32), np.array(_F32_EDGES).astype(np.float32), 0.12)
    out["d32"] = _column(rng, E.DATE32, n, rng.integers(-5, 12, n), [-2**31, 2**31 - 1, 0, 1, -1], 0.12)
    out["b"] = OCol(E.BOOLEAN, rng.random(n) < 0.5, rng.random(n) >= 0.12)
    out["c"] = OCol(E.BOOLEAN, rng.random(n) < 0.8, rng.random(n) >= 0.12)
    for g in (3, 7, 300):                                                  # plain group columns: the register, merge and hash paths
        out[f"k{g}"] = OCol(E.INT32, rng.integers(0, g, n).astype(np.int32))
    return out


SCHEMA = {"i8": E.INT8, "i16": E.INT16, "i32": E.INT32, "i64": E.INT64, "u8": E.UINT8, "u16": E.UINT16, "u32": E.UINT32, "u64": E.UINT64,
          "u8nz": E.UINT8, "u16nz": E.UINT16, "u32nz": E.UINT32, "u64nz": E.UINT64, "f64": E.FLOAT64, "g64": E.FLOAT64, "f32": E.FLOAT32,
          "d32": E.DATE32, "b": E.BOOLEAN, "c": E.BOOLEAN, "k3": E.INT32, "k7": E.INT32, "k300": E.INT32}
_COLUMNS_OF = {t: [n for n, u in SCHEMA.items() if u == t and not n.endswith("nz") and not n.startswith("k")] for t in set(SCHEMA.values())}
_NZ_COLUMN = {E.UINT8: "u8nz", E.UINT16: "u16nz", E.UINT32: "u32nz", E.UINT64: "u64nz"}


@functools.lru_cache(maxsize=None)
def float_batch(n: int, nulls: bool, seed: int = 9) -> "OrderedDict[str, OCol]":
    """the limit cases' batch: seventeen Float64 columns f0 .. f16 around 1.0 (products of sixteen stay finite) with a few
    specials and, with nulls, 3 % NULLs each (about 60 % of the rows have all sixteen), and a NULL-free Int32 column k of three
    values.  nulls=False: no validity buffer anywhere"""
    rng = np.random.default_rng(77 * seed + n + (1 if nulls else 0))
    out = OrderedDict()
    for i in range(17):
        body = np.round(rng.uniform(0.5, 1.5, n) * 64) / 64
        out[f"f{i}"] = _column(rng, E.FLOAT64, n, body, [math.nan, math.inf, -0.0, 0.0, -1.25][i % 5:i % 5 + 1], 0.03 if nulls else 0.0)
    out["k"] = OCol(E.INT32, rng.integers(0, 3, n).astype(np.int32))
    return out


# ---- rendering and measuring trees ------------------------------------------------------------------------------------------
def to_string(e) -> str:
    """the tree as text, in the form of the library's Expr::to_string()"""
    k = type(e).__name__
    if k == "Column":
        return e.name
    if k == "Literal":
        return f"NULL:{e.dtype}" if e.value is None else (repr(e.value) if e.dtype == E.FLOAT64 else f"{e.dtype}({e.value!r})")
    if k == "BinaryExpr":
        return f"({to_string(e.left)} {e.op} {to_string(e.right)})"
    if k == "CastExpr":
        return f"CAST({to_string(e.expr)} AS {e.dtype})"
    if k == "NotExpr":
        return f"NOT {to_string(e.expr)}"
    if k == "IsNullExpr":
        return f"{to_string(e.expr)} IS NULL"
    if k == "IsNotNullExpr":
        return f"{to_string(e.expr)} IS NOT NULL"
    if k == "NegativeExpr":
        return f"(- {to_string(e.expr)})"
    if k == "InListExpr":
        return f"{to_string(e.expr)} {'NOT IN' if e.negated else 'IN'} ({', '.join(to_string(x) for x in e.list)})"
    if k == "CaseExpr":
        s = "CASE " + (to_string(e.expr) + " " if e.expr is not None else "")
        s += "".join(f"WHEN {to_string(w)} THEN {to_string(t)} " for w, t in e.when_then)
        return s + (f"ELSE {to_string(e.else_expr)} " if e.else_expr is not None else "") + "END"
    if k == "ScalarFunctionExpr":
        return f"{e.fun}({', '.join(to_string(a) for a in e.args)})"
    raise TypeError(k)


def children(e):
    k = type(e).__name__
    if k == "BinaryExpr":
        return [e.left, e.right]
    if k in ("CastExpr", "NotExpr", "IsNullExpr", "IsNotNullExpr", "NegativeExpr"):
        return [e.expr]
    if k == "InListExpr":
        return [e.expr] + list(e.list)
    if k == "CaseExpr":
        return ([e.expr] if e.expr is not None else []) + [x for wt in e.when_then for x in wt] + ([e.else_expr] if e.else_expr is not None else [])
    if k == "ScalarFunctionExpr":
        return list(e.args)
    return []


def walk(e):
    yield e
    for c in children(e):
        yield from walk(c)


def _is_null_lit(e):
    return isinstance(e, E.Literal) and e.value is None


def kinds_of(e, schema=SCHEMA):
    """the NODE_KINDS names and the CAST_PAIRS that occur in the tree"""
    kinds, casts = set(), set()
    for x in walk(e):
        k = type(x).__name__
        if k == "Column":
            kinds.add("Column")
        elif k == "Literal":
            kinds.add("NullLiteral" if x.value is None else "Literal")
        elif k == "BinaryExpr":
            if x.op == "Divide":
                kinds.add("DivideFloat" if E.expr_type(x.left, schema) in FLOATS else "DivideUnsigned")
            else:
                kinds.add(x.op)
        elif k == "CastExpr":
            kinds.add("Cast")
            casts.add((E.expr_type(x.expr, schema), x.dtype))
        elif k == "NotExpr":
            kinds.add("Not")
        elif k == "IsNullExpr":
            kinds.add("IsNull")
        elif k == "IsNotNullExpr":
            kinds.add("IsNotNull")
        elif k == "NegativeExpr":
            kinds.add("Negative")
        elif k == "InListExpr":
            kinds.add("NotIn" if x.negated else "In")
            if any(_is_null_lit(i) for i in x.list):
                kinds.add("InNullItem")
        elif k == "CaseExpr":
            kinds.add(("CaseBase" if x.expr is not None else "CaseWhen") + ("Else" if x.else_expr is not None else ""))
            if x.expr is not None and _is_null_lit(x.expr):
                kinds.add("CaseNullBase")
            if x.expr is None and any(_is_null_lit(w) for w, _ in x.when_then):
                kinds.add("CaseNullCondition")
        elif k == "ScalarFunctionExpr":
            kinds.add(x.fun)
    return kinds, casts


def cost(e, schema=SCHEMA):
    """an UPPER estimate of what the tree asks of the compiler (no CSE assumed): VM instructions, and the sets of columns and of
    literal bit patterns.  The generator keeps a plan under budgets well inside the limits of vm_isa.h by it"""
    instr, cols, lits = 0, set(), set()
    for x in walk(e):
        k = type(x).__name__
        if k == "Column":
            cols.add(x.name)
        elif k == "Literal":
            lits.add((x.dtype in FLOATS, x.value))
            instr += 1                                # (a Boolean or NULL literal, or a literal that has to be materialised)
        elif k == "BinaryExpr":
            t = E.expr_type(x.left, schema)
            instr += 3 if t == E.BOOLEAN and x.op in COMPARES else 2 if x.op in E.ARITH_OPS and t in NARROW else 1
        elif k in ("CastExpr", "NegativeExpr"):
            instr += 2
        elif k == "InListExpr":
            instr += 2 * len(x.list) + 1
        elif k == "CaseExpr":
            instr += 2 * len(x.when_then) + 1
        else:
            instr += 1
    return instr, cols, lits


def depth(e):
    return 1 + max([depth(c) for c in children(e)], default=0)


# ---- the generator ------------------------------------------------------------------------------------------------------------
_INT_LITS = (0, 1, 2, 3, 5, 7, 10, 100)
_FLOAT_LITS = (0.0, 0.5, 1.0, 1.5, 2.0, -1.0, 2.5, 10.0, -0.0, 1e10, 0.1, 255.9)


class TreeGen:
    """typed trees to a depth budget.  `rand` is random.Random: only random() and randrange() are used, whose sequences Python
    keeps stable across versions"""

    def __init__(self, seed, cast_use=None):
        self.r = random.Random(seed)
        self.math_use = 0
        self.pool = {}                               # type -> subtrees made so far: drawn again so that CSE has work
        self.cast_use = cast_use if cast_use is not None else {p: 0 for p in CAST_PAIRS}

    def pick(self, seq):
        return seq[self.r.randrange(len(seq))]

    def chance(self, p):
        return self.r.random() < p

    # -- leaves
    def literal(self, t, allow_null=True):
        if allow_null and self.chance(0.025):
            return E.Literal(None, t)
        if t == E.BOOLEAN:
            return E.Literal(self.chance(0.5), t)
        if t in FLOATS:
            return E.Literal(self.pick(_FLOAT_LITS), t)
        lo, hi = E._INT_RANGE[t]
        v = self.pick(_INT_LITS + ((-1, -2, -7) if lo < 0 else ()) + ((lo, hi) if self.chance(0.15) else ()))
        return E.Literal(v if lo <= v <= hi else 1, t)

    def leaf(self, t):
        cols = _COLUMNS_OF.get(t, [])
        if cols and self.chance(0.97 if t == E.BOOLEAN else 0.92):        # (a constant operand decides an AND / OR for every row)
            return E.col(self.pick(cols))
        return self.literal(t)

    def remember(self, t, e):
        if not isinstance(e, (E.Column, E.Literal)):
            self.pool.setdefault(t, []).append(e)
        return e

    def shared(self, t, d):
        have = [e for e in self.pool.get(t, []) if depth(e) <= d + 1]
        return self.pick(have) if have else None

    # -- casts: the least used source type first, so that the whole matrix is covered
    def cast_to(self, t, d):
        srcs = [s for (s, u) in CAST_PAIRS if u == t]
        if not srcs:
            return None
        least = min(self.cast_use[(s, t)] for s in srcs)
        s = self.pick([s for s in srcs if self.cast_use[(s, t)] == least])
        self.cast_use[(s, t)] += 1
        return E.CastExpr(self.gen(s, d - 1), t)

    def two(self, t, d):
        """the operands of a binary node: left-deep, right-deep or balanced"""
        shape = self.r.randrange(3)
        a, b = (self.gen(t, d - 1), self.leaf(t)) if shape == 0 else (self.leaf(t), self.gen(t, d - 1)) if shape == 1 else \
            (self.gen(t, d - 1), self.gen(t, d - 1))
        if isinstance(a, E.Column) and isinstance(b, E.Column) and a.name == b.name:       # x - x, x < x: nothing to compute
            b = self.literal(t, allow_null=False)
        return a, b

    def case(self, t, d):
        n_when = 1 + self.r.randrange(2)
        with_else = self.chance(0.5)
        if self.chance(0.5):                         # CASE WHEN cond THEN ..
            wt = [(E.Literal(None, E.BOOLEAN) if self.chance(0.05) else self.gen(E.BOOLEAN, d - 1), self.gen(t, d - 1)) for _ in range(n_when)]
            return E.CaseExpr(None, wt, self.gen(t, d - 1) if with_else else None)
        bt = self.pick((E.INT8, E.INT32, E.UINT8, E.INT64, E.DATE32, E.UINT16))      # CASE base WHEN value THEN ..
        base = E.Literal(None, bt) if self.chance(0.05) else self.gen(bt, min(d - 1, 1))
        wt = [(self.literal(bt), self.gen(t, d - 1)) for _ in range(n_when)]
        return E.CaseExpr(base, wt, self.gen(t, d - 1) if with_else else None)

    def gen(self, t, d):
        if d <= 0:
            return self.leaf(t)
        if self.chance(0.12):
            e = self.shared(t, d)
            if e is not None:
                return e
        return self.remember(t, self.gen_boolean(d) if t == E.BOOLEAN else self.gen_date(d) if t == E.DATE32 else self.gen_numeric(t, d))

    def gen_numeric(self, t, d):
        x = self.r.random()
        if x < 0.42:
            a, b = self.two(t, d)
            return E.BinaryExpr(a, self.pick(("Plus", "Minus", "Multiply")), b)
        if x < 0.50 and (t in FLOATS or t in UNSIGNED):
            if t in FLOATS:
                a, b = self.two(t, d)
                return E.BinaryExpr(a, "Divide", b)
            lo, hi = E._INT_RANGE[t]
            divisor = E.col(_NZ_COLUMN[t]) if self.chance(0.5) else E.Literal(self.pick((1, 2, 3, 7, 10, hi)), t)
            return E.BinaryExpr(self.gen(t, d - 1), "Divide", divisor)
        if x < 0.56 and (t in SIGNED or t in FLOATS):
            return E.NegativeExpr(self.gen(t, d - 1))
        if x < 0.80:
            return self.cast_to(t, d)
        if t == E.FLOAT64 and x >= 0.86:
            self.math_use += 1                       # (in turn, so that all seven occur)
            return E.ScalarFunctionExpr(MATH_FNS[self.math_use % len(MATH_FNS)], [self.gen(t, d - 1)])
        if x < 0.90:
            return self.case(t, d)
        return self.cast_to(t, d)

    def gen_date(self, d):
        if self.chance(0.5):
            return self.cast_to(E.DATE32, d)
        return self.case(E.DATE32, d)

    def compare(self, d):
        t = self.pick(NUMERIC + (E.DATE32, E.BOOLEAN, E.FLOAT64, E.INT32))
        op = self.pick(("Lt", "LtEq", "Gt", "GtEq", "Lt", "Gt", "Eq", "NotEq"))
        if self.chance(0.5):
            return E.BinaryExpr(self.gen(t, d - 1), op, self.literal(t, allow_null=False))
        a, b = self.two(t, d)
        return E.BinaryExpr(a, op, b)

    def gen_boolean(self, d):
        x = self.r.random()
        if x < 0.36:
            return self.compare(d)
        if x < 0.56:
            a, b = self.two(E.BOOLEAN, d)
            return E.BinaryExpr(a, self.pick(("And", "Or")), b)
        if x < 0.63:
            return E.NotExpr(self.gen(E.BOOLEAN, d - 1))
        if x < 0.72:
            t = self.pick(NUMERIC + (E.DATE32, E.BOOLEAN))
            inner = self.gen(t, d - 1)
            return E.IsNullExpr(inner) if self.chance(0.5) else E.IsNotNullExpr(inner)
        if x < 0.82:
            t = self.pick((E.INT8, E.INT32, E.UINT8, E.INT64, E.UINT64, E.FLOAT64, E.DATE32, E.INT16))
            items = [self.literal(t, allow_null=False) for _ in range(1 + self.r.randrange(3))]
            negated = self.chance(0.4)
            if self.chance(0.12 if negated else 0.35):          # (x NOT IN (.., NULL) is never TRUE: kept rare)
                items.insert(self.r.randrange(len(items) + 1), E.Literal(None, t))
            return E.InListExpr(self.gen(t, min(d - 1, 1)), items, negated=negated)
        if x < 0.92:
            return self.cast_to(E.BOOLEAN, d)
        return self.case(E.BOOLEAN, d)


# ---- families ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    family: str
    seed: int
    index: int
    n_rows: int
    trees: List[object]                      # the generated trees of the case (what the CPU tier evaluates)
    exprs: list = field(default_factory=list)         # projection: [(expr, name)]
    predicate: Optional[object] = None                # filter, fused
    group: list = field(default_factory=list)         # [(expr, name)]
    aggs: list = field(default_factory=list)          # [AggregateExpr]

    @property
    def id(self):
        return f"{self.family}-seed{self.seed}-{self.index}"

    def describe(self):
        return f"[{self.id}, {self.n_rows} rows] " + " ; ".join(to_string(t) for t in self.trees)


# budgets per PLAN (one VM program), well inside vm_isa.h: 96 instructions, 16 columns, 32 literals, 24 value and 16 Boolean slots
_MAX_INSTR, _MAX_COLS, _MAX_LITS, _MAX_SLOTS = 64, 11, 20, 17


class _Plan:
    """what a plan's trees add up to, by `cost`; `fits` says whether one more tree stays inside the budgets"""

    def __init__(self, held=0):
        self.instr, self.cols, self.lits, self.held, self.deepest = 0, set(), set(), held, 0

    def fits(self, e, holds=1):
        i, c, l = cost(e)
        # slots: every column and every held result (output, accumulator input, key part) stays live, plus the pending intermediates
        slots = len(self.cols | c) + self.held + holds + max(self.deepest, depth(e))
        return self.instr + i <= _MAX_INSTR and len(self.cols | c) <= _MAX_COLS and len(self.lits | l) <= _MAX_LITS and slots <= _MAX_SLOTS

    def add(self, e, holds=1):
        i, c, l = cost(e)
        self.instr += i
        self.cols |= c
        self.lits |= l
        self.held += holds
        self.deepest = max(self.deepest, depth(e))


def _draw(g, plan, t, d, holds=1):
    """a tree of type t that fits the plan: the depth shrinks until it does (a leaf always fits the budgets' margins)"""
    while True:
        e = g.gen(t, d)
        if plan.fits(e, holds) or d == 0:
            return e
        d -= 1


def _n_rows(seed, index):
    return ROW_COUNTS[(index + seed) % len(ROW_COUNTS)]


def _family_seed(family, seed):
    return 7919 * seed + 104729 * FAMILIES.index(family)


@functools.lru_cache(maxsize=None)
def cases(family: str, seed: int, count: int = TREES_PER_FAMILY):
    """the cases of one family and seed; about `count` generated trees.  Cached: one list per argument list, never modified"""
    g = TreeGen(_family_seed(family, seed))
    out = []
    made = 0
    while made < count:
        i = len(out)
        n = _n_rows(seed, i)
        plan = _Plan()
        if family == "projection":
            # some projections are many small outputs (up to 16), some a few deep ones
            n_out = g.pick((16, 12, 3, 2, 1, 5, 8))
            d = 1 if n_out >= 12 else 2 if n_out >= 5 else 4
            exprs = []
            for j in range(n_out):
                t = g.pick(NUMERIC + (E.BOOLEAN, E.DATE32, E.FLOAT64, E.INT32))
                e = _draw(g, plan, t, d)
                if j == 0:                                   # the seven bit-exact functions in turn, one per projection
                    e = E.ScalarFunctionExpr(MATH_FNS[i % len(MATH_FNS)], [_draw(g, plan, E.FLOAT64, min(d, 2))])
                if isinstance(e, E.Column):                  # (a bare column is passed through, not computed)
                    e = E.CastExpr(e, E.FLOAT64) if t in INTS else E.IsNullExpr(e)
                if not plan.fits(e):
                    break
                plan.add(e)
                exprs.append((e, f"o{j}"))
            if not exprs:
                continue
            out.append(Case(family, seed, i, n, [e for e, _ in exprs], exprs=exprs))
            made += len(exprs)
            continue
        if family == "filter":
            p = _draw(g, plan, E.BOOLEAN, g.pick((2, 3, 4, 5)))
            out.append(Case(family, seed, i, n, [p], predicate=p))
            made += 1
            continue
        if family == "fused":
            # an ungrouped partial aggregate over FilterExec(pred): the predicate's slot guards the integer divisions of the arguments
            p = _draw(g, plan, E.BOOLEAN, g.pick((2, 3, 4)))
            plan.add(p)
            t = g.pick(UNSIGNED)
            a1 = E.BinaryExpr(_draw(g, plan, t, 2), "Divide", E.col(_NZ_COLUMN[t]) if g.chance(0.5) else E.Literal(g.pick((1, 2, 3, 7)), t))
            plan.add(a1)
            a2 = E.CastExpr(_draw(g, plan, g.pick(NUMERIC), 2), g.pick((E.INT8, E.INT16)))
            aggs = [E.Count(a1, "cnt"), E.Max(a1, "mx"), E.Sum(a2, "sm"), E.Min(E.col("i32"), "mn")]
            out.append(Case(family, seed, i, n, [p, a1, a2], predicate=p, aggs=aggs))
            made += 1
            continue
        if family == "aggarg":
            # COUNT / MIN / MAX over any numeric tree, SUM over trees cast to Int8 / Int16 (exact, cannot overflow);
            # ungrouped and by 3, 7 and about 300 groups: the register, merge and hash paths interpret the same programs
            key = g.pick((None, "k3", "k7", "k300"))
            t = g.pick(NUMERIC)
            a = _draw(g, plan, t, g.pick((2, 3, 4)), holds=2)
            if isinstance(a, E.Literal):
                a = E.BinaryExpr(a, "Plus", g.leaf(t))
            plan.add(a, 2)
            s = E.CastExpr(_draw(g, plan, g.pick(NUMERIC), 2), g.pick((E.INT8, E.INT16)))
            aggs = [E.Count(a, "cnt"), E.Min(a, "mn"), E.Max(a, "mx"), E.Sum(s, "sm")]
            out.append(Case(family, seed, i, n, [a, s], group=[(E.col(key), key)] if key else [], aggs=aggs))
            made += 1
            continue
        if family == "groupkey":
            # one to three computed key parts: integer, Date32 and Boolean trees, nullable
            keys = []
            for j in range(1 + g.r.randrange(3)):
                t = g.pick(INTS + (E.DATE32, E.BOOLEAN, E.INT8, E.UINT8))
                e = _draw(g, plan, t, g.pick((1, 2, 3)))
                plan.add(e)
                keys.append((e, f"g{j}"))
            aggs = [E.Count(E.col("i16"), "cnt"), E.Sum(E.col("i8"), "sm"), E.Min(E.col("u64"), "mn")]
            out.append(Case(family, seed, i, n, [e for e, _ in keys], group=keys, aggs=aggs))
            made += 1
            continue
        raise ValueError(family)
    return out


def build_plan(P, case: Case, leaf):
    """the case's plan over `leaf`, with the operator classes of module P (ballista_amd, or tests/plan_nodes.py for the oracle)"""
    if case.family == "projection":
        return P.ProjectionExec(case.exprs, leaf)
    if case.family == "filter":
        return P.FilterExec(case.predicate, leaf)
    if case.family == "fused":
        return P.HashAggregateExec("Partial", [], case.aggs, P.FilterExec(case.predicate, leaf))
    return P.HashAggregateExec("Partial", case.group, case.aggs, leaf)


def key_columns(case: Case):
    """None: the rows compare in order (Projection, Filter); else the key columns the aggregate's rows are matched by"""
    return None if case.family in ("projection", "filter") else [n for _, n in case.group]


def zero_sign_columns(case: Case):
    """MIN / MAX of a float argument: a tie of -0.0 and +0.0 may give either zero (helpers.assert_rows_equal)"""
    return tuple(f"{a.name}[{a.fun.lower()}]" for a in case.aggs if a.fun in ("MIN", "MAX") and E.expr_type(a.expr, SCHEMA) in FLOATS)
