"""Physical expressions — the host-side mirror of the expression kinds a Ballista executor
can receive.

The set is exactly what the reference's physical-plan serde accepts
(rust/core/src/serde/physical_plan/to_proto.rs:380-511; rebuilt by `compile_expr`,
from_proto.rs:348-364): Column, Literal, BinaryExpr, CastExpr, CaseExpr, NotExpr,
IsNullExpr, IsNotNullExpr, InListExpr, NegativeExpr, ScalarFunctionExpr — and the
aggregate kinds of to_proto.rs:348-378 (Sum, Avg, Count; Min/Max exist in the proto but
are not serialisable there, we accept them anyway).  Binary operator names are the wire
strings of rust/core/src/serde/logical_plan/from_proto.rs:937-957.

These classes are plain descriptions; `ballista_amd.plan` lowers them to the flat VM
program the C-ABI takes (include/ballista_hip.h, `bhip_expr_*`).  As in DataFusion's
*physical* plans both sides of a BinaryExpr must already have equal types — use
`coerce()` to insert the casts DataFusion's planner would.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

# Arrow type names as in rust/benchmarks/tpch/src/main.rs:267-360 / SURVEY §8(b)
INT32, INT64, UINT8, UINT64 = "Int32", "Int64", "UInt8", "UInt64"
FLOAT64, DATE32, BOOLEAN, UTF8 = "Float64", "Date32", "Boolean", "Utf8"
# the other primitive types the serde ships (rust/core/proto/ballista.proto:755-790)
INT8, INT16, UINT16, UINT32, FLOAT32, DATE64 = "Int8", "Int16", "UInt16", "UInt32", "Float32", "Date64"
TIMESTAMP_S, TIMESTAMP_MS = "Timestamp(Second)", "Timestamp(Millisecond)"
TIMESTAMP_US, TIMESTAMP_NS = "Timestamp(Microsecond)", "Timestamp(Nanosecond)"
BINARY = "Binary"              # schemas only: variable-length bytes (the sha* digests) in the buffer layout of Utf8
LARGE_UTF8 = "LargeUtf8"       # schemas only (Arrow / IPC form of a Utf8 device column with 64-bit offsets)
ALL_TYPES = (INT32, INT64, UINT8, UINT64, FLOAT64, DATE32, BOOLEAN, UTF8, INT8, INT16, UINT16, UINT32, FLOAT32, DATE64,
             TIMESTAMP_S, TIMESTAMP_MS, TIMESTAMP_US, TIMESTAMP_NS)

BINARY_OPS = ("And", "Or", "Eq", "NotEq", "LtEq", "Lt", "Gt", "GtEq",
              "Plus", "Minus", "Multiply", "Divide", "Like", "NotLike")
COMPARE_OPS = ("Eq", "NotEq", "LtEq", "Lt", "Gt", "GtEq")
ARITH_OPS = ("Plus", "Minus", "Multiply", "Divide")

MATH_FUNCTIONS = ("sqrt", "abs", "floor", "ceil", "round", "trunc", "signum",
                  "exp", "ln", "log2", "log10", "sin", "cos", "tan", "asin", "acos", "atan")
# Utf8 -> Utf8 (rust/core/src/serde/logical_plan/from_proto.rs:914-918) and Utf8 -> Int32 (:910)
STRING_FUNCTIONS = ("lower", "upper", "trim", "ltrim", "rtrim")
# Utf8 -> Binary digests (from_proto.rs:924-927)
SHA_FUNCTIONS = ("sha224", "sha256", "sha384", "sha512")
# concat(a1 .. a8) -> Utf8, nullif(a, b) -> type of a, date_trunc('granularity', t) -> type of t, to_timestamp(s) ->
# Timestamp(Nanosecond) (from_proto.rs:913-923 leaves them out; the rules are DESIGN.md §3.2).  md5 and array stay refused.
# The code-point string functions and date_part (no wire form either): substr(s, start[, count]), left(s, n),
# right(s, n) -> Utf8; char_length(s), strpos(s, sub) -> Int32; starts_with(s, prefix) -> Boolean; date_part('part', x) -> Int32.
MULTI_ARG_FUNCTIONS = {"concat": (1, 8), "nullif": (2, 2), "date_trunc": (2, 2), "substr": (2, 3), "left": (2, 2), "right": (2, 2),
                       "strpos": (2, 2), "starts_with": (2, 2), "date_part": (2, 2)}
DATE_TRUNC_GRANULARITIES = ("second", "minute", "hour", "day", "week", "month", "year")
DATE_PART_PARTS = ("year", "quarter", "month", "day", "dow", "doy", "hour", "minute", "second")
SUBSTRING_FUNCTIONS = ("substr", "left", "right")
FUNCTION_ALIASES = {"substring": "substr", "length": "char_length", "character_length": "char_length"}
SCALAR_FUNCTIONS = (MATH_FUNCTIONS + STRING_FUNCTIONS + SHA_FUNCTIONS + SUBSTRING_FUNCTIONS +
                    ("octet_length", "concat", "nullif", "date_trunc", "to_timestamp", "char_length", "strpos", "starts_with", "date_part"))


class PhysicalExpr:
    """Base class (DataFusion `PhysicalExpr`)."""

    # small builder sugar used by tests / tpch plans
    def _bin(self, op, other):
        return BinaryExpr(self, op, other if isinstance(other, PhysicalExpr) else lit(other))

    def __add__(self, o): return self._bin("Plus", o)
    def __sub__(self, o): return self._bin("Minus", o)
    def __mul__(self, o): return self._bin("Multiply", o)
    def __truediv__(self, o): return self._bin("Divide", o)
    def __lt__(self, o): return self._bin("Lt", o)
    def __le__(self, o): return self._bin("LtEq", o)
    def __gt__(self, o): return self._bin("Gt", o)
    def __ge__(self, o): return self._bin("GtEq", o)
    def eq(self, o): return self._bin("Eq", o)
    def ne(self, o): return self._bin("NotEq", o)
    def and_(self, o): return self._bin("And", o)
    def or_(self, o): return self._bin("Or", o)
    def __neg__(self): return NegativeExpr(self)


@dataclass(eq=False)
class Column(PhysicalExpr):
    name: str


@dataclass(eq=False)
class Literal(PhysicalExpr):
    """ScalarValue (rust/core/proto/ballista.proto:685-709). value None = typed NULL."""
    value: object
    dtype: str


@dataclass(eq=False)
class BinaryExpr(PhysicalExpr):
    left: PhysicalExpr
    op: str
    right: PhysicalExpr

    def __post_init__(self):
        if self.op not in BINARY_OPS:
            raise ValueError(f"Unsupported binary operator '{self.op}'")


@dataclass(eq=False)
class CastExpr(PhysicalExpr):
    expr: PhysicalExpr
    dtype: str


@dataclass(eq=False)
class CaseExpr(PhysicalExpr):
    """CASE [expr] WHEN w THEN t ... [ELSE e] END."""
    expr: Optional[PhysicalExpr]
    when_then: Sequence[Tuple[PhysicalExpr, PhysicalExpr]]
    else_expr: Optional[PhysicalExpr] = None


@dataclass(eq=False)
class NotExpr(PhysicalExpr):
    expr: PhysicalExpr


@dataclass(eq=False)
class IsNullExpr(PhysicalExpr):
    expr: PhysicalExpr


@dataclass(eq=False)
class IsNotNullExpr(PhysicalExpr):
    expr: PhysicalExpr


@dataclass(eq=False)
class InListExpr(PhysicalExpr):
    expr: PhysicalExpr
    list: Sequence[PhysicalExpr]
    negated: bool = False


@dataclass(eq=False)
class NegativeExpr(PhysicalExpr):
    expr: PhysicalExpr


@dataclass(eq=False)
class ScalarFunctionExpr(PhysicalExpr):
    fun: str
    args: Sequence[PhysicalExpr]

    def __post_init__(self):
        self.fun = FUNCTION_ALIASES.get(self.fun, self.fun)
        if self.fun not in SCALAR_FUNCTIONS:
            raise NotImplementedError(f"scalar function '{self.fun}' is not supported")
        lo, hi = MULTI_ARG_FUNCTIONS.get(self.fun, (1, 1))
        if len(self.args) > hi and self.fun == "concat":
            raise NotImplementedError("concat with more than 8 arguments")
        if not lo <= len(self.args) <= hi:
            raise ValueError(f"scalar function '{self.fun}' takes {lo if lo == hi else f'{lo} to {hi}'} argument(s), not {len(self.args)}")


# ---- aggregates (DataFusion `AggregateExpr`) -----------------------------------------

@dataclass(eq=False)
class AggregateExpr:
    fun: str            # "SUM" | "AVG" | "COUNT" | "MIN" | "MAX" | "COUNT_DISTINCT" | "SUM_DISTINCT" | "AVG_DISTINCT" (plan.SINGLE only)
    expr: PhysicalExpr
    name: str

    def __post_init__(self):
        if self.fun not in ("SUM", "AVG", "COUNT", "MIN", "MAX", "COUNT_DISTINCT", "SUM_DISTINCT", "AVG_DISTINCT"):
            raise NotImplementedError(f"aggregate function '{self.fun}' is not supported")


def Sum(expr, name): return AggregateExpr("SUM", expr, name)
def Avg(expr, name): return AggregateExpr("AVG", expr, name)
def Count(expr, name): return AggregateExpr("COUNT", expr, name)
def Min(expr, name): return AggregateExpr("MIN", expr, name)
def Max(expr, name): return AggregateExpr("MAX", expr, name)
def CountDistinct(expr, name): return AggregateExpr("COUNT_DISTINCT", expr, name)
def SumDistinct(expr, name): return AggregateExpr("SUM_DISTINCT", expr, name)
def AvgDistinct(expr, name): return AggregateExpr("AVG_DISTINCT", expr, name)


@dataclass(eq=False)
class PhysicalSortExpr:
    """ballista.proto PhysicalSortExprNode; SQL default ASC NULLS FIRST (Appendix A)."""
    expr: PhysicalExpr
    descending: bool = False
    nulls_first: bool = True


# ---- window expressions (WindowAggExec; no wire form) ---------------------------------

WINDOW_FUNCTIONS = ("ROW_NUMBER", "RANK", "DENSE_RANK", "LAG", "LEAD", "FIRST_VALUE", "LAST_VALUE", "SUM", "AVG", "COUNT", "MIN", "MAX")
# DEFAULT is SQL's: RANGE_TO_CURRENT with an ORDER BY, PARTITION without one (resolved when the plan is made)
WINDOW_FRAMES = ("DEFAULT", "PARTITION", "ROWS_TO_CURRENT", "RANGE_TO_CURRENT")


@dataclass(frozen=True)
class RowsFrame:
    """ROWS BETWEEN start AND end by signed offsets from the current row: -2 = 2 PRECEDING, 0 = CURRENT ROW, 3 = 3 FOLLOWING;
    None = UNBOUNDED PRECEDING (start) / UNBOUNDED FOLLOWING (end).  Any Int64 offset; a finite start after a finite end is refused
    when the plan is made."""
    start: Optional[int]
    end: Optional[int]

    def __post_init__(self):
        for side in (self.start, self.end):
            if side is not None and (isinstance(side, bool) or not isinstance(side, int) or not -2**63 <= side < 2**63):
                raise TypeError(f"a rows frame offset is None or an Int64, got {side!r}")


class _CurrentRow:
    """the CURRENT ROW side of a RangeFrame / GroupsFrame: the row's first (start) or last (end) peer"""
    _instance = None

    def __new__(cls):
        if cls._instance is None:
            cls._instance = super().__new__(cls)
        return cls._instance

    def __repr__(self):
        return "CURRENT_ROW"


CURRENT_ROW = _CurrentRow()


def _check_value_sides(what, sides, floats):
    for side in sides:
        if side is None or side is CURRENT_ROW:
            continue
        if isinstance(side, int) and not isinstance(side, bool) and -2**63 <= side < 2**63:
            continue
        if floats and isinstance(side, float) and math.isfinite(side):
            continue
        raise TypeError(f"a {what} frame side is None, CURRENT_ROW, an Int64{' or a finite float' if floats else ''}, got {side!r}")


@dataclass(frozen=True)
class RangeFrame:
    """RANGE BETWEEN start AND end, measured in values of the single order key.  A side is None (UNBOUNDED PRECEDING / FOLLOWING),
    CURRENT_ROW (the row's first / last peer), or a signed offset: -7 = 7 PRECEDING, 0.5 = 0.5 FOLLOWING — an int for integer, date and
    timestamp keys, a float (or an int a double holds exactly) for float keys."""
    start: Union[None, _CurrentRow, int, float]
    end: Union[None, _CurrentRow, int, float]

    def __post_init__(self):
        _check_value_sides("RANGE", (self.start, self.end), True)


@dataclass(frozen=True)
class GroupsFrame:
    """GROUPS BETWEEN start AND end, measured in peer groups: -1 = 1 PRECEDING (the group before the row's), CURRENT_ROW = 0, None =
    unbounded."""
    start: Union[None, _CurrentRow, int]
    end: Union[None, _CurrentRow, int]

    def __post_init__(self):
        _check_value_sides("GROUPS", (self.start, self.end), False)


@dataclass(eq=False)
class WindowExpr:
    """one function over the operator's window: fun(expr[, offset]) [frame] AS name.  ROW_NUMBER / RANK / DENSE_RANK take no
    argument; offset is LAG / LEAD's k (a plain non-negative integer); frame, one of WINDOW_FRAMES or a RowsFrame / RangeFrame /
    GroupsFrame, matters for the aggregates and LAST_VALUE, a frame object for FIRST_VALUE too."""
    fun: str
    expr: Optional[PhysicalExpr]
    name: str
    offset: int = 1
    frame: Union[str, RowsFrame, RangeFrame, GroupsFrame] = "DEFAULT"

    def __post_init__(self):
        if self.fun not in WINDOW_FUNCTIONS:
            raise NotImplementedError(f"window function '{self.fun}' is not supported")
        if not isinstance(self.frame, (RowsFrame, RangeFrame, GroupsFrame)) and self.frame not in WINDOW_FRAMES:
            raise NotImplementedError(f"window frame '{self.frame}' is not supported")


def count_star(name, frame="DEFAULT"):
    """COUNT(*) OVER (...): COUNT of a UInt8 literal 1"""
    return WindowExpr("COUNT", Literal(1, UINT8), name, frame=frame)


# ---- helpers -------------------------------------------------------------------------

def col(name: str) -> Column:
    return Column(name)


def lit(v, dtype: Optional[str] = None) -> Literal:
    if isinstance(v, Literal):
        return v
    if dtype is None:
        if isinstance(v, bool):
            dtype = BOOLEAN
        elif isinstance(v, int):
            dtype = INT64
        elif isinstance(v, float):
            dtype = FLOAT64
        elif isinstance(v, str):
            dtype = UTF8
        else:
            raise TypeError(f"cannot infer literal type of {v!r}")
    return Literal(v, dtype)


def date32(s: str) -> Literal:
    """`date 'YYYY-MM-DD'` literal as days since 1970-01-01 (Appendix A)."""
    import datetime
    d = datetime.date.fromisoformat(s)
    return Literal((d - datetime.date(1970, 1, 1)).days, DATE32)


# DataFusion's numerical_coercion (4.0.0-SNAPSHOT, physical_plan/expressions/coercion.rs): equal types stay, otherwise the FIRST of
# Float64, Float32, Int64, Int32, Int16, Int8, UInt64, UInt32, UInt16, UInt8 that either side has
_NUMERIC_RANK = {FLOAT64: 10, FLOAT32: 9, INT64: 8, INT32: 7, INT16: 6, INT8: 5, UINT64: 4, UINT32: 3, UINT16: 2, UINT8: 1}
_TEMPORAL = (DATE32, DATE64, TIMESTAMP_S, TIMESTAMP_MS, TIMESTAMP_US, TIMESTAMP_NS)
_INT_RANGE = {INT8: (-2**7, 2**7 - 1), INT16: (-2**15, 2**15 - 1), INT32: (-2**31, 2**31 - 1), INT64: (-2**63, 2**63 - 1),
              UINT8: (0, 2**8 - 1), UINT16: (0, 2**16 - 1), UINT32: (0, 2**32 - 1), UINT64: (0, 2**64 - 1), DATE32: (-2**31, 2**31 - 1),
              DATE64: (-2**63, 2**63 - 1), TIMESTAMP_S: (-2**63, 2**63 - 1), TIMESTAMP_MS: (-2**63, 2**63 - 1),
              TIMESTAMP_US: (-2**63, 2**63 - 1), TIMESTAMP_NS: (-2**63, 2**63 - 1)}


def expr_type(e: PhysicalExpr, schema: dict) -> str:
    """Result type of `e` over `schema` (name -> Arrow type name)."""
    if isinstance(e, Column):
        if e.name not in schema:
            raise KeyError(f"No field named '{e.name}'")
        return schema[e.name]
    if isinstance(e, Literal):
        return e.dtype
    if isinstance(e, BinaryExpr):
        if e.op in ARITH_OPS:
            return expr_type(e.left, schema)
        return BOOLEAN
    if isinstance(e, CastExpr):
        return e.dtype
    if isinstance(e, CaseExpr):
        return expr_type(e.when_then[0][1], schema)
    if isinstance(e, (NotExpr, IsNullExpr, IsNotNullExpr, InListExpr)):
        return BOOLEAN
    if isinstance(e, NegativeExpr):
        return expr_type(e.expr, schema)
    if isinstance(e, ScalarFunctionExpr):
        if e.fun == "nullif":
            return expr_type(e.args[0], schema)
        if e.fun == "date_trunc":
            return expr_type(e.args[1], schema)
        if e.fun == "to_timestamp":
            return TIMESTAMP_NS
        if e.fun == "concat" or e.fun in SUBSTRING_FUNCTIONS:
            return UTF8
        if e.fun in ("char_length", "strpos", "date_part"):
            return INT32
        if e.fun == "starts_with":
            return BOOLEAN
        return UTF8 if e.fun in STRING_FUNCTIONS else BINARY if e.fun in SHA_FUNCTIONS else INT32 if e.fun == "octet_length" else FLOAT64
    raise TypeError(f"not a PhysicalExpr: {e!r}")


def coerce(e: PhysicalExpr, schema: dict) -> PhysicalExpr:
    """Insert the casts DataFusion's physical planner inserts so that both sides of every
    BinaryExpr / InList / Case branch have one type (numeric literals and columns are
    widened towards the higher-ranked side; e.g. Int64 literal 1 -> Float64)."""
    def cast_to(x, t):
        if expr_type(x, schema) == t:
            return x
        if isinstance(x, Literal) and x.value is not None and (t in _NUMERIC_RANK or t in _TEMPORAL) and x.dtype in _NUMERIC_RANK:
            # a numeric literal is re-typed when the value survives; otherwise it stays a CAST (NULL at run time)
            if t in (FLOAT64, FLOAT32):
                import struct
                v = float(x.value)
                return Literal(struct.unpack("f", struct.pack("f", v))[0] if t == FLOAT32 else v, t)
            if not isinstance(x.value, float) or float(x.value).is_integer():
                v = int(x.value)
                if _INT_RANGE[t][0] <= v <= _INT_RANGE[t][1]:
                    return Literal(v, t)
        return CastExpr(x, t)

    def common(a, b):
        if a == b:
            return a
        if a in _NUMERIC_RANK and b in _NUMERIC_RANK:
            return a if _NUMERIC_RANK[a] >= _NUMERIC_RANK[b] else b
        if a in _TEMPORAL and b in _NUMERIC_RANK and b not in (FLOAT64, FLOAT32):
            return a
        if b in _TEMPORAL and a in _NUMERIC_RANK and a not in (FLOAT64, FLOAT32):
            return b
        raise TypeError(f"cannot coerce {a} and {b}")

    if isinstance(e, BinaryExpr):
        l, r = coerce(e.left, schema), coerce(e.right, schema)
        if e.op in ARITH_OPS or e.op in COMPARE_OPS:
            t = common(expr_type(l, schema), expr_type(r, schema))
            l, r = cast_to(l, t), cast_to(r, t)
        return BinaryExpr(l, e.op, r)
    if isinstance(e, CastExpr):
        return CastExpr(coerce(e.expr, schema), e.dtype)
    if isinstance(e, NotExpr):
        return NotExpr(coerce(e.expr, schema))
    if isinstance(e, IsNullExpr):
        return IsNullExpr(coerce(e.expr, schema))
    if isinstance(e, IsNotNullExpr):
        return IsNotNullExpr(coerce(e.expr, schema))
    if isinstance(e, NegativeExpr):
        return NegativeExpr(coerce(e.expr, schema))
    if isinstance(e, InListExpr):
        x = coerce(e.expr, schema)
        t = expr_type(x, schema)
        return InListExpr(x, [cast_to(coerce(v, schema), t) for v in e.list], e.negated)
    if isinstance(e, CaseExpr):
        base = coerce(e.expr, schema) if e.expr is not None else None
        wt = [(coerce(w, schema), coerce(t, schema)) for w, t in e.when_then]
        el = coerce(e.else_expr, schema) if e.else_expr is not None else None
        t = expr_type(wt[0][1], schema)
        for _, th in wt[1:]:
            t = common(t, expr_type(th, schema))
        if el is not None:
            t = common(t, expr_type(el, schema))
        wt = [(w if base is None else cast_to(w, expr_type(base, schema)), cast_to(th, t)) for w, th in wt]
        return CaseExpr(base, wt, cast_to(el, t) if el is not None else None)
    if isinstance(e, ScalarFunctionExpr):
        if e.fun == "nullif":
            # the two sides of `a = b`: one common type, which is the result's
            a, b = (coerce(x, schema) for x in e.args)
            ta, tb = expr_type(a, schema), expr_type(b, schema)
            if UTF8 not in (ta, tb):
                t = common(ta, tb)
                a, b = cast_to(a, t), cast_to(b, t)
            return ScalarFunctionExpr("nullif", [a, b])
        if e.fun in SUBSTRING_FUNCTIONS:
            # start, count, n: integers of any width, brought to Int64 like a side of a comparison
            s, *ints = (coerce(x, schema) for x in e.args)
            return ScalarFunctionExpr(e.fun, [s] + [cast_to(x, INT64) if expr_type(x, schema) in _NUMERIC_RANK and
                                                    expr_type(x, schema) not in (FLOAT64, FLOAT32) else x for x in ints])
        if e.fun not in MATH_FUNCTIONS:
            return ScalarFunctionExpr(e.fun, [coerce(a, schema) for a in e.args])
        return ScalarFunctionExpr(e.fun, [cast_to(coerce(a, schema), FLOAT64) for a in e.args])
    return e
