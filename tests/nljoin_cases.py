"""TEST INFRASTRUCTURE shared by test_nljoin_plan.py (CPU), test_nljoin_gpu.py and nljoin_gpu_child.py: the inputs, the predicates and
the EXPECTED rows of NestedLoopJoinExec.

A build row and a probe row are partners when the filter is TRUE for the pair (no filter: always).  The expected pairs are the numpy
cross product of the two sides' row numbers filtered by the CPU oracle's expression evaluator; the rows of all eight join types follow
from the pairs (join_filter_cases.from_pairs).  test_nljoin_plan.py checks that derivation against a nested loop in plain Python
(join_filter_cases.nested_loop_pairs) for every predicate below, so the witness is not the evaluator alone.  Rows compare as multisets
keyed by the row ids li / ri, floats by bit pattern."""
import functools
import operator
import os
import re
from collections import OrderedDict

import numpy as np

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle import engine as og
from oracle.engine import OCol

import helpers
import join_filter_cases as JF
import join_types_cases as JT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TYPES = JF.ALL_TYPES
ONE_PARTITION = (JF.LEFT, JT.FULL, JT.SEMI, JT.ANTI)          # a build row's fate depends on every probe row
PYOP = {"Eq": operator.eq, "NotEq": operator.ne, "Lt": operator.lt, "LtEq": operator.le, "Gt": operator.gt, "GtEq": operator.ge}
FLIP = {"Eq": "Eq", "NotEq": "NotEq", "Lt": "Gt", "LtEq": "GtEq", "Gt": "Lt", "GtEq": "LtEq"}
I32, I64, U63 = 2 ** 31, 2 ** 63, 2 ** 63
NAN, INF = float("nan"), float("inf")
WORDS = JF.WORDS


def header_constant(name):
    """a constexpr of csrc/nljoin_kernels.h"""
    text = open(os.path.join(ROOT, "ballista_amd", "csrc", "nljoin_kernels.h")).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return int(eval(m.group(1).replace("ull", ""), {}))


TILE = header_constant("NLJ_BUILD_TILE")

# the value pools of the typed column pairs (l<x> on the build side, r<x> on the probe side): every edge the compare can get wrong
POOLS = OrderedDict([
    ("a", ("Int32", [-I32, -1, 0, 1, 7, I32 - 1])),
    ("d", ("Date32", [-I32, 9000, 9001, 10471, I32 - 1])),
    ("b", ("Int64", [-I64, -1, 0, 1, 5, I64 - 1])),
    ("u", ("UInt64", [0, 1, U63 - 1, U63, U63 + 1, 2 ** 64 - 1])),
    ("f", ("Float64", [NAN, -INF, -1.5, -0.0, 0.0, 2.5, INF])),
    ("g", ("Float32", [NAN, -INF, -0.0, 0.0, 1.25, 3.0e38, INF])),
])


@functools.lru_cache(maxsize=None)
def sides(nulls, nl, nr, seed=5):
    """-> (left, right): nl build rows and nr probe rows.  l<x> / r<x>: the typed pairs of POOLS; lx, rlo, rhi: the band
    (rlo <= lx < rhi, a width of 0 .. 2 around a value of lx's range); lz / rz, ls / rs, ry, li / ri: the columns of
    join_filter_cases.PREDICATES; l0 = 0 and r1 = 1 without NULLs.  nulls: about 15 % NULL in every typed column and in lz / rz, and
    rows 63 and 64 (one validity word's last row and the next one's first) NULL in la / ra.  One object per argument list: never modified"""
    rng = np.random.default_rng(seed + 31 * nl + nr)

    def side(p, n):
        s = OrderedDict()
        for x, (t, pool) in POOLS.items():
            vals = np.array(pool, dtype=og.NP_TYPES[t])[rng.integers(0, len(pool), n)]
            valid = rng.random(n) > 0.15 if nulls else None
            if nulls and x == "a" and n > 64:
                valid[[63, 64]] = False
            s[p + x] = OCol(t, vals, valid)
        s[p + "z"] = OCol("Int32", rng.integers(0, 6, n).astype(np.int32), (rng.random(n) > 0.15) if nulls else None)
        s[p + "s"] = OCol("Utf8", [WORDS[int(i)] for i in rng.integers(0, len(WORDS), n)])
        return s
    left, right = side("l", nl), side("r", nr)
    left["lx"] = OCol("Float64", rng.integers(0, 1000, nl) / 8.0)
    left["l0"] = OCol("Int64", np.zeros(nl, np.int64))
    lo = rng.integers(0, 1000, nr) / 8.0
    right["rlo"] = OCol("Float64", lo)
    right["rhi"] = OCol("Float64", lo + rng.integers(0, 17, nr) / 8.0)
    right["ry"] = OCol("Int64", rng.integers(0, 10 ** 6, nr))
    right["r1"] = OCol("Int64", np.ones(nr, np.int64))
    return JT.with_ids("l", nl, left.items()), JT.with_ids("r", nr, right.items())


def schema_of(left, right):
    return JF.inner_schema(left, right, [])


# ---- predicates ----------------------------------------------------------------------------------------------------------------------
# a fused-route case: terms (build column, op, probe column, right_first) meaning `build op probe`; right_first writes the same term
# as `probe FLIP[op] build`

def terms_expr(terms):
    e = None
    for lc, op, rc, right_first in terms:
        t = E.BinaryExpr(col(rc), FLIP[op], col(lc)) if right_first else E.BinaryExpr(col(lc), op, col(rc))
        e = t if e is None else e.and_(t)
    return e


def terms_pred(terms):
    """the same conjunction over one build row and one probe row as dicts of Python values: True / False / None (Kleene AND)"""
    def f(l, r):
        res = True
        for lc, op, rc, _ in terms:
            a, b = l[lc], r[rc]
            t = None if a is None or b is None else bool(PYOP[op](a, b))
            if t is False:
                return False
            res = None if t is None else res
        return res
    return f


FUSED = OrderedDict()
for _x in POOLS:
    for _op in PYOP:
        FUSED["%s_%s" % (_x, _op)] = [("l" + _x, _op, "r" + _x, False)]
FUSED["right_first"] = [("lb", "Lt", "rb", True)]
FUSED["band"] = [("lx", "GtEq", "rlo", True), ("lx", "Lt", "rhi", False)]                   # rlo <= lx AND lx < rhi: sparse
FUSED["two_terms"] = [("la", "LtEq", "ra", False), ("lz", "NotEq", "rz", False)]
FUSED["four_terms"] = [("la", "LtEq", "ra", False), ("lf", "NotEq", "rf", False), ("lu", "GtEq", "ru", True), ("ld", "GtEq", "rd", False)]
FUSED["none"] = [("lb", "Lt", "rb", False), ("lb", "Gt", "rb", False)]
FUSED["all"] = [("l0", "Lt", "r1", False)]
# what the fused kernel declines: arithmetic, Utf8, one-sided terms, constants over a column
GENERAL = OrderedDict((n, JF.PREDICATES[n]) for n in ("two_sided", "utf8", "probe_only", "build_only", "never", "always"))
GENERAL["mixed"] = (terms_expr(FUSED["band"]).and_(col("ry") < E.lit(900000)),
                    lambda l, r: terms_pred(FUSED["band"])(l, r) is True and r["ry"] < 900000)
CASES = OrderedDict([(n, (terms_expr(t), terms_pred(t), "compare")) for n, t in FUSED.items()] +
                    [(n, (e, p, "general")) for n, (e, p) in GENERAL.items()])

_COERCED = {}


def predicate(name, left, right):
    """the case's expression coerced against the sides' Inner schema; one object per (name, schema), so that pairs() is shared"""
    schema = schema_of(left, right)
    key = (name, tuple(schema.items()))
    if key not in _COERCED:
        _COERCED[key] = E.coerce(CASES[name][0], dict(schema))
    return _COERCED[key]


def columns_of(e):
    """the column names an expression tree reads"""
    if type(e).__name__ == "Column":
        return {e.name}
    out = set()
    for v in vars(e).values():
        for x in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(x, E.PhysicalExpr):
                out |= columns_of(x)
    return out


# ---- expected rows -------------------------------------------------------------------------------------------------------------------

_PAIRS = {}


def pairs(left, right, flt):
    """(li, ri): the partner pairs as row numbers, probe-major (pair p = ri * nL + li, ascending) — the numpy cross product of the row
    numbers through the oracle's evaluator; flt None: all of them.  Computed once per (sides, filter object)"""
    key = (id(left), id(right), id(flt))
    if key not in _PAIRS:
        nl, nr = og.batch_len(left), og.batch_len(right)
        li, ri = np.tile(np.arange(nl, dtype=np.int64), nr), np.repeat(np.arange(nr, dtype=np.int64), nl)
        if flt is not None and len(li):
            used = columns_of(flt)
            both = OrderedDict([(k, c.take(li)) for k, c in left.items() if k in used] + [(k, c.take(ri)) for k, c in right.items() if k in used])
            p = og.evaluate(flt, both)
            assert p.dtype == "Boolean"
            keep = p.values.astype(np.bool_) & p.is_valid()
            li, ri = li[keep], ri[keep]
        _PAIRS[key] = (left, right, flt, li, ri)
    return _PAIRS[key][3:]


def expected(jt, left, right, flt):
    li, ri = pairs(left, right, flt)
    return JF.from_pairs(jt, left, right, [], li, ri)


def bit_patterns(batch):
    """float columns as the integers of their bits: NaN equals NaN of the same bits, -0.0 differs from +0.0"""
    out = OrderedDict()
    for k, c in batch.items():
        if c.dtype in ("Float64", "Float32"):
            wide = c.dtype == "Float64"
            c = OCol("Int64" if wide else "Int32", np.ascontiguousarray(c.values).view(np.int64 if wide else np.int32), c.valid)
        out[k] = c
    return out


def assert_same_rows(got, want):
    if got and want:
        assert [c.dtype for c in got.values()] == [c.dtype for c in want.values()]
    JT.assert_same_rows(bit_patterns(got), bit_patterns(want))


# ---- plans ---------------------------------------------------------------------------------------------------------------------------

PROBE_BATCHES = [0, 1, 63, 64, 65, 255, 256, 257, 1025]        # rows of the probe batches of the shape tests, in this order
NR_SHAPES = sum(PROBE_BATCHES)


def build_exec(ctx, left):
    """the build rows in two partitions"""
    n = og.batch_len(left)
    cut = n // 3
    return helpers.memory_exec(ctx, [[helpers.slice_batch(left, 0, cut)], [helpers.slice_batch(left, cut, n)]])


def probe_exec(ctx, right, jt, batch_rows=None, merge=False):
    """the probe rows cut into batches of batch_rows (default: three about equal ones), the first half of the batches in one
    partition and the rest in another; the types that need one right partition get them all in one, or (merge) the two under a MergeExec"""
    n = og.batch_len(right)
    batch_rows = batch_rows or [n // 3, n // 3, n - 2 * (n // 3)]
    assert sum(batch_rows) == n
    cuts = np.concatenate([[0], np.cumsum(batch_rows)])
    b = [helpers.slice_batch(right, int(lo), int(hi)) for lo, hi in zip(cuts, cuts[1:])]
    h = (len(b) + 1) // 2
    if jt in ONE_PARTITION and not merge:
        return helpers.memory_exec(ctx, [b])
    two = helpers.memory_exec(ctx, [b[:h], b[h:]])
    return ba.MergeExec(two) if jt in ONE_PARTITION else two


def join_plan(ctx, left, right, jt, flt, batch_rows=None, merge=False):
    return ba.NestedLoopJoinExec(build_exec(ctx, left), probe_exec(ctx, right, jt, batch_rows, merge), jt, filter=flt)


def check(ctx, left, right, jt, flt, form, batch_rows=None, merge=False):
    got = JF.rows(join_plan(ctx, left, right, jt, flt, batch_rows, merge))
    assert_same_rows(got, expected(jt, left, right, flt))
    if form is not None:
        assert ctx.nested_loop_form() == form, (ctx.nested_loop_form(), form)
    return got


# ---- the case lists that run in process and, under a switch, in a child process (nljoin_gpu_child.py) ----------------------------------

NL, NR = 150, 400                                               # the value and general-route cases: 60000 pairs


def value_cases():
    """(name, nulls, join type): every fused predicate as Inner with and without NULLs, and — spread over the cases — the other types"""
    others = [t for t in ALL_TYPES if t != JF.INNER]
    out = []
    for i, name in enumerate(FUSED):
        out += [(name, False, JF.INNER), (name, True, JF.INNER), (name, True, others[i % len(others)])]
    return out


def general_cases():
    return [(name, True, jt) for name in GENERAL for jt in ALL_TYPES]


def run_case(ctx, name, nulls, jt, form):
    left, right = sides(nulls, NL, NR)
    return check(ctx, left, right, jt, predicate(name, left, right), form, merge=nulls and jt in (JT.FULL, JT.ANTI))
