"""TEST INFRASTRUCTURE shared by test_join_filter_plan.py (CPU) and test_join_filter_gpu.py: the inputs, the predicates and the EXPECTED
rows of HashJoinExec with a residual join filter.

A build row and a probe row are partners when their keys are equal AND the filter is TRUE.  The expected rows of all eight join
types are derived from the kept pairs: the CPU oracle's Inner join (which carries the row ids li / ri) filtered by the oracle's
expression evaluator, plus the rows of either side that are left without a partner.  test_join_filter_plan.py checks this derivation
against a nested loop in plain Python, so it has a witness that is neither the oracle's join, nor its evaluator, nor the product."""
import functools
from collections import OrderedDict

import numpy as np

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og
from oracle.engine import OCol

import helpers
import join_types_cases as JT
import plan_nodes as N
import proto_encode as pe

INNER, LEFT, RIGHT = "Inner", "Left", "Right"
ALL_TYPES = [INNER, LEFT, RIGHT] + JT.TYPES
BUILD_SIDE, PROBE_SIDE = (JT.SEMI, JT.ANTI), (JT.RIGHT_SEMI, JT.RIGHT_ANTI)
FORMS = ["int64_unique", "int64_dup", "hot_key", "int32_date32", "utf8_long"]
WORDS = ["", "a", "ab", "b", "ba", "m", "mm", "z", "zebra", "Zebra"]


@functools.lru_cache(maxsize=None)
def sides(form, nulls, seed=3, nl=JT.NL, nr=JT.NR):
    """join_types_cases.sides plus two nullable Int32 columns (lz / rz, about 15 % NULL each) and two short Utf8 columns (ls / rs).
    One object per argument list: the tests share the sides and never modify them"""
    left, right, on = JT.sides(form, nulls, seed, nl, nr)
    rng = np.random.default_rng(1000 + seed + 17 * JT.FORMS.index(form))
    left, right = OrderedDict(left), OrderedDict(right)
    left["lz"] = OCol("Int32", rng.integers(0, 6, nl).astype(np.int32), rng.random(nl) > 0.15)
    right["rz"] = OCol("Int32", rng.integers(0, 6, nr).astype(np.int32), rng.random(nr) > 0.15)
    left["ls"] = OCol("Utf8", [WORDS[int(i)] for i in rng.integers(0, len(WORDS), nl)])
    right["rs"] = OCol("Utf8", [WORDS[int(i)] for i in rng.integers(0, len(WORDS), nr)])
    return left, right, on


def inner_schema(left, right, on):
    """name -> Arrow type name of the Inner join's output: what the filter is typed (and coerced) against"""
    drop = {b for a, b in on if a == b}
    s = OrderedDict((k, c.dtype) for k, c in left.items())
    for k, c in right.items():
        if k not in drop:
            s[k] = c.dtype
    return s


# name -> (expression, the same predicate over one build row and one probe row as dicts of Python values: True / False / None)
PREDICATES = OrderedDict([
    ("two_sided", (col("lx") * lit(8000.0) > col("ry"), lambda l, r: l["lx"] * 8000.0 > float(r["ry"]))),
    ("nullable_ne", (col("lz").ne(col("rz")), lambda l, r: None if l["lz"] is None or r["rz"] is None else l["lz"] != r["rz"])),
    ("probe_only", (col("ry") < lit(500000), lambda l, r: r["ry"] < 500000)),
    ("build_only", (col("lx") >= lit(60.0), lambda l, r: l["lx"] >= 60.0)),
    ("utf8", (col("ls") < col("rs"), lambda l, r: l["ls"].encode() < r["rs"].encode())),
    ("never", (col("li") < lit(0), lambda l, r: False)),
    ("always", (col("li") >= lit(0), lambda l, r: True)),
])


_COERCED = {}


def predicate(name, left, right, on):
    """the predicate coerced against the sides' Inner schema; one object per (name, schema), so that kept_pairs is shared"""
    schema = inner_schema(left, right, on)
    key = (name, tuple(schema.items()))
    if key not in _COERCED:
        _COERCED[key] = E.coerce(PREDICATES[name][0], dict(schema))
    return _COERCED[key]


def _gather(c, idx):
    safe = np.where(idx < 0, 0, idx)
    if len(c) == 0:
        return OCol(c.dtype, ["" if c.dtype == "Utf8" else 0] * len(idx), np.zeros(len(idx), np.bool_))
    t = c.take(safe)
    return OCol(c.dtype, t.values, t.is_valid() & (idx >= 0))


def rows_of_pairs(left, right, on, li, ri):
    """the join's output rows for build rows li and probe rows ri (-1: no row of that side, NULL columns)"""
    li, ri = np.asarray(li, np.int64), np.asarray(ri, np.int64)
    drop = {b for a, b in on if a == b}
    out = OrderedDict((k, _gather(c, li)) for k, c in left.items())
    for k, c in right.items():
        if k not in drop:
            out[k] = _gather(c, ri)
    return out


def from_pairs(jt, left, right, on, li, ri):
    """all eight join types from the partner pairs (li[i], ri[i]) and the two sides"""
    li, ri = np.asarray(li, np.int64), np.asarray(ri, np.int64)
    nl, nr = og.batch_len(left), og.batch_len(right)
    lhas, rhas = np.zeros(nl, np.bool_), np.zeros(nr, np.bool_)
    lhas[li] = True
    rhas[ri] = True
    if jt in BUILD_SIDE:
        return JT.rows_where(left, lhas if jt == JT.SEMI else ~lhas)
    if jt in PROBE_SIDE:
        return JT.rows_where(right, rhas if jt == JT.RIGHT_SEMI else ~rhas)
    lone_l = np.nonzero(~lhas)[0] if jt in (LEFT, JT.FULL) else np.zeros(0, np.int64)
    lone_r = np.nonzero(~rhas)[0] if jt in (RIGHT, JT.FULL) else np.zeros(0, np.int64)
    minus = lambda n: np.full(n, -1, np.int64)
    return rows_of_pairs(left, right, on, np.concatenate([li, lone_l, minus(len(lone_r))]), np.concatenate([ri, minus(len(lone_l)), lone_r]))


_KEPT = {}


def _positions(side_ids, ids):
    """the rows of a side by their row ids (a sliced or filtered side's ids are not its row numbers)"""
    order = np.argsort(side_ids, kind="stable")
    return order[np.searchsorted(side_ids[order], ids)].astype(np.int64)


def kept_pairs(left, right, on, flt):
    """(candidates, li, ri): the number of key-equal pairs and the pairs the filter keeps (TRUE and valid) as ROW NUMBERS of the two
    sides; flt None: all of them.
    Computed once per (sides, filter object): pass the same objects to share it"""
    key = (id(left), id(right), tuple(on), id(flt))
    if key not in _KEPT:
        inner = JT.oracle_join(left, right, on, INNER)
        n = og.batch_len(inner)
        keep = np.ones(n, np.bool_)
        if flt is not None and n:
            p = og.evaluate(flt, inner)
            assert p.dtype == "Boolean"
            keep = p.values.astype(np.bool_) & p.is_valid()
        ids = (_positions(left["li"].values, inner["li"].values[keep]), _positions(right["ri"].values, inner["ri"].values[keep])) if n else \
            (np.zeros(0, np.int64), np.zeros(0, np.int64))
        _KEPT[key] = (left, right, flt, n, ids[0], ids[1])
    return _KEPT[key][3:]


def expected(jt, left, right, on, flt):
    """the rows of HashJoinExec(left, right, on, jt, flt); both sides carry their row ids li / ri"""
    _, li, ri = kept_pairs(left, right, on, flt)
    return from_pairs(jt, left, right, on, li, ri)


# ---- plans -------------------------------------------------------------------------------------------------------------------------------

def build_exec(ctx, left):
    """the build rows in two partitions"""
    n = og.batch_len(left)
    cut = min(400, n)
    return helpers.memory_exec(ctx, [[helpers.slice_batch(left, 0, cut)], [helpers.slice_batch(left, cut, n)]])


def probe_exec(ctx, right, partitions):
    """the probe rows cut at JT.CUTS: 2: two partitions (two batches, one batch); 1: one partition; "merge": the two under a MergeExec"""
    n = og.batch_len(right)
    b = [helpers.slice_batch(right, lo, hi) for lo, hi in zip(JT.CUTS, JT.CUTS[1:]) if lo < n or lo == 0]
    if partitions == 1:
        return helpers.memory_exec(ctx, [b])
    two = helpers.memory_exec(ctx, [b[:2], b[2:]])
    return ba.MergeExec(two) if partitions == "merge" else two


def rows(plan):
    return helpers.concat(helpers.collect_product(plan))


_NP = {"Int64": np.int64, "Int32": np.int32, "Date32": np.int32, "Float64": np.float64}


def decoded_leaf(name, cols):
    """a leaf of the schema cols = [(name, type, nullable)] that needs no device: an empty scan, encoded and decoded as a wire plan"""
    m = N.MemoryExec([[OrderedDict((n, OCol(t, [] if t == "Utf8" else np.zeros(0, _NP[t]), np.zeros(0, np.bool_) if u else None)) for n, t, u in cols)]],
                     schema=cols)
    m.name = "mem://" + name
    return ba.ExecutionPlan.from_proto(None, pe.plan(m))


def nested_loop_pairs(left, right, on, py_pred):
    """the partner pairs by the definition: every build row against every probe row, in plain Python"""
    lrows = [dict(zip(left.keys(), r)) for r in zip(*[c.to_pylist() for c in left.values()])]
    rrows = [dict(zip(right.keys(), r)) for r in zip(*[c.to_pylist() for c in right.values()])]
    li, ri = [], []
    for j, r in enumerate(rrows):
        for i, l in enumerate(lrows):
            if all(l[a] is not None and r[b] is not None and l[a] == r[b] for a, b in on) and py_pred(l, r) is True:
                li.append(i)
                ri.append(j)
    return li, ri
