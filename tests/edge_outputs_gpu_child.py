"""The cases of test_batch_plumbing_gpu.py::test_zero_and_word_edge_outputs: one batch of every column kind (Int32, Int64, Float64,
Boolean, Utf8, all nullable) of 0, 1, 63, 64 and 65 rows pushed through the operators that allocate their own output columns, each
result exported with to_pyarrow() and compared to pyarrow computing the same on the CPU: values, validity, and for Utf8 the offsets
(n + 1 of them, from 0, in step with the values).

Imported by that test; started by it as a program with BHIP_NO_ROWSORT=1 in the environment (the library reads the switch once) for
the sort cases off the rowsort route: never collected by pytest (no test_ prefix)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import pyarrow.compute as pc  # noqa: E402

import ballista_amd as ba  # noqa: E402
from ballista_amd import expr as E  # noqa: E402
from ballista_amd.expr import col, lit  # noqa: E402

ROW_COUNTS = [0, 1, 63, 64, 65]
TYPES = [("i32", "Int32", pa.int32()), ("i64", "Int64", pa.int64()), ("f64", "Float64", pa.float64()), ("b", "Boolean", pa.bool_()),
         ("s", "Utf8", pa.string())]
STRINGS = ["", "Ab", "cDe", "XyZzY!"]


def columns(n, prefix=""):
    """-> [(name, type name, values, validity)]: NULLs in every column (from 2 rows on), at other rows in each; i32 and i64 hold no
    value twice, so that (i32, i64) orders the rows but for ties between NULLs, which a stable sort leaves in input order"""
    i = np.arange(n)
    vals = [(i * 7919 % 1009 - 500).astype(np.int32), (i * 1000003 - 31).astype(np.int64), (i % 17 - 8) * 0.5, i % 3 == 0,
            [STRINGS[k % 4] for k in range(n)]]
    valid = [i % 7 != 1, i % 5 != 3, i % 4 != 2, i % 6 != 4, i % 9 != 5]
    if n == 1:
        valid[0] = np.zeros(1, bool)               # the one row: a NULL in the first column, values in the others
    return [(prefix + name, t, v, ok) for (name, t, _), v, ok in zip(TYPES, vals, valid)]


def device(ctx, cols):
    return ba.RecordBatch.from_columns(ctx, cols)


def table(cols):
    """the same rows as a pyarrow table"""
    types = {t: a for _, t, a in TYPES}
    return pa.table([pa.array(list(v), types[t], mask=~ok) for _, t, v, ok in cols], names=[name for name, _, _, _ in cols])


def check_offsets(arrow):
    """every Utf8 column of an exported batch: n + 1 offsets from 0, a valid row's step the byte length of its value"""
    n = arrow.num_rows
    for a in arrow.columns:
        if a.type != pa.string():
            continue
        off = np.frombuffer(a.buffers()[1], np.int32)[:n + 1]
        assert len(off) == n + 1 and off[0] == 0 and (np.diff(off) >= 0).all(), off
        want = [None if v is None else len(v.encode()) for v in a.to_pylist()]
        assert all(w is None or w == d for w, d in zip(want, np.diff(off).tolist())), (off, want)


def collect(plan_or_batches):
    """-> the device's rows as one pyarrow table (None when it yields no batch at all), every batch's offsets checked on the way"""
    batches = plan_or_batches if isinstance(plan_or_batches, list) else plan_or_batches.collect()
    arrow = [b.to_pyarrow() for b in batches]
    for a, b in zip(arrow, batches):
        assert a.num_rows == b.num_rows
        check_offsets(a)
    return pa.Table.from_batches(arrow) if arrow else None


def rows(t):
    return list(zip(*[c.to_pylist() for c in t.columns])) if t.num_columns else []


def order_key(row):
    return tuple((v is None, 0 if v is None else v) for v in row)


def assert_same(got, want, what, ordered=True):
    """values and validity, column by column (by position: the names are the operators' business); an operator may yield nothing
    for no rows"""
    if got is None:
        assert want.num_rows == 0, what
        return
    assert got.num_rows == want.num_rows and got.num_columns == want.num_columns, what
    assert [c.type for c in got.columns] == [c.type for c in want.columns], what
    assert [c.null_count for c in got.columns] == [c.null_count for c in want.columns], what
    g, w = rows(got), rows(want)
    if not ordered:
        g, w = sorted(g, key=order_key), sorted(w, key=order_key)
    assert g == w, what


SORT_KEYS = [("i32", "ascending", "at_end"), ("i64", "ascending", "at_end")]


def sort_case(ctx, n):
    """ORDER BY i32, i64 NULLS LAST"""
    cols = columns(n)
    plan = ba.SortExec([E.PhysicalSortExpr(col("i32"), False, False), E.PhysicalSortExpr(col("i64"), False, False)],
                       ba.MemoryExec([[device(ctx, cols)]], ctx))
    t = table(cols)
    assert_same(collect(plan), t.take(pc.sort_indices(t, SORT_KEYS)), ("sort", n))


def projection_case(ctx, n):
    cols = columns(n)
    schema = {name: t for name, t, _, _ in cols}
    exprs = [(col("i64") + col("i64"), "twice"), (E.coerce(col("i32") > lit(0, "Int32"), schema), "positive"),
             (E.ScalarFunctionExpr("lower", [col("s")]), "low"), (col("f64"), "f64")]
    t = table(cols)
    want = pa.table([pc.add(t["i64"], t["i64"]), pc.greater(t["i32"], pa.scalar(0, pa.int32())), pc.utf8_lower(t["s"]), t["f64"]],
                    names=["twice", "positive", "low", "f64"])
    assert_same(collect(ba.ProjectionExec(exprs, ba.MemoryExec([[device(ctx, cols)]], ctx))), want, ("projection", n))


def concat_case(ctx, n):
    cols = columns(n)
    rb, none = device(ctx, cols), device(ctx, columns(0))
    for what, parts in (("before", [none, rb]), ("after", [rb, none]), ("both", [none, rb, none])):
        assert_same(collect([ba.plan.concat(ctx, parts)]), table(cols), ("concat", what, n))


def left_join_case(ctx, n):
    """nothing on the right: every left row once, with a NULL in every right column"""
    cols, right = columns(n), columns(0, "r_")
    plan = ba.HashJoinExec(ba.MemoryExec([[device(ctx, cols)]], ctx), ba.MemoryExec([[device(ctx, right)]], ctx), [("i64", "r_i64")],
                           ba.plan.LEFT)
    t = table(cols)
    nulls = [pa.nulls(n, a) for _, _, a in TYPES]
    want = pa.table(t.columns + nulls, names=t.column_names + [name for name, _, _, _ in right])
    assert_same(collect(plan), want, ("left join", n), ordered=False)


def aggregate_case(ctx, n):
    """GROUP BY b, s (NULL is a group of its own): COUNT(i32), SUM(i64), MIN(f64), MAX(i32); the Partial states are the values"""
    cols = columns(n)
    aggs = [E.Count(col("i32"), "c"), E.Sum(col("i64"), "t"), E.Min(col("f64"), "lo"), E.Max(col("i32"), "hi")]
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("b"), "b"), (col("s"), "s")], aggs, ba.MemoryExec([[device(ctx, cols)]], ctx))
    g = table(cols).group_by(["b", "s"], use_threads=False).aggregate([("i32", "count"), ("i64", "sum"), ("f64", "min"), ("i32", "max")])
    want = pa.table([g["b"], g["s"], g["i32_count"].cast(pa.uint64()), g["i64_sum"], g["f64_min"], g["i32_max"]],
                    names=["b", "s", "c", "t", "lo", "hi"])
    assert_same(collect(plan), want, ("aggregate", n), ordered=False)


def main():
    assert os.environ["BHIP_NO_ROWSORT"] == "1"
    ctx = ba.Context(0)
    for n in ROW_COUNTS:
        sort_case(ctx, n)
    print("OK norowsort", len(ROW_COUNTS))


if __name__ == "__main__":
    main()
