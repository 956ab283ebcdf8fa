"""The code between operators on the device, at bitmap-word and offset edges: concat_batches (copy_bits_kernel, rebase_offsets_kernel;
host/ops_basic.cpp), the zero-copy head slice of LimitExec, and CoalesceBatchesExec / LimitExec / MergeExec as stream operators.

Cases and expected values: tests/batch_plumbing_cases.py (numpy concatenation and slicing of the inputs; test_batch_plumbing_cpu.py
proves that the part lists reach the alignments).  Every comparison is bit for bit (helpers.assert_bit_exact: validity, and under it the
values as unsigned integers of their width, so NaN payloads and the sign of zero count).  Rows compare in order wherever the operator
defines one; a join's rows are matched by the row ids both sides carry, a grouped aggregate's by the group key.  Sums are over integers.

The contract of part 2: a head slice keeps the buffers of the longer batch, so its validity and Boolean words still hold
the bits of the rows past the cut — no operator's result may depend on them.  Variant A leaves ones there, variant B zeros."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd._lib import EINVAL
from ballista_amd.expr import col, lit
from oracle import engine as og, plan_eval

import batch_plumbing_cases as K
import helpers
import join_types_cases as JT
import window_cases as WC

pytestmark = pytest.mark.gpu


def memory(ctx, partitions, oracle_partitions):
    """MemoryExec over device batches that exist already, with the oracle's view of the same rows for plan_eval"""
    m = ba.MemoryExec(partitions, ctx)
    m._oracle_partitions = [list(p) for p in oracle_partitions]
    return m


def both(plan):
    """-> (the device's rows, plan_eval's) as one batch each"""
    return helpers.concat(helpers.collect_product(plan)), plan_eval.collect(plan)


def check(plan):
    got, want = both(plan)
    helpers.assert_bit_exact(got, want)
    return got


# ---- 1. concat_batches through ba.plan.concat ------------------------------------------------------------------------------------------------

CASES = K.concat_cases()


def device_part(ctx, part):
    rb = ba.RecordBatch.from_columns(ctx, part.columns())
    if part.head is None:
        return rb
    out = ba.LocalLimitExec(ba.MemoryExec([[rb]], ctx), part.head).collect()
    assert len(out) == 1 and out[0].num_rows == part.n
    assert out[0].column_device(0)[0] == rb.column_device(0)[0]                 # a slice: the buffers of the longer batch
    return out[0]


def dirty_the_allocator(ctx, case):
    """best effort: the same concat over parts of the same sizes whose validity and Boolean bitmaps are ones (but for a validity's
    first bit: the import drops a buffer whose bits are all set) and whose value bytes are 0xFF (Utf8: 0x7F, a byte a string may hold), built and released in the same context just before the concat under test.  The
    caching allocator then has blocks of exactly the sizes the real concat asks for, full of ones, and is LIKELY to hand them back, so
    a word or byte the code forgot to write shows.  It raises the chance and guarantees nothing: which block a request gets is the
    allocator's business."""
    parts = []
    for p in case.parts:
        cols, n = [], p.rows
        ones = np.ones(n, bool)
        ones[:1] = n < 2
        for name, (t, v, _) in p.cols.items():
            if t == "Utf8":
                vals = ["\x7f" * len(s.encode()) for s in v]
            elif t == "Boolean":
                vals = np.ones(n, bool)
            else:
                vals = np.frombuffer(b"\xff" * (n * v.dtype.itemsize), dtype=v.dtype)
            cols.append((name, t, vals, ones))
        parts.append(ba.RecordBatch.from_columns(ctx, cols))
    out = ba.plan.concat(ctx, parts)
    del out, parts


def concat_case(ctx, case):
    dev = [device_part(ctx, p) for p in case.parts]
    dirty_the_allocator(ctx, case)
    return dev, ba.plan.concat(ctx, dev)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_concat(ctx, case):
    """the result read back; which columns have a validity buffer (any part's: a part without one is all valid over exactly its rows);
    the Utf8 byte counts (a head slice's bytes past its cut must not come along: the offsets end at the sum of the kept bytes)"""
    dev, rb = concat_case(ctx, case)
    want = case.expected()
    assert rb.num_rows == og.batch_len(want) == sum(case.lengths())
    assert [(n, t) for n, t in rb.schema()] == list(zip(K.NAMES, K.TYPES))
    got = helpers.from_device(rb)
    helpers.assert_bit_exact(got, want)
    for i, name in enumerate(K.NAMES):
        info = rb.column_info(i)
        assert info[4] == any(p.has_buffer(name) for p in case.parts), name
        assert info[2] == any(p.nullable(name) for p in case.parts), name         # nullable when it is in any part, whichever comes first
        if K.TYPES[i] == "Utf8":
            assert info[3] == case.expected_data_bytes(name), name
    if len(dev) == 1:                                                           # a single part comes back as it is
        assert [rb.column_device(i) for i in range(rb.num_columns)] == [dev[0].column_device(i) for i in range(rb.num_columns)]
    # the offsets buffer itself, as Arrow sees it
    arrow = rb.to_pyarrow()
    for i, name in enumerate(K.NAMES):
        if K.TYPES[i] == "Utf8":
            off = np.frombuffer(arrow.column(i).buffers()[1], np.int32)[:rb.num_rows + 1]
            lens = [len(s.encode()) for s in np.concatenate([p.kept()[name].values for p in case.parts])] if rb.num_rows else []
            assert off.tolist() == np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist(), name
        assert arrow.column(i).null_count == int((~want[name].is_valid()).sum()), name


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_concat_feeds_filter_and_count(ctx, case):
    """the concatenated batch under FilterExec(IsNotNull(c)) and an ungrouped COUNT(c), for every column that has a validity buffer"""
    cols = [n for n in K.NAMES if any(p.has_buffer(n) for p in case.parts)]
    _, rb = concat_case(ctx, case)
    m = memory(ctx, [[rb]], [[case.expected()]])
    for at in range(0, len(cols), 8):
        aggs = [E.Count(col(c), c) for c in cols[at:at + 8]] + [E.Count(lit(1, E.UINT8), "n")]
        check(ba.HashAggregateExec(ba.plan.PARTIAL, [], aggs, m))
    for c in cols:
        check(ba.FilterExec(E.IsNotNullExpr(col(c)), ba.ProjectionExec([(col(c), c)], m)))
    if not cols:                                                                # no NULL anywhere: every row counts
        got = check(ba.HashAggregateExec(ba.plan.PARTIAL, [], [E.Count(col("c16"), "c"), E.Count(col("c18"), "s")], m))
        assert got["c[count]"].values.tolist() == [rb.num_rows]


def test_concat_refuses_parts_of_another_schema(ctx):
    """the result takes the first part's schema: a part with another column count or another type at some position is refused
    (copied at the first part's width it would be read past its end).  Nullability may differ."""
    def batch(cols):
        return ba.RecordBatch.from_columns(ctx, cols)
    i32 = ("a", "Int32", np.arange(40, dtype=np.int32), None)
    a = batch([i32, ("s", "Utf8", ["x"] * 40, None)])
    for other in ([("a", "Int64", np.arange(40, dtype=np.int64), None), ("s", "Utf8", ["x"] * 40, None)],      # wider
                  [("a", "Int8", np.arange(40, dtype=np.int8), None), ("s", "Utf8", ["x"] * 40, None)],        # narrower: a read past the end
                  [i32, ("s", "Boolean", np.ones(40, bool), None)],
                  [("a", "Float32", np.zeros(40, np.float32), None), ("s", "Utf8", ["x"] * 40, None)],         # same width, another type
                  [i32], [i32, ("s", "Utf8", ["x"] * 40, None), ("t", "Int32", np.arange(40, dtype=np.int32), None)]):
        for parts in ([a, batch(other)], [batch(other), a], [a, a, batch(other)]):
            with pytest.raises(ba.BallistaError) as err:
                ba.plan.concat(ctx, parts)
            assert err.value.code == EINVAL
    nullable = batch([("a", "Int32", np.arange(3, dtype=np.int32), np.array([True, False, True])), ("s", "Utf8", ["p", "q", "r"], None)])
    assert ba.plan.concat(ctx, [a, nullable]).num_rows == 43 and ba.plan.concat(ctx, [nullable, a]).num_rows == 43


# ---- 2. the bits after a head slice ------------------------------------------------------------------------------------------------------------

SLICES = [(kind, v, k) for kind in ("local", "global") for v in K.VARIANTS for k in K.SLICE_KS]
slices = pytest.mark.parametrize("kind, variant, k", SLICES, ids=lambda x: str(x))
_DEVICE = {}


def source(ctx, variant, k):
    """the 1100-row source on the device.  Every column but rn has a validity BUFFER: the import drops one whose bits are all set
    (variant A with no NULL before a small k), so the batch is itself the 1100-row head of one whose last row is NULL everywhere"""
    if (variant, k) not in _DEVICE:
        src = K.slice_source(variant, k)
        n = K.SLICE_ROWS
        cols = []
        for name, c in src.items():
            values = np.concatenate([c.values, c.values[:1]])
            cols.append((name, c.dtype, list(values) if c.dtype == "Utf8" else values,
                         None if name == "rn" else np.concatenate([c.is_valid(), [False]])))
        longer = ba.RecordBatch.from_columns(ctx, cols)
        rb = ba.LocalLimitExec(ba.MemoryExec([[longer]], ctx), n).collect()[0]
        assert rb.num_rows == n and all(rb.column_info(i)[4] == (rb.column_info(i)[0] != "rn") for i in range(rb.num_columns))
        _DEVICE[variant, k] = (rb, src)
    return _DEVICE[variant, k]


def sliced(ctx, kind, variant, k):
    rb, src = source(ctx, variant, k)
    m = memory(ctx, [[rb]], [[src]])
    return (ba.LocalLimitExec if kind == "local" else ba.GlobalLimitExec)(m, k)


SCHEMA = dict(zip(K.NAMES, K.TYPES), rn="Int64", key="Int64", v="Int32", x="Float64")


@slices
def test_slice_reads_back(ctx, kind, variant, k):
    plan = sliced(ctx, kind, variant, k)
    out = plan.collect()
    assert len(out) == 1 and out[0].num_rows == k
    assert out[0].column_device(1) == source(ctx, variant, k)[0].column_device(1)        # zero copy: the stale bits ARE there
    got = check(plan)
    assert og.batch_len(got) == k


@slices
def test_slice_under_filters(ctx, kind, variant, k):
    s = sliced(ctx, kind, variant, k)
    check(ba.FilterExec(col("c16"), s))                                         # the Boolean column itself
    check(ba.FilterExec(E.NotExpr(col("c16")), s))
    for c in ("v", "c16", "c17", "c3"):
        check(ba.FilterExec(E.IsNullExpr(col(c)), s))
        check(ba.FilterExec(E.IsNotNullExpr(col(c)), s))
    # range predicates over nullable numeric columns (kernels_range.hip); the rows past the cut would pass both in variant A
    check(ba.FilterExec(E.coerce((col("x") > lit(-60.0)).and_(col("x") < lit(45.0)), SCHEMA), s))
    check(ba.FilterExec(E.coerce(col("v") >= lit(-20, "Int32"), SCHEMA), s))
    check(ba.FilterExec(E.coerce((col("v") >= lit(-20, "Int32")).and_(col("key") > lit(0)), SCHEMA), s))


AGGS = [E.Count(col("v"), "cv"), E.Count(col("c17"), "cs"), E.Count(col("c16"), "cb"), E.Count(lit(1, E.UINT8), "n"), E.Sum(col("v"), "sv"),
        E.Min(col("v"), "mn"), E.Max(col("v"), "mx"), E.Sum(col("key"), "sk"), E.Min(col("x"), "mnx"), E.Max(col("x"), "mxx")]


def check_aggregates(child):
    check(ba.HashAggregateExec(ba.plan.PARTIAL, [], AGGS, child))
    grouped = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("c16"), "g")], AGGS, child)
    got, want = both(grouped)
    helpers.assert_rows_equal(got, want, ordered=False, key_cols=["g"])         # float_rtol 0: MIN / MAX of doubles bit for bit


@slices
def test_slice_under_aggregates(ctx, kind, variant, k):
    check_aggregates(sliced(ctx, kind, variant, k))


@slices
def test_slice_under_filtered_aggregates(ctx, kind, variant, k):
    """an aggregate directly over a filter runs as one fused scan"""
    s = sliced(ctx, kind, variant, k)
    check_aggregates(ba.FilterExec(E.coerce(col("x") > lit(-60.0), SCHEMA), s))
    check_aggregates(ba.FilterExec(col("c16"), s))
    check_aggregates(ba.FilterExec(E.IsNotNullExpr(col("key")), s))


@slices
def test_slice_under_sort_and_topk(ctx, kind, variant, k):
    s = sliced(ctx, kind, variant, k)
    for nulls_first in (True, False):
        for desc in (False, True):
            keys = [E.PhysicalSortExpr(col("key"), desc, nulls_first), E.PhysicalSortExpr(col("rn"))]
            sort = ba.SortExec(keys, s)
            check(sort)
            for top in (10, 100):
                check(ba.GlobalLimitExec(sort, top))
    check(ba.SortExec([E.PhysicalSortExpr(col("c17"), False, False), E.PhysicalSortExpr(col("rn"))], s))


def other_side(prefix):
    """180 rows to join with: keys of the source's domain and some it never has, NULLs among them"""
    rng = np.random.default_rng(77)
    n = 180
    return OrderedDict([(prefix + "k", og.OCol("Int64", rng.integers(0, 60, n) * 1000003 - 7, rng.random(n) > 0.15)),
                        (prefix + "i", og.OCol("Int64", np.arange(n, dtype=np.int64)))])


@slices
def test_slice_under_hash_join(ctx, kind, variant, k):
    """the slice as build side and as probe side, on its nullable key; Inner, Left, Anti"""
    def narrow(idname):
        return ba.ProjectionExec([(col("rn"), idname), (col("key"), "key"), (col("v"), "v"), (col("c16"), "c16"), (col("c17"), "c17")],
                                 sliced(ctx, kind, variant, k))
    for as_build in (True, False):
        if as_build:
            left, right, on = narrow("li"), helpers.memory_exec(ctx, [[other_side("r")]]), [("key", "rk")]
        else:
            left, right, on = helpers.memory_exec(ctx, [[other_side("l")]]), narrow("ri"), [("lk", "key")]
        for jt in (ba.plan.INNER, ba.plan.LEFT):
            got, want = both(ba.HashJoinExec(left, right, on, jt))
            JT.assert_same_rows(got, want)
        got = helpers.concat(helpers.collect_product(ba.HashJoinExec(left, right, on, ba.plan.ANTI)))
        JT.assert_same_rows(got, JT.expected(JT.ANTI, plan_eval.collect(left), plan_eval.collect(right), on))


@slices
def test_slice_under_window(ctx, kind, variant, k):
    """running COUNT of nullable columns in row order"""
    s = ba.ProjectionExec([(col("rn"), "rn"), (col("v"), "v"), (col("key"), "key"), (col("c3"), "c3")], sliced(ctx, kind, variant, k))
    order = [WC.asc("rn")]
    ws = [WC.W("COUNT", c, "count_" + c, frame="ROWS_TO_CURRENT") for c in ("v", "key", "c3")] + [WC.W("SUM", "v", "sum_v", frame="PARTITION")]
    got = helpers.concat(helpers.collect_product(ba.WindowAggExec([], order, ws, s)))
    helpers.assert_bit_exact(got, WC.restate(plan_eval.collect(ba.SortExec(order, s)), [], order, ws))


@slices
def test_slice_under_hash_repartition(ctx, kind, variant, k):
    plan = ba.RepartitionExec(sliced(ctx, kind, variant, k), ba.Partitioning.Hash([col("key")], 4))
    total = 0
    for p in range(4):
        got = helpers.concat([helpers.from_device(b) for b in plan.execute(p)])
        helpers.assert_bit_exact(got, helpers.concat(plan_eval.execute(plan, p)))
        total += og.batch_len(got)
    assert total == k


@pytest.mark.parametrize("k", K.SLICE_KS)
def test_two_slices_coalesced(ctx, k):
    """CoalesceBatchesExec concatenates a slice with ones past its cut and one with zeros; then the result feeds a COUNT"""
    (a, sa), (b, sb) = source(ctx, "A", k), source(ctx, "B", k)
    lim = ba.LocalLimitExec(memory(ctx, [[a], [b]], [[sa], [sb]]), k)
    plan = ba.CoalesceBatchesExec(ba.MergeExec(lim), 10 ** 6)
    out = plan.collect()
    assert [x.num_rows for x in out] == [2 * k]
    check(plan)
    check_aggregates(plan)
    check(ba.FilterExec(col("c16"), plan))


@slices
def test_slice_packed_and_unpacked(ctx, kind, variant, k):
    plan = sliced(ctx, kind, variant, k)
    rb = plan.collect()[0]
    header, block = ba.plan.pack_batch(rb)
    back = ba.plan.unpack_batch(ctx, rb.schema3(), header, block)
    assert back.num_rows == k
    want = plan_eval.collect(plan)
    helpers.assert_bit_exact(helpers.from_device(back), want)
    check_aggregates(memory(ctx, [[back]], [[want]]))


def arrow_plain(arrow):
    """a pyarrow batch as name -> list of Python values, the temporal types as the integers they store"""
    import pyarrow as pa
    out = OrderedDict()
    for name, a in zip(arrow.schema.names, arrow.columns):
        if pa.types.is_temporal(a.type):
            a = a.cast(pa.int32() if a.type == pa.date32() else pa.int64())
        out[name] = pa.RecordBatch.from_arrays([a], names=[name]).to_pydict()[name]
    return out


def same_values(a, b):
    if isinstance(b, float) and isinstance(a, float):
        return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64) or (a != a and b != b)
    return a == b and (a is None) == (b is None)


def assert_arrow_matches(arrow, want, k):
    assert arrow.num_rows == k
    plain = arrow_plain(arrow)
    for i, (name, c) in enumerate(want.items()):
        assert arrow.column(i).null_count == int((~c.is_valid()).sum()), name
        w = c.to_pylist()
        assert len(plain[name]) == len(w) and all(same_values(x, y) for x, y in zip(plain[name], w)), name


@slices
def test_slice_to_pyarrow_and_ipc(ctx, kind, variant, k, tmp_path):
    """null_count counts validity bits: one that read the whole last word would count the rows past the cut"""
    import pyarrow as pa
    plan = sliced(ctx, kind, variant, k)
    want = plan_eval.collect(plan)
    arrow = plan.collect()[0].to_pyarrow()
    assert_arrow_matches(arrow, want, k)
    # the library's own host writer, from a pyarrow stream of that batch
    path = str(tmp_path / "host.arrow")
    stats = ba.plan.ipc_write_file(pa.RecordBatchReader.from_batches(arrow.schema, [arrow]), path)
    assert stats["num_rows"] == k
    back = pa.ipc.open_file(path).read_all().combine_chunks().to_batches()[0]
    assert back.schema.types == arrow.schema.types
    assert_arrow_matches(back, want, k)
    # and the stage writer straight from the device stream
    path = str(tmp_path / "stage.arrow")
    assert plan.execute(0).write_ipc(path)["num_rows"] == k
    assert_arrow_matches(pa.ipc.open_file(path).read_all().combine_chunks().to_batches()[0], want, k)


def test_zero_and_word_edge_outputs(ctx):
    """the columns the operators allocate themselves, at 0 rows and around a bitmap word, against pyarrow on the CPU: cases, inputs and
    comparison in edge_outputs_gpu_child.py, which runs the sort cases once more in a process that has BHIP_NO_ROWSORT=1"""
    import subprocess
    import sys
    import edge_outputs_gpu_child as EO
    for n in EO.ROW_COUNTS:
        EO.projection_case(ctx, n)
        EO.concat_case(ctx, n)
        EO.sort_case(ctx, n)
        EO.left_join_case(ctx, n)
        EO.aggregate_case(ctx, n)
    p = subprocess.run([sys.executable, EO.__file__], env=dict(EO.os.environ, BHIP_NO_ROWSORT="1"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK norowsort %d" % len(EO.ROW_COUNTS) in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---- 3. CoalesceBatchesExec, LimitExec, MergeExec as stream operators --------------------------------------------------------------------------

def stream_partitions(ctx, size_lists, seed0=0):
    """-> (MemoryExec, the oracle's batches per partition, the device batches per partition)"""
    oracle, s = [], seed0
    for sizes in size_lists:
        part = []
        for n in sizes:
            s += 1
            part.append(K.stream_batch(n, s))
        oracle.append(part)
    if not any(oracle):
        raise ValueError("no batch at all")
    dev = [[helpers.to_device(ctx, b) for b in part] for part in oracle]
    return memory(ctx, dev, oracle), oracle, dev


def assert_batches(got, want_batches):
    """the stream's batches one by one: sizes, then rows"""
    assert [og.batch_len(b) for b in got] == [og.batch_len(b) for b in want_batches]
    for g, w in zip(got, want_batches):
        helpers.assert_bit_exact(g, w)


@pytest.mark.parametrize("name", sorted(K.COALESCE_SEQUENCES))
def test_coalesce_batch_sizes_and_rows(ctx, name):
    target, size_lists = K.COALESCE_SEQUENCES[name]
    m, oracle, dev = stream_partitions(ctx, size_lists)
    plan = ba.CoalesceBatchesExec(m, target)
    assert plan.output_partitioning().count == len(size_lists) and plan.schema() == m.schema()
    for p, sizes in enumerate(size_lists):
        out = list(plan.execute(p))
        want_sizes = K.coalesce_sizes(sizes, target)
        assert [b.num_rows for b in out] == want_sizes, (name, p)
        assert_batches([helpers.from_device(b) for b in out], K.split_by_sizes(oracle[p], want_sizes))
        # a batch of at least `target` rows with nothing pending passes untouched: the same buffers
        pending = 0
        passed = []
        for i, n in enumerate(sizes):
            if n >= target and pending == 0:
                passed.append(i)
            elif n:
                pending = 0 if pending + n >= target else pending + n
        ptrs = {b.column_device(0)[0] for b in out}
        assert all(dev[p][i].column_device(0)[0] in ptrs for i in passed), (name, p, passed)


def limit_partitions(ctx):
    return stream_partitions(ctx, K.LIMIT_PARTITIONS, seed0=50)


@pytest.mark.parametrize("limit", K.LIMITS)
def test_local_limit_over_three_partitions(ctx, limit):
    m, oracle, _ = limit_partitions(ctx)
    plan = ba.LocalLimitExec(m, limit)
    assert plan.schema() == m.schema() and plan.output_partitioning().count == 3
    for p, sizes in enumerate(K.LIMIT_PARTITIONS):
        out = [helpers.from_device(b) for b in plan.execute(p)]
        want_sizes = K.limit_sizes(sizes, limit)
        assert_batches(out, K.split_by_sizes([og.limit(helpers.concat(oracle[p]), limit)] if oracle[p] else [], want_sizes))
        helpers.assert_bit_exact(helpers.concat(out) if out else OrderedDict(), helpers.concat(plan_eval.execute(plan, p)))


@pytest.mark.parametrize("limit", K.LIMITS + [629 + 129, 629 + 130])
def test_global_limit_over_merge(ctx, limit):
    m, oracle, _ = limit_partitions(ctx)
    plan = ba.GlobalLimitExec(ba.MergeExec(m), limit)
    assert plan.schema() == m.schema() and plan.output_partitioning().count == 1
    flat = [n for sizes in K.LIMIT_PARTITIONS for n in sizes]
    whole = helpers.concat([b for part in oracle for b in part])
    out = [helpers.from_device(b) for b in plan.execute(0)]
    assert_batches(out, K.split_by_sizes([og.limit(whole, limit)], K.limit_sizes(flat, limit)))
    helpers.assert_bit_exact(helpers.concat(out) if out else OrderedDict(), plan_eval.collect(plan))


def test_limit_zero_keeps_the_schema(ctx):
    m, _, _ = limit_partitions(ctx)
    for plan in (ba.LocalLimitExec(m, 0), ba.GlobalLimitExec(ba.MergeExec(m), 0)):
        assert plan.schema() == m.schema()
        assert plan.execute(0).schema() == m.schema()
        assert sum(b.num_rows for b in plan.collect()) == 0


def test_merge_keeps_partition_and_batch_order(ctx):
    size_lists = [[], [5, 0, 64], [], [1], [65, 63], []]
    m, oracle, dev = stream_partitions(ctx, size_lists, seed0=80)
    plan = ba.MergeExec(m)
    assert plan.output_partitioning().count == 1 and plan.schema() == m.schema()
    out = list(plan.execute(0))
    assert_batches([helpers.from_device(b) for b in out], [b for part in oracle for b in part])
    assert [b.column_device(0)[0] for b in out] == [b.column_device(0)[0] for part in dev for b in part]      # handed on, not copied
    helpers.assert_bit_exact(helpers.concat(helpers.collect_product(plan)), plan_eval.collect(plan))
