"""Hash repartitioning (hash_partition_batch, host/ops_sort.cpp) on both of its device routes at the keys, partition counts and sizes
where a route can go wrong without the other tests noticing.  The two routes state the row hash separately (partition_of in
kernels_sort.hip, hash_row in kernels_scan.hip) and a shuffle join needs them to agree on every key.

Routes, and the cases that reach each:

  scatter pass (partition_hist + partition_scatter): ONE NULL-free Int32 / Date32 / Int64 / UInt64 key column, every column fixed-width
  and NULL-free, n_parts <= 256, n > 0, at most 32 columns.
    - test_scatter_sizes_and_counts: n_parts {1, 2, 3, 7, 255, 256} x sizes {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193} (every
      size at 3 and 256, the rest pruned to pairs) x the four key types; keys = the types' extremes (INT32_MIN, -1, INT64_MIN, 2^63,
      2^64 - 1, ...), dense small values, values that differ only above bit 32; payload columns of 1, 2, 4 and 8 bytes
    - test_scatter_skew: all rows in one partition (distinct keys, and one repeated key), two alternating keys, the first / the last /
      interior partitions empty, all 256 live, a single row, more partitions than rows
    - test_scatter_route_switch (32 columns), test_scatter_partitions_feed_operators, test_routes_agree ("lone"),
      test_types_agree (Int32, Int64, Date32), the "fixed" batches of test_repartition_exec_alternates_routes
    - the streaming shuffle runs the same partition_of over chunks: test_streaming_shuffle_key_extremes

  sort pass (scan_keys -> hash_to_pid -> radix_sort_pairs -> partition_bounds -> one take_batch per partition): everything else.
    - the one-workgroup sort (n <= 1024), no pass at all (all ids equal), one LSD pass per differing byte (two from 257 partitions):
      test_sort_sizes_and_counts: sizes {1, 2, 1023, 1024, 1025, 4097} x n_parts {1, 2, 3, 255, 256, 257, 1000}, keys (Int64 with NULLs,
      Utf8 with NULLs); test_sort_keys["key_all_equal"], ["key_all_null"] (the `diff == 0` return above 1024 rows);
      ["more_partitions_than_rows_sorted"] (1000 partitions over 300 rows)
    - test_sort_keys: (Int64, Utf8) and (Utf8, Int64); Utf8 with '', NULL, 300-byte and non-ASCII values; a nullable Boolean; Float64 /
      Float32 specials with -0.0 and +0.0; a sum of two columns; a narrowing CAST (NULL where it does not fit) and a CAST to Float64
    - test_scatter_route_switch (33 columns; 257 partitions), test_routes_agree ("utf8", "bitmap"), test_types_agree (the other types),
      the "nulls" batches of test_repartition_exec_alternates_routes
    - test_switch_sends_the_scatter_cases_through_the_sort_pass: every test_scatter_* case again in a child process under
      BHIP_NO_PARTITION_SCATTER=1 (read once per process)

  neither (n = 0): test_empty_batch.

Every comparison is exact and ordered: partition p of the device equals partition p of oracle.engine.repartition_hash row for row in
input order (bit for bit where a table holds NaN payloads or signed zeros).  tests/test_repartition_cases_cpu.py checks the oracle's
hash against published vectors and against a second statement.  Every case asserts its route from the launch names of a context
that times every launch: the sort pass shows one `hash_to_pid` per batch, the scatter pass none."""
import os
import re
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og, plan_eval

import helpers
import repartition_cases as K
from test_exchange_gpu import rank_batch, run_world

pytestmark = pytest.mark.gpu

SCATTER_OFF = os.environ.get("BHIP_NO_PARTITION_SCATTER") == "1"          # the child run of the switch test


@pytest.fixture(scope="module")
def tctx():
    """a context that times every launch, however small (BHIP_KERNEL_TIMING is read when a context is created)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("BHIP_KERNEL_TIMING", "2")
    try:
        return ba.Context(0)
    finally:
        mp.undo()


def assert_route(ks, route, batches=1):
    """ks: kernel_stats() of `batches` calls of hash_partition_batch that all took `route`"""
    if route == "scatter" and SCATTER_OFF:
        route = "sort"
    if route == "sort":
        assert ks.get("hash_to_pid", (0, 0, 0))[1] == batches and ks.get("scan_keys", (0, 0, 0))[1] == batches, (route, sorted(ks))
    else:
        assert "hash_to_pid" not in ks and "scan_keys" not in ks and "partition_bounds" not in ks, (route, sorted(ks))


def split(tctx, dev, exprs, n_parts, route):
    tctx.kernel_stats(reset=True)
    got = ba.plan.hash_partition(dev, exprs, n_parts)
    assert_route(tctx.kernel_stats(reset=True), route)
    assert len(got) == n_parts
    return got


_WANT = {}


def expected(case, n_parts):
    """the oracle's partitions, computed once per (table, keys, count)"""
    key = (id(case.batch), tuple(id(e) for e in case.exprs), n_parts)
    if key not in _WANT:
        _WANT[key] = og.repartition_hash(case.batch, case.exprs, n_parts)
    return _WANT[key]


def compare(got, want, bit_exact):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.num_rows == og.batch_len(w)
        g = helpers.from_device(g)
        helpers.assert_same_schema(g, w)
        if bit_exact:
            helpers.assert_bit_exact(g, w)
        else:
            helpers.assert_rows_equal(g, w, ordered=True)


def check(tctx, case, n_parts, dev=None):
    dev = helpers.to_device(tctx, case.batch) if dev is None else dev
    got = split(tctx, dev, case.exprs, n_parts, case.route)
    compare(got, expected(case, n_parts), case.bit_exact)
    return got


def row_numbers(parts):
    return [helpers.from_device(p)["rn"].values.tolist() for p in parts]


# ---- the scatter pass (every test_scatter_* runs again in the child process of the switch test, on the sort pass) ------------------------------

@pytest.mark.parametrize("dtype", K.KEY_TYPES)
@pytest.mark.parametrize("n_parts,n", K.SCATTER_PAIRS)
def test_scatter_sizes_and_counts(tctx, n_parts, n, dtype):
    """wave (64), sub-tile (256) and workgroup (4096) edges against partition counts that are no power of two, with the key types'
    extremes among the keys and a payload column of every width beside them"""
    check(tctx, K.scatter_case(dtype, n_parts, n), n_parts)


@pytest.mark.parametrize("case", K.SKEW_CASES, ids=repr)
def test_scatter_skew(tctx, case):
    """one live partition (all 64 lanes of every ballot share a digit), empty partitions at either end and inside, all 256 live, one
    row, fewer rows than partitions"""
    check(tctx, case, case.n_parts[0])


def test_scatter_route_switch(tctx):
    """32 columns: the scatter pass; 33 columns, or 257 partitions: the sort pass — the same rows land in the same partitions"""
    c32, c33, c32_257, c33_257 = K.SWITCH_CASES
    a, b = row_numbers(check(tctx, c32, 256)), row_numbers(check(tctx, c33, 256))
    assert a == b
    a, b = row_numbers(check(tctx, c32_257, 257)), row_numbers(check(tctx, c33_257, 257))
    assert a == b


def test_scatter_partitions_feed_operators(tctx):
    """a partition's columns are slices of the scattered columns at arbitrary element offsets of 1-, 2-, 4- and 8-byte values: each
    must work as operator input"""
    case = K.scatter_case("Int32", 3, 4097)
    parts = check(tctx, case, 3)
    # MIN and MAX of every integer and temporal payload, SUM of the narrow ones (the float payloads are arbitrary bit patterns, NaNs
    # among them: compared bit for bit above); an aggregate holds at most 16 accumulators, so the narrow and the wide columns take turns
    narrow = [name for name, dtype in K.PAYLOADS if np.dtype(og.NP_TYPES[dtype]).itemsize <= 2]
    wide = [name for name, dtype in K.PAYLOADS if np.dtype(og.NP_TYPES[dtype]).itemsize >= 4 and dtype not in og.FLOAT_TYPES]
    assert narrow == ["p_i8", "p_u8", "p_i16", "p_u16"] and wide == ["p_i32", "p_d32", "p_i64", "p_u64", "p_ts"]
    agg_lists = [[E.Count(col("rn"), "n")] + [f(col(name), tag + name) for name in names for f, tag in ((E.Min, "mn_"), (E.Max, "mx_"))] + sums
                 for names, sums in ((narrow, [E.Sum(col(name), "s_" + name) for name in narrow]), (wide, [E.Sum(col("p_i32"), "s_p_i32")]))]
    for p, w in zip(parts, expected(case, 3)):
        assert og.batch_len(w) > 1000
        src = ba.MemoryExec([[p]], tctx)
        src._oracle_partitions = [[w]]
        for aggs in agg_lists:
            plan = ba.HashAggregateExec(ba.plan.PARTIAL, [], aggs, ba.FilterExec(E.BinaryExpr(col("p_i16"), "Gt", lit(0, "Int16")), src))
            helpers.assert_rows_equal(helpers.concat(helpers.collect_product(plan)), plan_eval.collect(plan), ordered=False)
        plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("p_u8"), "g")], [E.Count(col("rn"), "n"), E.Max(col("p_i64"), "mx"), E.Min(col("p_u16"), "mn")], src)
        helpers.assert_rows_equal(helpers.concat(helpers.collect_product(plan)), plan_eval.collect(plan), ordered=False, key_cols=["g"])


N_SCATTER_TESTS = len(K.SCATTER_PAIRS) * len(K.KEY_TYPES) + len(K.SKEW_CASES) + 2


def test_switch_sends_the_scatter_cases_through_the_sort_pass():
    """BHIP_NO_PARTITION_SCATTER is read once per process: the test_scatter_* cases in a child process with the switch set, where
    assert_route expects a hash_to_pid launch of every one of them"""
    assert not SCATTER_OFF, "the switch is set in this process: the scatter-pass cases of this file cannot reach their route"
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BHIP_NO_PARTITION_SCATTER="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-k", "test_scatter", os.path.abspath(__file__)],
                       cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert re.search(r"(?<!\d)%d passed" % N_SCATTER_TESTS, p.stdout) and "skipped" not in p.stdout, p.stdout[-2000:]


# ---- the empty batch -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.EMPTY_CASES, ids=repr)
def test_empty_batch(tctx, case):
    """n = 0 gives n_parts empty batches with the full schema, on either side of the 256-partition limit"""
    dev = helpers.to_device(tctx, case.batch)
    for n_parts in case.n_parts:
        got = split(tctx, dev, case.exprs, n_parts, "none")
        for g in got:
            assert g.num_rows == 0 and g.schema3() == dev.schema3()
        compare(got, expected(case, n_parts), case.bit_exact)


# ---- the sort pass -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_parts,n", K.SORT_PAIRS)
def test_sort_sizes_and_counts(tctx, n_parts, n):
    """the last size of the one-workgroup sort and the first of the LSD passes; one differing id byte up to 256 partitions, two
    from 257; keys (Int64, Utf8) with NULLs in one column, in the other and in both"""
    check(tctx, K.sort_size_case(n_parts, n), n_parts)


@pytest.mark.parametrize("case", K.KEY_CASES, ids=repr)
def test_sort_keys(tctx, case):
    dev = helpers.to_device(tctx, case.batch)
    for n_parts in case.n_parts:
        check(tctx, case, n_parts, dev)


def test_sort_key_order_counts(tctx):
    """[a, s] and [s, a] over one table give different partitions, each the oracle's"""
    ab, sa = (c for c in K.KEY_CASES if c.name in ("keys_int64_utf8", "keys_utf8_int64"))
    dev = helpers.to_device(tctx, ab.batch)
    assert row_numbers(check(tctx, ab, 7, dev)) != row_numbers(check(tctx, sa, 7, dev))


# ---- agreement between the routes and between the types --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["Int32", "Int64", "UInt64"])
def test_routes_agree(tctx, dtype):
    """one set of key values as a lone NULL-free column (scatter pass), beside a Utf8 payload (sort pass) and under a validity bitmap
    none of whose rows is NULL (sort pass): identical partitions"""
    t = K.route_agreement_tables(dtype)
    n, p = K.AGREE_ROWS, K.AGREE_NPARTS
    want = [w["rn"].values.tolist() for w in og.repartition_hash(t["lone"], K.K, p)]
    lone = row_numbers(split(tctx, helpers.to_device(tctx, t["lone"]), K.K, p, "scatter"))
    utf8 = row_numbers(split(tctx, helpers.to_device(tctx, t["utf8"]), K.K, p, "sort"))
    # the import drops a validity buffer whose bits are all set: cut the NULL last row off a longer batch instead (a zero-copy slice)
    head = ba.LocalLimitExec(ba.MemoryExec([[helpers.to_device(tctx, t["bitmap"])]], tctx), n).collect()[0]
    assert head.num_rows == n and head.column_info(0)[4] and helpers.from_device(head)["k"].valid is None
    bitmap = row_numbers(split(tctx, head, K.K, p, "sort"))
    assert lone == want and utf8 == want and bitmap == want
    assert sum(len(x) for x in want) == n and all(want)


@pytest.mark.parametrize("group", list(K.TYPE_GROUPS))
def test_types_agree(tctx, group):
    """integers hash as their sign- or zero-extended 64-bit value, a Float32 as the double it equals: the same values held as
    different types go to the same partitions, whichever route the type takes"""
    values, types = K.TYPE_GROUPS[group]
    seen = []
    for dtype in types:
        t = K.type_table(group, dtype)
        got = row_numbers(split(tctx, helpers.to_device(tctx, t), K.K, K.AGREE_NPARTS, K.TYPE_ROUTE.get(dtype, "sort")))
        assert got == [w["rn"].values.tolist() for w in og.repartition_hash(t, K.K, K.AGREE_NPARTS)], dtype
        seen.append(got)
    assert all(s == seen[0] for s in seen[1:]) and sum(len(x) for x in seen[0]) == len(values)


# ---- RepartitionExec over batches that alternate between the routes ----------------------------------------------------------------------------

def test_repartition_exec_alternates_routes(tctx):
    """two input partitions of empty batches, NULL-free batches (scatter pass) and batches of the same schema whose key has a validity
    bitmap (sort pass); the output partitions are read in reverse order, then each a second time (the split cache)"""
    stream = K.repartition_stream()
    dev = [[ba.RecordBatch.from_columns(tctx, [(name, c.dtype, c.values, c.is_valid() if name == "k" else None) for name, c in b.items()])
            for _, b in part] for part in stream]
    for part, dpart in zip(stream, dev):
        for (kind, _), d in zip(part, dpart):
            assert d.column_info(0)[2] and d.column_info(0)[4] == (kind == "nulls")        # nullable everywhere, a buffer only with NULLs
    m = ba.MemoryExec(dev, tctx)
    m._oracle_partitions = [[b for _, b in part] for part in stream]
    kinds = [kind for part in stream for kind, _ in part]
    n_sort = kinds.count("nulls") + (kinds.count("fixed") if SCATTER_OFF else 0)
    total = sum(og.batch_len(b) for part in stream for _, b in part)

    def read(plan, p):
        return helpers.concat([helpers.from_device(b) for b in plan.execute(p)])

    plan = ba.RepartitionExec(m, ba.Partitioning.Hash(K.K, K.REPART_NPARTS))
    assert plan.output_partitioning().partition_count() == K.REPART_NPARTS
    tctx.kernel_stats(reset=True)
    first = {}
    for p in reversed(range(K.REPART_NPARTS)):
        first[p] = read(plan, p)
        helpers.assert_rows_equal(first[p], helpers.concat(plan_eval.execute(plan, p)), ordered=True)
    ks = tctx.kernel_stats(reset=True)
    assert ks.get("hash_to_pid", (0, 0, 0))[1] == n_sort and 0 < n_sort, sorted(ks)        # every batch was split once, each on its route
    assert sum(og.batch_len(b) for b in first.values()) == total
    for p in range(K.REPART_NPARTS):
        helpers.assert_rows_equal(read(plan, p), first[p], ordered=True)
    assert "hash_to_pid" not in tctx.kernel_stats(reset=True)                              # the second read came from the cache

    one = ba.RepartitionExec(m, ba.Partitioning.Hash(K.K, 1))
    got = read(one, 0)
    helpers.assert_rows_equal(got, helpers.concat(plan_eval.execute(one, 0)), ordered=True)
    assert got["rn"].values.tolist() == list(range(total))


# ---- the streaming shuffle: partition_of over chunks ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["k", "d"])
def test_streaming_shuffle_key_extremes(key):
    """a loopback world of 3 over a UInt64 key at or above 2^63 and over a negative Date32 key; every row of rank 0 goes to rank 1"""
    world = K.SHUFFLE_WORLD

    def make(rank):
        b = rank_batch(rank, K.SHUFFLE_SIZES[rank], seed=12, fixed=True)
        s = K.shuffle_batch(rank, key)
        b["k"], b["d"] = s["k"], s["d"]
        return b

    def fn(rank, c, comm):
        out, st = comm.shuffle(helpers.to_device(c, make(rank)), key, 4096, with_stats=True)
        return helpers.from_device(out), st

    got = run_world(world, fn)
    parts = [og.repartition_hash(make(s), [col(key)], world) for s in range(world)]
    assert [og.batch_len(x) for x in parts[0]] == [0, K.SHUFFLE_SIZES[0], 0]
    for d in range(world):
        batch, st = got[d]
        live = [parts[s][d] for s in range(world) if og.batch_len(parts[s][d])]
        want = og.concat_batches(live)
        helpers.assert_rows_equal(batch, want, ordered=True)
        assert st["streamed"] == 1 and st["rows_in"] == K.SHUFFLE_SIZES[d] and st["rows_out"] == og.batch_len(want)
        assert st["rows_to"] == [og.batch_len(parts[d][t]) for t in range(world)]
