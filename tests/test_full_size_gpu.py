"""Parity at BASELINE.json's full size (TPC-H SF100: 600,037,902 lineitem rows resident in HBM), where the oracle
cannot run: size-independent properties of the operators themselves.

  * linearity of the Partial / Final split (rust/scheduler/src/planner.rs:136-171): Q1 over the whole table ==
    Final merge of Q1 partials over two disjoint halves — groups and counts exactly, sums within 1e-9 relative;
  * the filter's row count: sum of count_order == number of rows FilterExec keeps for the same predicate (exact);
  * Q6 likewise.

These are checks of the device against itself.  The comparison of the full-size results with an independent CPU reference
(every group of Q1 / Q6 / Q3 / Q5 at SF100, through bench.py's Workload) is tests/test_full_size_oracle_gpu.py.

The halves are generated separately on the device (the generator is a pure function of the row index), so the
whole-table run and the split run share no intermediate state."""
import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E, tpch
from ballista_amd.expr import col

pytestmark = pytest.mark.gpu
N = 600_037_902
SF = 100.0


def rows_of(batches, keys):
    out = {}
    for b in batches:
        d = b.to_pydict()
        names = list(d)
        for i in range(b.num_rows):
            out[tuple(d[k][i] for k in keys)] = {n: d[n][i] for n in names if n not in keys}
    return out


def close(a, b, rtol=1e-9):
    return abs(a - b) <= rtol * max(abs(a), abs(b))


@pytest.fixture(scope="module")
def big_ctx():
    c = ba.Context(0)
    free = None
    try:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        if hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0:
            free = f.value
    except OSError:
        pass
    if free is not None and free < 100 * 2 ** 30:
        pytest.skip(f"needs ~80 GB of free HBM, {free / 2 ** 30:.0f} GiB available")
    return c


def test_q1_whole_equals_merge_of_halves_and_filter_count(big_ctx):
    ctx = big_ctx
    whole = ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, 0, N)
    full = tpch.q1_plan(ba.MemoryExec([[whole]], ctx)).collect()
    keys = ["l_returnflag", "l_linestatus"]
    want = rows_of(full, keys)
    assert sorted(want) == [("A", "F"), ("N", "F"), ("N", "O"), ("R", "F")]
    assert [k for b in full for k in zip(*(b.to_pydict()[c] for c in keys))] == sorted(want)       # SortExec order

    # exact row count of the predicate, by the standalone filter on the date column alone
    dates = ba.ProjectionExec([(col("l_shipdate"), "l_shipdate")], ba.MemoryExec([[whole]], ctx))
    kept = sum(b.num_rows for b in ba.FilterExec(tpch.q1_parts(tpch.LINEITEM_SCHEMA)["predicate"], dates).collect())
    assert sum(v["count_order"] for v in want.values()) == kept
    assert 0.98 * N < kept < 0.99 * N                              # 98.6 % pass

    half = N // 2 + 12345                                          # not a tile multiple
    a = ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, 0, half)
    b = ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, half, N - half)
    split = tpch.q1_final(tpch.q1_stage1(ba.MemoryExec([[a], [b]], ctx))).collect()
    got = rows_of(split, keys)
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k]
        assert g["count_order"] == w["count_order"], k
        for name in ("sum_qty", "sum_base_price", "sum_disc_price", "sum_charge", "avg_qty", "avg_price", "avg_disc"):
            assert close(g[name], w[name]), (k, name, g[name], w[name])
        # quantities are integers 1..50: their sum is exact in Float64 either way
        assert g["sum_qty"] == w["sum_qty"]
        assert close(w["avg_qty"], w["sum_qty"] / w["count_order"], 1e-15)


def test_q6_whole_equals_sum_of_halves(big_ctx):
    ctx = big_ctx
    whole = ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, 0, N)
    rev = tpch.q6_plan(ba.MemoryExec([[whole]], ctx)).collect()[0].to_pydict()["revenue"][0]
    half = N // 3
    parts = [ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, 0, half), ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, half, N - half)]
    rev2 = tpch.q6_plan(ba.MemoryExec([[parts[0]], [parts[1]]], ctx)).collect()[0].to_pydict()["revenue"][0]
    assert close(rev, rev2)
    # the selected rows, counted independently by the filter operator
    narrow = ba.ProjectionExec([(col(n), n) for n in ["l_shipdate", "l_discount", "l_quantity"]], ba.MemoryExec([[whole]], ctx))
    sel = sum(b.num_rows for b in ba.FilterExec(tpch.q6_predicate(tpch.LINEITEM_SCHEMA), narrow).collect())
    assert 0.011 * N < sel < 0.014 * N                             # (1/6.6 years) x (3/11 discounts) x (23/50 quantities)
    cnt = ba.HashAggregateExec(ba.plan.PARTIAL, [], [E.Count(E.lit(1, E.UINT8), "n")],
                               ba.FilterExec(tpch.q6_predicate(tpch.LINEITEM_SCHEMA), ba.MemoryExec([[whole]], ctx))).collect()
    assert cnt[0].to_pydict()["n[count]"][0] == sel


def _q3_tables(ctx):
    dims = tpch.dimension_tables(ctx, SF)
    n = tpch.table_rows(SF)
    orders = ba.plan.tpch_orders(ctx, SF, tpch.SEED, 0, n["orders"])
    return dims["customer"], orders, n


def test_q3_sf100_join_counts_and_halves(big_ctx):
    """Q3 at SF100 (two hash joins, 1.13 M groups, sort), properties no oracle run is needed for:
      * the rows the order-key join emits == the lineitem rows whose key is among the surviving orders, counted on an
        independent path (Inner join against the bare key list + COUNT, no aggregate-over-join pruning, CAS table forced off/on is
        not involved: a different operator shape);
      * whole table == Final merge of partials over two lineitem halves: same groups, revenue within 1e-9;
      * ORDER BY revenue DESC, o_orderdate; every group key is a surviving order; group count == distinct matched orders."""
    ctx = big_ctx
    cust, orders, n = _q3_tables(ctx)
    m = lambda b: ba.MemoryExec([[b]], ctx)
    li = ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, 0, N)
    res = tpch.q3_plan(m(cust), m(orders), m(li)).collect()
    n_groups = sum(b.num_rows for b in res)
    assert 1_000_000 < n_groups < 1_300_000
    # sortedness on the device result: revenue descending (ties by date ascending)
    rev = np.concatenate([np.asarray(b.column([c[0] for c in b.schema()].index("revenue"))[1]) for b in res])
    dat = np.concatenate([np.asarray(b.column([c[0] for c in b.schema()].index("o_orderdate"))[1]) for b in res])
    assert np.all((rev[:-1] > rev[1:]) | ((rev[:-1] == rev[1:]) & (dat[:-1] <= dat[1:])))
    keys = np.concatenate([np.asarray(b.column([c[0] for c in b.schema()].index("l_orderkey"))[1]) for b in res])
    assert len(np.unique(keys)) == n_groups                                   # one group per order key

    # independent count of the join's output rows and of its distinct keys
    j1 = tpch.q3_build_side(m(cust), m(orders))
    key_only = ba.ProjectionExec([(col("o_orderkey"), "o_orderkey")], j1)
    probe = ba.ProjectionExec([(col("l_orderkey"), "l_orderkey")], ba.FilterExec(E.coerce(col("l_shipdate") > E.date32("1995-03-15"), tpch.LINEITEM_SCHEMA), m(li)))
    joined = ba.HashJoinExec(key_only, probe, [("o_orderkey", "l_orderkey")], ba.plan.INNER)
    cnt = ba.HashAggregateExec(ba.plan.PARTIAL, [], [E.Count(E.lit(1, E.UINT8), "n")], joined).collect()[0].to_pydict()["n[count]"][0]
    per_key = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("l_orderkey"), "k")], [E.Count(E.lit(1, E.UINT8), "n")], joined).collect()
    assert sum(b.num_rows for b in per_key) == n_groups
    assert sum(int(np.sum(np.asarray(b.column(1)[1]))) for b in per_key) == cnt
    # only orders placed in the ~4 months before the cut-off date still have lineitems shipping after it
    assert 2_000_000 < cnt < 5_000_000 and 2.0 < cnt / n_groups < 3.5
    # every result key is one of the surviving orders: an Inner join of the result with the build keys keeps every row
    back = ba.HashJoinExec(key_only, ba.ProjectionExec([(col("l_orderkey"), "l_orderkey")], ba.MemoryExec([res], ctx)), [("o_orderkey", "l_orderkey")], ba.plan.INNER)
    assert sum(b.num_rows for b in back.collect()) == n_groups

    # whole == merge of halves
    half = N // 2 + 777
    a = ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, 0, half)
    b = ba.plan.tpch_lineitem(ctx, SF, tpch.SEED, half, N - half)
    del li
    split = tpch.q3_final(tpch.q3_partial(tpch.q3_build_side(m(cust), m(orders)), tpch.q3_probe_side(ba.MemoryExec([[a], [b]], ctx)))).collect()
    assert sum(x.num_rows for x in split) == n_groups
    rev2 = np.concatenate([np.asarray(x.column([c[0] for c in x.schema()].index("revenue"))[1]) for x in split])
    keys2 = np.concatenate([np.asarray(x.column([c[0] for c in x.schema()].index("l_orderkey"))[1]) for x in split])
    o1, o2 = np.argsort(keys, kind="stable"), np.argsort(keys2, kind="stable")
    assert np.array_equal(keys[o1], keys2[o2])
    assert np.allclose(rev[o1], rev2[o2], rtol=1e-9, atol=0)


def test_q3_is_bit_reproducible_run_to_run(big_ctx):
    """two executions of the same plan over the same tables give bit-identical revenue sums and the same row order
    (fixed-order reductions; the join emits in probe order, the aggregate sums each group in row order)"""
    ctx = big_ctx
    sf = 1.0
    n = tpch.table_rows(sf)
    dims = tpch.dimension_tables(ctx, sf)
    m = lambda b: ba.MemoryExec([[b]], ctx)
    orders = ba.plan.tpch_orders(ctx, sf, tpch.SEED, 0, n["orders"])
    li = ba.plan.tpch_lineitem(ctx, sf, tpch.SEED, 0, n["lineitem"])
    runs = []
    for _ in range(3):
        res = tpch.fresh(tpch.q3_plan(m(dims["customer"]), m(orders), m(li))).collect()
        rev = np.concatenate([np.asarray(b.column(1)[1]) for b in res])
        key = np.concatenate([np.asarray(b.column(0)[1]) for b in res])
        runs.append((rev.view(np.uint64).copy(), key.copy()))
    for r, k in runs[1:]:
        assert np.array_equal(k, runs[0][1]) and np.array_equal(r, runs[0][0])
