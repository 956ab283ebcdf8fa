"""CPU tests that pin oracle/fullsize.py, the chunked extended-precision reference the full-size GPU tests compare against
(tests/test_full_size_oracle_gpu.py), before anything is compared with it:

  * at sf 0.01 it reproduces the committed goldens (tests/golden/q{1,6,3,5}_synth.json: pyarrow + exact rational sums): keys,
    counts and row order exactly, sums within 1e-13 relative (the reference's own bound is 1e-17; the goldens are correctly
    rounded Float64, 1.1e-16), Q3's per-group revenue within n_max * 2^-53;
  * chunking does not matter: chunk sizes 1000, 4097 and "one chunk" give identical counts and sums equal to 1e-15 relative;
  * at SF1 the C ports that bench.py times as its CPU baseline agree with it: counts exactly, sums within
    rows-in-the-largest-partition * 2^-53 relative (a sequential Float64 sum of n positives is within (n - 1) * 2^-53 of exact);
    this is the first result check oracle_q3_join_port / oracle_q5_join_port get;
  * oracle/plan_eval.py (what the GPU tier trusts at small sizes) over the sf 0.01 plans of ballista_amd/tpch.py equals it.

Sanity of these tests, tried on a scratch copy: with the reference's `o_orderdate < 1995-03-15` turned into `<=`, the two SF1
join-port tests fail (11,199 groups against 11,319; at sf 0.01 no BUILDING order falls on that day); with one lineitem chunk
dropped, 9 of the 17 tests fail (goldens, chunking, prefix, plan_eval)."""
import json
import os

import numpy as np
import pytest

from ballista_amd import tpch
from oracle import fullsize, gen, plan_eval

import helpers
import plan_nodes as N

U = 2.0 ** -53
SF1_ROWS = 6_001_215          # dbgen's SF1 lineitem count, the generator's own (bench.py --sf 1 uses 6,000,379 of them)
Q1_SUMS = ("sum_qty", "sum_base_price", "sum_disc_price", "sum_charge", "avg_qty", "avg_price", "avg_disc")


def golden(name):
    with open(os.path.join(helpers.GOLDEN, name)) as f:
        return json.load(f)


def rel(a, b):
    """|a - b| / |b| in the reference's precision (longdouble where the platform has one)"""
    a, b = np.longdouble(a), np.longdouble(b)
    return float(abs(a - b) / abs(b)) if b != 0 else float(abs(a))


def generator_dims(sf):
    """the small tables of oracle/tpch_gen.c (what the goldens were made from) in the layout of tpch.dimension_arrays"""
    c, s = gen.customer_arrays(sf), gen.supplier_arrays(sf)
    off, data = c["c_mktsegment.off"], c["c_mktsegment.data"].tobytes()
    seg = np.array([tpch.SEGMENTS.index(data[off[i]:off[i + 1]].decode()) for i in range(len(off) - 1)], np.int32)
    return dict(customer=dict(c_custkey=c["c_custkey"], c_nationkey=c["c_nationkey"], c_mktsegment=seg),
                supplier=dict(s_suppkey=s["s_suppkey"], s_nationkey=s["s_nationkey"]))


@pytest.fixture(scope="module")
def ref_small():
    return fullsize.reference(0.01, dims=generator_dims(0.01), chunk_rows=7001)


@pytest.fixture(scope="module")
def dims_sf1():
    return tpch.dimension_arrays(1.0)


@pytest.fixture(scope="module")
def ref_sf1(dims_sf1):
    return {k64: fullsize.reference(1.0, rows=SF1_ROWS, key64=k64, dims=dims_sf1) for k64 in (False, True)}


def test_constants_are_the_products():
    assert fullsize.SEGMENTS == tpch.SEGMENTS and fullsize.NATIONS == tpch.NATIONS and fullsize.REGIONS == tpch.REGIONS
    assert gen.cardinalities(1.0)["lineitem"] == SF1_ROWS and gen.cardinalities(1.0)["orders"] == tpch.table_rows(1.0)["orders"]
    assert gen.cardinalities(100.0)["lineitem"] == tpch.table_rows(100.0)["lineitem"] == 600_037_902
    # the error bound the module states is at least four decimal orders below every tolerance it is used with
    assert fullsize.SUM_REL_ERROR(144) * 1e4 <= 1e-13 and fullsize.SUM_REL_ERROR(6002) * 1e4 <= 1e-9


# ---- goldens ---------------------------------------------------------------------------------------------------------------

def test_q1_q6_reproduce_the_goldens(ref_small):
    g = golden("q1_synth.json")
    assert g["n_rows"] == ref_small["rows"]
    assert list(ref_small["q1"]) == [(r["l_returnflag"], r["l_linestatus"]) for r in g["rows"]]           # ORDER BY order
    for r in g["rows"]:
        w = ref_small["q1"][(r["l_returnflag"], r["l_linestatus"])]
        assert w["count_order"] == r["count_order"] and isinstance(w["count_order"], int)
        assert float(w["sum_qty"]) == r["sum_qty"]
        for k in Q1_SUMS:
            assert rel(w[k], r[k]) <= 1e-13, (k, w[k], r[k])
    g6 = golden("q6_synth.json")
    assert ref_small["q6"]["selected"] == g6["selected"]
    assert rel(ref_small["q6"]["revenue"], g6["revenue"]) <= 1e-13


def test_q3_reproduces_the_golden(ref_small):
    rows = golden("q3_synth.json")["rows"]
    q3 = ref_small["q3"]
    o = q3["order"]
    assert q3["revenue_exact"] == fullsize.EXTENDED
    assert [int(k) for k in q3["keys"][o]] == [r["l_orderkey"] for r in rows]                              # row order
    assert [int(d) for d in q3["date"][o]] == [r["o_orderdate"] for r in rows]
    assert [int(p) for p in q3["prio"][o]] == [r["o_shippriority"] for r in rows]
    assert q3["n_joined"] == int(q3["rows_in_group"].sum()) and 1 <= q3["n_max"] <= 7
    for got, r in zip(q3["revenue"][o], rows):
        assert abs(np.longdouble(r["revenue"]) - got) <= q3["n_max"] * U * got, (r, got)
        assert float(got) == r["revenue"]                    # an exact sum rounds to the golden's correctly rounded value
    assert np.all(np.diff(q3["keys"]) > 0)


def test_q5_reproduces_the_golden(ref_small):
    rows = golden("q5_synth.json")["rows"]
    q5 = ref_small["q5"]
    assert [name for name, _, _ in q5["rows"]] == [r["n_name"] for r in rows]
    for (name, rev, cnt), r in zip(q5["rows"], rows):
        assert rel(rev, r["revenue"]) <= 1e-13 and cnt > 0, (name, rev, r)
    asia = {n for n, reg in tpch.NATIONS if tpch.REGIONS[reg] == "ASIA"}
    for i, (n, _) in enumerate(tpch.NATIONS):
        assert (q5["count_by_nationkey"][i] == 0 and q5["revenue_by_nationkey"][i] == 0) or n in asia


# ---- chunking --------------------------------------------------------------------------------------------------------------

def same_counts_close_sums(a, b, rtol=1e-15):
    assert list(a["q1"]) == list(b["q1"])
    for k in a["q1"]:
        assert a["q1"][k]["count_order"] == b["q1"][k]["count_order"]
        assert a["q1"][k]["sum_qty"] == b["q1"][k]["sum_qty"]
        for name in Q1_SUMS:
            assert rel(a["q1"][k][name], b["q1"][k][name]) <= rtol, (k, name)
    assert a["q6"]["selected"] == b["q6"]["selected"] and rel(a["q6"]["revenue"], b["q6"]["revenue"]) <= rtol
    for f in ("keys", "date", "prio", "rows_in_group", "order"):
        assert np.array_equal(a["q3"][f], b["q3"][f]), f
    assert (a["q3"]["n_joined"], a["q3"]["n_max"]) == (b["q3"]["n_joined"], b["q3"]["n_max"])
    if fullsize.EXTENDED:
        assert np.array_equal(a["q3"]["revenue"], b["q3"]["revenue"])                   # exact sums: no order dependence at all
    assert np.all(np.abs(a["q3"]["revenue"] - b["q3"]["revenue"]) <= rtol * b["q3"]["revenue"])
    assert [r[0] for r in a["q5"]["rows"]] == [r[0] for r in b["q5"]["rows"]]
    assert a["q5"]["count_by_nationkey"] == b["q5"]["count_by_nationkey"]
    for x, y in zip(a["q5"]["rows"], b["q5"]["rows"]):
        assert rel(x[1], y[1]) <= rtol


@pytest.mark.parametrize("chunk", [1000, 4097])
def test_chunking_does_not_matter_small(ref_small, chunk):
    one = fullsize.reference(0.01, dims=generator_dims(0.01), chunk_rows=None, threads=1)
    assert one["n_chunks"] == 1
    same_counts_close_sums(fullsize.reference(0.01, dims=generator_dims(0.01), chunk_rows=chunk), one)
    same_counts_close_sums(ref_small, one)


@pytest.mark.parametrize("chunk", [1000, 4097, None])
def test_chunking_does_not_matter_sf1(ref_sf1, dims_sf1, chunk):
    other = fullsize.reference(1.0, rows=SF1_ROWS, dims=dims_sf1, chunk_rows=chunk)
    assert other["n_chunks"] == (1 if chunk is None else -(-SF1_ROWS // chunk))
    same_counts_close_sums(other, ref_sf1[False])


def test_key_width_and_row_prefix(ref_sf1, dims_sf1):
    same_counts_close_sums(ref_sf1[True], ref_sf1[False])
    assert ref_sf1[True]["q3"]["keys"].dtype == np.int64 and ref_sf1[False]["q3"]["keys"].dtype == np.int32
    # a prefix of the table: fewer rows counted, and exactly those of the prefix (against a second call over the remainder's
    # complement is not possible with row0 = 0 only, so against plain numpy over the materialised prefix)
    rows = 1_000_003
    r = fullsize.reference(1.0, rows=rows, dims=dims_sf1, chunk_rows=250_000)
    a = gen.lineitem_arrays(1.0, 0, rows)
    assert sum(g["count_order"] for g in r["q1"].values()) == int(np.count_nonzero(a["l_shipdate"] <= 10471))
    assert r["rows"] == rows and r["n_chunks"] == 5
    assert r["q3"]["n_joined"] < ref_sf1[False]["q3"]["n_joined"] * rows / SF1_ROWS * 1.1


# ---- the C ports (bench.py's published CPU baseline) ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lineitem_sf1():
    return gen.lineitem_arrays(1.0, 0, SF1_ROWS)


@pytest.mark.parametrize("parts,threads", [(1, 1), (4, 2), (7, 3), (64, 8)])
def test_q1_q6_ports_agree_at_sf1(ref_sf1, lineitem_sf1, parts, threads):
    ref = ref_sf1[False]
    n = len(lineitem_sf1["l_quantity"])
    bound = -(-n // parts) * U                                # rows in the largest partition x 2^-53
    port = gen.q1_final_from_port(*gen.q1_partial_port(lineitem_sf1, parts, threads))
    assert sorted(port) == list(ref["q1"])
    for k, w in ref["q1"].items():
        p = port[k]
        assert p["count_order"] == w["count_order"]
        assert p["sum_qty"] == float(w["sum_qty"])
        for name in Q1_SUMS:
            assert rel(p[name], w[name]) <= bound, (k, name, p[name], w[name])
    s, c = gen.q6_partial_port(lineitem_sf1, parts, threads)
    assert int(c.sum()) == ref["q6"]["selected"]
    assert rel(np.sum(s.astype(np.longdouble)), ref["q6"]["revenue"]) <= bound


@pytest.mark.parametrize("key64", [False, True])
def test_join_ports_agree_at_sf1(ref_sf1, dims_sf1, key64):
    ref = ref_sf1[key64]
    rows = SF1_ROWS
    for parts, threads in ((1, 1), (16, 4)):
        n_groups, total = gen.JoinQueryPort("q3", 1.0, rows, dims_sf1, key64=key64).run(parts, threads)
        q3 = ref["q3"]
        assert n_groups == len(q3["keys"])
        want = np.sum(q3["revenue"], dtype=q3["revenue"].dtype)
        # group sums of at most n_max rows each, then one sequential sum over the groups
        assert rel(total, want) <= (len(q3["keys"]) + q3["n_max"]) * U, (total, want)
        rev = gen.JoinQueryPort("q5", 1.0, rows, dims_sf1, key64=key64).run(parts, threads)
        assert len(rev) == 25
        for i, (name, reg) in enumerate(tpch.NATIONS):
            w = ref["q5"]["revenue_by_nationkey"][i]
            if tpch.REGIONS[reg] != "ASIA":
                assert rev[i] == 0.0 and w == 0
            else:
                assert w > 0 and rel(rev[i], w) <= max(1, ref["q5"]["count_by_nationkey"][i]) * U, (name, rev[i], w)


# ---- plan_eval ----------------------------------------------------------------------------------------------------------------

def test_plan_eval_equals_the_reference_at_sf001(ref_small, monkeypatch):
    monkeypatch.setattr(tpch, "P", N)
    sf = 0.01
    li = gen.lineitem(sf)
    n = len(li["l_quantity"].values)
    m = lambda b: N.MemoryExec([[b]])
    lim = N.MemoryExec([[helpers.slice_batch(li, 0, n // 3)], [helpers.slice_batch(li, n // 3, n)]])

    q1 = plan_eval.collect(tpch.q1_plan(lim))
    assert list(zip(q1["l_returnflag"].values, q1["l_linestatus"].values)) == list(ref_small["q1"])
    for i, w in enumerate(ref_small["q1"].values()):
        assert int(q1["count_order"].values[i]) == w["count_order"]
        for name in Q1_SUMS:
            assert rel(q1[name].values[i], w[name]) <= n * U, name
    q6 = plan_eval.collect(tpch.q6_plan(lim))
    assert rel(q6["revenue"].values[0], ref_small["q6"]["revenue"]) <= n * U

    q3 = plan_eval.collect(tpch.q3_plan(m(gen.customer(sf)), m(gen.orders(sf)), lim))
    r3 = ref_small["q3"]
    o = r3["order"]
    assert [int(k) for k in q3["l_orderkey"].values] == [int(k) for k in r3["keys"][o]]
    assert np.array_equal(np.asarray(q3["o_orderdate"].values), r3["date"][o])
    assert np.array_equal(np.asarray(q3["o_shippriority"].values), r3["prio"][o])
    assert np.all(np.abs(np.asarray(q3["revenue"].values).astype(np.longdouble) - r3["revenue"][o]) <= r3["n_max"] * U * r3["revenue"][o])

    q5 = plan_eval.collect(tpch.q5_plan(m(gen.customer(sf)), m(gen.orders(sf)), lim, m(gen.supplier(sf)), m(gen.nation()), m(gen.region())))
    assert list(q5["n_name"].values) == [name for name, _, _ in ref_small["q5"]["rows"]]
    for got, (name, rev, cnt) in zip(q5["revenue"].values, ref_small["q5"]["rows"]):
        assert rel(got, rev) <= cnt * U, name
