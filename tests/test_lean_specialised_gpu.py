"""GPU parity of the shape-specialised wide-load scan + aggregate kernels (ballista_amd/csrc/lean_spec_kernel.h) against the
CPU oracle, and of the generic lean kernel they replace for those shapes (BHIP_LEAN_GENERIC=1, in a child process: the
switch is read once per process).

Shapes: Q1 (one Int32 range, two Utf8 keys, 5 chain steps) and one Utf8 key with Q1's sums run specialised; Q6 (Int32 +
two Float64 ranges, no key, 2 steps) and Q1's sums without a key stay on the generic kernel, which the tests check too.  Sizes straddle the 1024-row tile; the device-generated tables give every
workgroup exactly 1, 2 or 3 full tiles (the prefetch re-pointed at the last own tile) plus a ragged tail.  Group keys and
counts are compared exactly, SUM / AVG within 1e-9 relative (small inputs) or 1e-6 (millions of rows, against the C port)."""
import os
import subprocess
import sys
from collections import OrderedDict

os.environ.setdefault("BHIP_KERNEL_TIMING", "1")

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import plan_eval
from oracle.engine import OCol

import helpers

pytestmark = pytest.mark.gpu

RTOL = 1e-9
GENERIC = os.environ.get("BHIP_LEAN_GENERIC", "0") not in ("", "0")


def grid(c, blocks_per_cu):
    """the lean launch's grid: the device's CUs x blocks per CU (3 for the GMAX 4 kernels: LDS; 4 for GMAX 1: launch
    bounds), or BHIP_AGG_BLOCKS_PER_CU where it is set"""
    forced = int(os.environ.get("BHIP_AGG_BLOCKS_PER_CU", "0") or 0)
    return c.device_cus() * (forced or blocks_per_cu)


SCHEMA = dict([("ks", "Utf8"), ("kt", "Utf8"), ("d", "Date32"), ("x", "Float64"), ("y", "Float64"), ("z", "Float64"),
               ("q", "Float64")])
AGGS_Q1 = [E.Sum(col("q"), "sq"), E.Sum(col("x"), "sx"), E.Sum(col("x") * (lit(1.0) - col("y")), "sd"),
           E.Sum(col("x") * (lit(1.0) - col("y")) * (lit(1.0) + col("z")), "sc"), E.Avg(col("q"), "aq"), E.Avg(col("y"), "ay"),
           E.Count(lit(1, E.UINT8), "n")]
Q1_PRED = col("d") <= E.date32("1998-09-02")
Q6_PRED = ((col("d") >= E.date32("1994-01-01")).and_(col("d") < E.date32("1995-01-01"))
           .and_(col("y") >= lit(0.05)).and_(col("y") <= lit(0.07)).and_(col("q") < lit(24.0)))
SHAPES = {   # name: (group, aggregates, predicate)
    "q1": ([(col("ks"), "ks"), (col("kt"), "kt")], AGGS_Q1, Q1_PRED),
    "key1": ([(col("ks"), "ks")], AGGS_Q1, Q1_PRED),
    "q6": ([], [E.Sum(col("x") * col("y"), "revenue")], Q6_PRED),
    "nokey": ([], AGGS_Q1, Q1_PRED),
}


SPECIALISED = ("q1", "key1")      # kernels_lean_spec.hip; Q6 and "nokey" measured faster on the generic kernel


def expected_variant(shape):
    return "lean_spec_" + shape if shape in SPECIALISED and not GENERIC else "lean_generic"


def batch(n, seed, vocab=("A", "N"), vocab2=("F", "O")):
    """at most 4 groups over (ks, kt) with the default vocabularies: the lean path holds 4 per workgroup"""
    rng = np.random.default_rng(seed)
    return OrderedDict([
        ("ks", OCol("Utf8", [vocab[k] for k in rng.integers(0, len(vocab), n)])),
        ("kt", OCol("Utf8", [vocab2[k] for k in rng.integers(0, len(vocab2), n)])),
        ("d", OCol("Date32", rng.integers(8700, 10600, n).astype(np.int32))),
        ("x", OCol("Float64", np.round(rng.uniform(900.0, 105000.0, n), 2))),
        ("y", OCol("Float64", rng.integers(0, 11, n) / 100.0)),
        ("z", OCol("Float64", rng.integers(0, 9, n) / 100.0)),
        ("q", OCol("Float64", rng.integers(1, 51, n).astype(np.float64))),
    ])


def run(ctx, shape, batches, partitions=None):
    group, aggs, pred = SHAPES[shape]
    parts = partitions if partitions is not None else [[b] for b in batches]
    src = ba.FilterExec(E.coerce(pred, SCHEMA), helpers.memory_exec(ctx, parts))
    part = ba.HashAggregateExec(ba.plan.PARTIAL, group, aggs, src)
    fin = ba.HashAggregateExec(ba.plan.FINAL, group, aggs, ba.MergeExec(part))
    ctx.kernel_time(reset=True)
    got = helpers.concat(helpers.collect_product(fin))
    helpers.assert_rows_equal(got, plan_eval.collect(fin), ordered=False, float_rtol=RTOL, key_cols=[n for _, n in group])
    return got


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047])
def test_tile_boundaries(ctx, shape, n):
    run(ctx, shape, [batch(n, 1000 + n)])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_batches_of_unequal_size(ctx, shape):
    bs = [batch(n, 2000 + i) for i, n in enumerate((1, 1024, 17, 4096, 1023, 3, 2049))]
    run(ctx, shape, bs, partitions=[bs[:2], bs[2:5], bs[5:]])


@pytest.mark.parametrize("shape,vocab,vocab2", [
    ("q1", ("", "BB"), ("F", "xyz")), ("key1", ("A", "BB", "CCC", ""), ("F",)),        # 0-3 bytes
    ("q1", ("A", "BBBB"), ("F", "O")), ("key1", ("A", "BBBB", "CC"), ("F",)),          # 4 bytes: the KEY_TOO_LONG rerun
])
def test_string_key_lengths(ctx, shape, vocab, vocab2):
    run(ctx, shape, [batch(3000, 3001, vocab, vocab2), batch(1500, 3002, vocab, vocab2)])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_large_batch_names_the_kernel_that_ran(ctx, shape):
    """a launch over >= 65536 rows is timed, and the timing hook names the instantiation that served it"""
    run(ctx, shape, [batch(70_001, 4000, vocab=("A", "N", "R", "") if shape == "key1" else ("A", "N"))])
    ms, launches = ctx.kernel_time(reset=True)
    assert launches == 1
    assert ctx.kernel_name() == "scan_agg_lean_kernel"
    assert ctx.kernel_name(variant=True) == "scan_agg_lean_kernel/" + expected_variant(shape)


@pytest.mark.parametrize("tiles_per_group", [1, 2, 3])
def test_q1_tiles_per_workgroup(tiles_per_group):
    """device-generated lineitem, every workgroup owning exactly 1, 2 or 3 full tiles, + a ragged tail"""
    from ballista_amd import tpch
    from oracle import gen
    c = ba.Context(0)
    n = grid(c, 3) * 1024 * tiles_per_group + 77
    plan = tpch.q1_stage1(ba.MemoryExec([[ba.plan.tpch_lineitem(c, 1.0, tpch.SEED, 0, n)]], c))
    c.kernel_time(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    assert c.kernel_time(reset=True)[1] == 1 and c.kernel_name(variant=True) == "scan_agg_lean_kernel/" + expected_variant("q1")
    keys, state, count = gen.q1_partial_port(gen.lineitem_arrays(1.0, 0, n), 8, 8)
    want = gen.q1_final_from_port(keys, state, count)
    order = {k: i for i, k in enumerate(zip(got["l_returnflag"].values, got["l_linestatus"].values))}
    assert sorted(order) == sorted(want)
    for k, w in want.items():
        i = order[k]
        assert int(got["count_order[count]"].values[i]) == w["count_order"]
        for name, wname in (("sum_qty[sum]", "sum_qty"), ("sum_base_price[sum]", "sum_base_price"),
                            ("sum_disc_price[sum]", "sum_disc_price"), ("sum_charge[sum]", "sum_charge")):
            assert abs(got[name].values[i] - w[wname]) <= 1e-6 * abs(w[wname]), name


@pytest.mark.parametrize("tiles_per_group", [1, 2, 3])
def test_q6_tiles_per_workgroup(tiles_per_group):
    from ballista_amd import tpch
    from oracle import gen
    c = ba.Context(0)
    n = grid(c, 4) * 1024 * tiles_per_group + 77
    plan = tpch.q6_stage1(ba.MemoryExec([[ba.plan.tpch_lineitem(c, 1.0, tpch.SEED, 0, n)]], c))
    c.kernel_time(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    assert c.kernel_time(reset=True)[1] == 1 and c.kernel_name(variant=True) == "scan_agg_lean_kernel/" + expected_variant("q6")
    s, _ = gen.q6_partial_port(gen.lineitem_arrays(1.0, 0, n), 8, 8)
    want = float(s.sum())
    col_name = [k for k in got if k.startswith("revenue")][0]
    assert abs(float(np.nansum(got[col_name].values)) - want) <= 1e-6 * abs(want)


@pytest.mark.skipif(GENERIC, reason="this is the generic run's parent")
def test_generic_lean_kernel_passes_the_same_checks():
    """BHIP_LEAN_GENERIC=1 forces the generic lean kernel: the same file, in a child process, must pass with it"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BHIP_LEAN_GENERIC="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
