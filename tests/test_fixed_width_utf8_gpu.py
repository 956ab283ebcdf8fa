"""GPU parity of the fixed-width Utf8 key form of the shape-specialised wide-load scan + aggregate kernels
(ballista_amd/csrc/lean_spec_kernel.h, LK_UTF8_FIXED), and of how a column comes to be known as fixed-width.

A Utf8 column whose values all have one width w needs no offsets: row i's bytes are data[offsets[0] + i*w, +w).  The
generator's flag columns are born with that fact; a host batch earns it on its first scan, which ORs and ANDs every length
it reads (equal, and 1..3: uniform) and records the width on the offsets buffer, so the second scan of the same batch runs
the fixed form.  Context.lean_key_form() tells which form the last launch used; BHIP_NO_FIXED_UTF8=1 (read once per process:
the same file runs again in a child) keeps every launch on the offsets form.

Keys and counts are compared exactly, SUM / AVG within 1e-9 relative against the CPU oracle (host batches) or 1e-6 against
the C port (device-generated tables), as in test_lean_specialised_gpu.py.

offsets[0] != 0: no producer inside the library makes such a column today (the generator writes each block's offsets from
0 whatever its first row is, host batches are rebuilt from Python lists, and nothing slices a Utf8 column), so that line
of the kernel is covered by reading only: test_generator_block_at_a_row_offset runs a block that starts at a later row."""
import os
import subprocess
import sys
from collections import OrderedDict

os.environ.setdefault("BHIP_KERNEL_TIMING", "1")

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd import tpch
from ballista_amd.expr import col, lit
from oracle import gen, plan_eval
from oracle.engine import OCol

import helpers

pytestmark = pytest.mark.gpu

RTOL = 1e-9
NO_FIXED = os.environ.get("BHIP_NO_FIXED_UTF8", "0") not in ("", "0")
GENERIC = os.environ.get("BHIP_LEAN_GENERIC", "0") not in ("", "0")
KNOWN = "offsets" if NO_FIXED or GENERIC else "fixed"        # the form of a launch over columns of known width

SCHEMA = dict([("ks", "Utf8"), ("kt", "Utf8"), ("d", "Date32"), ("x", "Float64"), ("y", "Float64"), ("z", "Float64"),
               ("q", "Float64")])
AGGS = [E.Sum(col("q"), "sq"), E.Sum(col("x"), "sx"), E.Sum(col("x") * (lit(1.0) - col("y")), "sd"),
        E.Sum(col("x") * (lit(1.0) - col("y")) * (lit(1.0) + col("z")), "sc"), E.Avg(col("q"), "aq"), E.Avg(col("y"), "ay"),
        E.Count(lit(1, E.UINT8), "n")]
PRED = col("d") <= E.date32("1998-09-02")
GROUPS = {"q1": [(col("ks"), "ks"), (col("kt"), "kt")], "key1": [(col("ks"), "ks")]}
UNIFORM = {1: (("A", "N"), ("F", "O")), 2: (("AA", "NB"), ("FX", "OY")), 3: (("AAA", "NBC"), ("FXY", "OZZ"))}


def batch(n, seed, vocab, vocab2):
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


def collect(ctx, shape, dev, host):
    """the aggregate over device batches `dev` (one partition; `host`: the same rows for the oracle), checked against the
    oracle -> (result, key form of the last launch)"""
    group = GROUPS[shape]
    m = ba.MemoryExec([list(dev)], ctx)
    m._oracle_partitions = [list(host)]
    part = ba.HashAggregateExec(ba.plan.PARTIAL, group, AGGS, ba.FilterExec(E.coerce(PRED, SCHEMA), m))
    fin = ba.HashAggregateExec(ba.plan.FINAL, group, AGGS, ba.MergeExec(part))
    got = helpers.concat(helpers.collect_product(fin))
    form = ctx.lean_key_form()
    helpers.assert_rows_equal(got, plan_eval.collect(fin), ordered=False, float_rtol=RTOL, key_cols=[n for _, n in group])
    return got, form


SAME_RTOL = 1e-14


def same_result(second, first, key_cols):
    """two collects over the same batches: keys and counts exact, sums within 1e-14.  Not bit for bit: two collects of one
    plan on one form already differ in the last bit of a sum now and then (measured here: sx 53914571.05 vs
    53914571.050000004, 1.4e-16 relative, the run-to-run spread profiles/r04_lean_spec_ab.txt records for Q1).  1e-14 is
    some 50 ulp: room for that spread in each of the few partial sums a result is merged from, and far below what a
    different summation order over these 4500 rows gives (about sqrt(n) ulp per partial sum and more)"""
    helpers.assert_rows_equal(second, first, ordered=False, float_rtol=SAME_RTOL, key_cols=key_cols)


def two_batches(ctx, vocab, vocab2, seed=5000):
    host = [batch(3000, seed, vocab, vocab2), batch(1500, seed + 1, vocab, vocab2)]
    return [helpers.to_device(ctx, b) for b in host], host


def q1_on_generator(n, row0=0):
    c = ba.Context(0)
    plan = tpch.q1_stage1(ba.MemoryExec([[ba.plan.tpch_lineitem(c, 1.0, tpch.SEED, row0, n)]], c))
    got = helpers.concat(helpers.collect_product(plan))
    assert c.lean_key_form() == KNOWN
    keys, state, count = gen.q1_partial_port(gen.lineitem_arrays(1.0, row0, n), 8, 8)
    want = gen.q1_final_from_port(keys, state, count)
    order = {k: i for i, k in enumerate(zip(got["l_returnflag"].values, got["l_linestatus"].values))}
    assert sorted(order) == sorted(want)
    for k, w in want.items():
        i = order[k]
        assert int(got["count_order[count]"].values[i]) == w["count_order"]
        for name, wname in (("sum_qty[sum]", "sum_qty"), ("sum_base_price[sum]", "sum_base_price"),
                            ("sum_disc_price[sum]", "sum_disc_price"), ("sum_charge[sum]", "sum_charge")):
            assert abs(got[name].values[i] - w[wname]) <= 1e-6 * abs(w[wname]), name


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047])
def test_generator_tile_boundaries(n):
    q1_on_generator(n)


@pytest.mark.parametrize("tiles_per_group", [1, 2])
def test_generator_last_tile_of_a_workgroup(tiles_per_group):
    """every workgroup owns exactly 1 or 2 full tiles, + a ragged tail: the last own tile is the one the offsets form's
    prefetch is re-pointed at, which the fixed form has no need of"""
    c = ba.Context(0)
    forced = int(os.environ.get("BHIP_AGG_BLOCKS_PER_CU", "0") or 0)
    q1_on_generator(c.device_cus() * (forced or 3) * 1024 * tiles_per_group + 77)


def test_generator_block_at_a_row_offset():
    q1_on_generator(3001, row0=5000)


@pytest.mark.parametrize("shape", ["q1", "key1"])
@pytest.mark.parametrize("w", [1, 2, 3])
def test_host_batches_earn_the_width_on_their_first_scan(ctx, shape, w):
    dev, host = two_batches(ctx, *UNIFORM[w], seed=5100 + w)
    first, form = collect(ctx, shape, dev, host)
    assert form == "offsets"
    second, form = collect(ctx, shape, dev, host)
    assert form == KNOWN
    same_result(second, first, [n for _, n in GROUPS[shape]])


@pytest.mark.parametrize("shape", ["q1", "key1"])
@pytest.mark.parametrize("vocab", [("A", "BB"), ("", "B"), ("",), ("A", "BBBB")],
                         ids=["lengths-1-2", "lengths-0-1", "all-empty", "4-bytes-rerun"])
def test_columns_that_never_earn_it(ctx, shape, vocab):
    dev, host = two_batches(ctx, vocab, vocab, seed=5200)
    for _ in range(3):
        _, form = collect(ctx, shape, dev, host)
        assert form == "offsets"


def test_one_known_and_one_mixed_key_read_the_offsets(ctx):
    """ks: width 1 throughout (known after the first scan), kt: lengths 1 and 2 — no mixed instantiation exists"""
    dev, host = two_batches(ctx, ("A", "N"), ("F", "OO"), seed=5300)
    first, form = collect(ctx, "q1", dev, host)
    assert form == "offsets"
    _, form = collect(ctx, "key1", dev, host)            # ks alone: known
    assert form == KNOWN
    second, form = collect(ctx, "q1", dev, host)
    assert form == "offsets"
    same_result(second, first, ["ks", "kt"])


def test_concatenation_and_filter_of_known_columns(ctx):
    """whatever becomes of the fact in a concatenation or a filter (today: dropped, the new buffers start unknown), an
    aggregate over the result is right, and so is a second one"""
    dev, host = two_batches(ctx, *UNIFORM[2], seed=5400)
    _, form = collect(ctx, "q1", dev, host)
    assert form == "offsets"
    whole = ba.plan.concat(ctx, dev)
    whole_host = OrderedDict((k, OCol(c.dtype, list(host[0][k].values) + list(host[1][k].values) if c.dtype == "Utf8"
                                      else np.concatenate([host[0][k].values, host[1][k].values]))) for k, c in host[0].items())
    for _ in range(2):
        collect(ctx, "q1", [whole], [whole_host])
    # a filter that is not fused into the aggregate: its output columns are new ones
    group = GROUPS["q1"]
    m = ba.MemoryExec([[b] for b in dev], ctx)
    m._oracle_partitions = [[b] for b in host]
    kept = ba.CoalesceBatchesExec(ba.FilterExec(E.coerce(col("q") < lit(40.0), SCHEMA), m), 4096)
    part = ba.HashAggregateExec(ba.plan.PARTIAL, group, AGGS, ba.FilterExec(E.coerce(PRED, SCHEMA), kept))
    fin = ba.HashAggregateExec(ba.plan.FINAL, group, AGGS, ba.MergeExec(part))
    got = helpers.concat(helpers.collect_product(fin))
    helpers.assert_rows_equal(got, plan_eval.collect(fin), ordered=False, float_rtol=RTOL, key_cols=["ks", "kt"])


@pytest.mark.skipif(NO_FIXED, reason="this is the switched-off run's parent")
def test_switched_off_passes_the_same_checks():
    """BHIP_NO_FIXED_UTF8=1 makes dispatch ignore the widths: the same file, in a child process, with every form `offsets`"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BHIP_NO_FIXED_UTF8="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
