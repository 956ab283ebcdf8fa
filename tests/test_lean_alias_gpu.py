"""GPU parity of step aliasing in the shape-specialised wide-load scan + aggregate kernels
(ballista_amd/csrc/lean_spec_kernel.h): two chain steps of a plan that read one column (Q1: `1 - y` inside the products and
`y` for avg(y)) share one load of it.  Context.lean_step_alias() tells which code ran: "0,1,2,3,2" for the aliased
instantiation, "none" where every step loaded its own column.  BHIP_LEAN_NO_ALIAS=1 (read once per process, so it is set in a
child process) sends every plan to the un-aliased instantiations.

Tables follow tests/test_lean_specialised_gpu.py: sizes around the 1024-row tile, and device CUs x 3 workgroups x 1024 x k +
1000 rows, which gives every workgroup exactly k full tiles (odd and even counts, the last tile on both parities of the
two-tile loop) plus a ragged tail.  Every result is compared with the CPU oracle (oracle/plan_eval.py): keys and counts
exact, SUM / AVG within 1e-9 relative.

Bit for bit (n <= 2047): aliasing changes where a step's value comes from, not the order in which an accumulator receives a
thread's rows, so every per-thread partial is the same number.  With n <= 2047 at most two workgroups hold rows (one full
tile, and the tail), so the merge adds at most two partials per group, and a + b == b + a: the sums of the aliased and the
un-aliased run must be the same 64-bit patterns.  That is derived, not measured."""
import functools
import json
import os
import struct
import subprocess
import sys
from collections import OrderedDict

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
Q1_ALIAS = "0,1,2,3,2"
NO_ALIAS = os.environ.get("BHIP_LEAN_NO_ALIAS", "0") not in ("", "0")
GENERIC = os.environ.get("BHIP_LEAN_GENERIC", "0") not in ("", "0")
NO_FIXED = os.environ.get("BHIP_NO_FIXED_UTF8", "0") not in ("", "0")
ALIASED = "none" if NO_ALIAS or GENERIC else Q1_ALIAS        # what a plan with Q1's pattern reports
KNOWN = "offsets" if NO_FIXED or GENERIC else "fixed"        # the key form of a launch over columns of known width

SCHEMA = dict([("ks", "Utf8"), ("kt", "Utf8"), ("d", "Date32"), ("x", "Float64"), ("y", "Float64"), ("z", "Float64"),
               ("q", "Float64"), ("w", "Float64")])
PRED = col("d") <= E.date32("1998-09-02")
HEAD = [E.Sum(col("q"), "sq"), E.Sum(col("x"), "sx"), E.Sum(col("x") * (lit(1.0) - col("y")), "sd"),
        E.Sum(col("x") * (lit(1.0) - col("y")) * (lit(1.0) + col("z")), "sc"), E.Avg(col("q"), "aq")]
COUNT = [E.Count(lit(1, E.UINT8), "n")]
AGGS_Q1 = HEAD + [E.Avg(col("y"), "ay")] + COUNT             # steps q, x, 1-y, 1+z, y: {0,1,2,3,2}
AGGS_DISTINCT = HEAD + [E.Sum(col("w"), "sw")] + COUNT       # steps q, x, 1-y, 1+z, w: five columns
AGGS_OTHER = HEAD + [E.Sum(col("z"), "sz")] + COUNT          # steps q, x, 1-y, 1+z, z: {0,1,2,3,3}
GROUPS = {"q1": [(col("ks"), "ks"), (col("kt"), "kt")], "key1": [(col("ks"), "ks")]}
SMALL = [1023, 1024, 1025, 2047]


def batch(n, seed, y=None, d=None):
    rng = np.random.default_rng(seed)
    ks, kt = np.array(["A", "N"], dtype=object), np.array(["F", "O"], dtype=object)
    return OrderedDict([
        ("ks", OCol("Utf8", list(ks[rng.integers(0, 2, n)]))),
        ("kt", OCol("Utf8", list(kt[rng.integers(0, 2, n)]))),
        ("d", OCol("Date32", rng.integers(8700, 10600, n).astype(np.int32) if d is None else d)),
        ("x", OCol("Float64", np.round(rng.uniform(900.0, 105000.0, n), 2))),
        ("y", OCol("Float64", rng.integers(0, 11, n) / 100.0 if y is None else y)),
        ("z", OCol("Float64", rng.integers(0, 9, n) / 100.0)),
        ("q", OCol("Float64", rng.integers(1, 51, n).astype(np.float64))),
        ("w", OCol("Float64", np.round(rng.uniform(-50.0, 50.0, n), 3))),
    ])


def twice(ctx, shape, aggs, host, pred=PRED):
    """two collects of the aggregate over the same device batch, each checked against the oracle (evaluated once): the first
    reads the key offsets and learns the width, the second takes it as given -> [(result, step alias)] of the two forms"""
    group = GROUPS[shape]
    dev = helpers.to_device(ctx, host)
    out, want = [], None
    for want_form in ("offsets", KNOWN):
        m = ba.MemoryExec([[dev]], ctx)
        m._oracle_partitions = [[host]]
        part = ba.HashAggregateExec(ba.plan.PARTIAL, group, aggs, ba.FilterExec(E.coerce(pred, SCHEMA), m))
        fin = ba.HashAggregateExec(ba.plan.FINAL, group, aggs, ba.MergeExec(part))
        got = helpers.concat(helpers.collect_product(fin))
        assert ctx.lean_key_form() == want_form
        alias = ctx.lean_step_alias()
        want = plan_eval.collect(fin) if want is None else want
        helpers.assert_rows_equal(got, want, ordered=False, float_rtol=RTOL, key_cols=[n for _, n in group])
        out.append((got, alias))
    return out


def grid_rows(ctx, k):
    forced = int(os.environ.get("BHIP_AGG_BLOCKS_PER_CU", "0") or 0)
    return ctx.device_cus() * (forced or 3) * 1024 * k + 1000


@pytest.mark.parametrize("shape", ["q1", "key1"])
@pytest.mark.parametrize("n", SMALL)
def test_tile_boundaries(ctx, shape, n):
    for _, alias in twice(ctx, shape, AGGS_Q1, batch(n, 7000 + n)):
        assert alias == ALIASED


@functools.lru_cache(maxsize=1)
def grid_table(n, seed):
    return batch(n, seed)


@pytest.mark.parametrize("shape", ["q1", "key1"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_tiles_per_workgroup(ctx, shape, k):
    """every workgroup owns exactly k full tiles (+ a tail): one table per k, shared by the two shapes"""
    for _, alias in twice(ctx, shape, AGGS_Q1, grid_table(grid_rows(ctx, k), 7100 + k)):
        assert alias == ALIASED


def sum_bits(got, key_cols):
    """{key: {column: 64-bit pattern}} of the Float64 columns of a result"""
    names = list(got.keys())
    out = {}
    for row in helpers.rows_of(got):
        r = dict(zip(names, row))
        out["|".join(str(r[k]) for k in key_cols)] = {
            n: "%016x" % struct.unpack("<Q", struct.pack("<d", r[n]))[0] for n in names if got[n].dtype == "Float64"}
    return out


def small_sums(ctx):
    """{"shape/n/form": sum_bits} of Q1's aggregates over the SMALL tables, offsets and fixed form"""
    out = {}
    for shape in ("q1", "key1"):
        for n in SMALL:
            for form, (got, alias) in zip(("offsets", "fixed"), twice(ctx, shape, AGGS_Q1, batch(n, 7000 + n))):
                assert alias == ALIASED
                out[f"{shape}/{n}/{form}"] = sum_bits(got, [name for _, name in GROUPS[shape]])
    return out


@pytest.mark.skipif(NO_ALIAS, reason="this is the switched-off run's parent")
def test_sums_bit_for_bit_against_the_unaliased_kernel(ctx):
    """BHIP_LEAN_NO_ALIAS=1 in a child process: every sum and average of the SMALL tables has the default run's bits"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BHIP_LEAN_NO_ALIAS="1",
               PYTHONPATH=os.pathsep.join([os.path.dirname(here), here] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    p = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], cwd=os.path.dirname(here), env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    theirs = json.loads(p.stdout.strip().splitlines()[-1])
    mine = small_sums(ctx)
    assert sorted(mine) == sorted(theirs)
    for case in mine:
        assert mine[case] == theirs[case], case


def test_five_distinct_step_columns(ctx):
    """SUM(w) in place of avg(y): no step repeats a column, the plan runs un-aliased (after an aliased one, so the
    accessor's answer is this launch's)"""
    host = batch(3 * 1024 + 500, 7200)
    for shape in ("q1", "key1"):
        assert twice(ctx, shape, AGGS_Q1, host)[1][1] == ALIASED
        for _, alias in twice(ctx, shape, AGGS_DISTINCT, host):
            assert alias == "none"


def test_another_duplicate_pattern(ctx):
    """SUM(z) as the fifth aggregate: step 4 repeats step 3's column, {0,1,2,3,3}, which no instantiation aliases"""
    host = batch(3 * 1024 + 500, 7300)
    for shape in ("q1", "key1"):
        assert twice(ctx, shape, AGGS_Q1, host)[1][1] == ALIASED
        for _, alias in twice(ctx, shape, AGGS_OTHER, host):
            assert alias == "none"


@pytest.mark.parametrize("n", [1025, 2 * 1024 + 3])
def test_negative_zero_and_one_in_the_shared_column(ctx, n):
    """y holds -0.0 and 1.0 (no NULLs): 1 - y is 1.0 and 0.0 through the sign flip, while avg(y) takes y as it is — both from
    one set of registers.  Rows of both kinds in the full tile and in the tail"""
    rng = np.random.default_rng(7400 + n)
    y = rng.integers(0, 11, n) / 100.0
    y[[0, 1, 511, 1024, n - 1]] = [-0.0, 1.0, -0.0, 1.0, -0.0]
    y[rng.integers(2, n - 1, 40)] = -0.0
    y[rng.integers(2, n - 1, 40)] = 1.0
    for shape in ("q1", "key1"):
        for _, alias in twice(ctx, shape, AGGS_Q1, batch(n, 7500 + n, y=y)):
            assert alias == ALIASED


def test_ranges_that_filter_a_threads_rows_and_every_row(ctx):
    """thread 5's row pair of both sub-tiles of the first tile fails the range, then every row does: the branch-free add of
    +0.0 takes the aliased step's value like any other"""
    n = 2 * 1024 + 100
    d = np.random.default_rng(7600).integers(8700, 10400, n).astype(np.int32)          # all pass PRED ...
    d[[10, 11, 512 + 10, 512 + 11]] = 10590                                              # ... but thread 5's four rows
    host = batch(n, 7601, d=d)
    for shape in ("q1", "key1"):
        for _, alias in twice(ctx, shape, AGGS_Q1, host):
            assert alias == ALIASED
        for got, alias in twice(ctx, shape, AGGS_Q1, host, pred=col("d") <= E.date32("1990-01-01")):
            assert alias == ALIASED and len(helpers.rows_of(got)) == 0


if __name__ == "__main__":
    # the child of test_sums_bit_for_bit_against_the_unaliased_kernel: the SMALL sums of this process, as one JSON line
    print(json.dumps(small_sums(ba.Context(0))))
