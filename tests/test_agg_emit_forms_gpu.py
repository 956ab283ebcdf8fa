"""GPU parity of the three forms in which HashAggregateExec turns its group table into the output batch, and that each one ran.

All three fill columns that ONE allocator made (ballista_amd/csrc/host/ops_agg.cpp: alloc_emit_columns):
  * emit_all      every column in one launch, queued behind the merge of the register path with the count read on the device;
  * per column    emit_group_key per fixed-width key, emit_group_utf8_small or emit_group_key + emit_group_utf8 per Utf8 key,
                  emit_group_values per EMIT_BATCH_MAX = 16 state columns: whatever emit_all does not take — more than
                  TAIL_TOTALS = 5 keys, a table of the hash path, BHIP_NO_EARLY_EMIT=1;
  * emit_slots    every column in one launch straight from the run slots of a clustered hash aggregate.
Every case asserts its result against the CPU oracle, from Context.kernel_stats() at BHIP_KERNEL_TIMING=2 which emit
launches ran, and on the returned batch: the row count, that a Utf8 key column's offsets end at (and its byte count is) the
oracle's byte total, and that a non-nullable field carries no validity buffer.  Every input builder first asserts in numpy
the shape it is meant to have.

Keys, COUNT and integer SUM compare exactly; Float64 SUM within 1e-9 relative over positive addends.

Two inputs differ from the sizes first proposed for them, because the register path gives up per WORKGROUP (a 512-row tile
that meets more than 4 / 8 groups), not on the number of groups of the whole input:
  * more than 16 state columns: 12 groups, not 3 — three groups stay on the register path, whose early emit is emit_all;
  * run slots: 4 096 sorted rows in 512 groups of 8 rows, not 16 groups of 256 — a tile of 16 sorted groups holds two or three
    of them, the register path keeps the input and emit_all runs (test_sixteen_sorted_groups_stay_on_the_register_path pins that).
"""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import plan_eval
from oracle.engine import OCol

import helpers

pytestmark = pytest.mark.gpu

RTOL = 1e-9
NO_EARLY_EMIT = os.environ.get("BHIP_NO_EARLY_EMIT", "0") not in ("", "0")      # read once per process by the library
TILE = 512                                                                      # rows a workgroup of the register path meets at least


def timed_context(monkeypatch):
    monkeypatch.setenv("BHIP_KERNEL_TIMING", "2")             # every launch, however small (read when a context is created)
    return ba.Context(0)


def launches(ks, name):
    return ks[name][1] if name in ks else 0


def utf8_offsets(rb, i):
    """the offsets of Utf8 column i as the batch holds them"""
    n, nbytes = rb.num_rows, rb.column_info(i)[3]
    off, data = np.zeros(n + 1, np.int32), np.zeros(max(1, nbytes), np.uint8)
    vbuf = np.zeros((n + 7) // 8 + 8, np.uint8)
    L.check(L.lib().bhip_batch_column_to_host(rb._h, i, data.ctypes.data, off.ctypes.data,
                                              vbuf.ctypes.data if rb.column_info(i)[4] else None))
    return off


def run(ctx, plan, key_cols):
    """partition 0 of `plan` on the device against the oracle -> (the launches it made, the oracle's batch)"""
    want = helpers.concat(plan_eval.execute(plan, 0))
    ctx.kernel_stats(reset=True)
    batches = list(plan.execute(0))
    ks = ctx.kernel_stats(reset=True)
    helpers.assert_rows_equal(helpers.concat([helpers.from_device(b) for b in batches]), want, ordered=False, float_rtol=RTOL,
                              key_cols=key_cols)
    assert len(batches) == 1
    rb, n_groups = batches[0], len(helpers.rows_of(want))
    assert rb.num_rows == n_groups
    for i, (name, c) in enumerate(want.items()):
        _, dtype, nullable, nbytes, has_valid = rb.column_info(i)
        assert nullable or (not has_valid and not rb.column_device(i)[2]), name
        if dtype == "Utf8" and name in key_cols:
            total = sum(len(s.encode()) for s in c.to_pylist() if s is not None)
            off = utf8_offsets(rb, i)
            assert off[0] == 0 and off[-1] == total and nbytes == total, (name, int(off[-1]), nbytes, total)
    return ks, want


def values(rng, n, valid=None):
    """a positive Float64 column"""
    return OCol("Float64", np.round(rng.random(n) * 100 + 1, 2), valid)


# ---- every column in one launch, and the same plan column by column ----------------------------------------------------------

def three_key_batch():
    """1 000 rows, 3 groups over three keys: a nullable Int32 (one group's key is NULL), a Boolean, a 2-byte Utf8"""
    rng = np.random.default_rng(11)
    n = 1000
    g = rng.integers(0, 3, n)
    g[:3] = [0, 1, 2]
    a = np.array([5, 0, -7], np.int32)[g]
    a_valid = g != 1
    b = np.array([True, False, True])[g]
    s = [("ab", "cd", "ef")[k] for k in g]
    assert len({(x if v else None, y, z) for x, v, y, z in zip(a, a_valid, b, s)}) == 3
    assert {len(x.encode()) for x in s} == {2} and not a_valid.all() and a_valid.any() and len(set(b)) == 2
    return OrderedDict([("a", OCol("Int32", a, a_valid)), ("b", OCol("Boolean", b)), ("s", OCol("Utf8", s)),
                        ("x", values(rng, n, rng.random(n) > 0.1)), ("q", OCol("Int32", rng.integers(0, 50, n)))])


def test_all_columns_in_one_launch(monkeypatch):
    """three keys are within TAIL_TOTALS: the register path queues emit_all behind its merge.  Under BHIP_NO_EARLY_EMIT=1 (the
    child process of the next test) the same table is emitted column by column once the host knows the count"""
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[three_key_batch()]])
    aggs = [E.Sum(col("x"), "sx"), E.Count(col("x"), "cx"), E.Count(lit(1, E.UINT8), "n"), E.Sum(col("q"), "sq")]
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("a"), "a"), (col("b"), "b"), (col("s"), "s")], aggs, m)
    ks, want = run(ctx, plan, ["a", "b", "s"])
    assert len(helpers.rows_of(want)) == 3 and None in want["a"].to_pylist()
    if NO_EARLY_EMIT:
        assert launches(ks, "emit_group_key") == 2 and launches(ks, "emit_group_utf8_small") == 1 and launches(ks, "emit_group_values") == 1, ks
        assert "emit_all" not in ks, ks
    else:
        assert launches(ks, "emit_all") == 1 and "emit_group_key" not in ks and "emit_group_values" not in ks, ks
        assert "emit_group_utf8_small" not in ks and "emit_group_utf8" not in ks, ks


def test_same_plan_without_the_early_emit():
    """BHIP_NO_EARLY_EMIT is read once per process: the case above in a child process with the switch set"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BHIP_NO_EARLY_EMIT="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-k", "test_all_columns_in_one_launch",
                        os.path.abspath(__file__)], cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert "1 passed" in p.stdout, p.stdout[-2000:]


# ---- per column ------------------------------------------------------------------------------------------------------------

def test_more_keys_than_the_early_emit_takes(monkeypatch):
    """six Int16 keys (12 bytes of packed key): more than TAIL_TOTALS, so nothing is queued early and every key column is one
    emit_group_key launch"""
    rng = np.random.default_rng(12)
    n = 1000
    g = rng.integers(0, 3, n)
    g[:3] = [0, 1, 2]
    parts = np.array([[1, -2, 300], [7, 7, 7], [-32768, 0, 32767], [4, 5, 4], [9, 8, 8], [-1, -1, -2]], np.int16)
    assert len({tuple(parts[:, k]) for k in range(3)}) == 3 and len(parts) > 5
    batch = OrderedDict([(f"k{j}", OCol("Int16", parts[j][g])) for j in range(6)])
    batch["x"], batch["q"] = values(rng, n, rng.random(n) > 0.1), OCol("Int32", rng.integers(0, 50, n))
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[batch]])
    keys = [f"k{j}" for j in range(6)]
    aggs = [E.Sum(col("x"), "sx"), E.Count(lit(1, E.UINT8), "n"), E.Sum(col("q"), "sq")]
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col(k), k) for k in keys], aggs, m)
    ks, want = run(ctx, plan, keys)
    assert len(helpers.rows_of(want)) == 3
    assert launches(ks, "emit_group_key") == 6 and launches(ks, "emit_group_values") == 1 and "emit_all" not in ks, ks


def test_more_value_columns_than_one_launch_takes(monkeypatch):
    """nine AVGs over distinct Float64 columns are 18 state columns in Partial mode: two emit_group_values launches.  Nine
    accumulators leave the register path at four groups per workgroup; 12 groups in random order send the plan to the hash table,
    whose GroupRec table (a Utf8 key: no slot emit) is emitted column by column"""
    rng = np.random.default_rng(13)
    n = 1000
    vocab = [f"g{k:02d}" for k in range(12)]
    g = rng.integers(0, len(vocab), n)
    g[:len(vocab)] = np.arange(len(vocab))
    rng.shuffle(g)
    s = [vocab[k] for k in g]
    assert len(set(s)) == 12 > 8 and s != sorted(s) and {len(x) for x in s} == {3}
    assert all(len(set(s[lo:lo + 256])) > 4 for lo in range(0, n, 256))          # every workgroup overflows (16 accumulators: 256-row tiles)
    batch = OrderedDict([("s", OCol("Utf8", s))] + [(f"v{j}", values(rng, n)) for j in range(9)])
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[batch]])
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("s"), "s")], [E.Avg(col(f"v{j}"), f"a{j}") for j in range(9)], m)
    ks, want = run(ctx, plan, ["s"])
    assert len(want) == 1 + 18 and len(helpers.rows_of(want)) == 12
    assert "scan_agg_hash" in ks and launches(ks, "emit_group_values") == 2 and launches(ks, "emit_group_utf8_small") == 1, ks


def test_utf8_key_of_a_large_table(monkeypatch):
    """more than EMIT_UTF8_SMALL_MAX = 4096 groups with a Utf8 key: lengths (emit_group_key), a device-wide scan, then the bytes
    (emit_group_utf8)"""
    rng = np.random.default_rng(14)
    n, distinct = 5000, 4500
    vocab = [f"{k:04d}" for k in rng.permutation(10000)[:distinct]]
    g = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    rng.shuffle(g)
    s = [vocab[k] for k in g]
    assert len(s) == n and len(set(s)) == distinct >= 4097 and {len(x.encode()) for x in s} == {4}
    batch = OrderedDict([("s", OCol("Utf8", s)), ("q", OCol("Int32", rng.integers(0, 50, n)))])
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[batch]])
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("s"), "s")], [E.Count(lit(1, E.UINT8), "n"), E.Sum(col("q"), "sq")], m)
    ks, want = run(ctx, plan, ["s"])
    assert len(helpers.rows_of(want)) == distinct
    assert launches(ks, "emit_group_key") == 1 and launches(ks, "emit_group_utf8") == 1 and "emit_group_utf8_small" not in ks, ks
    assert launches(ks, "emit_group_values") == 1, ks


# ---- run slots -------------------------------------------------------------------------------------------------------------

def sorted_batch(n, groups):
    """n rows sorted by an Int32 key in `groups` runs of equal length, one nullable Float64"""
    rng = np.random.default_rng(15)
    k = np.repeat(np.arange(groups, dtype=np.int32) * 3 + 10, n // groups)
    assert len(k) == n >= 4096 and (np.diff(k) >= 0).all() and len(np.unique(k)) == groups and 2 * groups <= n
    valid = rng.random(n) > 0.1
    assert not valid.all()
    return OrderedDict([("k", OCol("Int32", k)), ("x", values(rng, n, valid))]), k


def sorted_plan(ctx, batch):
    m = helpers.memory_exec(ctx, [[batch]])
    return ba.HashAggregateExec(ba.plan.PARTIAL, [(col("k"), "k")], [E.Sum(col("x"), "sx")], m)


def test_run_slots(monkeypatch):
    """4 096 rows (what the run detection needs) sorted by the key, 8 rows per group: every 512-row tile holds 64 groups, the
    register path gives up, the hash path finds every run a group of its own and emits straight from the run slots"""
    batch, k = sorted_batch(4096, 512)
    assert all(len(np.unique(k[lo:lo + TILE])) > 8 for lo in range(0, len(k), TILE))
    ctx = timed_context(monkeypatch)
    ks, want = run(ctx, sorted_plan(ctx, batch), ["k"])
    assert len(helpers.rows_of(want)) == 512
    assert launches(ks, "emit_slots") == 1 and "emit_group_key" not in ks and "emit_group_values" not in ks, ks
    assert "run_heads" in ks and "scan_agg_hash" in ks, ks


def test_sixteen_sorted_groups_stay_on_the_register_path(monkeypatch):
    """the same input in 16 groups of 256 rows: more than 8 groups in all, but two per 512-row tile — no workgroup overflows, the
    merge holds up to 1 024 groups, and the table leaves through emit_all; no hash path, no run slots"""
    batch, k = sorted_batch(4096, 16)
    assert all(len(np.unique(k[lo:lo + TILE])) <= 4 for lo in range(0, len(k), TILE))
    ctx = timed_context(monkeypatch)
    ks, want = run(ctx, sorted_plan(ctx, batch), ["k"])
    assert len(helpers.rows_of(want)) == 16
    if not NO_EARLY_EMIT:
        assert launches(ks, "emit_all") == 1, ks
    assert "emit_slots" not in ks and "scan_agg_hash" not in ks, ks
