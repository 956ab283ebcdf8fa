"""GPU parity of HashAggregateExec when what the operator LEARNED is false for the rows it is applied to next.

The operator does not pick its kernel from the plan alone (ballista_amd/csrc/host/ops_agg.cpp): it keeps, on itself and on
the column buffers,
  * path_hint_       the register path's group width (4 -> 8 -> hash table), from an overflow of an earlier run or, on a plan
                     that has not run, from the leading 32768 rows of the FIRST batch;
  * clustered_hint_  "the input is clustered by group key" (hash path), from the leading min(rows, 2^20) rows; 1 forces the
                     run path without looking, -1 never looks again;
  * distinct_runs    runs are groups / two ascending stretches / the run table, from the breaks counted in that sample and
                     re-read after the full pass;
  * Buffer::uniform_width  "every value of this Utf8 key column is w bytes", from the lengths the wide-load scan read.
plan.execute(p) for different p shares one operator and so its hints.  Every case here makes the learned fact wrong for
the next rows: another partition, a tail unlike the head, rows behind a predicate.  Each case asserts the result against
the CPU oracle AND, from Context.kernel_stats() at BHIP_KERNEL_TIMING=2 (every launch is named), that the path it was
written for ran.  Every input builder first asserts in numpy the shape it is meant to have.

Keys, COUNT, MIN, MAX and integer SUM compare exactly; Float64 SUM / AVG within 1e-9 relative over positive addends (an
equally valid order of addition over cancelling sums defeats any relative gate: test_operators_gpu.py).

Launches each section asserts (read off ops_agg.cpp), per section:
  1  scan_agg_lowcard_g8 (the head probe), scan_agg_lowcard_g4 / _g8 (and _batches), merge_partials once per round,
     scan_agg_hash after the last overflow; second run: only the width the hint names
  2  scan_agg_lowcard_g4 -> _g8 -> scan_agg_hash over the partitions, then scan_agg_hash alone; Utf8 key:
     scan_agg_lean_kernel -> scan_agg_sop_kernel -> scan_agg_hash
  3  run_heads, run_slots, run_groups, run_tail_resolve, run_tail_remap, emit_slots, det_spill_combine as asserted per case
  4  Context.lean_key_form() "offsets" throughout where a length differs, "fixed" once a width was earned
"""
import os
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
HEAD = 32768                      # rows of the first batch the register path's sampler reads
N_MID = (1 << 17) + 1000          # sampled with more than four accumulators
N_BIG = (1 << 20) + 1000          # sampled whatever the accumulators
SAMPLE = 1 << 20                  # rows the hash path's run detection reads first
N_RUNS = SAMPLE + 8192            # the smallest input whose run sample is not the whole of it
NO_FIXED = os.environ.get("BHIP_NO_FIXED_UTF8", "0") not in ("", "0") or os.environ.get("BHIP_LEAN_GENERIC", "0") not in ("", "0")
KNOWN = "offsets" if NO_FIXED else "fixed"


def timed_context(monkeypatch):
    monkeypatch.setenv("BHIP_KERNEL_TIMING", "2")             # every launch, however small (read when a context is created)
    return ba.Context(0)


def launches(ks, *names):
    return sum(ks[n][1] for n in names if n in ks)


def g4(ks):
    return launches(ks, "scan_agg_lowcard_g4", "scan_agg_lowcard_g4_batches")


def g8(ks):
    return launches(ks, "scan_agg_lowcard_g8", "scan_agg_lowcard_g8_batches")


def run_partition(ctx, plan, p, want, key_cols):
    """one partition of `plan` on the device against `want` -> the launches it made"""
    ctx.kernel_stats(reset=True)
    got = helpers.concat([helpers.from_device(b) for b in plan.execute(p)])
    ks = ctx.kernel_stats(reset=True)
    helpers.assert_rows_equal(got, want, ordered=False, float_rtol=RTOL, key_cols=key_cols)
    return ks


def oracle_partition(plan, p):
    return helpers.concat(plan_eval.execute(plan, p))


def n_runs(key):
    return 1 + int(np.count_nonzero(key[1:] != key[:-1])) if len(key) else 0


def breaks(key):
    """rows that start a run whose key does not exceed the key in front of it (what run_heads counts)"""
    return np.flatnonzero(key[1:] < key[:-1]) + 1


# ---- sections 1 and 2: an Int32 key, a nullable summed Float64, an Int32 value ---------------------------------------------

# six accumulators (SUM x, COUNT x, MIN q, MAX q, SUM q as double, SUM q): more than four, so a plan that has not run samples
# from 2^17 rows on and has no "start at 8" shortcut; MIN / MAX / COUNT(x) keep the plan on the expression VM's register
# kernel (scan_agg_lowcard_*), whose launches are named by width
AGGS6 = [E.Sum(col("x"), "sx"), E.Count(col("x"), "cx"), E.Count(lit(1, E.UINT8), "n"), E.Min(col("q"), "mn"), E.Max(col("q"), "mx"),
         E.Avg(col("q"), "aq"), E.Sum(col("q"), "sq")]
# two accumulators (SUM x, COUNT x)
AGGS2 = [E.Sum(col("x"), "sx"), E.Count(col("x"), "cx"), E.Count(lit(1, E.UINT8), "n")]
KEY_VALUES = np.array([-2**31, -7, 0, 3, 11, 4096, 65536, 2**31 - 1, 42, 100, 101, 102], dtype=np.int64)


def int_batch(key, rng, key_valid=None):
    n = len(key)
    return OrderedDict([("k", OCol("Int32", np.asarray(key, dtype=np.int32), key_valid)),
                        ("x", OCol("Float64", np.round(rng.random(n) * 100 + 1, 2), rng.random(n) > 0.1)),
                        ("q", OCol("Int32", rng.integers(0, 50, n)))])


def key_pool(n_keys):
    """the first n_keys of KEY_VALUES, then 5000, 5003, ... (a smaller pool is a prefix of a larger one)"""
    return np.concatenate([KEY_VALUES, np.arange(max(n_keys - len(KEY_VALUES), 0), dtype=np.int64) * 3 + 5000])[:n_keys]


def draw(rng, n, n_keys):
    """n rows in random order over n_keys keys, every key present"""
    pool = key_pool(n_keys)
    k = pool[rng.integers(0, n_keys, n)]
    k[:n_keys] = pool
    rng.shuffle(k)
    return k


def head_tail(rng, n, head_keys, all_keys, head=HEAD):
    """the first `head` rows over head_keys keys, the rest over all_keys"""
    k = np.concatenate([draw(rng, head, head_keys), draw(rng, n - head, all_keys)])
    assert len(np.unique(k[:head])) == head_keys and len(np.unique(k)) == all_keys
    # a workgroup overflows on what IT meets (512-row tiles): every tile behind the head holds more groups than a narrower width
    assert all(len(np.unique(k[lo:lo + 512])) >= min(all_keys, 9) for lo in range(head, n - 512, 512))
    return k


# case -> (key arrays of the batches of the one partition, launches of the first run, hint afterwards)
# rounds = merge_partials launches: one per turn of the ladder, the head probe included
def sampler_case(name, n):
    rng = np.random.default_rng(sum(map(ord, name)) + n)
    if name == "head3_whole7":
        return [head_tail(rng, n, 3, 7)], dict(rounds=3, g4=True, g8=True, hash=False), 8
    if name == "head3_whole9":
        return [head_tail(rng, n, 3, 9)], dict(rounds=3, g4=True, g8=True, hash=True), -1
    if name == "head3_whole3000":
        return [head_tail(rng, n, 3, 3000)], dict(rounds=3, g4=True, g8=True, hash=True), -1
    if name == "head6_ninth_in_last_tile":
        k = head_tail(rng, n, 6, 8)
        last = 300                                             # within the ragged last tile of 512 and of 1024 rows
        assert last <= n % 512
        k[n - last:] = draw(rng, last, 9)
        ninth = KEY_VALUES[8]
        assert len(np.unique(k[:HEAD])) == 6 and len(np.unique(k[:n - last])) == 8 and len(np.unique(k[n - last:])) == 9
        assert np.flatnonzero(k == ninth).min() >= n - n % 512
        return [k], dict(rounds=2, g4=False, g8=True, hash=True), -1
    if name in ("second_batch_adds_to_7", "second_batch_adds_to_12"):
        total = 7 if name.endswith("_7") else 12
        b0, b1 = draw(rng, n, 3), draw(rng, 5000, total)
        assert len(np.unique(b0)) == 3 and len(np.unique(np.concatenate([b0, b1]))) == total
        return [b0, b1], dict(rounds=3, g4=True, g8=True, hash=total > 8), 8 if total <= 8 else -1
    if name == "first_batch_shorter_than_the_head":
        b0, b1 = draw(rng, 20000, 3), draw(rng, n - 20000, 7)
        assert len(b0) < HEAD and len(np.unique(b0)) == 3 and len(np.unique(b1)) == 7
        return [b0, b1], dict(rounds=3, g4=True, g8=True, hash=False), 8
    if name == "empty_first_batch":
        b1 = head_tail(rng, n, 3, 7)
        return [np.zeros(0, np.int64), b1], dict(rounds=3, g4=True, g8=True, hash=False), 8
    raise KeyError(name)


SAMPLER_CASES = ["head3_whole7", "head3_whole9", "head3_whole3000", "head6_ninth_in_last_tile", "second_batch_adds_to_7",
                 "second_batch_adds_to_12", "first_batch_shorter_than_the_head", "empty_first_batch"]


@pytest.mark.parametrize("size", ["mid", "big"])
@pytest.mark.parametrize("name", SAMPLER_CASES)
def test_head_that_misleads_the_register_path_sampler(name, size, monkeypatch):
    """the leading 32768 rows of the first batch pick the width; the rest of the input has more groups.  mid: 2^17 + 1000 rows and
    six accumulators; big: 2^20 + 1000 rows and two (no "start at 8" shortcut there either).  The second run starts from the
    stored hint and must give the same result"""
    n, aggs = (N_MID, AGGS6) if size == "mid" else (N_BIG, AGGS2)
    keys, first, hint = sampler_case(name, n)
    rng = np.random.default_rng(n)
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[int_batch(k, rng) for k in keys]])
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("k"), "k")], aggs, m)
    want = oracle_partition(plan, 0)
    ks = run_partition(ctx, plan, 0, want, ["k"])
    assert launches(ks, "merge_partials") == first["rounds"], ks
    assert (g4(ks) > 0) == first["g4"] and (g8(ks) > 0) == first["g8"] and ("scan_agg_hash" in ks) == first["hash"], ks
    assert launches(ks, "scan_agg_lowcard_g8") >= 1, ks          # the head probe: one batch at the wider width
    ks = run_partition(ctx, plan, 0, want, ["k"])
    if hint == 8:
        assert g8(ks) > 0 and g4(ks) == 0 and "scan_agg_hash" not in ks and launches(ks, "merge_partials") == 1, ks
    else:
        assert "scan_agg_hash" in ks and g4(ks) == 0 and g8(ks) == 0 and "merge_partials" not in ks, ks


def hint_partitions(rng):
    """-> [3 groups, 6 groups, 5000 groups, 2 groups in 300 rows]"""
    parts = [draw(rng, 6000, 3), draw(rng, 6000, 6), draw(rng, 20000, 5000), draw(rng, 300, 2)]
    assert [len(np.unique(k)) for k in parts] == [3, 6, 5000, 2] and len(parts[3]) < 4096
    # an overflow is per workgroup (512-row tiles): every tile of the 6-group partition holds more than four groups
    assert all(len(np.unique(parts[1][lo:lo + 512])) > 4 for lo in range(0, 6000, 512))
    assert all(len(np.unique(parts[2][lo:lo + 512])) > 8 for lo in range(0, 20000, 512))
    return parts


def test_path_hint_carried_to_partitions_it_does_not_fit(monkeypatch):
    """one PARTIAL plan, four partitions executed in order: 3 groups (hint stays unknown), 6 (-> 8), 5000 (-> hash), then 2 groups
    in 300 rows on the hash table, below its run threshold; then all four again in reverse order with the hint at -1"""
    rng = np.random.default_rng(202)
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[int_batch(k, rng)] for k in hint_partitions(rng)])
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("k"), "k")], AGGS6, m)
    want = [oracle_partition(plan, p) for p in range(4)]
    ks = run_partition(ctx, plan, 0, want[0], ["k"])
    assert g4(ks) == 1 and g8(ks) == 0 and "scan_agg_hash" not in ks and launches(ks, "merge_partials") == 1, ks
    ks = run_partition(ctx, plan, 1, want[1], ["k"])
    assert g4(ks) == 1 and g8(ks) == 1 and "scan_agg_hash" not in ks and launches(ks, "merge_partials") == 2, ks
    ks = run_partition(ctx, plan, 2, want[2], ["k"])
    assert g4(ks) == 0 and g8(ks) == 1 and "scan_agg_hash" in ks and launches(ks, "merge_partials") == 1, ks
    ks = run_partition(ctx, plan, 3, want[3], ["k"])
    assert g4(ks) == 0 and g8(ks) == 0 and "scan_agg_hash" in ks and "merge_partials" not in ks and "run_heads" not in ks, ks
    for p in (3, 2, 1, 0):
        ks = run_partition(ctx, plan, p, want[p], ["k"])
        assert g4(ks) == 0 and g8(ks) == 0 and "scan_agg_hash" in ks and "merge_partials" not in ks, (p, ks)


def test_small_partitions_behind_one_that_sent_the_plan_to_the_hash_table(monkeypatch):
    """the 5000-group partition first: every later partition starts on the hash path — few groups, no rows at all, a key column
    that is NULL throughout"""
    rng = np.random.default_rng(203)
    parts = hint_partitions(rng)
    nulls = np.zeros(500, np.int64)
    keys = [parts[2], parts[0], np.zeros(0, np.int64), nulls, parts[3]]
    valid = [None, None, None, np.zeros(500, np.bool_), None]
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[int_batch(k, rng, v)] for k, v in zip(keys, valid)])
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("k"), "k")], AGGS6, m)
    want = [oracle_partition(plan, p) for p in range(5)]
    assert [len(w["k"].values) for w in want] == [5000, 3, 0, 1, 2] and want[3]["k"].to_pylist() == [None]
    ks = run_partition(ctx, plan, 0, want[0], ["k"])
    assert g4(ks) == 1 and g8(ks) == 1 and "scan_agg_hash" in ks and launches(ks, "merge_partials") == 2, ks
    for p in (1, 2, 3, 4, 0, 3, 2, 1):
        ks = run_partition(ctx, plan, p, want[p], ["k"])
        assert g4(ks) == 0 and g8(ks) == 0 and "merge_partials" not in ks, (p, ks)
        assert ("scan_agg_hash" in ks) == (p != 2), (p, ks)       # the empty partition launches no scan at all


# ---- Utf8 keys on the wide-load path (sections 2 and 4) --------------------------------------------------------------------

U_SCHEMA = dict([("ks", "Utf8"), ("kt", "Utf8"), ("d", "Date32"), ("x", "Float64"), ("y", "Float64"), ("z", "Float64"), ("q", "Float64")])
U_AGGS = [E.Sum(col("q"), "sq"), E.Sum(col("x"), "sx"), E.Sum(col("x") * (lit(1.0) - col("y")), "sd"),
          E.Sum(col("x") * (lit(1.0) - col("y")) * (lit(1.0) + col("z")), "sc"), E.Avg(col("q"), "aq"), E.Avg(col("y"), "ay"),
          E.Count(lit(1, E.UINT8), "n")]
CUTOFF = 10471                                                  # 1998-09-02 as days
PRED = col("d") <= E.date32("1998-09-02")
PRED_ALL = col("d") <= E.date32("1999-06-01")                   # accepts every row of utf8_batch


def utf8_batch(n, seed, ks, kt=("F", "O")):
    """ks, kt: the vocabularies of the two key columns"""
    rng = np.random.default_rng(seed)
    ks = [ks[k] for k in rng.integers(0, len(ks), n)]
    d = rng.integers(8700, 10600, n).astype(np.int32)
    assert d.max() < 10743                                      # 1999-06-01
    return OrderedDict([
        ("ks", OCol("Utf8", list(ks))),
        ("kt", OCol("Utf8", [kt[k] for k in rng.integers(0, len(kt), n)])),
        ("d", OCol("Date32", d)),
        ("x", OCol("Float64", np.round(rng.uniform(900.0, 105000.0, n), 2))),
        ("y", OCol("Float64", rng.integers(0, 11, n) / 100.0)),
        ("z", OCol("Float64", rng.integers(0, 9, n) / 100.0)),
        ("q", OCol("Float64", rng.integers(1, 51, n).astype(np.float64))),
    ])


def utf8_partial(ctx, dev, host, group, pred, limit=None):
    """PARTIAL aggregate over the device batches `dev` of one partition (host: the same rows for the oracle)"""
    m = ba.MemoryExec([list(dev)], ctx)
    m._oracle_partitions = [list(host)]
    src = m if limit is None else limit(m)
    return ba.HashAggregateExec(ba.plan.PARTIAL, [(col(g), g) for g in group], U_AGGS, ba.FilterExec(E.coerce(pred, U_SCHEMA), src))


def test_path_hint_with_a_utf8_key_on_the_wide_load_path(monkeypatch):
    """the same walk with a Utf8 key of 1-3 bytes: the wide-load kernel serves widths 1 and 4 and is abandoned at 8 (the 7-byte
    register kernel), then the hash table.  66000-row partitions: launches of 2^16 rows and more are named by kernel"""
    rng = np.random.default_rng(204)
    letters = "ABCDEFGHJKLMNPQRSTUV"
    many = [a + b + c for a in letters[:18] for b in letters[:18] for c in letters[:16]][:5000]
    vocab = [("A", "BB", "CCC"), ("A", "BB", "CCC", "D", "EE", "FFF"), many, ("A", "CCC")]
    sizes = [66000, 66000, 66000, 300]
    host = [utf8_batch(n, 2040 + i, v) for i, (n, v) in enumerate(zip(sizes, vocab))]
    for b, v in zip(host, vocab):
        assert set(b["ks"].values) == set(v) and {len(s) for s in v} <= {1, 2, 3}
    assert all(len(set(host[1]["ks"].values[lo:lo + 1024])) > 4 for lo in range(0, 66000, 1024))
    assert all(len(set(host[2]["ks"].values[lo:lo + 1024])) > 8 for lo in range(0, 66000, 1024))
    ctx = timed_context(monkeypatch)
    m = helpers.memory_exec(ctx, [[b] for b in host])
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("ks"), "ks")], U_AGGS, ba.FilterExec(E.coerce(PRED, U_SCHEMA), m))
    want = [oracle_partition(plan, p) for p in range(4)]
    vm = lambda ks: g4(ks) + g8(ks)
    ks = run_partition(ctx, plan, 0, want[0], ["ks"])
    assert "scan_agg_lean_kernel" in ks and "scan_agg_sop_kernel" not in ks and "scan_agg_hash" not in ks and vm(ks) == 0, ks
    assert ctx.lean_key_form() == "offsets" and launches(ks, "merge_partials") == 1, ks
    ks = run_partition(ctx, plan, 1, want[1], ["ks"])
    assert "scan_agg_lean_kernel" in ks and "scan_agg_sop_kernel" in ks and "scan_agg_hash" not in ks and vm(ks) == 0, ks
    assert launches(ks, "merge_partials") == 2, ks
    ks = run_partition(ctx, plan, 2, want[2], ["ks"])
    assert "scan_agg_lean_kernel" not in ks and "scan_agg_sop_kernel" in ks and "scan_agg_hash" in ks and vm(ks) == 0, ks
    for p in (3, 2, 1, 0):
        ks = run_partition(ctx, plan, p, want[p], ["ks"])
        assert "scan_agg_hash" in ks and "scan_agg_lean_kernel" not in ks and "scan_agg_sop_kernel" not in ks and "merge_partials" not in ks, (p, ks)


# ---- section 3: clustered_hint_ and the run paths ---------------------------------------------------------------------------

# hash path, no fused predicate: SUM(Float64) with NULLs and AVG make the ordered sums of kernels_dagg.hip and their spill lists run
RUN_AGGS = [E.Sum(col("x"), "sx"), E.Count(col("x"), "cx"), E.Count(lit(1, E.UINT8), "n"), E.Min(col("q"), "mn"), E.Avg(col("q"), "aq")]


def run_batch(key, rng):
    n = len(key)
    return OrderedDict([("k", OCol("Int64", np.asarray(key, dtype=np.int64))),
                        ("x", OCol("Float64", np.round(rng.random(n) * 100 + 1, 3), rng.random(n) > 0.1)),
                        ("q", OCol("Int32", rng.integers(0, 50, n)))])


def ascending_runs(rng, n, lo_len=1, hi_len=9, first=10, step=3):
    """n rows of runs of lo_len .. hi_len-1 equal keys, the keys first, first + step, ..."""
    sizes = rng.integers(lo_len, hi_len, n // lo_len + 1)
    return np.repeat(np.arange(len(sizes), dtype=np.int64) * step + first, sizes)[:n]


def clustered_part(rng, n=40_000):
    k = ascending_runs(rng, n)
    assert 2 * n_runs(k) <= n and len(breaks(k)) == 0
    return k


def random_part(rng, n=40_000, groups=150):
    k = rng.integers(0, groups, n).astype(np.int64) * 7
    assert len(np.unique(k)) == groups and 2 * n_runs(k) > n and len(breaks(k)) > 1
    return k


def distinct_part(rng, n=40_000):
    k = rng.permutation(n).astype(np.int64) * 5 + 1
    assert n_runs(k) == n and len(np.unique(k)) == n and len(breaks(k)) > 1
    return k


def run_plan(ctx, rng, parts):
    m = helpers.memory_exec(ctx, [[run_batch(k, rng)] for k in parts])
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("k"), "k")], RUN_AGGS, m)
    return plan, [oracle_partition(plan, p) for p in range(len(parts))]


def test_stale_clustered_hint_forces_the_run_path(monkeypatch):
    """a clustered partition sets the hint to 1; the next two — 150 groups in random order (hundreds of runs per group: the sorted
    spill combine), and every row a key of its own in random order (runs = rows) — go through the run table without a look"""
    rng = np.random.default_rng(301)
    ctx = timed_context(monkeypatch)
    plan, want = run_plan(ctx, rng, [clustered_part(rng), random_part(rng), distinct_part(rng)])
    ks = run_partition(ctx, plan, 0, want[0], ["k"])
    assert "run_heads" in ks and "run_slots" in ks and "run_groups" not in ks and "emit_slots" in ks, ks
    ks = run_partition(ctx, plan, 1, want[1], ["k"])
    assert "run_heads" in ks and "run_groups" in ks and "det_spill_combine" in ks and "scan_agg_hash" in ks, ks
    ks = run_partition(ctx, plan, 2, want[2], ["k"])
    assert "run_heads" in ks and "run_groups" in ks and "scan_agg_hash" in ks, ks
    ks = run_partition(ctx, plan, 0, want[0], ["k"])
    assert "run_slots" in ks and "run_groups" not in ks and "emit_slots" in ks, ks


def test_stale_unclustered_hint_never_looks_again(monkeypatch):
    """the random partition first: the hint is -1 and the clustered partition is aggregated row by row in the table"""
    rng = np.random.default_rng(302)
    ctx = timed_context(monkeypatch)
    plan, want = run_plan(ctx, rng, [random_part(rng), clustered_part(rng), distinct_part(rng)])
    ks = run_partition(ctx, plan, 0, want[0], ["k"])
    assert "run_heads" in ks and "run_slots" not in ks and "scan_agg_hash" in ks, ks
    for p in (1, 2, 0, 1):
        ks = run_partition(ctx, plan, p, want[p], ["k"])
        assert "run_heads" not in ks and "run_slots" not in ks and "emit_slots" not in ks and "scan_agg_hash" in ks, (p, ks)


def test_run_threshold_after_the_hint_was_learned(monkeypatch):
    """hint 1, then unclustered partitions of 4095 rows (below the run threshold: the table) and of 4096 (forced onto the runs)"""
    rng = np.random.default_rng(303)
    ctx = timed_context(monkeypatch)
    plan, want = run_plan(ctx, rng, [clustered_part(rng), random_part(rng, 4095), random_part(rng, 4096)])
    ks = run_partition(ctx, plan, 0, want[0], ["k"])
    assert "run_slots" in ks and "emit_slots" in ks, ks
    ks = run_partition(ctx, plan, 1, want[1], ["k"])
    assert "run_heads" not in ks and "run_groups" not in ks and "scan_agg_hash" in ks, ks
    ks = run_partition(ctx, plan, 2, want[2], ["k"])
    assert "run_heads" in ks and "run_groups" in ks and "scan_agg_hash" in ks, ks


def head_tail_runs(shape, rng):
    """2^20 + 8192 rows: the run sample is the first 2^20"""
    n, tail = N_RUNS, N_RUNS - SAMPLE
    head = ascending_runs(rng, SAMPLE + 1000, 32, 97)           # long runs: some 16 K groups; ascends 1000 rows past the sample
    old = np.unique(head)
    if shape == "tail_random_over_the_heads_keys":
        k = np.concatenate([head[:SAMPLE], old[rng.integers(0, len(old), tail)]])
        assert set(k[SAMPLE:]) <= set(old) and len(breaks(k)) > 1
    elif shape in ("one_break_in_the_tail", "two_breaks_in_the_tail"):
        rest = tail - 1000
        fresh = np.concatenate([old[::5][:300] + 1, old.max() + 3 * np.arange(1, 301)])      # between the head's keys, and beyond them
        stretch = np.sort(np.concatenate([old[::7][:400], fresh]))
        assert stretch[0] < head[-1] and len(np.unique(stretch)) == 1000
        if shape == "one_break_in_the_tail":
            second = np.repeat(stretch, rest // len(stretch) + 1)[:rest]
            k = np.concatenate([head, second])
            assert list(breaks(k)) == [SAMPLE + 1000]
        else:
            half = rest // 2
            second = np.repeat(stretch, half // len(stretch) + 1)
            k = np.concatenate([head, second[:half], second[:rest - half]])
            assert list(breaks(k)) == [SAMPLE + 1000, SAMPLE + 1000 + half]
    elif shape == "head_random_tail_clustered":
        k = np.concatenate([rng.integers(0, 5000, SAMPLE).astype(np.int64) * 3, ascending_runs(rng, tail, 32, 97, first=20000)])
        assert 2 * n_runs(k[:SAMPLE]) > SAMPLE and 2 * n_runs(k[SAMPLE:]) <= tail
        return k
    else:
        raise KeyError(shape)
    assert len(k) == n and len(breaks(k[:SAMPLE])) == 0 and 2 * n_runs(k[:SAMPLE]) <= SAMPLE
    if shape != "tail_random_over_the_heads_keys":              # the tail mixes keys of the head with keys of its own
        t = k[SAMPLE + 1000:]
        assert len(np.intersect1d(t, old)) > 100 and len(np.setdiff1d(t, old)) > 100
    return k


@pytest.mark.parametrize("shape", ["tail_random_over_the_heads_keys", "one_break_in_the_tail", "two_breaks_in_the_tail",
                                   "head_random_tail_clustered"])
def test_run_sample_against_a_tail_that_differs(shape, monkeypatch):
    """what the leading 2^20 rows say about runs and breaks is re-read after the full pass: the tail decides between distinct
    runs, two ascending stretches (first break beyond the sample) and the run table; an unclustered head takes no runs at all"""
    rng = np.random.default_rng(304)
    key = head_tail_runs(shape, rng)
    ctx = timed_context(monkeypatch)
    plan, want = run_plan(ctx, rng, [key])
    for _ in range(2):                                          # the second run starts from the hints of the first
        ks = run_partition(ctx, plan, 0, want[0], ["k"])
        if shape == "head_random_tail_clustered":
            if _ == 0:
                assert launches(ks, "run_heads") == 1, ks
            else:
                assert "run_heads" not in ks, ks
            assert "run_slots" not in ks and "run_groups" not in ks and "scan_agg_hash" in ks, ks
        elif shape == "one_break_in_the_tail":
            assert launches(ks, "run_heads") == 2 and "run_tail_resolve" in ks and "run_groups" not in ks and "emit_slots" in ks, ks
        else:
            assert launches(ks, "run_heads") == 2 and "run_groups" in ks and "run_tail_resolve" not in ks, ks


def two_stretches(rng, n, at, kind):
    """n rows with exactly one break, at row `at`.  kind "old": the second stretch brings keys of the first back; "fresh": it
    holds none of them"""
    if at == 1:
        top = np.int64(10**7)                                   # one row, then everything else below it
        body = ascending_runs(rng, n - 1 - (6 if kind == "old" else 0), 2, 9)
        k = np.concatenate([[top], body, np.full(6 if kind == "old" else 0, top)])
    elif at == n - 1:
        body = ascending_runs(rng, n - 1, 2, 9)
        k = np.concatenate([body, [body[n // 2] if kind == "old" else np.int64(5)]])
    else:
        first = ascending_runs(rng, at, 2, 9)
        old = np.unique(first)[:-1]                             # (the last key again would extend its run: no break)
        pool = old[::2] if kind == "old" else old[::2] + 1      # keys are 10, 13, ...: + 1 is a key of neither stretch
        pool = pool[:(n - at) // 5]
        sizes = np.full(len(pool), 5)
        sizes[-1] += n - at - 5 * len(pool)
        k = np.concatenate([first, np.repeat(pool, sizes)])
    a, b = set(k[:at]), set(k[at:])
    assert len(k) == n and list(breaks(k)) == [at] and 2 * n_runs(k) <= n
    if kind == "fresh":
        assert not (a & b)
    elif 1 < at < n - 1:
        assert b <= a
    else:
        assert a & b
    return k


@pytest.mark.parametrize("kind", ["old", "fresh"])
@pytest.mark.parametrize("at", [1, 39_999, 20 * 1024])
def test_two_ascending_stretches(at, kind, monkeypatch):
    """40000 rows, one break: at row 1, at the last row, exactly on a 1024-row tile edge; the second stretch is matched against
    the first by binary search (run_tail_resolve), no table"""
    rng = np.random.default_rng(305 + at)
    key = two_stretches(rng, 40_000, at, kind)
    ctx = timed_context(monkeypatch)
    plan, want = run_plan(ctx, rng, [key])
    for _ in range(2):
        ks = run_partition(ctx, plan, 0, want[0], ["k"])
        assert "run_heads" in ks and "run_tail_resolve" in ks and "run_tail_remap" in ks and "run_groups" not in ks and "emit_slots" in ks, ks


# ---- section 4: a learned Utf8 width and rows hidden by the predicate ----------------------------------------------------------

HIDDEN_N = (3000, 1500)
# rows of batch 0 / batch 1 that hold the odd value: the first row of a later workgroup's first 1024-row tile, both rows of one
# thread's pair, the second row of another pair, and the last row of the ragged final tile
HIDDEN_ROWS = ([2048, 1536, 1537, 2051, 2999], [1024, 1499])


def hidden_batches(odd):
    """every ks value is one byte, except `odd` in rows the date predicate PRED rejects"""
    host = []
    for i, (n, rows) in enumerate(zip(HIDDEN_N, HIDDEN_ROWS)):
        b = utf8_batch(n, 4000 + i, ("A", "N"))
        ks, d = list(b["ks"].values), b["d"].values.copy()
        for r in rows:
            ks[r], d[r] = odd, 10590
        b["ks"], b["d"] = OCol("Utf8", ks), OCol("Date32", d)
        lens = np.array([len(s) for s in ks])
        assert set(np.flatnonzero(lens != 1)) == set(rows) and (d[rows] > CUTOFF).all() and (d <= CUTOFF).sum() > n // 2
        assert rows[-1] == n - 1 and n % 1024 != 0 and rows[0] % 1024 == 0 and rows[0] > 0
        host.append(b)
    return host


@pytest.mark.parametrize("odd", ["BB", "", "ABCD"], ids=["two-bytes", "no-byte", "four-bytes"])
def test_width_is_not_learned_from_rows_the_predicate_hides(odd, monkeypatch):
    """run 1 filters the odd values out, run 2 scans the same device batches under a predicate that accepts them: had run 1
    recorded "one byte wide", run 2 would read the wrong bytes.  The scan reads every length, so the key form stays "offsets".
    Four bytes: longer than the wide-load kernel holds, so it hands over to the 7-byte register kernel"""
    host = hidden_batches(odd)
    ctx = timed_context(monkeypatch)
    dev = [helpers.to_device(ctx, b) for b in host]
    for pred, groups in ((PRED, 2), (PRED_ALL, 3), (PRED, 2), (PRED_ALL, 3)):
        plan = utf8_partial(ctx, dev, host, ["ks"], pred)
        want = oracle_partition(plan, 0)
        assert len(want["ks"].values) == groups and (odd in list(want["ks"].values)) == (groups == 3)
        ks = run_partition(ctx, plan, 0, want, ["ks"])
        assert ctx.lean_key_form() == "offsets" and g4(ks) + g8(ks) == 0 and "scan_agg_hash" not in ks, ks
        if groups == 3:
            assert launches(ks, "merge_partials") == (2 if odd == "ABCD" else 1), ks


def test_learned_width_applied_to_other_views_of_the_buffers(monkeypatch):
    """the width is earned by a plan over two batches; plans over the second batch alone and over a row prefix of the first
    (Local / GlobalLimitExec hand on the same buffers) find it on those buffers and must be right whichever form they use"""
    host = [utf8_batch(3000, 4100, ("AA", "NB"), ("FX", "OY")), utf8_batch(1500, 4101, ("AA", "NB"), ("FX", "OY"))]
    assert {len(s) for b in host for s in list(b["ks"].values) + list(b["kt"].values)} == {2}
    ctx = timed_context(monkeypatch)
    dev = [helpers.to_device(ctx, b) for b in host]
    for form in ("offsets", KNOWN):
        plan = utf8_partial(ctx, dev, host, ["ks", "kt"], PRED)
        ks = run_partition(ctx, plan, 0, oracle_partition(plan, 0), ["ks", "kt"])
        assert ctx.lean_key_form() == form and g4(ks) + g8(ks) == 0, ks
    views = [(dev[1:], host[1:], None), (dev[:1], host[:1], lambda m: ba.LocalLimitExec(m, 2500)),
             (dev[:1], host[:1], lambda m: ba.GlobalLimitExec(m, 1025)), (dev[:1], host[:1], lambda m: ba.LocalLimitExec(m, 1))]
    for d, h, limit in views:
        for group in (["ks", "kt"], ["ks"]):
            plan = utf8_partial(ctx, d, h, group, PRED_ALL, limit)
            ks = run_partition(ctx, plan, 0, oracle_partition(plan, 0), group)
            assert ctx.lean_key_form() == KNOWN and g4(ks) + g8(ks) == 0 and "scan_agg_hash" not in ks, ks
