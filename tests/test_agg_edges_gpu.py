"""MIN / MAX, SUM / AVG and float GROUP BY keys at the edges of their value domains, through every aggregate path that holds
them, against the oracle:

- UInt64 across 2^63 (unsigned compares), Int64 extremes equal to the signed identities, the narrow integer extremes, pre-1970
  Date64 / Timestamp values;
- Float64 / Float32 NaN of three bit patterns, +-inf, +-0.0, +-subnormal, +-max: NaN is skipped unless a group holds nothing
  else (then NaN); a -0.0 / +0.0 tie may give either sign (zero results only);
- SUM / AVG carrying +-inf and NaN through the register and the fixed-order hash sums;
- Utf8 MIN / MAX: empty strings, prefixes, bytes >= 0x80, embedded NUL bytes;
- Float64 / Float32 group keys holding the special values: equal by bit pattern.

Paths: no GROUP BY, <= 4 and 5..8 groups (register kernel + merge of the per-workgroup partials), > 8 groups (hash table,
atomics), input clustered by the key (runs; the run table and the per-slot emit in child processes), wide keys, several
batches in one launch, Partial over partitions -> Merge -> Final, hash repartitioning.  Every case reads the kernel list
(BHIP_KERNEL_TIMING=2) and asserts that its path ran."""
import math
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle import plan_eval
from oracle.engine import OCol
from tests import helpers

pytestmark = pytest.mark.gpu

CHILD = os.environ.get("BHIP_NO_DISTINCT_RUNS") == "1" or os.environ.get("BHIP_NO_SLOT_EMIT") == "1"
REPS = 700                     # rows per listed value: a group's values span several workgroup tiles


@pytest.fixture(scope="module")
def ctx():
    old = os.environ.get("BHIP_KERNEL_TIMING")
    os.environ["BHIP_KERNEL_TIMING"] = "2"                 # every launch, however small (read when a context is created)
    try:
        yield ba.Context(0)
    finally:
        if old is None:
            os.environ.pop("BHIP_KERNEL_TIMING", None)
        else:
            os.environ["BHIP_KERNEL_TIMING"] = old


# ---- value domains ------------------------------------------------------------------------------------------------------------

def _f64(bits):
    return float(np.array([bits], np.uint64).view(np.float64)[0])


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def float_specials(dtype):
    """(nan, negative quiet nan, nan with a payload, smallest subnormal, largest finite) of the type"""
    if dtype == "Float64":
        return math.nan, _f64(0xFFF8000000000000), _f64(0x7FF8000000000123), 5e-324, float(np.finfo(np.float64).max)
    return _f32(0x7FC00000), _f32(0xFFC00000), _f32(0x7FC00123), _f32(0x00000001), np.finfo(np.float32).max


def float_groups(dtype):
    nan, nnan, pnan, sub, big = float_specials(dtype)
    inf = math.inf
    return [
        [nan, nnan, pnan],                        # all NaN, three bit patterns -> NaN
        [nan, None],                              # NaN + NULL -> NaN
        [None],                                   # all NULL -> NULL
        [inf],                                    # MIN = the old identity
        [-inf],                                   # MAX = the old identity
        [nan, -0.0, 0.0, sub, -sub],              # NaN first, then zeros and subnormals
        [nan, big, -big, inf, -inf, nnan],        # NaN at both ends, infinities in between
        [-0.0, 0.0],                              # a zero tie
        [pnan, 1.0, None, 0.0],
        [big, nan],
    ]


def int_groups(dtype):
    info = np.iinfo(np.dtype(dtype.lower()))
    lo, hi = int(info.min), int(info.max)
    return [[lo, hi], [lo], [hi], [0, None], [None], [hi, lo + 1, hi - 1]]


U63 = 2**63
DAY_MS = 86400000
DOMAINS = {
    "UInt64": [[0, 1, 5], [U63, U63 + 5, 2**64 - 1], [3, U63 + 5, U63 - 1, None], [2**64 - 1, 0], [None], [U63 - 1, U63],
               [U63 + 5, 2]],
    "Int64": [[2**63 - 1], [-2**63], [-2**63, 2**63 - 1, 0, None], [-1, 1], [None], [2**63 - 1, -2**63 + 1]],
    "Int8": int_groups("Int8"), "Int16": int_groups("Int16"), "Int32": int_groups("Int32"),
    "UInt8": int_groups("UInt8"), "UInt16": int_groups("UInt16"), "UInt32": int_groups("UInt32"),
    "Date64": [[-DAY_MS * 365 * 40, 0, 5], [-1], [-DAY_MS, None, DAY_MS], [-2**62, 2**62]],
    "Timestamp(Microsecond)": [[-86400 * 10**6 * 1000, 3], [-1, -2], [None, -5, 7], [-2**63, 2**63 - 1]],
    "Float64": float_groups("Float64"),
    "Float32": float_groups("Float32"),
}


def filler_value(dtype, i):
    return float(i) + 0.5 if dtype.startswith("Float") else i % 100


def build(dtype, groups, reps=REPS, order="spread", singles=(), seed=0):
    """rows of (g, v, w): group i holds every value of groups[i] `reps` times.  order: "spread" = value-major (a group's first
    values in the early tiles, its last ones in later tiles), "shuffled", "clustered" (ascending by g).  w holds each group's
    values in the reverse row order.  singles: groups of exactly one row, appended."""
    gs, vs = [], []
    for j in range(max(len(x) for x in groups)):
        for i, vals in enumerate(groups):
            if j < len(vals):
                gs += [i] * reps
                vs += [vals[j]] * reps
    for k, v in enumerate(singles):
        gs.append(len(groups) + k)
        vs.append(v)
    n = len(gs)
    idx = np.arange(n)
    if order == "shuffled":
        idx = np.random.default_rng(seed).permutation(n)
    elif order == "clustered":
        idx = np.argsort(np.array(gs), kind="stable")
    gs = [gs[i] for i in idx]
    vs = [vs[i] for i in idx]
    ws = list(vs)
    by_group = {}
    for r, g in enumerate(gs):
        by_group.setdefault(g, []).append(r)
    for rows in by_group.values():
        for a, b in zip(rows, reversed(rows)):
            ws[a] = vs[b]
    return OrderedDict([("g", OCol("Int32", gs)), ("v", value_col(dtype, vs)), ("w", value_col(dtype, ws))])


def value_col(dtype, vals):
    valid = [v is not None for v in vals]
    if dtype == "Utf8":
        return OCol(dtype, ["" if v is None else v for v in vals], valid)
    z = 0.0 if dtype.startswith("Float") else 0
    return OCol(dtype, np.array([z if v is None else v for v in vals], dtype=object).astype(
        {"Float64": np.float64, "Float32": np.float32}.get(dtype, np.uint64 if dtype.startswith("UInt") else np.int64)), valid)


def minmax_aggs(dtype):
    """MIN / MAX of both value columns, COUNT and MAX of the key: at least five accumulators (more than four: the 4-group kernel,
    not the 8-group one, is where a small input starts)"""
    return [E.Min(col("v"), "mn"), E.Max(col("v"), "mx"), E.Count(col("v"), "c"), E.Min(col("w"), "mnw"), E.Max(col("w"), "mxw"),
            E.Max(col("g"), "mxg")]


ZERO_SIGN = tuple(x + s for x in ("mn", "mx", "mnw", "mxw") for s in ("", "[min]", "[max]"))


def check(ctx, plan, expect=(), expect_any=(), forbid=(), key_cols=None, float_rtol=0.0):
    ctx.kernel_stats(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    ks = set(ctx.kernel_stats(reset=True))
    want = plan_eval.collect(plan)
    helpers.assert_rows_equal(got, want, ordered=False, float_rtol=float_rtol, key_cols=key_cols, zero_sign_cols=ZERO_SIGN)
    for k in expect:
        assert k in ks, (k, sorted(ks))
    if expect_any:
        assert ks & set(expect_any), (expect_any, sorted(ks))
    for k in forbid:
        assert k not in ks, (k, sorted(ks))
    return got


def partial(group, aggs, m):
    return ba.HashAggregateExec(ba.plan.PARTIAL, group, aggs, m)


def final(group, aggs, p):
    return ba.HashAggregateExec(ba.plan.FINAL, [(col(n), n) for _, n in group], aggs, ba.MergeExec(p))


def chunks(groups, lo, hi):
    """the groups in runs of hi, each padded with plain groups up to lo"""
    out = []
    for i in range(0, len(groups), hi):
        c = groups[i:i + hi]
        out.append(c + [[j, j + 1] for j in range(len(c), lo)])
    return out


def with_fillers(dtype, groups, total):
    return groups + [[filler_value(dtype, i), filler_value(dtype, i + 1)] for i in range(len(groups), total)]


G = [(col("g"), "g")]
LOWCARD = ("scan_agg_hash", "run_heads")


# ---- MIN / MAX over every path -------------------------------------------------------------------------------------------------

@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", list(DOMAINS))
def test_minmax_without_group_by(ctx, dtype):
    """one group: each listed group's rows on their own (and no rows at all: the host's identity row)"""
    aggs = minmax_aggs(dtype)
    for vals in DOMAINS[dtype]:
        b = build(dtype, [vals])
        check(ctx, partial([], aggs, helpers.memory_exec(ctx, [[b]])), expect=["scan_agg_lowcard_g1", "merge_partials"])
    empty = helpers.slice_batch(build(dtype, [[None]]), 0, 0)
    check(ctx, partial([], aggs, helpers.memory_exec(ctx, [[empty]])))


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", list(DOMAINS))
def test_minmax_register_paths(ctx, dtype):
    """<= 4 groups per workgroup: the 4-group kernel; 5..8: the 8-group kernel.  A group's NaN-only rows sit in other tiles
    than its numbers, so that the merge of the per-workgroup partials combines all-NaN, numeric and empty (identity) partials"""
    aggs = minmax_aggs(dtype)
    groups = DOMAINS[dtype]
    for c in chunks(groups, 1, 4):
        m = helpers.memory_exec(ctx, [[build(dtype, c)]])
        check(ctx, partial(G, aggs, m), expect=["scan_agg_lowcard_g4", "merge_partials"], forbid=LOWCARD + ("scan_agg_lowcard_g8",),
              key_cols=["g"])
    for c in chunks(groups, 5, 8):                        # shuffled: a workgroup sees more than four groups
        m = helpers.memory_exec(ctx, [[build(dtype, c, order="shuffled")]])
        check(ctx, partial(G, aggs, m), expect=["scan_agg_lowcard_g8", "merge_partials"], forbid=LOWCARD, key_cols=["g"])


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", list(DOMAINS))
def test_minmax_hash_path(ctx, dtype):
    """> 8 groups in shuffled rows: the device-wide table, MIN / MAX by atomics; one group of a single row"""
    groups = with_fillers(dtype, DOMAINS[dtype], 12)
    single = [g for g in DOMAINS[dtype] if g[0] is not None][-1][:1]
    b = build(dtype, groups, order="shuffled", singles=single)
    m = helpers.memory_exec(ctx, [[b]])
    check(ctx, partial(G, minmax_aggs(dtype), m), expect=["scan_agg_hash", "hash_agg_init"], forbid=("emit_slots", "run_slots"),
          key_cols=["g"])


@pytest.mark.parametrize("dtype", list(DOMAINS))
def test_minmax_run_path(ctx, dtype):
    """input clustered by the key, many small groups: a table lookup per run of rows.  Distinct runs with the per-slot emit by default; the run
    table (BHIP_NO_DISTINCT_RUNS=1) and the table compaction (BHIP_NO_SLOT_EMIT=1) in the child processes below"""
    groups = with_fillers(dtype, DOMAINS[dtype], 2500)     # a few rows per group: a tile holds more than 8 groups
    b = build(dtype, groups, reps=2, order="clustered", singles=[groups[0][0]])
    m = helpers.memory_exec(ctx, [[b]])
    expect = ["run_heads", "run_slots", "scan_agg_hash"]
    if os.environ.get("BHIP_NO_DISTINCT_RUNS") == "1":
        expect, forbid = expect + ["run_groups", "hash_agg_compact"], ["emit_slots", "run_compact"]
    elif os.environ.get("BHIP_NO_SLOT_EMIT") == "1":
        expect, forbid = expect + ["run_compact"], ["emit_slots", "run_groups"]
    else:
        expect, forbid = expect + ["emit_slots"], ["run_groups", "run_compact"]
    check(ctx, partial(G, minmax_aggs(dtype), m), expect=expect, forbid=forbid, key_cols=["g"])


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", list(DOMAINS))
def test_minmax_batches_partitions_and_final(ctx, dtype):
    """several batches of one partition in one launch; Partial over three partitions -> Merge -> Final, which takes MIN / MAX of
    the state columns (an all-NaN state meets a numeric one, an empty partition's groups are missing)"""
    aggs = minmax_aggs(dtype)
    for c in chunks(DOMAINS[dtype], 1, 4):
        b = build(dtype, c)
        n = len(b["g"])
        batches = [helpers.slice_batch(b, lo, lo + n // 3 + 1) for lo in range(0, n, n // 3 + 1)]
        check(ctx, partial(G, aggs, helpers.memory_exec(ctx, [batches])), expect=["scan_agg_lowcard_g4_batches"],
              forbid=LOWCARD, key_cols=["g"])
    for total, order in ((4, "spread"), (12, "shuffled")):
        b = build(dtype, with_fillers(dtype, DOMAINS[dtype], total), order=order)
        n = len(b["g"])
        parts = [[helpers.slice_batch(b, 0, n // 2)], [helpers.slice_batch(b, n // 2, n)], [helpers.slice_batch(b, 0, 0)]]
        p = partial(G, aggs, helpers.memory_exec(ctx, parts))
        check(ctx, p, key_cols=["g"])
        check(ctx, final(G, aggs, p), expect_any=["scan_agg_lowcard_g4_batches", "scan_agg_lowcard_g8_batches", "scan_agg_hash"],
              key_cols=["g"])


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", ["UInt64", "Int64", "Float64", "Float32"])
def test_minmax_wide_group_keys(ctx, dtype):
    """a key wider than the packed key (a long string with the group number): the representative-row path"""
    groups = with_fillers(dtype, DOMAINS[dtype], 10)
    b = build(dtype, groups, reps=60, order="shuffled")
    b["s"] = OCol("Utf8", [f"a long group key string, group {g:03d}" for g in b["g"].values])
    gk = [(col("g"), "g"), (col("s"), "s")]
    aggs = minmax_aggs(dtype)
    m = helpers.memory_exec(ctx, [[helpers.slice_batch(b, 0, 250)], [helpers.slice_batch(b, 250, len(b["g"]))]])
    p = partial(gk, aggs, m)
    check(ctx, p, expect=["wide_key_assign"], key_cols=["g", "s"])
    check(ctx, final(gk, aggs, p), key_cols=["g", "s"])


# ---- SUM / AVG with non-finite values ---------------------------------------------------------------------------------------

@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_sum_avg_carry_infinities_and_nan(ctx, dtype):
    """+inf and -inf -> NaN, only +inf -> +inf, a NaN -> NaN, a NULL-only group -> NULL, on the register path, the hash path
    with its fixed-order sums (kernels_dagg.hip) and through Partial -> Final"""
    nan, _, _, sub, big = float_specials(dtype)
    inf = math.inf
    groups = [[inf, -inf, 1.0], [inf, 2.0], [nan, 1.0], [-inf, None], [None], [big], [sub, -sub, 0.5], [1.25, 2.5]]
    aggs = [E.Sum(col("v"), "s"), E.Avg(col("v"), "a"), E.Count(col("v"), "c"), E.Min(col("v"), "mn"), E.Max(col("w"), "mx"),
            E.Min(col("w"), "mnw")]
    rtol = 1e-9 if dtype == "Float64" else 2e-7
    for total, order, path in ((4, "spread", "scan_agg_lowcard_g4"), (8, "shuffled", "scan_agg_lowcard_g8"),
                               (12, "shuffled", "det_segments")):
        for c in chunks(with_fillers(dtype, groups, total), 1, total):
            b = build(dtype, c, order=order)
            check(ctx, partial(G, aggs, helpers.memory_exec(ctx, [[b]])), expect=[path], key_cols=["g"], float_rtol=rtol)
            n = len(b["g"])
            p = partial(G, aggs, helpers.memory_exec(ctx, [[helpers.slice_batch(b, 0, n // 3)], [helpers.slice_batch(b, n // 3, n)]]))
            check(ctx, final(G, aggs, p), key_cols=["g"], float_rtol=rtol)
    b = build(dtype, [[inf, 1.0], [nan]])
    check(ctx, partial([], aggs, helpers.memory_exec(ctx, [[b]])), expect=["scan_agg_lowcard_g1"], float_rtol=rtol)


# ---- Utf8 MIN / MAX ---------------------------------------------------------------------------------------------------------

STRING_GROUPS = [["", "a"], ["ab", "a", "abc"], ["z", "é", "\x7f"], ["a\x00b", "a\x00", "a"], [None], ["€", "ÿ", None],
                 ["", None], ["\U0001f600", "￿", "zz"]]


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
def test_utf8_minmax_compares_unsigned_bytes(ctx):
    """empty strings, prefixes, multi-byte UTF-8 (bytes >= 0x80 above every ASCII byte), embedded NUL bytes"""
    aggs = [E.Min(col("v"), "mn"), E.Max(col("v"), "mx"), E.Count(col("v"), "c")]
    for order in ("spread", "shuffled"):
        b = build("Utf8", STRING_GROUPS, reps=40, order=order)
        m = helpers.memory_exec(ctx, [[helpers.slice_batch(b, 0, 300)], [helpers.slice_batch(b, 300, len(b["g"]))]])
        p = partial(G, aggs, m)
        check(ctx, p, expect=["rank_to_row"], key_cols=["g"])
        check(ctx, final(G, aggs, p), key_cols=["g"])
    b = build("Utf8", [STRING_GROUPS[2] + STRING_GROUPS[3]], reps=5)
    check(ctx, partial([], aggs, helpers.memory_exec(ctx, [[b]])), expect=["rank_to_row"])


# ---- float GROUP BY keys -------------------------------------------------------------------------------------------------------

def float_key_batch(dtype, keys, reps, order, seed=5):
    ks, xs = [], []
    for j in range(reps):
        for i, k in enumerate(keys):
            ks.append(k)
            xs.append(i * 10 + j % 7)
    idx = np.arange(len(ks))
    if order == "shuffled":
        idx = np.random.default_rng(seed).permutation(len(ks))
    elif order == "clustered":
        idx = np.argsort(np.array([i for _ in range(reps) for i in range(len(keys))]), kind="stable")
    ks = [ks[i] for i in idx]
    xs = [xs[i] for i in idx]
    return OrderedDict([("k", value_col(dtype, ks)), ("x", OCol("Int32", xs))])


def special_keys(dtype):
    nan, nnan, pnan, sub, big = float_specials(dtype)
    return [nan, nnan, pnan, math.inf, -math.inf, -0.0, 0.0, sub, -sub, big, None, 1.5]


KAGGS = [E.Count(col("x"), "c"), E.Min(col("x"), "mn"), E.Sum(col("x"), "s")]
K = [(col("k"), "k")]


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_float_group_keys(ctx, dtype):
    """NaN of three bit patterns, +-inf, -0.0 and +0.0, subnormals and NULL as keys: equal by bit pattern on the register, hash
    and run paths and through Partial -> Final over partitions"""
    keys = special_keys(dtype)
    for c in (keys[0:4], keys[4:8], keys[8:12]):
        b = float_key_batch(dtype, c, 300, "spread")
        check(ctx, partial(K, KAGGS, helpers.memory_exec(ctx, [[b]])), expect=["merge_partials"], forbid=LOWCARD, key_cols=["k"])
    c = keys[0:7] + [keys[10]]
    b = float_key_batch(dtype, c, 300, "spread")
    check(ctx, partial(K, KAGGS, helpers.memory_exec(ctx, [[b]])), expect=["scan_agg_lowcard_g8"], forbid=LOWCARD, key_cols=["k"])
    fillers = [1000.5 + i for i in range(2000)]           # clustered: a few rows per key, so that a tile holds more than 8 keys
    for order, path, ks, reps in (("shuffled", "hash_agg_compact", keys, 400), ("clustered", "run_slots", keys + fillers, 3)):
        b = float_key_batch(dtype, ks, reps, order)
        m = helpers.memory_exec(ctx, [[b]])
        check(ctx, partial(K, KAGGS, m), expect=["scan_agg_hash", path], key_cols=["k"])
        n = len(b["k"])
        for nparts in (2, 3):
            parts = [[helpers.slice_batch(b, i * n // nparts, (i + 1) * n // nparts)] for i in range(nparts)]
            check(ctx, final(K, KAGGS, partial(K, KAGGS, helpers.memory_exec(ctx, parts))), key_cols=["k"])


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_hash_repartition_over_float_keys(ctx, dtype):
    """RepartitionExec(Hash) over the special keys, then an aggregate per partition: every key in exactly one partition, so
    the union of the per-partition results is the single aggregate"""
    b = float_key_batch(dtype, special_keys(dtype), 200, "shuffled")
    m = helpers.memory_exec(ctx, [[helpers.slice_batch(b, 0, 1000)], [helpers.slice_batch(b, 1000, len(b["k"]))]])
    rp = ba.RepartitionExec(m, ba.Partitioning.Hash([col("k")], 3))
    got = check(ctx, partial(K, KAGGS, rp), key_cols=["k"])
    single = plan_eval.collect(partial(K, KAGGS, helpers.memory_exec(ctx, [[b]])))
    helpers.assert_rows_equal(got, single, key_cols=["k"])


# ---- switches read once per process ------------------------------------------------------------------------------------------

@pytest.mark.skipif(CHILD, reason="this is the child run's parent")
@pytest.mark.parametrize("switch", ["BHIP_NO_DISTINCT_RUNS", "BHIP_NO_SLOT_EMIT"])
def test_run_path_switches_pass_the_same_checks(switch):
    """the run-path cases in a child process with the switch set: the run table / the table compaction instead of the per-slot
    emit"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, **{switch: "1"})
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-k", "test_minmax_run_path",
                        os.path.abspath(__file__)], cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{len(DOMAINS)} passed" in p.stdout, p.stdout[-2000:]
