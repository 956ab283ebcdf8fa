"""A limit directly over a sort runs as a top-k selection (kernels_topk.hip, SortExec::execute_top): the result must be exactly the
first k rows of the stable sort — same rows, same order, same tie order, one batch — and Context.sort_limit_form() tells which
route ran ("topk", "topk_fallback", "sort").

Expected values come from oracle/plan_eval.py on the same plan; its sort orders Float64 keys by the same total order as the device
(NaNs by sign and payload, -0.0 before +0.0: DESIGN.md "Sort order of floating-point keys").  The 2^20-row cases cut a plain
SortExec plan's output to k in numpy, so that the three of them share one sort per key list; that output is itself checked against
the oracle before it is used.  Every comparison is bit exact: row order, every column, validity."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E, tpch
from ballista_amd.expr import col
from oracle import engine as og, gen, plan_eval
from oracle.engine import OCol

import helpers
import plan_nodes as N
import proto_encode as pe

pytestmark = pytest.mark.gpu

SMALL_SORT = 1024              # kernels_sort.hip SMALL_SORT_MAX: at or below it a batch keeps the plain sort
BIG = (1 << 20) + 37           # not a multiple of 64, of a 1024-row tile or of a 16-byte load


def S(name, desc=False, nulls_first=True):
    return E.PhysicalSortExpr(col(name), descending=desc, nulls_first=nulls_first)


assert_bit_exact = helpers.assert_bit_exact


def head(batch, k):
    return og.limit(batch, k) if batch else batch


def gpu_sorted(sort_plan):
    """the rows of a plain SortExec plan (no limit above it: the sort every limit used to run on)"""
    return helpers.concat(helpers.collect_product(sort_plan))


def run_limit(ctx, limit_plan, form, want):
    out = limit_plan.collect()
    assert len(out) <= 1, "one output batch"
    got = helpers.concat([helpers.from_device(b) for b in out])
    if form is not None:
        assert ctx.sort_limit_form() == form
    assert_bit_exact(got, want)
    return got


def check(ctx, batches, keys, k, form, limit=ba.GlobalLimitExec, coalesce=None):
    m = helpers.memory_exec(ctx, [batches])
    if coalesce == "below":
        m2 = ba.CoalesceBatchesExec(m, 2048)
        m2._oracle_partitions = m._oracle_partitions
        srt = ba.SortExec(keys, m2)
    else:
        srt = ba.SortExec(keys, m)
    node = ba.CoalesceBatchesExec(srt, 4096) if coalesce == "above" else srt
    plan = limit(node, k)
    return run_limit(ctx, plan, form, plan_eval.collect(plan))


# ---- tails: the smallest selectable batch, one past 64 Ki, one past 1 Mi --------------------------------------------------------

def tail_batch(n):
    rng = np.random.default_rng(n)
    return OrderedDict([("f", OCol("Float64", rng.permutation(n).astype(np.float64) * 0.25 - n / 16)),      # distinct: exactly k candidates
                        ("i", OCol("Int64", rng.integers(-2**40, 2**40, n))),
                        ("g", OCol("Int32", rng.choice(3, n, p=[0.507, 0.247, 0.246]))),      # l_returnflag's shares, 'N' first
                        ("p", OCol("Int32", np.arange(n)))])


@pytest.fixture(scope="module")
def big(ctx):
    """the 2^20 + 37 rows shared by the big cases: the device MemoryExec and, per key list, the plain sort's output (checked
    against the oracle's sort of the same plan when it is first made)"""
    b = tail_batch(BIG)
    m = helpers.memory_exec(ctx, [[b]])
    cache = {}

    def sorted_by(keys, tag):
        if tag not in cache:
            srt = ba.SortExec(keys, m)
            cache[tag] = gpu_sorted(srt)
            assert_bit_exact(cache[tag], plan_eval.collect(srt))
        return cache[tag]
    return m, sorted_by


@pytest.mark.parametrize("k", [1, 10, 1000])
@pytest.mark.parametrize("n", [SMALL_SORT + 1, (1 << 16) + 1])
def test_tails(ctx, n, k):
    """f is distinct, so the candidates are exactly k rows: the selection sorts them unless they are more than half the batch"""
    keys = [S("f", desc=True), S("i")]
    check(ctx, [tail_batch(n)], keys, k, "topk" if 2 * k <= n else "topk_fallback")


@pytest.mark.parametrize("k", [1, 10, 1000])
def test_tail_one_mi(ctx, big, k):
    m, sorted_by = big
    keys = [S("f", desc=True), S("i")]
    run_limit(ctx, ba.GlobalLimitExec(ba.SortExec(keys, m), k), "topk", head(sorted_by(keys, "f"), k))


def test_q1_shape_falls_back(ctx, big):
    """first-key cardinality 3 over 2^20 rows in the shares of Q1's l_returnflag, the value that half the rows carry sorting first:
    more than half the rows tie with the threshold (a uniform key of three values would leave a third: selected, not a fallback)"""
    m, sorted_by = big
    keys = [S("g"), S("f", desc=True)]
    run_limit(ctx, ba.GlobalLimitExec(ba.SortExec(keys, m), 10), "topk_fallback", head(sorted_by(keys, "g"), 10))


# ---- first key types ----------------------------------------------------------------------------------------------------------

N_TYPES = 5000


def typed_batch(kind):
    rng = np.random.default_rng(7)
    n = N_TYPES
    if kind == "Int32":
        key = OCol("Int32", np.concatenate([rng.integers(-2**31, 2**31, n - 4), [2**31 - 1, -2**31, 0, -1]]))
    elif kind == "Int64":
        key = OCol("Int64", np.concatenate([rng.integers(-2**62, 2**62, n - 4), [2**63 - 1, -2**63, 0, -1]]))
    elif kind == "Date32":
        key = OCol("Date32", rng.integers(-20000, 20000, n))
    elif kind == "Float64":
        v = np.round(rng.normal(0, 1e3, n), 1)
        v[:12] = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 0.0, -0.0, np.nan, 5e-324, -5e-324, np.inf]
        v[12] = np.frombuffer(np.uint64(0xFFF8000000000001).tobytes(), np.float64)[0]          # a negative NaN with a payload
        key = OCol("Float64", rng.permutation(v))
    else:
        # 1500 values that share their first 8 bytes and differ later; ~500 values shorter than 8 bytes, among them prefixes of each
        # other with trailing NUL bytes; the rest sort after both groups
        edge = ["", "a", "a\0", "ab", "ab\0", "ab\0c", "abc"]
        vals = ["commonpr" + "".join(rng.choice(list("xyz\0"), 4)) for _ in range(1500)]
        vals += [edge[j] for j in rng.integers(0, len(edge), 500)]
        vals += ["".join(rng.choice(list("defghijklmnopqrstuvw"), rng.integers(3, 13))) for _ in range(n - 2000)]
        key = OCol("Utf8", [vals[j] for j in rng.permutation(n)])
    return OrderedDict([("key", key), ("t", OCol("Int32", rng.integers(0, 4, n))), ("p", OCol("Int32", np.arange(n)))])


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("kind", ["Int32", "Int64", "Float64", "Date32", "Utf8"])
def test_first_key_types(ctx, kind, desc):
    b = typed_batch(kind)
    keys = [S("key", desc=desc), S("t", desc=True)]
    ks = [37, 1200] if kind == "Utf8" else [37]       # Utf8 ascending, k = 1200: the threshold falls among the values that share 8 bytes
    for k in ks:
        check(ctx, [b], keys, k, "topk")


# ---- nullable first key -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_null", [20, 50, 90])            # below, equal to and above k
@pytest.mark.parametrize("nulls_first", [True, False])
@pytest.mark.parametrize("desc", [False, True])
def test_nullable_first_key(ctx, nulls_first, n_null, desc):
    n, k = 6000, 50
    rng = np.random.default_rng(n_null)
    valid = np.ones(n, bool)
    valid[rng.choice(n, n_null, replace=False)] = False
    b = OrderedDict([("f", OCol("Float64", np.round(rng.normal(0, 100, n), 3) + 0.0, valid)), ("t", OCol("Int32", rng.integers(0, 4, n))),
                     ("p", OCol("Int32", np.arange(n)))])
    check(ctx, [b], [S("f", desc=desc, nulls_first=nulls_first), S("t", desc=True)], k, "topk")


def test_nullable_utf8_and_int_keys(ctx):
    n, k = 4000, 30
    rng = np.random.default_rng(3)
    b = OrderedDict([("s", OCol("Utf8", [f"v{v:05d}" for v in rng.integers(0, 3000, n)], rng.random(n) > 0.004)),
                     ("i", OCol("Int32", rng.integers(-1000, 1000, n), rng.random(n) > 0.004)), ("p", OCol("Int32", np.arange(n)))])
    for first in ("s", "i"):
        for nf in (True, False):
            check(ctx, [b], [S(first, nulls_first=nf), S("p", desc=True)], k, "topk")


# ---- ties ------------------------------------------------------------------------------------------------------------------

def test_threshold_value_shared_by_more_than_k_rows(ctx):
    n, k = 8000, 100
    rng = np.random.default_rng(11)
    a = rng.integers(6, 1000, n)
    a[rng.choice(n, 320, replace=False)] = np.concatenate([np.full(300, 5), rng.integers(0, 5, 20)])
    b = OrderedDict([("a", OCol("Int64", a)), ("t", OCol("Int32", rng.integers(0, 9, n))), ("p", OCol("Int32", np.arange(n)))])
    check(ctx, [b], [S("a"), S("t", desc=True)], k, "topk")             # 320 candidates; the second key and input order pick 80 of the 300


def test_all_rows_equal_on_the_first_key(ctx):
    n = 5000
    rng = np.random.default_rng(12)
    b = OrderedDict([("a", OCol("Int32", np.full(n, 7))), ("t", OCol("Int32", rng.integers(0, 9, n))), ("p", OCol("Int32", np.arange(n)))])
    check(ctx, [b], [S("a"), S("t", desc=True)], 25, "topk_fallback")


# ---- byte positions: the byte skip, the first pass and the last ------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["lowest", "highest"])
@pytest.mark.parametrize("desc", [False, True])
def test_keys_that_differ_in_one_byte(ctx, shape, desc):
    n, k = 3000, 20
    rng = np.random.default_rng(13)
    byte = rng.integers(0, 256, n)
    a = (0x0123456789ABCD00 + byte) if shape == "lowest" else ((byte - 128) << 56) + 0x00CDEF0123456789
    b = OrderedDict([("a", OCol("Int64", a)), ("t", OCol("Int32", rng.integers(0, 9, n))), ("p", OCol("Int32", np.arange(n)))])
    check(ctx, [b], [S("a", desc=desc), S("t", desc=True)], k, "topk")


# ---- several input batches ---------------------------------------------------------------------------------------------------

def multi_batches():
    """8 batches of uneven sizes, two of them empty; few distinct (a, t) pairs, so the k-th value is spread over the batches and
    rows equal on every key sit in different ones: `p` (the global row number) shows the tie order"""
    rng = np.random.default_rng(14)
    sizes = [0, 1500, 1, 3000, 0, 2047, 1025, 700]
    out, row0 = [], 0
    for s in sizes:
        out.append(OrderedDict([("a", OCol("Int32", rng.integers(0, 41, s))), ("t", OCol("Int32", rng.integers(0, 3, s))),
                                ("p", OCol("Int32", np.arange(row0, row0 + s)))]))
        row0 += s
    return out


@pytest.mark.parametrize("coalesce", [None, "above", "below"])
def test_multi_batch(ctx, coalesce):
    got = check(ctx, multi_batches(), [S("a"), S("t", desc=True)], 200, "topk", coalesce=coalesce)
    a, t, p = got["a"].values, got["t"].values, got["p"].values
    same = (a[1:] == a[:-1]) & (t[1:] == t[:-1])
    assert same.sum() > 50 and np.all(p[1:][same] > p[:-1][same])        # ties: batch order, then row order


# ---- limits, the local limit, the wire ----------------------------------------------------------------------------------------

def test_limits_at_and_beyond_the_row_count(ctx):
    n = 3000
    b = tail_batch(n)
    keys = [S("f", desc=True), S("i")]
    m = helpers.memory_exec(ctx, [[b]])
    assert ba.GlobalLimitExec(ba.SortExec(keys, m), 0).collect() == []
    check(ctx, [b], keys, n, "sort")
    check(ctx, [b], keys, n + 5, "sort")
    check(ctx, multi_batches(), [S("a"), S("t", desc=True)], 10 ** 6, "sort")


def test_local_limit_over_sort(ctx):
    check(ctx, [tail_batch(5000)], [S("f"), S("i")], 17, "topk", limit=ba.LocalLimitExec)


def test_limit_over_something_else_and_sort_alone_do_not_report(ctx):
    """a SortExec without a limit above it and a limit over anything else are untouched: the hook keeps its last value"""
    b = tail_batch(3000)
    check(ctx, [b], [S("f")], 5, "topk")
    m = helpers.memory_exec(ctx, [[b]])
    got = helpers.concat(helpers.collect_product(ba.GlobalLimitExec(ba.MergeExec(m), 7)))
    assert og.batch_len(got) == 7 and list(got["p"].values) == list(range(7))
    srt = ba.SortExec([S("g")], m)
    assert_bit_exact(helpers.concat(helpers.collect_product(srt)), plan_eval.collect(srt))
    assert ctx.sort_limit_form() == "topk"
    assert [p.as_any() for p in ba.GlobalLimitExec(srt, 3).children()] == ["SortExec"]
    assert ba.GlobalLimitExec(srt, 3).display().splitlines()[0] == "GlobalLimitExec: limit=3"


def test_wire_plan_global_limit_over_sort(ctx):
    b = tail_batch(4000)
    leaf = N.MemoryExec([[b]])
    leaf.name = "mem://t"
    keys = [S("f", desc=True), S("i")]
    described = N.GlobalLimitExec(N.SortExec(keys, leaf), 12)
    decoded = ba.ExecutionPlan.from_proto(ctx, pe.plan(described), lambda leaf_: helpers.memory_exec(ctx, [[b]]))
    assert decoded.display().splitlines()[0] == "GlobalLimitExec: limit=12" and decoded.children()[0].as_any() == "SortExec"
    run_limit(ctx, decoded, "topk", plan_eval.collect(described))


def test_q3_with_its_limit(ctx):
    import json, os
    sf = json.load(open(os.path.join(helpers.GOLDEN, "q3_synth.json")))["sf"]
    m = lambda b: helpers.memory_exec(ctx, [[b]])
    plan = tpch.q3_plan(m(gen.customer(sf)), m(gen.orders(sf)), m(gen.lineitem(sf)), limit=10)
    out = plan.collect()
    assert len(out) == 1
    got, want = helpers.from_device(out[0]), plan_eval.collect(plan)
    assert og.batch_len(got) == 10
    helpers.assert_rows_equal(got, want, ordered=True, float_rtol=1e-9)        # revenue is a sum of products: the aggregate's own tolerance
    assert ctx.sort_limit_form() in ("topk", "topk_fallback")


# ---- the kernels are timed under their own names -------------------------------------------------------------------------------

def test_kernel_stats_name_the_topk_kernels(monkeypatch):
    monkeypatch.setenv("BHIP_KERNEL_TIMING", "2")             # every launch, however small (read when a context is created)
    c = ba.Context(0)
    rng = np.random.default_rng(5)
    b = OrderedDict([("f", OCol("Float64", rng.random(5000), rng.random(5000) > 0.01)), ("p", OCol("Int32", np.arange(5000)))])
    c.kernel_stats(reset=True)
    check(c, [b], [S("f")], 9, "topk")
    ks = c.kernel_stats(reset=True)
    for name in ("topk_diff", "topk_hist", "topk_pick", "topk_mark", "select_indices"):
        assert name in ks, ks
    assert "topk_fallback" != c.sort_limit_form() and ks["topk_diff"][1] == 1


# ---- memory: the input is never held whole ---------------------------------------------------------------------------------------

def test_peak_memory_is_one_batch_not_the_input():
    """16 generated lineitem batches of 2^20 rows (X bytes in use), ORDER BY l_extendedprice DESC, l_orderkey LIMIT 100 over them.
    A full sort concatenates and gathers the whole input: at least 2X above X.  The selection holds one batch's candidates and
    scratch: the bound X / 4 is a condition with a 4x margin over one batch (X / 16), not a measured value."""
    c = ba.Context(0)
    rows = 1 << 20
    parts = [ba.plan.tpch_lineitem(c, 10.0, tpch.SEED, i * rows, rows) for i in range(16)]
    c.synchronize()
    x, _ = c.memory()
    plan = ba.GlobalLimitExec(ba.SortExec([S("l_extendedprice", desc=True), S("l_orderkey")], ba.MemoryExec([parts], c)), 100)
    out = plan.collect()
    c.synchronize()
    _, peak = c.memory()
    print(f"in use before {x} B, peak {peak} B, above {peak - x} B, bound {x // 4} B")
    assert c.sort_limit_form() == "topk"
    assert len(out) == 1 and out[0].num_rows == 100
    assert peak - x < x / 4
    price = helpers.from_device(out[0])["l_extendedprice"].values
    assert np.all(price[:-1] >= price[1:])
