"""GPU parity of HashJoinExec on keys wider than the 16-byte packed key: the third build-side form, a hash table over 64-bit row
hashes whose equality test reads the key columns (kernels_hash.hip: join_build_wide / join_probe_{match,count,emit}_wide).
It is taken when the key LAYOUT does not fit (plan time), when a build value does not fit (build time), for the probe batches
whose values do not fit a packed build side (the wide table is then built beside the packed one), and under BHIP_JOIN_WIDE=1.

The reference for results is the CPU oracle (oracle.plan_eval: hash_join keys on Python tuples, no width limit); rows compare as
multisets.  Sizes: 900 build rows in two partitions, 5000 probe rows in two partitions, the first cut at 1025 rows (one past the
1024-row selection tile).  Every row carries its row number (li / ri), so an output row is identified by the pair."""
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
JOIN_TYPES = [ba.plan.INNER, ba.plan.LEFT, ba.plan.RIGHT]
NL, NR = 900, 5000
IDS = ["li", "ri"]


def with_ids(prefix, n, cols):
    return OrderedDict(list(cols) + [(prefix + "i", OCol("Int64", np.arange(n, dtype=np.int64)))])


def build_exec(ctx, left, n=None):
    n = len(left["li"].values) if n is None else n
    cut = min(400, n)
    return helpers.memory_exec(ctx, [[helpers.slice_batch(left, 0, cut)], [helpers.slice_batch(left, cut, n)]])


def probe_exec(ctx, right):
    return helpers.memory_exec(ctx, [[helpers.slice_batch(right, 0, 1025), helpers.slice_batch(right, 1025, 3000)], [helpers.slice_batch(right, 3000, NR)]])


def check_partitions(plan, form=None, ctx=None):
    """every output partition against the oracle's (a Left join emits its unmatched build rows once per task)"""
    for p in range(2):
        got = helpers.concat([helpers.from_device(b) for b in plan.execute(p)])
        want = helpers.concat(plan_eval.execute(plan, p))
        helpers.assert_rows_equal(got, want, ordered=False, key_cols=IDS)
    if form is not None:
        assert ctx.join_key_form() == form


def check(plan, keys=IDS, **kw):
    got = helpers.concat(helpers.collect_product(plan))
    helpers.assert_rows_equal(got, plan_eval.collect(plan), ordered=False, key_cols=keys, **kw)
    return got


# ---- 1. one Utf8 key: value lengths and near-equal values ----------------------------------------------------------------------

P15 = "ABCDEFGHIJKLMNO"                      # 15 bytes: the most a single Utf8 join key holds in the packed key
assert len(P15) == 15


def string_pool(rng, n):
    """n distinct strings: lengths 0, 1, 14 .. 17, 40, 300; values equal in their first 15 bytes; a value and its proper prefixes;
    values that differ in the last byte only; then fillers of 2 .. 44 bytes"""
    special = ["", "a", "b", P15[:14], P15, P15 + "x", P15 + "y", P15 + "xy", P15 + "xz", P15[:14] + "P", "Q" * 16, "Q" * 15 + "R", "Q" * 17,
               "w" * 39 + "1", "w" * 39 + "2", "w" * 40 + "1", "z" * 299 + "A", "z" * 299 + "B", "z" * 300, "z" * 298]
    assert sorted(len(s) for s in special)[:2] == [0, 1] and {14, 15, 16, 17, 40, 300} <= {len(s) for s in special}
    out = list(special)
    i = 0
    while len(out) < n:
        out.append("k%05d-" % i + "f" * int(rng.integers(0, 38)))
        i += 1
    assert len(set(out)) == len(out)
    return out[:n]


def utf8_sides(unique, nulls, seed=1):
    rng = np.random.default_rng(seed)
    pool = string_pool(rng, NL if unique else 300)
    lk = [pool[i] for i in (rng.permutation(NL) if unique else np.concatenate([np.arange(300), rng.integers(0, 300, NL - 300)]))]
    # probe values: build values, their 15-byte truncations, values one byte longer, values with the last byte changed, strangers
    rk = []
    for j in range(NR):
        s = pool[int(rng.integers(0, len(pool)))]
        how = int(rng.integers(0, 10))
        rk.append(s if how < 6 else s[:15] if how == 6 else s + "x" if how == 7 else (s[:-1] + "~" if s else "~") if how == 8 else "stranger-%d" % j)
    lv = (rng.random(NL) > 0.1) if nulls else None
    rv = (rng.random(NR) > 0.1) if nulls else None
    if nulls:                                          # the empty string next to NULL, on both sides
        lk[0], lk[1], lv[0], lv[1] = "", "", True, False
        rk[0], rk[1], rk[1026], rv[0], rv[1], rv[1026] = "", "", "", True, False, True
    left = with_ids("l", NL, [("lk", OCol("Utf8", lk, lv)), ("lx", OCol("Float64", rng.random(NL)))])
    right = with_ids("r", NR, [("rk", OCol("Utf8", rk, rv)), ("rd", OCol("Date32", rng.integers(9000, 10000, NR).astype(np.int32)))])
    return left, right


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("unique", [True, False])
@pytest.mark.parametrize("nulls", [False, True])
def test_one_utf8_key_of_any_length(ctx, jt, unique, nulls):
    left, right = utf8_sides(unique, nulls)
    plan = ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right), [("lk", "rk")], jt)
    check_partitions(plan, "wide", ctx)


# ---- 2. layouts the packed key cannot hold ---------------------------------------------------------------------------------------

LAYOUTS = {
    "int64x3": (["Int64", "Int64", "Int64"], 12),
    "utf8x2": (["Utf8", "Utf8"], 40),
    "int64_utf8": (["Int64", "Utf8"], 40),
    "int32_date32_int64_utf8": (["Int32", "Date32", "Int64", "Utf8"], 7),
}


def part_column(dtype, v, valid):
    if dtype == "Utf8":                                                      # 9 .. 13 bytes: more than any of these layouts leaves a string
        return OCol("Utf8", ["part-%03d-" % x + "x" * (x % 5) for x in v], valid)
    if dtype == "Int64":
        return OCol("Int64", v.astype(np.int64) * 10 ** 10 - 5, valid)
    return OCol(dtype, (v + (9000 if dtype == "Date32" else -3)).astype(np.int32), valid)


def layout_sides(types, radix, unique, seed):
    rng = np.random.default_rng(seed)
    space = radix ** len(types)
    lc = rng.permutation(space)[:NL] if unique else rng.integers(0, 300, NL)
    rc = rng.integers(0, space, NR)
    digits = lambda c: [(c // radix ** i) % radix for i in range(len(types))]
    lcols, rcols = [], []
    for i, (t, lv, rv) in enumerate(zip(types, digits(lc), digits(rc))):
        # NULLs in ONE part only (the second): a row with a NULL there matches nothing, whatever the other parts hold
        lcols.append(("l%d" % i, part_column(t, lv, (rng.random(NL) > 0.1) if i == 1 else None)))
        rcols.append(("r%d" % i, part_column(t, rv, (rng.random(NR) > 0.1) if i == 1 else None)))
    left = with_ids("l", NL, lcols + [("lx", OCol("Float64", rng.random(NL)))])
    right = with_ids("r", NR, rcols + [("rs", OCol("Utf8", ["r%d" % (j % 7) for j in range(NR)]))])
    return left, right, [("l%d" % i, "r%d" % i) for i in range(len(types))]


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("unique", [True, False])
def test_key_layouts_wider_than_the_packed_key(ctx, jt, layout, unique):
    types, radix = LAYOUTS[layout]
    left, right, on = layout_sides(types, radix, unique, seed=len(layout))
    plan = ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right), on, jt)
    check_partitions(plan, "wide", ctx)


# ---- 3. run-time discovery ----------------------------------------------------------------------------------------------------------

def discovery_sides(long_build, long_probe, seed=4):
    rng = np.random.default_rng(seed)
    lk = ["b%04d" % i + "-" * (i % 10) for i in range(NL)]                  # 5 .. 14 bytes, distinct
    rk = [lk[int(i)] if i < NL else "none-%d" % i for i in rng.integers(0, NL + 200, NR)]
    long_value = "0123456789abcdef"                                          # 16 bytes: one more than the packed key holds
    if long_build:
        lk[7] = long_value
        lk[8] = long_value[:15]
    if long_probe:
        rk[2000] = long_value                                                # in the SECOND batch of the first probe partition
    rk[5], rk[3500] = long_value[:15], long_value[:15]
    assert all(len(s.encode()) <= 15 for s in rk[:1025] + rk[3000:]) and (long_build or all(len(s) <= 15 for s in lk))
    left = with_ids("l", NL, [("lk", OCol("Utf8", lk)), ("lx", OCol("Float64", rng.random(NL)))])
    right = with_ids("r", NR, [("rk", OCol("Utf8", rk)), ("ry", OCol("Int64", rng.integers(0, 10 ** 9, NR)))])
    return left, right


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("long_side,form", [("probe", "wide"), ("build", "wide"), ("both", "wide"), ("none", "packed")])
def test_a_long_value_is_discovered_at_run_time(ctx, jt, long_side, form):
    """a packed build side and a probe batch with one 16-byte value: that batch goes through the wide table built over the same
    build rows, the batches before and after it keep the packed probe, and a Left join's matched bits cover both; a long build
    value sends the build itself to the wide table; with no long value anywhere the join is the packed join it was"""
    left, right = discovery_sides(long_side in ("build", "both"), long_side in ("probe", "both"))
    plan = ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right), [("lk", "rk")], jt)
    check_partitions(plan, form, ctx)
    # the node has learned its form: executing it again gives the same rows and reports the same form
    check_partitions(plan, form, ctx)


# ---- 4. BHIP_JOIN_WIDE=1: the wide table where the packed one would be built ------------------------------------------------

def ab_sides(kind, seed=6):
    rng = np.random.default_rng(seed)
    lv = rng.random(NL) > 0.1
    rv = rng.random(NR) > 0.1
    if kind in ("Int32", "Int64", "Date32"):                                 # duplicates: the narrow structures decline them
        np_t = np.int64 if kind == "Int64" else np.int32
        scale = 10 ** 10 if kind == "Int64" else 1
        lk = OCol(kind, (rng.integers(0, 300, NL) * scale - 7).astype(np_t), lv)
        rk = OCol(kind, (rng.integers(0, 350, NR) * scale - 7).astype(np_t), rv)
    elif kind == "Utf8":                                                     # 0 .. 7 bytes
        lk = OCol("Utf8", ["s%d" % i if i else "" for i in rng.integers(0, 300, NL)], lv)
        rk = OCol("Utf8", ["s%d" % i if i else "" for i in rng.integers(0, 350, NR)], rv)
    else:                                                                    # Float64 with both zeros and two NaNs
        vals = np.concatenate([np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1.5, -1.5]), rng.random(40)])
        lk = OCol("Float64", vals[rng.integers(0, len(vals), NL)], lv)
        rk = OCol("Float64", vals[rng.integers(0, len(vals), NR)], rv)
    left = with_ids("l", NL, [("lk", lk), ("ls", OCol("Utf8", ["L%d" % (i % 11) for i in range(NL)]))])
    right = with_ids("r", NR, [("rk", rk), ("ry", OCol("Int64", rng.integers(0, 10 ** 9, NR)))])
    return left, right


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("kind", ["Int32", "Int64", "Date32", "Utf8", "Float64"])
def test_forced_wide_equals_packed(ctx, jt, kind, monkeypatch):
    """the same join through the packed table and, forced, through the wide table: equal rows, and equal to the oracle.  Float64
    keys compare by bits in both (-0.0 and +0.0 are different keys, a NaN matches the NaN of the same bits — DESIGN §3.3), which
    is not what Python tuples do: there the packed result is the reference"""
    left, right = ab_sides(kind)
    results = {}
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("BHIP_JOIN_WIDE", "1")
        else:
            monkeypatch.delenv("BHIP_JOIN_WIDE", raising=False)
        plan = ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right), [("lk", "rk")], jt)
        results[forced] = helpers.concat(helpers.collect_product(plan))
        assert ctx.join_key_form() == ("wide" if forced else "packed")
        if kind != "Float64":
            helpers.assert_rows_equal(results[forced], plan_eval.collect(plan), ordered=False, key_cols=IDS)
    helpers.assert_rows_equal(results[True], results[False], ordered=False, key_cols=IDS)
    if kind == "Float64":                                                     # the rule itself, on the packed result
        g = results[False]
        for a, b, av, bv in zip(g["lk"].values, g["rk"].values, g["lk"].is_valid(), g["rk"].is_valid()):
            if av and bv:
                assert np.float64(a).tobytes() == np.float64(b).tobytes()
        pairs = [(a, b) for a, b, av, bv in zip(g["lk"].values, g["rk"].values, g["lk"].is_valid(), g["rk"].is_valid()) if av and bv]
        assert any(a != a for a, _ in pairs) and any(a == 0 for a, _ in pairs)    # NaN keys and zero keys did find partners


# ---- 5. under parents ---------------------------------------------------------------------------------------------------------------

def test_an_aggregate_reads_two_columns_of_a_wide_join(ctx):
    left, right = utf8_sides(unique=False, nulls=True, seed=9)
    left["lg"] = OCol("Utf8", ["g%d" % (i % 13) for i in range(NL)])
    right["ry"] = OCol("Int64", np.arange(NR, dtype=np.int64) % 1000)
    for jt in JOIN_TYPES:
        j = ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right), [("lk", "rk")], jt)
        aggs = [E.Sum(col("ry"), "s"), E.Count(lit(1, E.UINT8), "n")]
        agg = ba.HashAggregateExec(ba.plan.PARTIAL, [(col("lg"), "lg")], aggs, j)
        fin = ba.HashAggregateExec(ba.plan.FINAL, [(col("lg"), "lg")], aggs, ba.MergeExec(agg))
        check(fin, ["lg"])
        assert ctx.join_key_form() == "wide"


@pytest.mark.parametrize("jt", JOIN_TYPES)
def test_projection_over_filter_on_the_probe_side_of_a_wide_join(ctx, jt):
    """late materialisation: the probe runs on the filter's input, only the key column of the surviving rows is gathered"""
    left, right = utf8_sides(unique=True, nulls=True, seed=10)
    flt = ba.FilterExec(E.coerce(col("rd") > E.date32("1996-01-01"), {"rk": "Utf8", "rd": "Date32", "ri": "Int64"}), probe_exec(ctx, right))
    proj = ba.ProjectionExec([(col("ri"), "ri"), (col("rk"), "key")], ba.CoalesceBatchesExec(flt, 4096))
    plan = ba.HashJoinExec(build_exec(ctx, left), proj, [("lk", "key")], jt)
    assert [n for n, _, _ in plan.schema()] == ["lk", "lx", "li", "ri", "key"]
    check(plan)
    assert ctx.join_key_form() == "wide"


@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("shape", ["probe_chain", "build_chain"])
def test_payload_columns_cross_a_wide_join_as_views(ctx, jt, shape):
    """three joins in a row (tests/test_join_paths_gpu.py: test_payload_columns_pass_through_joins_as_views) with a long-string key
    in the middle one: the columns it only passes on arrive and leave as views, its own key column is gathered"""
    rng = np.random.default_rng(5)
    na, nb, nc, nd = 60, 900, 4000, 300
    name = lambda i: "a-long-join-key-%06d" % i                              # 22 bytes
    a = OrderedDict([("ak", OCol("Int32", np.arange(na, dtype=np.int32))), ("aname", OCol("Utf8", ["name-%d" % (i % 13) for i in range(na)], rng.random(na) > 0.1))])
    b = OrderedDict([("bname", OCol("Utf8", [name(i + 5) for i in range(nb)])), ("b_ak", OCol("Int32", rng.integers(-3, na + 3, nb).astype(np.int32), rng.random(nb) > 0.05)),
                     ("bflag", OCol("Boolean", rng.random(nb) > 0.5, rng.random(nb) > 0.2))])
    c = OrderedDict([("c_bname", OCol("Utf8", [name(int(i)) for i in rng.integers(0, nb + 20, nc)])), ("cx", OCol("Float64", rng.random(nc), rng.random(nc) > 0.1)),
                     ("cs", OCol("Utf8", ["c%d" % (i % 29) for i in range(nc)])), ("c_dk", OCol("Int32", rng.integers(0, nd + 10, nc).astype(np.int32))),
                     ("ci", OCol("Int64", np.arange(nc, dtype=np.int64)))])
    d = OrderedDict([("dk", OCol("Int32", np.arange(nd, dtype=np.int32))), ("dy", OCol("Int64", rng.integers(0, 1000, nd)))])
    A, B, C, D = (helpers.memory_exec(ctx, [[t]]) for t in (a, b, c, d))
    proj = lambda names, p: ba.ProjectionExec([(col(n), n) for n in names], p)
    j1 = proj(["bname", "aname", "bflag"], ba.HashJoinExec(A, B, [("ak", "b_ak")], jt))
    mid = ba.HashJoinExec(j1, C, [("bname", "c_bname")], jt)
    if shape == "probe_chain":
        top = ba.HashJoinExec(D, proj(["aname", "bflag", "cx", "cs", "c_dk", "ci", "bname"], mid), [("dk", "c_dk")], jt)
    else:
        top = ba.HashJoinExec(proj(["c_dk", "aname", "cx", "bflag", "ci", "bname"], mid), D, [("c_dk", "dk")], jt)
    check(top, ["ci", "dk", "bname", "aname"])


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------------

LONG = "the-same-long-join-key-for-every-build-row"                            # 42 bytes


def test_empty_sides_one_build_row_and_all_null_keys(ctx):
    left, right = utf8_sides(unique=True, nulls=False, seed=12)
    long_row = next(i for i, s in enumerate(left["lk"].values) if len(s) > 15)
    e_left, e_right, one = helpers.slice_batch(left, 0, 0), helpers.slice_batch(right, 0, 0), helpers.slice_batch(left, long_row, long_row + 1)
    null_left = OrderedDict(left, lk=OCol("Utf8", list(left["lk"].values), np.zeros(NL, np.bool_)))
    null_right = OrderedDict(right, rk=OCol("Utf8", list(right["rk"].values), np.zeros(NR, np.bool_)))
    for jt in JOIN_TYPES:
        for l, r in [(e_left, right), (left, e_right), (one, right), (null_left, right), (left, null_right)]:
            plan = ba.HashJoinExec(helpers.memory_exec(ctx, [[l]]), helpers.memory_exec(ctx, [[r]]), [("lk", "rk")], jt)
            check(plan)


@pytest.mark.parametrize("jt", JOIN_TYPES)
def test_every_build_row_carries_the_same_long_key(ctx, jt):
    """one chain of 900 rows: the counts, the scan and the emit, for an output (150 x 900 rows) larger than either input"""
    rk = [LONG if j % 4 else LONG[:-1] + "?" for j in range(200)]
    left = with_ids("l", NL, [("lk", OCol("Utf8", [LONG] * NL))])
    right = with_ids("r", 200, [("rk", OCol("Utf8", rk))])
    plan = ba.HashJoinExec(build_exec(ctx, left), helpers.memory_exec(ctx, [[right]]), [("lk", "rk")], jt)
    got = check(plan)
    assert len(got["li"].values) == 150 * NL + (50 if jt == ba.plan.RIGHT else 0)
    assert ctx.join_key_form() == "wide"


def test_left_join_emits_each_unmatched_build_row_once_per_task(ctx):
    left, right = utf8_sides(unique=True, nulls=True, seed=14)
    plan = ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right), [("lk", "rk")], ba.plan.LEFT)
    for p in range(2):
        got = helpers.concat([helpers.from_device(b) for b in plan.execute(p)])
        helpers.assert_rows_equal(got, helpers.concat(plan_eval.execute(plan, p)), ordered=False, key_cols=IDS)
        li, rv = got["li"].values, got["ri"].is_valid()
        unmatched = sorted(int(i) for i, v in zip(li, rv) if not v)
        matched = {int(i) for i, v in zip(li, rv) if v}
        assert len(unmatched) == len(set(unmatched)) and not (set(unmatched) & matched)
        assert sorted(set(unmatched) | matched) == list(range(NL))               # every build row comes out, matched or once


# ---- 7. Q10-shaped: join on c_name, aggregate by (c_name, c_address) ------------------------------------------------------------

def test_q10_shaped_join_and_aggregate_on_names(ctx):
    rng = np.random.default_rng(10)
    nc, no = 2000, 10_000
    names = ["Customer#%09d" % (i + 1) for i in range(nc)]
    assert all(len(s) == 18 for s in names)
    customer = OrderedDict([("c_name", OCol("Utf8", names)), ("c_address", OCol("Utf8", ["addr-%d-" % i + "q" * int(k) for i, k in enumerate(rng.integers(0, 30, nc))])),
                            ("c_acctbal", OCol("Float64", rng.random(nc) * 1e4))])
    picks = rng.integers(0, nc + 100, no)
    orders = OrderedDict([("o_name", OCol("Utf8", ["Customer#%09d" % (int(i) + 1) for i in picks])), ("o_totalprice", OCol("Float64", rng.random(no) * 1e5))])
    cm = helpers.memory_exec(ctx, [[helpers.slice_batch(customer, 0, 900)], [helpers.slice_batch(customer, 900, nc)]])
    om = helpers.memory_exec(ctx, [[helpers.slice_batch(orders, 0, 1025), helpers.slice_batch(orders, 1025, 6000)], [helpers.slice_batch(orders, 6000, no)]])
    j = ba.HashJoinExec(cm, om, [("c_name", "o_name")], ba.plan.INNER)
    group = [(col("c_name"), "c_name"), (col("c_address"), "c_address")]
    aggs = [E.Sum(col("o_totalprice"), "revenue"), E.Count(lit(1, E.UINT8), "n")]
    fin = ba.HashAggregateExec(ba.plan.FINAL, group, aggs, ba.MergeExec(ba.HashAggregateExec(ba.plan.PARTIAL, group, aggs, j)))
    got = check(fin, ["c_name", "c_address"], float_rtol=1e-9)
    assert ctx.join_key_form() == "wide"
    assert len(got["c_name"].values) == len({int(i) for i in picks if i < nc})
