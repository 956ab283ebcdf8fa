"""CPU tier of the join-route tests: the expectation test_join_routes_gpu.py compares against (join_route_cases.reference_pairs, a dict
from key to build rows) agrees with the CPU oracle's join on every case and join type, and every case IS what its name says — its
rows and its key range on the stated side of the tiny build's and of window_ok's limits, sorted or not, with or without a duplicate,
its collision keys in the stated slots — computed from the keys and from constants read out of the sources."""
import re

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L
from oracle import engine as og

import helpers
import join_filter_cases as JF
import join_types_cases as JT
import join_route_cases as RC

ALL = RC.all_cases()
IDS = [RC.case_id(c) for c in ALL]


# ---- the constants ---------------------------------------------------------------------------------------------------------------------------

def test_constants_are_the_sources():
    assert (RC.TINY_BUILD_ROWS, RC.TINY_BUILD_WINDOW, RC.SEL_TILE, RC.JOIN_FILTER_MAX) == (1024, 1 << 16, 1024, 3)
    assert (RC.WINDOW_DIV, RC.WINDOW_SLACK) == (4096, 256)
    join = RC.source_text("host/ops_join.cpp")
    assert 'env_int("BHIP_RANK_WINDOW_LOG2", %d)' % RC.RANK_WINDOW_LOG2 in join
    assert "if (any_key && range <= (1ull << 30) && n >= (1 << 18)) {" in join               # PRESENT_MAX_RANGE, PRESENT_MIN_ROWS
    assert (RC.PRESENT_MAX_RANGE, RC.PRESENT_MIN_ROWS) == (1 << 30, 1 << 18)
    assert "n <= tiny_rank_build_max_rows()" in join and "int tiny_rank_build_max_rows() { return TINY_BUILD_ROWS; }" in RC.source_text("kernels_join.hip")
    assert "const bool build = any_key && range < TINY_BUILD_WINDOW;" in RC.source_text("kernels_join.hip")
    assert RC.TABLE_CAPACITY_SOURCE in RC.source_text("host/core.hpp")
    assert [RC.table_capacity(n) for n in (0, 1, 512, 513, 5000)] == [1024, 1024, 1024, 2048, 16384]
    # no data reaches the key-set bitmap: a range the bitmap takes is a range the rank map takes at the rows the bitmap needs
    assert RC.window_ok(RC.PRESENT_MAX_RANGE, RC.PRESENT_MIN_ROWS)
    assert sum(RC.BATCH_ROWS) == RC.N_PROBE == 6682 and RC.PROBE_BATCHES == [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
    assert RC.N_ALL > 192 and RC.N_NONE > 192                                               # more than the rank probe's LDS strip holds


def test_mix64_by_hand():
    """vm_device.h mix64: its four lines stand there as restated, and three values are pinned that do not come from the restatement —
    the lines are SplitMix64's output function behind its increment, so mix64(0), mix64(g) and mix64(2g) (g = 0x9E3779B97F4A7C15) are
    the first three numbers of the published SplitMix64 sequence for the seed 0; `by_hand` works the four lines out again with
    unbounded integers, reduced once per line"""
    text = RC.source_text("vm_device.h")
    at = text.index("__device__ inline uint64_t mix64(uint64_t z) {")
    body = text[at:text.index("}", at)]
    assert [ln.strip() for ln in body.splitlines()[1:]] == RC.MIX64_SOURCE
    m = RC.M64

    def by_hand(z):
        z = (z + 0x9E3779B97F4A7C15) % (1 << 64)
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 % (1 << 64)
        z = (z ^ (z >> 27)) * 0x94D049BB133111EB % (1 << 64)
        return z ^ (z >> 31)
    # splitmix64's published first outputs for the state 0 and the states one and two increments further on
    assert RC.mix64(0) == 0xE220A8397B1DCDAF == by_hand(0)
    assert RC.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4 == by_hand(0x9E3779B97F4A7C15)
    assert RC.mix64((2 * 0x9E3779B97F4A7C15) & m) == 0x06C45D188009454F == by_hand((2 * 0x9E3779B97F4A7C15) & m)
    assert RC.mix64(m) == by_hand(m) and RC.mix64(0xFFFFFFFF) == by_hand(0xFFFFFFFF)
    assert og.mix64(12345) == RC.mix64(12345)                                               # the oracle's own restatement agrees


def test_narrow_key_width_admits_the_types_the_cases_cover():
    text = RC.source_text("host/ops_join.cpp")
    assert "static int int_key_width(int t) { return (t == DT_INT32 || t == DT_DATE32) ? 4 : (t == DT_INT64 || t == DT_UINT64) ? 8 : 0; }" in text
    assert RC.WIDTH == {"Int32": 4, "Date32": 4, "Int64": 8, "UInt64": 8} and RC.DTYPES == list(RC.WIDTH)
    for t in RC.DTYPES:
        names = [c.name for c in RC.cases(dtype=t)]
        assert names == [c.name for c in RC.cases(dtype="Int32")] and len(set(names)) == len(names)


# ---- every case is what its name says -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_case_is_what_its_name_says(case):
    n, kmin, kmax = RC.key_stats(case)
    span = None if kmin is None else kmax - kmin
    dup, srt = RC.has_duplicates(case), RC.is_sorted(case)
    tiny_builds = n <= RC.TINY_BUILD_ROWS and span is not None and span < RC.TINY_BUILD_WINDOW and not dup
    # the route follows from the keys by try_narrow's rules
    if tiny_builds:
        route = "tiny"
    elif RC.window_ok(span, n):
        route = "packed/" + ("tiny" if n <= RC.TINY_BUILD_ROWS and span < RC.TINY_BUILD_WINDOW else "rank") if dup else "rank_sorted" if srt else "rank_any"
    else:
        route = "packed/table" if dup else "table"
    assert route == case.route, (route, case.route, n, span)
    assert dup == case.route.startswith("packed/") == ("duplicate" in case.name)
    name = case.name.split("/")[1]
    if "sorted" in name and "shuffled" not in name and "unsorted" not in name and "duplicate" not in name:
        assert srt
    if "shuffled" in name or "nulls" in name or "unsorted" in name:
        assert not srt or n == 1
    if "nulls" in name:
        bad = np.nonzero(~case.bvalid)[0].tolist()
        assert bad == sorted(set(r for r in (0, 63, 64, n - 1) if r < n)) or (n == 2 and bad == [0])
    else:
        assert case.bvalid is None
    m = re.search(r"_n(\d+)", name)
    if m:
        assert n == int(m.group(1))
    m = re.search(r"range_(\d+)", name)
    if m:
        assert span == int(m.group(1))
    lo, hi = RC.domain(RC.WIDTH[case.dtype])
    if case.name.startswith("tiny/") and case.route == "tiny":
        assert n <= RC.TINY_BUILD_ROWS and span < RC.TINY_BUILD_WINDOW
    if name == "n1025":
        assert n == RC.TINY_BUILD_ROWS + 1 and span < RC.TINY_BUILD_WINDOW                     # the rows alone decline it
    if name.startswith("range_65536"):
        assert span == RC.TINY_BUILD_WINDOW and n <= RC.TINY_BUILD_ROWS                        # the range alone declines it
    if name.startswith("window_limit_plus_1"):
        assert span == RC.window_limit(n) + 1 and not RC.window_ok(span, n) and RC.window_ok(span - 1, n) and span < 1 << RC.RANK_WINDOW_LOG2
    elif name.startswith("window_limit"):
        assert span == RC.window_limit(n) and RC.window_ok(span, n) and not RC.window_ok(span + 1, n)
    if name == "at_type_min":
        assert kmin == lo
    if name.startswith("at_type_max"):
        assert kmax == hi
    if name == "pieces_across_zero":
        assert kmin < 0 < kmax
    if case.name.startswith("table/") and case.route != "tiny":
        assert not RC.window_ok(span, n)                                                        # sparse by the data alone
    if name == "n1":                                                                            # ... which one row cannot be
        assert n == 1 and span == 0 and RC.window_ok(0, 1)
    keys = RC.signed_view(case.dtype, case.bkeys)
    if name == "type_ends":
        want = [lo, -1, 0, 1, hi] if RC.WIDTH[case.dtype] == 4 else [lo, -1, 0, hi]
        assert set(want) <= set(keys.tolist()) and span == hi - lo
    if name == "key_0_at_row_0":
        assert keys[0] == 0
    if name == "collisions":
        cap = RC.table_capacity(n)
        cluster, absent = RC.collision_keys(case.dtype, cap)
        homes = [RC.home_slot(case.dtype, k, cap) for k in cluster]
        assert len(cluster) >= 5 and all(h in (cap - 1, cap - 2) for h in homes) and set(cluster) <= set(keys.tolist())
        assert cap == 1024 and RC.home_slot(case.dtype, absent, cap) in (cap - 1, cap - 2) and absent not in set(keys.tolist())
        assert RC.signed_view(case.dtype, case.pkeys)[RC.EXTRA_ROW] == absent and case.pvalid[RC.EXTRA_ROW]
        # more keys than the two slots hold: the cluster wraps to slot 0 whatever else the table holds
        assert len(cluster) > 2


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_piece_logic_case_holds_the_runs_it_names(dtype):
    """rank_bits_sorted: 32-bit pieces of the bitmap holding exactly 1, 31 and 32 keys; 33, 63 and 64 consecutive key values; runs of one
    piece that start on a wave's lane 0, end on its lane 63 and straddle lane 63 -> lane 0; the last run ends on the last row with n not a
    multiple of 64"""
    for name in ("rank/pieces", "rank/pieces_across_zero"):
        case = RC.find(dtype, name)
        keys = RC.signed_view(dtype, case.bkeys)
        n = len(keys)
        piece = (keys - keys[0]) >> 5
        per_piece = np.bincount(piece)
        assert {1, 31, 32} <= set(per_piece.tolist())
        brk = np.nonzero(np.diff(keys) != 1)[0]
        runs = np.diff(np.concatenate([[-1], brk, [n - 1]]))
        assert {33, 63, 64} <= set(runs.tolist())
        rows = np.arange(n)
        same_next = np.concatenate([piece[1:] == piece[:-1], [False]])
        assert np.any(same_next & (rows % 64 == 63))                                            # one piece over two waves
        first = np.concatenate([[True], piece[1:] != piece[:-1]])
        last = ~same_next
        assert np.any(first & (rows % 64 == 0) & same_next) and np.any(last & (rows % 64 == 63) & ~first)
        assert np.any(last & ~first & (rows % 64 != 63) & (rows % 64 != 0))                     # a run strictly inside a wave: the plain store
        assert n % 64 != 0 and piece[-1] == piece[-2] and n > RC.TINY_BUILD_ROWS


# ---- the probe keys ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_probe_side_of_every_case(case):
    width = RC.WIDTH[case.dtype]
    lo, hi = RC.domain(width)
    n, kmin, kmax = RC.key_stats(case)
    pk = RC.signed_view(case.dtype, case.pkeys)
    assert len(pk) == RC.N_PROBE
    assert np.nonzero(~case.pvalid)[0].tolist() == RC.NULL_ROWS and {0, 63, 64, 1023, 1024, RC.N_PROBE - 1} <= set(RC.NULL_ROWS)
    live = set(pk[case.pvalid].tolist())
    valid = RC.signed_view(case.dtype, case.bkeys)
    valid = valid if case.bvalid is None else valid[case.bvalid]
    present = set(valid.tolist())
    if kmin is None:
        assert not present
        return
    span = kmax - kmin
    want = [kmin - 1, kmin, kmax, kmax + 1, kmin + 64 * ((span >> 6) + 1) - 1, kmin + 64 * ((span >> 6) + 1), lo, hi]
    if width == 4:
        want += [kmin - 1 - k for k in (0, 31, 32)]
    else:
        want += [kmin + (1 << 32), kmin + (1 << 34) - 1, kmin + (1 << 34), kmin + (1 << 63), kmin - 1]
        aliases = [k for k in live if k not in present and (k - (1 << 32) in present or k - (1 << 34) in present)]
        assert aliases or kmax + (1 << 32) > hi                                                 # the low 32 bits of a present key's offset
    for k in want:
        assert k in live or not lo <= k <= hi, k
    # the edge keys are on the stated side
    assert kmin in present and kmax in present
    assert kmin - 1 not in present and kmax + 1 not in present
    if width == 4 and kmin > lo + 33:
        assert all(kmin - 1 - k in live for k in (0, 31, 32))
    # the two closing batches
    none = pk[RC.N_MAIN:RC.N_MAIN + RC.N_NONE]
    every = pk[RC.N_MAIN + RC.N_NONE:]
    assert not set(none.tolist()) & present and set(every.tolist()) <= present
    hits = np.isin(pk[:RC.N_MAIN], valid).mean()
    assert 0.4 < hits < 0.6, hits


# ---- the reference against the oracle -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probe_nulls", [False, True], ids=["no_probe_nulls", "probe_nulls"])
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_reference_equals_the_oracle(case, probe_nulls):
    """og.hash_join is what plan_eval evaluates a HashJoinExec with (Inner / Left / Right); Full by join_types_cases' derivation from it"""
    left, right = RC.sides(case, probe_nulls)
    for jt in RC.TYPES:
        want = JT.expected(jt, left, right, RC.ON) if jt == JT.FULL else JT.oracle_join(left, right, RC.ON, jt)
        RC.assert_same_rows(RC.expected(jt, left, right), want)
    li, ri = RC.pairs(left, right)
    nl, nr = og.batch_len(left), og.batch_len(right)
    if case.name == "tiny/nulls_n1":                                                            # the all-NULL build side
        assert len(li) == 0 and not left["lk"].is_valid().any()
        return
    assert 0 < len(li) < nl * nr                                                               # neither empty nor the cross product
    assert left["lk"].is_valid()[li].all() and right["rk"].is_valid()[ri].all()
    assert len(set(zip(li.tolist(), ri.tolist()))) == len(li)
    if not RC.has_duplicates(case):
        assert len(set(ri.tolist())) == len(ri)                                                # a unique build side: at most one partner
    if probe_nulls:
        assert not set(ri.tolist()) & set(RC.NULL_ROWS)


# ---- the probe shapes ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_shape_sides_and_their_filters(order):
    left, right = RC.shape_sides(order)
    lk = left["lk"].values
    assert (bool(np.all(lk[1:] > lk[:-1]))) == (order == "sorted") and len(np.unique(lk)) == len(lk) == RC.SHAPE_NL > RC.TINY_BUILD_ROWS
    assert RC.window_ok(int(lk.max()) - int(lk.min()), len(lk))
    other = RC.shape_sides("shuffled" if order == "sorted" else "sorted")[0]
    assert sorted(zip(other["lk"].values.tolist(), other["li"].values.tolist())) == sorted(zip(lk.tolist(), left["li"].values.tolist()))
    assert sum(RC.SHAPE_BATCHES) == RC.SHAPE_NR == og.batch_len(right)
    kept = {}
    for name, terms in RC.FILTERS.items():
        assert len(terms) in (1, RC.JOIN_FILTER_MAX)
        keep = RC.filter_keep(name, right)
        got = og.filter_batch(right, RC.filter_expr(name))                                      # the oracle's evaluator agrees with numpy
        assert np.array_equal(got["ri"].values, np.nonzero(keep)[0])
        kept[name] = int(keep.sum())
        for jt in RC.TYPES:
            side = RC.kept_side(name, right)
            want = JT.expected(jt, left, side, RC.ON) if jt == JT.FULL else JT.oracle_join(left, side, RC.ON, jt)
            RC.assert_same_rows(RC.expected(jt, left, side), want)
    assert kept["one_term_empty"] == kept["three_terms_one_empty"] == 0
    assert kept["one_term_int32_ends"] == kept["three_terms_all_pass"] == RC.SHAPE_NR
    assert 0 < kept["three_terms"] < kept["one_term"] < RC.SHAPE_NR
    ra, rc = right["ra"].values, right["rc"].values
    assert ra.min() == RC.I32_MIN and ra.max() == RC.I32_MAX and rc.min() == RC.I32_MIN and rc.max() == RC.I32_MAX


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("build", ["rank", "table"])
@pytest.mark.parametrize("form", ["first_column", "pairs"])
def test_pair_sides(form, build, order):
    left, right = RC.pair_sides(form, build, order)
    a, b = left["lk"].values.astype(np.int64), left["lb"].values.astype(np.int64)
    n = len(a)
    first_unique = len(np.unique(a)) == n
    assert first_unique == (form == "first_column")
    packed = (a << 32) | (b & 0xFFFFFFFF)
    assert len(np.unique(packed)) == n
    key = a if form == "first_column" else packed
    assert RC.window_ok(int(key.max()) - int(key.min()), n) == (build == "rank")
    if build == "rank":
        assert bool(np.all(key[1:] > key[:-1])) == (order == "sorted")
    for jt in (JF.INNER, JF.RIGHT):
        RC.assert_same_rows(RC.expected(jt, left, right, RC.PAIR_ON), JT.oracle_join(left, right, RC.PAIR_ON, jt))
    li, ri = RC.pairs(left, right, RC.PAIR_ON)
    first_only = RC.pairs(left, right, RC.ON)[0] if form == "first_column" else None
    assert 0 < len(li) < og.batch_len(right)
    if form == "first_column":
        assert len(li) < len(first_only)                                                        # the second column rejects some first-column matches


@pytest.mark.parametrize("dtype", ["Int32", "Int64"])
@pytest.mark.parametrize("n", [RC.PRESENT_MIN_ROWS, RC.PRESENT_MIN_ROWS + 37])
def test_key_set_bitmap_sides(dtype, n):
    left, right, span = RC.present_sides(dtype, n)
    assert og.batch_len(left) == n >= RC.PRESENT_MIN_ROWS and span <= RC.PRESENT_MAX_RANGE
    assert RC.window_ok(span, n)                                                                # by the data: the rank map; the table only when forced
    lk = RC.signed_view(dtype, left["lk"].values)[left["lk"].is_valid()]
    assert len(np.unique(lk)) == len(lk) == n - 4
    li, ri = RC.pairs(left, right)
    assert 2000 < len(li) < 3000
    rk = set(RC.signed_view(dtype, right["rk"].values)[right["rk"].is_valid()].tolist())
    assert {int(lk.min()) - 1, int(lk.min()), int(lk.max()), int(lk.max()) + 1} <= rk


# ---- the accessor ---------------------------------------------------------------------------------------------------------------------------------------

def test_join_probe_form_hook_is_declared_exported_and_mirrored():
    header = open(helpers.ROOT + "/include/ballista_hip.h").read()
    assert "const char* bhip_ctx_join_probe_form(bhip_ctx* ctx);" in header
    assert "bhip_ctx_join_probe_form" in L.SYMBOLS
    assert L.lib().bhip_ctx_join_probe_form(None) == b""                                        # no context: the empty form, not a crash
    assert callable(ba.Context.join_probe_form)
    assert RC.rank_probe_form() == "rank/mapbuf" and RC.rank_probe_form(perm=True, mode="rows8") == "rank/mapbuf+perm"
    assert RC.rank_probe_form(bits=True) == "rank/bits" and RC.rank_probe_form(bits=True, mode="nobits") == "rank/mapbuf"
    assert RC.rank_probe_form(bits=True, mode="flat") == "rank/flat" and RC.rank_probe_form(resid=True, mode="rows8") == "rank/mapbuf+resid+rows8"
    assert RC.rank_probe_form(mode="noscalar") == "rank/mapbuf+gather" and RC.rank_probe_form(mode="rows8", width=8) == "rank/mapbuf"
