"""CPU tier of the scan launch-form tests: every case of scan_cases.py lies on the side of each limit that its name says, with the
limits read out of kernels_util.hip, and the expectations test_scan_forms_gpu.py compares against agree with a second statement —
Python's str(int) for the digit counts and offsets, join_route_cases.reference_pairs (the plain loop) and the CPU oracle's join for
the pairs."""
import numpy as np
import pytest

from oracle import engine as og

import join_route_cases as RC
import scan_cases as SC


def test_constants_and_the_ladder_are_the_sources():
    assert (SC.C, SC.SCAN_ONE_LAUNCH_MAX, SC.SCAN_TWO_LAUNCH_CHUNKS, SC.RP_CHUNK) == (4096, 8 * 4096, 2048, 16384)
    util = RC.source_text("kernels_util.hip")
    for line in SC.LADDER_SOURCE:
        assert util.count(line) == 2, line                            # exclusive_scan_t and launch_rank_pack
    assert "if (n_chunks == 0) {" in util and "if (n <= 0) return total_out ?" in util
    assert "const int64_t n_chunks = (n + RP_CHUNK - 1) / RP_CHUNK;" in util and "const int64_t n_chunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;" in util
    assert SC.N_GRAN_SOURCE in RC.source_text("host/ops_join.cpp")
    # one apply kernel template, the raw carry and the ladder of shuffles stated once
    assert util.count("scan_apply_kernel(") == 1 and "scan_apply_raw_kernel" not in util
    assert util.count("before += chunk_sums[j]") == 1 and "before += chunk_offsets[j]" not in util
    assert "__shfl_up" not in util


@pytest.mark.parametrize("name, n, form", SC.SIZES, ids=SC.SIZE_IDS)
def test_each_size_lies_where_its_name_says(name, n, form):
    assert SC.launch_form(n) == form
    chunks = -(-n // SC.C)
    want = {"0": n == 0, "1": n == 1, "chunk_minus_1": n == SC.C - 1, "chunk": n == SC.C and chunks == 1, "chunk_plus_1": chunks == 2 and n % SC.C == 1,
            "one_launch_max": n == SC.SCAN_ONE_LAUNCH_MAX and SC.launch_form(n + 1) == "two",
            "one_launch_max_plus_1": SC.launch_form(n - 1) == "one",
            "two_launch_chunks": chunks == SC.SCAN_TWO_LAUNCH_CHUNKS and n % SC.C == 0 and SC.launch_form(n + 1) == "three",
            "two_launch_chunks_plus_1": SC.launch_form(n - 1) == "two" and chunks == SC.SCAN_TWO_LAUNCH_CHUNKS + 1,
            "two_launch_chunks_plus_chunk_plus_1": chunks == SC.SCAN_TWO_LAUNCH_CHUNKS + 2 and n % SC.C == 1}
    assert want[name]


def test_sizes_cover_every_form_and_both_sides_of_each_limit():
    assert [f for _, _, f in SC.SIZES] == ["none"] + ["one"] * 5 + ["two"] * 2 + ["three"] * 2
    assert SC.N_MAX == SC.TWO + SC.C + 1


# ---- cast ------------------------------------------------------------------------------------------------------------------------------

def test_cast_values_have_every_length_and_differ_across_every_chunk_boundary():
    v = SC.cast_values(SC.N_MAX)
    lens = SC.digit_counts(v)
    assert sorted(set(lens[:SC.C - 1].tolist())) == list(range(1, 12))           # all of 1 .. 11 already inside the smallest chunk case
    b = SC.chunk_boundaries(SC.N_MAX)
    assert len(b) == SC.SCAN_TWO_LAUNCH_CHUNKS + 1 and np.all(lens[b - 1] == 1) and np.all(lens[b] == 11)
    assert (v < 0).any() and (v == SC.I32_MIN).any() and (v == 0).any()
    assert int(lens.sum()) < (1 << 31)                                              # Int32 offsets hold the total


@pytest.mark.parametrize("name, n, form", SC.SIZES, ids=SC.SIZE_IDS)
def test_cast_offsets_are_the_lengths_of_str(name, n, form):
    """the numpy digit counts against len(str(int)): every row up to SMALL_MAX, the compared windows and a sample beyond; the offsets
    against a running Python sum"""
    v, off = SC.cast_values(n), SC.cast_offsets(n)
    assert len(off) == n + 1 and off[0] == 0
    lens = SC.digit_counts(v)
    rows = np.unique(np.concatenate([np.arange(a, b) for a, b in SC.windows(n)] + [np.random.default_rng(n).integers(0, max(n, 1), 20000 if n else 0)]))
    assert [len(str(x)) for x in v[rows].tolist()] == lens[rows].tolist()
    assert np.array_equal(np.diff(off), lens)
    for a, b in SC.windows(n):
        assert len(SC.cast_text(v[a:b])) == off[b] - off[a]
    total = 0
    for x in v[:min(n, SC.SMALL_MAX)].tolist():
        total += len(str(x))
    assert total == off[min(n, SC.SMALL_MAX)]


def test_windows_of_the_large_sizes():
    for _, n, _ in SC.SIZES:
        w = SC.windows(n)
        if n <= SC.SMALL_MAX:
            assert w == [(0, n)]
        else:
            last = (n - 1) // SC.C * SC.C
            assert w[0] == (0, 2 * SC.C) and w[2] == (n - 2 * SC.C, n) and w[1][0] == last - SC.C and last < w[1][1] <= n
            assert all(0 <= a < b <= n for a, b in w)


# ---- probe -----------------------------------------------------------------------------------------------------------------------------

def test_probe_keys_have_0_to_3_partners_and_differ_across_every_chunk_boundary():
    k = SC.probe_keys(SC.N_MAX)
    assert sorted(set(k.tolist())) == [0, 1, 2, 3]
    assert [SC.BUILD_KEYS.count(x) for x in range(4)] == [0, 1, 2, 3]
    b = SC.chunk_boundaries(SC.N_MAX)
    assert np.all(k[b - 1] != k[b]) and len(set((k[b].astype(int) - k[b - 1]).tolist())) > 2
    assert sorted(set(k[:SC.C - 1].tolist())) == [0, 1, 2, 3]


@pytest.mark.parametrize("name, n, form", [s for s in SC.SIZES if s[1] <= SC.SMALL_MAX], ids=[s[0] for s in SC.SIZES if s[1] <= SC.SMALL_MAX])
def test_probe_pairs_are_the_plain_dict_join_and_the_oracles(name, n, form):
    left, right = SC.id_side("l", SC.BUILD_KEYS), SC.id_side("r", SC.probe_keys(n))
    li, ri = SC.probe_pairs(n)
    wl, wr = RC.reference_pairs(left, right)
    assert np.array_equal(li, wl) and np.array_equal(ri, wr)
    o = og.hash_join(left, right, RC.ON, "Inner")
    assert np.array_equal(SC.pair_codes(o["li"].values, o["ri"].values, len(SC.BUILD_KEYS)), SC.pair_codes(li, ri, len(SC.BUILD_KEYS)))


def test_probe_pairs_of_the_large_sizes():
    """a size's pairs are a prefix of the largest size's; their number is the sum of the keys (key k has k partners); inside the compared
    windows they are the plain loop's"""
    k = SC.probe_keys(SC.N_MAX)
    for _, n, _ in SC.SIZES:
        li, ri = SC.probe_pairs(n)
        assert len(li) == len(ri) == int(k[:n].astype(np.int64).sum()) and (n == 0 or len(ri) == 0 or ri[-1] < n)
        if n > SC.SMALL_MAX:
            left = SC.id_side("l", SC.BUILD_KEYS)
            for a, b in SC.windows(n):
                wl, wr = RC.reference_pairs(left, SC.id_side("r", k[a:b]))
                lo, hi = np.searchsorted(ri, a), np.searchsorted(ri, b)
                assert np.array_equal(li[lo:hi], wl) and np.array_equal(ri[lo:hi], wr + a)


# ---- rank ------------------------------------------------------------------------------------------------------------------------------

def test_the_join_route_cases_reach_no_limit_of_the_rank_map():
    """why the rank cases exist: the maps the join-route cases build take the one- and the two-launch form, but none lies within a chunk
    of a limit, none has a guarded tail behind whole chunks, and none takes three launches"""
    reached = SC.route_case_granules()
    assert set(reached.values()) == {"one", "two"}
    for g in reached:
        assert abs(g - SC.SCAN_ONE_LAUNCH_MAX) > SC.C and g < SC.SCAN_TWO_LAUNCH_CHUNKS * SC.RP_CHUNK // 2
        assert not (g > SC.SCAN_ONE_LAUNCH_MAX and g % SC.RP_CHUNK in (0, 2))


@pytest.mark.parametrize("case", SC.rank_cases(), ids=SC.RANK_IDS)
def test_each_rank_case_lies_where_its_name_says(case):
    b = case.bkeys.astype(np.int64)
    assert len(np.unique(b)) == len(b) > RC.TINY_BUILD_ROWS
    key_range = int(b.max() - b.min())
    assert SC.granules(key_range) == case.n_gran and SC.rank_form(case.n_gran) == case.form == dict((s[0], s[2]) for s in SC.RANK_SIZES)[case.name]
    assert RC.window_ok(key_range, len(b)) and key_range >= RC.TINY_BUILD_WINDOW
    assert bool(np.all(b[1:] > b[:-1])) == (case.order == "sorted")
    g = case.n_gran
    want = {"one_launch_max": g == SC.SCAN_ONE_LAUNCH_MAX, "one_launch_max_plus_2": g == SC.SCAN_ONE_LAUNCH_MAX + 2,
            "three_chunks": g % SC.RP_CHUNK == 0 and g % 4 == 0, "three_chunks_plus_2": g % SC.RP_CHUNK == 2 and g % 4 == 2,
            "two_launch_chunks_plus_2": -(-g // SC.RP_CHUNK) == SC.SCAN_TWO_LAUNCH_CHUNKS + 1 and g % 4 == 2}
    assert want[case.name]
    # a key in the first and in the last granule of every chunk, and in both granules of the last word
    gran = np.unique((b - b.min()) >> 5)
    chunk = SC.C if g <= SC.SCAN_ONE_LAUNCH_MAX else SC.RP_CHUNK
    starts = np.arange(0, g, chunk)
    assert np.isin(starts, gran).all() and np.isin(np.minimum(starts + chunk, g) - 1, gran).all() and np.isin([g - 2, g - 1], gran).all()
    # every build key is probed, and absent keys beside them
    assert np.isin(case.bkeys, case.pkeys).all() and (~np.isin(case.pkeys, case.bkeys)).sum() > 8


@pytest.mark.parametrize("case", [c for c in SC.rank_cases() if c.form != "three"], ids=[i for i, c in zip(SC.RANK_IDS, SC.rank_cases()) if c.form != "three"])
def test_rank_pairs_are_the_plain_dict_join_and_the_oracles(case):
    left, right = SC.id_side("l", case.bkeys), SC.id_side("r", case.pkeys)
    li, ri = SC.dict_join(case.bkeys, case.pkeys)
    wl, wr = RC.reference_pairs(left, right)
    assert np.array_equal(li, wl) and np.array_equal(ri, wr)
    assert len(li) == len(case.bkeys)                                   # unique keys, each probed once
    o = og.hash_join(left, right, RC.ON, "Inner")
    assert np.array_equal(SC.pair_codes(o["li"].values, o["ri"].values, len(case.bkeys)), SC.pair_codes(li, ri, len(case.bkeys)))


def test_rank_pairs_of_the_three_launch_case():
    """264 K build rows: every build key has exactly its own row as partner, the absent keys have none"""
    for case in SC.rank_cases():
        if case.form == "three":
            li, ri = SC.dict_join(case.bkeys, case.pkeys)
            assert np.array_equal(case.bkeys[li], case.pkeys[ri]) and len(li) == len(case.bkeys) == len(np.unique(li))
            assert not np.isin(case.pkeys[np.setdiff1d(np.arange(len(case.pkeys)), ri)], case.bkeys).any()
