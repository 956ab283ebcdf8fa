"""The cases of tests/batch_plumbing_cases.py are what they claim to be (no GPU): the concat part lists reach every bitmap-word
alignment the issue names, so a later edit of the lists cannot quietly lose an edge; the special values, patterns and Utf8 forms are
present; and the restated CoalesceBatchesExec rule gives the pinned sizes."""
import numpy as np
import pytest

from oracle import engine as og

import batch_plumbing_cases as K
import helpers

CASES = K.concat_cases()


def all_offsets():
    return [(off, n) for c in CASES for off, n in K.dest_offsets(c.lengths())]


def test_destination_offsets_cover_the_word_edges():
    assert set(K.EDGES) <= {off for off, _ in all_offsets()}


def test_part_lengths_cover_the_word_edges():
    assert set(K.EDGES) <= {n % 64 for _, n in all_offsets()}


def test_a_part_lies_strictly_inside_one_word():
    inside = [(off, n) for off, n in all_offsets() if off > 0 and off + n < 64]
    assert inside, "no part with both ends partial inside one destination word"
    # and with a validity buffer on both neighbours' and its own side: at least one of them in a nullable case
    assert any(off > 0 and off + n < 64 and c.parts[0].has_buffer("c0")
               for c in CASES for off, n in K.dest_offsets(c.lengths()))


def test_every_offset_edge_meets_a_long_and_a_short_part():
    """an offset edge only counts if something is copied there that crosses a word (n >= 64) and something that does not"""
    for e in K.EDGES:
        ns = [n for off, n in all_offsets() if off == e]
        assert any(n >= 64 - e and n > 1 for n in ns) and any(n < 64 for n in ns), (e, ns)


def test_every_listed_length_is_used():
    used = {p.rows for c in CASES for p in c.parts if p.head is None}
    assert set(K.LENGTHS) <= used, sorted(set(K.LENGTHS) - used)
    assert max(sum(c.lengths()) for c in CASES) < 4000 and max(len(c.parts) for c in CASES) == 200


def test_named_cases_are_present():
    by = {c.name: c for c in CASES}
    assert len(by) == len(CASES)
    assert by["200_parts_of_one_row"].lengths() == [1] * 200
    z = by["zero_rows_first_last_middle_adjacent"].lengths()
    assert z[0] == 0 and z[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(z[1:-1], z[2:-1])) and any(z)
    assert not any(by["every_part_zero_rows"].lengths()) and len(by["every_part_zero_rows"].parts) > 1
    assert len(by["single_part"].parts) == 1
    for where, pos in [("first", 0), ("last", -1), ("middle", 1)]:
        c = by["no_buffer_" + where]
        flags = [p.has_buffer("c3") for p in c.parts]
        assert not flags[pos] and sum(flags) == len(flags) - 1, (where, flags)
    for cut in K.HEAD_CUTS:
        c = by["head_%d" % cut]
        assert [p.n for p in c.parts if p.head is not None] == [cut] * 3 and all(p.rows > cut for p in c.parts if p.head is not None)
        # the bytes past the cut exist, so leaving them in would show
        assert all(sum(len(s.encode()) for s in p.cols["c17"][1][cut:]) > 0 for p in c.parts if p.head is not None)


def test_patterns_and_special_values_are_there():
    rng = np.random.default_rng(0)
    assert K.bits("edge_zero", 5, rng).tolist() == [False, True, True, True, False]
    assert K.bits("edge_one", 5, rng).tolist() == [True, False, False, False, True]
    assert K.bits("edge_one", 1, rng).tolist() == [True] and K.bits("edge_zero", 0, rng).tolist() == []
    assert K.bits("alternating", 4, rng).tolist() == [True, False, True, False]
    p = K.make_part(129, seed=1)
    widths = {np.dtype(og.NP_TYPES[t]).itemsize for t in K.FIXED}
    assert widths == {1, 2, 4, 8} and len(p.cols) == len(K.FIXED) + 3
    for t in ("Float32", "Float64"):
        v = p.cols[K.NAMES[K.TYPES.index(t)]][1]
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (np.signbit(v) & (v == 0)).any()
    assert int(p.cols[K.NAMES[K.TYPES.index("UInt64")]][1].max()) > 2 ** 63
    # the patterns of validity and of the Boolean values differ inside one part
    used = set()
    for c in CASES:
        if c.name.startswith("pattern_"):
            part = c.parts[-2]
            used.add((tuple(part.cols["c0"][2]), tuple(part.cols["c16"][1])))
            assert not np.array_equal(part.cols["c0"][2], part.cols["c16"][1]) or part.rows < 2
    assert len(used) == len(K.PATTERNS)
    e = K.make_part(40, seed=2, utf8="empty")
    assert set(e.cols["c18"][1]) == {""} and set(e.cols["c17"][1]) != {""}
    a = K.make_part(40, seed=2, utf8="all_null")
    assert not a.cols["c17"][2].any() and not a.cols["c18"][2].any()
    m = K.make_part(40, seed=2, utf8="multibyte")
    assert all(len(s.encode()) > len(s) for s in m.cols["c18"][1])


def test_expected_values_are_plain_concatenation():
    c = next(x for x in CASES if x.name == "head_63")
    want = c.expected()
    assert og.batch_len(want) == sum(c.lengths()) == 63 + 31 + 63 + 2 + 63
    first = c.parts[0]
    assert want["c17"].values[:63].tolist() == list(first.cols["c17"][1][:63])
    assert want["c17"].values[63] == c.parts[1].cols["c17"][1][0]
    assert c.expected_data_bytes("c17") == sum(len(s.encode()) for s in want["c17"].values)
    nb = next(x for x in CASES if x.name == "no_buffer_middle").expected()
    assert nb["c0"].is_valid()[31:101].all() and not nb["c0"].is_valid().all()


def test_slice_source_variants():
    for k in K.SLICE_KS:
        a, b = K.slice_source("A", k), K.slice_source("B", k)
        assert og.batch_len(a) == K.SLICE_ROWS
        for name in a:
            if name == "rn":
                continue
            assert a[name].is_valid()[k:].all() and not b[name].is_valid()[k:].any(), name
            assert np.array_equal(a[name].is_valid()[:k], b[name].is_valid()[:k])
        assert a["c16"].values[k:].all() and not b["c16"].values[k:].any()
        if k > 60:
            assert not a["key"].is_valid()[:k].all() and a["key"].is_valid()[:k].any()
            assert a["c16"].values[:k].any() and not a["c16"].values[:k].all()


@pytest.mark.parametrize("sizes, target, want", [
    ([40, 60, 30], 100, [100, 30]),                 # pending reaches the target exactly: flushed at once (>=, not >)
    ([40, 59, 1, 7], 100, [100, 7]),
    ([40, 59], 100, [99]),
    ([40, 61, 5], 100, [101, 5]),
    ([250, 100, 30], 100, [250, 100, 30]),          # large batches pass untouched when nothing is pending
    ([30, 250, 100, 99, 100], 100, [280, 100, 199]),   # ... and are buffered like any other when something is
    ([0, 50, 0, 0, 50, 0, 20, 0], 100, [100, 20]),
    ([1, 0, 3, 1], 1, [1, 3, 1]),
    ([30, 250, 1], 10 ** 6, [281]),
    ([0, 0], 100, []),
    ([], 100, []),
])
def test_coalesce_rule_restated(sizes, target, want):
    assert K.coalesce_sizes(sizes, target) == want


def test_coalesce_sequences_hit_what_they_name():
    S = K.COALESCE_SEQUENCES
    assert all(K.coalesce_sizes(p, t) is not None for t, parts in S.values() for p in parts)
    for name, (t, parts) in S.items():
        for p in parts:
            out = K.coalesce_sizes(p, t)
            assert sum(out) == sum(p) and 0 not in out
            assert all(n >= t for n in out[:-1]), (name, out)           # only the last batch of a partition may be short
    assert K.coalesce_sizes(S["pending_exactly_target"][1][0], K.T)[0] == K.T
    assert K.coalesce_sizes(S["pending_target_plus_one"][1][0], K.T)[0] == K.T + 1
    assert K.coalesce_sizes(S["pending_target_minus_one_at_the_end"][1][0], K.T) == [K.T - 1]
    assert len(S["two_partitions"][1]) == 2 and S["two_partitions"][1][0] != S["two_partitions"][1][1]


def test_limits_hit_the_batch_boundaries():
    edges = np.cumsum(K.LIMIT_BATCHES).tolist()
    assert {0, 1, edges[0], edges[0] + 1, edges[-1], edges[-1] + 1} <= set(K.LIMITS)
    assert any(0 < n < edges[0] for n in K.LIMITS) and max(K.LIMITS) > edges[-1] + 1


def test_split_by_sizes():
    bs = [K.stream_batch(n, s) for s, n in enumerate([5, 0, 7])]
    out = K.split_by_sizes(bs, [3, 9])
    assert [og.batch_len(b) for b in out] == [3, 9]
    helpers.assert_bit_exact(helpers.concat(out), helpers.concat(bs))
