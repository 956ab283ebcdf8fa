"""The inputs of test_repartition_edges_gpu.py (tests/repartition_cases.py) are what their names say, and the two CPU statements of
the partition id — oracle/engine.py::row_hash, which the GPU tests compare the device with, and the numpy restatement of
repartition_cases.py, with which the skew cases were searched — agree row for row on every one of them.  The hash itself is pinned
to published vectors: splitmix64's first output and the FNV-1a-64 test vectors."""
import numpy as np
import pytest

from ballista_amd.expr import col
from oracle import engine as og
from oracle.engine import OCol

import repartition_cases as K

SKEW = {c.name: c for c in K.SKEW_CASES}
KEYS = {c.name: c for c in K.KEY_CASES}


# ---- the hash against published vectors ----------------------------------------------------------------------------------------------

def test_published_vectors():
    assert og.mix64(0) == 0xE220A8397B1DCDAF == int(K.mix64(0))                    # splitmix64 seeded with 0: the first output
    s = OCol("Utf8", ["", "a", "foobar", "stored"], [True, True, True, False])
    want = [0xCBF29CE484222325, 0xAF63DC4C8601EC8C, 0x85944171F73967E8, 0x6E756C6C6E756C6C]
    assert [og._value_bits(s, i) for i in range(4)] == want
    assert [int(b) for b in K.value_bits(s)] == want
    assert [K.fnv1a(b"") , K.fnv1a(b"a"), K.fnv1a(b"foobar")] == want[:3]
    assert K.NULL_BITS == int.from_bytes(b"nullnull", "big") == want[3]
    # a row hash is the fold of mix64 over the columns from 0
    assert int(og.row_hash([s], 4)[2]) == og.mix64(0x85944171F73967E8)
    assert int(og.row_hash([s, s], 4)[0]) == og.mix64(og.mix64(0xCBF29CE484222325) ^ 0xCBF29CE484222325)


def test_value_bits_extend_and_fold():
    """what the cross-type promises rest on: sign and zero extension, a Float32 as its double, -0.0 as +0.0, NaN payloads kept"""
    for dtype, v, bits in [("Int8", -1, 2 ** 64 - 1), ("Int16", -2 ** 15, 2 ** 64 - 2 ** 15), ("Int32", K.I32_MIN, 2 ** 64 - 2 ** 31),
                           ("Date32", -1, 2 ** 64 - 1), ("UInt32", 2 ** 32 - 1, 2 ** 32 - 1), ("UInt64", 2 ** 64 - 1, 2 ** 64 - 1),
                           ("UInt8", 255, 255), ("Boolean", True, 1), ("Timestamp(Second)", -5, 2 ** 64 - 5)]:
        c = OCol(dtype, [v])
        assert int(K.value_bits(c)[0]) == bits == og._value_bits(c, 0), dtype
    for dtype in ("Float32", "Float64"):
        c = OCol(dtype, [-0.0, 0.0, 1.5, np.nan])
        assert [int(b) for b in K.value_bits(c)] == [0, 0, 0x3FF8000000000000, 0x7FF8000000000000] == [og._value_bits(c, i) for i in range(4)]


# ---- the two statements agree on every case ------------------------------------------------------------------------------------------------

ALL = K.all_cases()


def test_the_case_list_covers_what_it_must():
    pairs = set(K.SCATTER_PAIRS)
    assert {p for p, _ in pairs} == set(K.SCATTER_NPARTS) and {n for _, n in pairs} == set(K.SCATTER_SIZES)
    assert all((p, n) in pairs for p in (3, 256) for n in K.SCATTER_SIZES)
    assert max(K.SCATTER_SIZES) <= 3 * 4096 + 1
    pairs = set(K.SORT_PAIRS)
    assert {p for p, _ in pairs} == set(K.SORT_NPARTS) and {n for _, n in pairs} == set(K.SORT_SIZES)
    assert all((p, n) in pairs for p in (3, 257) for n in K.SORT_SIZES)
    assert {w for _, t in K.PAYLOADS for w in [np.dtype(og.NP_TYPES[t]).itemsize]} == {1, 2, 4, 8}
    assert [len(c.batch) for c in K.SWITCH_CASES] == [32, 33, 32, 33]
    for c, _ in ALL:
        assert "rn" in c.batch and c.batch["rn"].dtype == "Int64" and np.array_equal(c.batch["rn"].values, np.arange(c.n)), c.name


def test_restatement_equals_the_oracle_on_every_case():
    seen = set()
    for c, p in ALL:
        if (id(c.batch), p, tuple(id(e) for e in c.exprs)) in seen:
            continue
        seen.add((id(c.batch), p, tuple(id(e) for e in c.exprs)))
        want = og.repartition_hash(c.batch, c.exprs, p)
        pid = K.restated_pid(c.batch, c.exprs, p)
        assert len(want) == p
        for q in range(p):
            assert np.array_equal(want[q]["rn"].values, np.nonzero(pid == q)[0]), (c.name, p, q)
        if c.n:
            cols = [og.evaluate(e, c.batch) for e in c.exprs]
            assert np.array_equal(og.row_hash(cols, c.n), K.restated_hash(cols)), c.name


def test_restatement_equals_the_oracle_on_the_other_tables():
    for dtype in ("Int32", "Int64", "UInt64"):
        for name, t in K.route_agreement_tables(dtype).items():
            pid = K.restated_pid(t, K.K, K.AGREE_NPARTS)
            for q, w in enumerate(og.repartition_hash(t, K.K, K.AGREE_NPARTS)):
                assert np.array_equal(w["rn"].values, np.nonzero(pid == q)[0]), (dtype, name, q)
    for part in K.repartition_stream():
        for kind, b in part:
            pid = K.restated_pid(b, K.K, K.REPART_NPARTS)
            for q, w in enumerate(og.repartition_hash(b, K.K, K.REPART_NPARTS)):
                assert np.array_equal(w["rn"].values, b["rn"].values[pid == q]), (kind, q)
    for key in ("k", "d"):
        for r in range(K.SHUFFLE_WORLD):
            b = K.shuffle_batch(r, key)
            pid = K.restated_pid(b, [col(key)], K.SHUFFLE_WORLD)
            for q, w in enumerate(og.repartition_hash(b, [col(key)], K.SHUFFLE_WORLD)):
                assert np.array_equal(w["rn"].values, np.nonzero(pid == q)[0]), (key, r, q)


# ---- every case is what its name says ---------------------------------------------------------------------------------------------------

def counts(c, p=None):
    p = c.n_parts[0] if p is None else p
    return np.bincount(K.restated_pid(c.batch, c.exprs, p), minlength=p)


def test_scatter_keys_hold_the_extremes_dense_and_high_bit_values():
    for dtype in K.KEY_TYPES:
        for n in (4097, 8193):
            v = K.scatter_table(dtype, n)["k"].values
            assert set(K.EXTREMES[dtype]) <= set(v.tolist()), dtype
            dense = v[1::4]
            assert dense.min() == 0 and dense.max() == 36
            high = v[2::4].astype(np.uint64) if dtype == "UInt64" else v[2::4].astype(np.int64).view(np.uint64)
            low_bits = 32 if dtype in ("Int64", "UInt64") else 16
            assert len(set(high.tolist())) == len(high) and set((high & np.uint64((1 << low_bits) - 1)).tolist()) == {7}
            # every partition of 256 is live at the large sizes, and no payload column is constant
            assert counts(K.scatter_case(dtype, 256, n)).min() > 0
    t = K.scatter_table("Int64", 257)
    for name, dtype in K.PAYLOADS:
        raw = np.ascontiguousarray(t[name].values).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[t[name].values.itemsize])
        assert len(set(raw.tolist())) > (200 if raw.itemsize > 1 else 100), name
    for name in ("p_f32", "p_f64"):
        v = K.scatter_table("Int64", 8193)[name].values
        assert np.isnan(v).any() and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()


def test_skew_cases_are_what_their_names_say():
    for name in ("one_partition", "one_partition_of_256"):
        c = SKEW[name]
        assert (counts(c) > 0).sum() == 1 and counts(c).max() == c.n == K.SKEW_ROWS
        assert len(set(c.batch["k"].values.tolist())) == c.n                 # by the hash, not by equal keys
    assert np.nonzero(counts(SKEW["one_partition"]))[0].tolist() == [4] and np.nonzero(counts(SKEW["one_partition_of_256"]))[0].tolist() == [255]
    c = SKEW["all_equal"]
    assert len(set(c.batch["k"].values.tolist())) == 1 and (counts(c) > 0).sum() == 1 and c.n > 4096
    c = SKEW["two_alternating"]
    k = c.batch["k"].values
    assert len(set(k.tolist())) == 2 and np.all(k[:-1] != k[1:]) and np.nonzero(counts(c))[0].tolist() == [0, 2]
    for name, empty in K.EMPTY_PARTITIONS.items():
        c = SKEW[name]
        assert np.nonzero(counts(c) == 0)[0].tolist() == empty, name
    assert 0 not in K.EMPTY_PARTITIONS["interior_empty"] and SKEW["interior_empty"].n_parts[0] - 1 not in K.EMPTY_PARTITIONS["interior_empty"]
    c = SKEW["all_256_live"]
    assert c.n_parts == [256] and counts(c).min() == 3
    assert SKEW["single_row"].n == 1 and SKEW["single_row_one_partition"].n == 1
    c = SKEW["more_partitions_than_rows"]
    assert c.n < c.n_parts[0] and counts(c)[0] > 0 and counts(c)[255] > 0
    c = KEYS["more_partitions_than_rows_sorted"]
    assert c.n == 300 < c.n_parts[0] == 1000 and c.route == "sort"
    for c in K.SKEW_CASES:
        assert c.route == "scatter" and c.n <= 3 * 4096 + 1


def test_signed_zeros_share_a_partition_and_a_plain_bit_hash_would_split_them():
    for name in ("key_float64", "key_float32"):
        c = KEYS[name]
        v = c.batch["k"].values
        assert v[0] == 0 and v[1] == 0 and np.signbit(v[0]) and not np.signbit(v[1]) and c.batch["k"].is_valid()[:2].all()
        pid = K.restated_pid(c.batch, c.exprs, c.n_parts[0])
        assert pid[0] == pid[1]
        # hashing -0.0 by its own bits would send it elsewhere: the case can tell
        assert K.pid_of_ints(np.array([1 << 63], np.uint64), c.n_parts[0])[0] != pid[1]
        assert np.isnan(v).any() and np.isinf(v).any() and not c.batch["k"].is_valid().all()


def test_empty_string_and_null_do_not_share_a_hash():
    c = KEYS["key_utf8"]
    s = c.batch["k"]
    assert s.values[0] == "" and s.is_valid()[0] and not s.is_valid()[1] and s.values[1] != ""
    h = K.restated_hash([s])
    assert h[0] != h[1] and h[0] == K.mix64(K.FNV_BASIS) and h[1] == K.mix64(K.NULL_BITS)
    for p in c.n_parts:
        pid = K.restated_pid(c.batch, c.exprs, p)
        assert pid[0] != pid[1], p                                              # and they part ways at the counts in use
    lens = [len(x.encode()) for x in s.values]
    assert max(lens) >= 300 and any(len(x.encode()) > len(x) for x in s.values)
    # the 300-byte values differ only in their last byte, and go to different partitions of 7
    a, b = K.STRINGS.index(K.LONG + "x"), K.STRINGS.index(K.LONG + "y")
    assert K.fnv1a(K.STRINGS[a].encode()) != K.fnv1a(K.STRINGS[b].encode())


def test_key_cases_are_what_their_names_say():
    t = K.two_key_table(K.KEY_ROWS)
    va, vs = t["a"].is_valid(), t["s"].is_valid()
    assert (va & ~vs).any() and (~va & vs).any() and (~va & ~vs).any() and (va & vs).any()
    ab, ba = KEYS["keys_int64_utf8"], KEYS["keys_utf8_int64"]
    assert ab.batch is ba.batch
    for p in ab.n_parts:
        assert (K.restated_pid(ab.batch, ab.exprs, p) != K.restated_pid(ba.batch, ba.exprs, p)).any()      # the key order counts
    # a row NULL in both keys is not a row NULL in one of them
    h = K.restated_hash([t["a"], t["s"]])
    assert len({int(h[1]), int(h[2]), int(h[0])}) == 3
    b = KEYS["key_boolean"].batch["k"]
    assert set(b.to_pylist()) == {True, False, None}
    assert not KEYS["key_all_null"].batch["k"].is_valid().any() and (counts(KEYS["key_all_null"]) > 0).sum() == 1
    c = KEYS["key_all_equal"]
    assert c.n > 1024 and len(set(c.batch["k"].values.tolist())) == 1 and (counts(c, 257) > 0).sum() == 1
    c = KEYS["key_sum_of_columns"]
    s = og.evaluate(c.exprs[0], c.batch)
    assert s.dtype == "Int32" and s.values[0] == K.I32_MIN and s.values[1] == K.I32_MAX                         # wrapped
    c = KEYS["key_cast_narrowing"]
    s = og.evaluate(c.exprs[0], c.batch)
    assert s.dtype == "Int32" and s.is_valid()[:4].tolist() == [True, False, True, False] and 0.2 < s.is_valid().mean() < 0.8
    assert og.evaluate(KEYS["key_cast_to_float"].exprs[0], KEYS["key_cast_to_float"].batch).dtype == "Float64"
    for c in K.KEY_CASES:
        assert c.route == "sort" and (c.n > 1024 or c.name.startswith("more_partitions"))
    # from 257 partitions the ids of a spread key differ in two bytes
    pid = K.restated_pid(K.two_key_table(4097), [col("a"), col("s")], 257)
    assert pid.max() >= 256 and (np.bitwise_or.reduce(pid ^ pid[0]) & 0xFF) != 0


def test_type_groups_hold_the_values_that_tell_extensions_apart():
    v, types = K.TYPE_GROUPS["signed_widths"]
    assert v.min() == -128 and v.max() == 127 and types == ["Int8", "Int16", "Int32", "Int64"]
    v, _ = K.TYPE_GROUPS["unsigned_as_int64"]
    assert v.min() == 0 and v.max() == 2 ** 32 - 1 and (v >= 2 ** 31).sum() > 100       # a sign-extended UInt32 would move these
    v, _ = K.TYPE_GROUPS["date_as_int32"]
    assert v.min() == K.I32_MIN and (v < 0).sum() > 100
    v, _ = K.TYPE_GROUPS["float_widths"]
    assert v.dtype == np.float32 and np.isnan(v).any() and np.isinf(v).any() and np.signbit(v[v == 0]).any()
    for group, (v, types) in K.TYPE_GROUPS.items():
        pids = [K.restated_pid(K.type_table(group, t), K.K, K.AGREE_NPARTS) for t in types]
        assert all(np.array_equal(pids[0], p) for p in pids[1:]), group
        assert len(np.unique(pids[0])) == K.AGREE_NPARTS


def test_route_agreement_tables_share_their_keys():
    for dtype in ("Int32", "Int64", "UInt64"):
        t = K.route_agreement_tables(dtype)
        k = t["lone"]["k"].values
        assert set(K.EXTREMES[dtype]) <= set(k.tolist())
        assert np.array_equal(t["utf8"]["k"].values, k) and np.array_equal(t["bitmap"]["k"].values[:-1], k)
        v = t["bitmap"]["k"].is_valid()
        assert v[:-1].all() and not v[-1] and t["lone"]["k"].valid is None


def test_repartition_stream_and_shuffle_inputs():
    kinds = [[k for k, _ in part] for part in K.repartition_stream()]
    assert len(kinds) == 2 and all({"empty", "fixed", "nulls"} <= set(ks) for ks in kinds)
    assert any(a == "fixed" and b == "nulls" for ks in kinds for a, b in zip(ks, ks[1:]))
    for part in K.repartition_stream():
        for kind, b in part:
            assert (og.batch_len(b) == 0) == (kind == "empty") and (b["k"].valid is not None) == (kind == "nulls")
    for key in ("k", "d"):
        b = K.shuffle_batch(0, key)
        assert set(K.restated_pid(b, [col(key)], K.SHUFFLE_WORLD).tolist()) == {1}
        for r in range(K.SHUFFLE_WORLD):
            b = K.shuffle_batch(r, key)
            assert b["k"].values.min() >= 2 ** 63 and b["d"].values.max() < 0 and og.batch_len(b) == K.SHUFFLE_SIZES[r]
            if r:
                assert len(set(K.restated_pid(b, [col(key)], K.SHUFFLE_WORLD).tolist())) == K.SHUFFLE_WORLD
