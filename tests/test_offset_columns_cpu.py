"""The arena that test_offset_columns_gpu.py borrows its columns from (offset_columns.py), checked where no device is needed: every
buffer at the residue asked for and in its Arrow size, poison everywhere else, margins of at least 256 bytes, and the input batch
back out of it."""
import itertools
from collections import OrderedDict

import numpy as np
import pytest

from oracle.engine import OCol

import helpers
import offset_columns as oc


def mixed_batch(n, seed=1):
    rng = np.random.default_rng(seed)
    words = ["", "a", "BUILDING", "MACHINERY", "x" * 17, "é日本"]
    return OrderedDict([
        ("i64", OCol("Int64", rng.integers(-2 ** 62, 2 ** 62, n), rng.random(n) > 0.3)),
        ("f64", OCol("Float64", rng.normal(0, 1, n))),
        ("i32", OCol("Int32", rng.integers(-2 ** 31, 2 ** 31, n))),
        ("f32", OCol("Float32", rng.normal(0, 1, n).astype(np.float32), rng.random(n) > 0.5)),
        ("i16", OCol("Int16", rng.integers(-2 ** 15, 2 ** 15, n))),
        ("u8", OCol("UInt8", rng.integers(0, 256, n))),
        ("b", OCol("Boolean", rng.random(n) > 0.5, rng.random(n) > 0.2)),
        ("s", OCol("Utf8", [words[j] for j in rng.integers(0, len(words), n)], rng.random(n) > 0.2)),
    ])


SCHEMA = [("i64", "Int64"), ("f64", "Float64"), ("i32", "Int32"), ("f32", "Float32"), ("i16", "Int16"), ("u8", "UInt8"), ("b", "Boolean"),
          ("s", "Utf8")]
SHIFT_SETS = [
    {},
    {"i64": 8, "f64": 8, "i32": 4, "f32": 12, "i16": 2, "u8": 1, "b": 8, "s": 1, ("s", "offsets"): 4, "validity": 8},
    {"i64": 0, "f64": 8, "i32": 8, "f32": 4, "i16": 14, "u8": 15, "b": 0, "s": 15, ("s", "offsets"): 12, "validity": 0, ("b", "validity"): 8},
]
SIZES = [1, 3, 63, 64, 65, 257]


def expected_sizes(batch, n):
    words = (n + 63) // 64 * 8
    out = {}
    for name, c in batch.items():
        if c.dtype == "Utf8":
            out[name, "data"] = sum(len(s.encode()) for s in c.values)
            out[name, "offsets"] = (n + 1) * 4
        elif c.dtype == "Boolean":
            out[name, "data"] = words
        else:
            out[name, "data"] = n * c.values.dtype.itemsize
        if c.valid is not None:
            out[name, "validity"] = words
    return out


@pytest.mark.parametrize("tail_bits", [0, 1])
@pytest.mark.parametrize("base", [0, 5])
@pytest.mark.parametrize("shifts", range(len(SHIFT_SETS)))
@pytest.mark.parametrize("n", SIZES)
def test_residues_sizes_margins_and_poison(n, shifts, base, tail_bits):
    shifts = SHIFT_SETS[shifts]
    batch = mixed_batch(n)
    for poison in (0x00, 0xFF):
        arr, layout = oc.arena(batch, shifts, poison, tail_bits, base)
        assert arr.dtype == np.uint8
        got = {(name, role): size for name, where in layout.items() for role, (_, size) in where.items()}
        assert got == expected_sizes(batch, n)
        for name, where in layout.items():
            for role, (off, _) in where.items():
                assert (base + off) % 16 == oc.shift_of(shifts, name, role), (name, role)
        mask = oc.buffer_mask(arr, layout)
        assert np.all(arr[~mask] == poison)
        assert mask.sum() == sum(got.values()), "buffers overlap"
        spans = sorted((off, off + size) for where in layout.values() for off, size in where.values())
        edges = [0] + [x for span in spans for x in span] + [len(arr)]
        gaps = [edges[i + 1] - edges[i] for i in range(0, len(edges), 2)]
        assert len(gaps) == len(spans) + 1 and min(gaps) >= oc.MARGIN >= 256
        helpers.assert_bit_exact(oc.decode(arr, layout, SCHEMA, n), batch)


@pytest.mark.parametrize("n", SIZES)
def test_both_poisons_hold_the_same_buffers(n):
    batch = mixed_batch(n)
    a, la = oc.arena(batch, SHIFT_SETS[1], 0x00)
    b, lb = oc.arena(batch, SHIFT_SETS[1], 0xFF)
    assert la == lb and len(a) == len(b)
    mask = oc.buffer_mask(a, la)
    assert np.array_equal(a[mask], b[mask]) and np.all(a[~mask] == 0x00) and np.all(b[~mask] == 0xFF)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_tail_bits_fill_the_last_bitmap_word_and_nothing_else(n):
    rng = np.random.default_rng(n)
    batch = OrderedDict([("b", OCol("Boolean", rng.random(n) > 0.5, np.arange(n) % 3 != 1 if n > 1 else [False]))])
    zero, layout = oc.arena(batch, {}, 0x00, tail_bits=0)
    ones, layout1 = oc.arena(batch, {}, 0x00, tail_bits=1)
    assert layout == layout1
    for role in ("data", "validity"):
        off, size = layout["b"][role]
        z = np.unpackbits(zero[off:off + size], bitorder="little")
        o = np.unpackbits(ones[off:off + size], bitorder="little")
        assert size == (n + 63) // 64 * 8 and np.array_equal(z[:n], o[:n])
        assert not z[n:].any() and o[n:].all()
    mask = oc.buffer_mask(zero, layout)
    assert np.array_equal(zero[~mask], ones[~mask])


def test_shift_lookup_order():
    shifts = {("s", "offsets"): 4, "s": 1, "validity": 8, "offsets": 12}
    assert [oc.shift_of(shifts, "s", r) for r in oc.ROLES] == [1, 4, 8]
    assert [oc.shift_of(shifts, "t", r) for r in oc.ROLES] == [0, 12, 8]


def test_the_shift_tables_cover_every_placement_a_width_allows_the_kernels_to_tell_apart():
    assert all(s % 8 == 0 for s in oc.SHIFTS_8 + oc.SHIFTS_BITMAP) and all(s % 4 == 0 for s in oc.SHIFTS_4)
    assert all(s % 2 == 0 for s in oc.SHIFTS_2) and set(oc.SHIFTS_4) == {0, 4, 8, 12}
    assert {s % 2 for s in oc.SHIFTS_1} == {0, 1} and max(oc.SHIFTS_1) == 15 and max(oc.SHIFTS_2) == 14


def test_partition_slices_start_off_alignment():
    """the seed the GPU tier uses: partition 1 of the scattered columns starts at an odd row, partition 2 off 16 bytes for 4-byte
    values (and for 8-byte ones), with more rows than the plain sort of small batches takes"""
    from oracle import engine as og
    from ballista_amd.expr import col
    table = oc.slice_table(oc.slice_seed())
    first = oc.slice_first(table)
    assert len(first) == oc.SLICE_PARTS + 1 and first[0] == 0 and first[-1] == oc.SLICE_ROWS
    assert first[1] % 2 == 1 and first[2] * 4 % 16 != 0
    assert first[1] * 8 % 16 == 8 and first[2] * 8 % 16 == 8 and first[3] - first[2] > 1024
    parts = og.repartition_hash(table, [col("k")], oc.SLICE_PARTS)              # the oracle's own hash gives the same counts
    assert [og.batch_len(p) for p in parts] == list(np.diff(first))
    assert all(c.valid is None and c.dtype not in ("Utf8", "Boolean") for c in table.values())
