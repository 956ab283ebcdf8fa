"""The oracle's sort (oracle/engine.py sort_batch) is what every GPU sort test compares with, so its order is pinned here against a
third, deliberately slow statement of the same order: Python's `sorted` over row numbers with a comparator on Python values.
Ints compare as ints, strings as bytes, floats by the sign, exponent and mantissa fields of their bit pattern (IEEE-754
totalOrder, DESIGN.md "Sort order of floating-point keys"); NULL placement and DESC per key; ties keep input order (`sorted` is
stable).  The comparator shares no formula with sort_batch's integer keys or with the device's key images."""
import functools
import struct
from collections import OrderedDict

import numpy as np
import pytest

from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle import engine as og
from oracle.engine import OCol

import sort_cases
from test_types_gpu import FIXED

TYPES = FIXED + ["Boolean", "Utf8"]
STRINGS = ["", "a", "a\0", "ab\0c", "ab", "abc", "b", "é", "ab\0"]
N_ROWS = [0, 1, 2, 300]
PLACEMENTS = [(False, False), (False, True), (True, False), (True, True)]          # (descending, nulls_first)


def S(name, desc, nulls_first):
    return E.PhysicalSortExpr(col(name), descending=desc, nulls_first=nulls_first)


def float_fields(raw):
    """(sign, exponent, mantissa) of a float's bytes (the bytes, not a Python float: a signalling Float32 NaN does not survive
    the widening to a double)"""
    if len(raw) == 8:
        b = struct.unpack("<Q", raw)[0]
        return b >> 63, (b >> 52) & 0x7FF, b & ((1 << 52) - 1)
    b = struct.unpack("<I", raw)[0]
    return b >> 31, (b >> 23) & 0xFF, b & ((1 << 23) - 1)


def python_values(c):
    """the column as Python values a comparator can order with `<`: int, bytes, or for floats (negative?, fields) handled below"""
    if c.dtype == "Utf8":
        return [s.encode() for s in c.values]
    if c.dtype in og.FLOAT_TYPES:
        return [float_fields(c.values[i].tobytes()) for i in range(len(c))]
    return [int(v) for v in c.values]


def compare_values(dtype, a, b):
    """ascending order of two valid values: -1, 0, 1"""
    if dtype in og.FLOAT_TYPES:
        (sa, ea, ma), (sb, eb, mb) = a, b
        if sa != sb:
            return -1 if sa else 1                                       # every sign-bit-set value before every other one
        c = (ea > eb) - (ea < eb) or (ma > mb) - (ma < mb)               # the magnitude: exponent, then mantissa
        return -c if sa else c
    return (a > b) - (a < b)


def slow_order(batch, keys):
    """row numbers in sorted order; keys: [(column name, descending, nulls_first)]"""
    cols = [(batch[name].dtype, python_values(batch[name]), list(batch[name].is_valid()), desc, nf) for name, desc, nf in keys]

    def cmp(i, j):
        for dtype, vals, valid, desc, nf in cols:
            if valid[i] and valid[j]:
                c = compare_values(dtype, vals[i], vals[j])
                c = -c if desc else c
            elif valid[i] == valid[j]:
                c = 0
            else:
                c = -1 if (not valid[i]) == nf else 1                    # the NULL row first iff nulls_first
            if c:
                return c
        return 0
    return sorted(range(og.batch_len(batch)), key=functools.cmp_to_key(cmp))


def check(batch, keys):
    got = og.sort_batch(batch, [S(*k) for k in keys])
    want = slow_order(batch, keys)
    assert list(got["row"].values) == want, keys
    return got


def pool_column(dtype, n, rng):
    """n values drawn from a dozen or two of the type's edge values, so that keys tie and later keys decide; 15 % NULL"""
    if dtype == "Utf8":
        pool = np.array(STRINGS, dtype=object)
    elif dtype == "Boolean":
        pool = np.array([False, True])
    elif dtype in og.FLOAT_TYPES:
        ft = og.NP_TYPES[dtype]
        pool = np.concatenate([sort_cases.special_bits(dtype).view(ft), np.array([2.5, -2.5, 1e-3, -7e20], ft)])
    else:
        info = np.iinfo(og.NP_TYPES[dtype])
        pool = np.array(sorted({info.min, info.min + 1, info.max, info.max - 1, 0, 1, max(info.min, -1), min(info.max, 1 << 40)}), og.NP_TYPES[dtype])
    return OCol(dtype, pool[rng.integers(0, len(pool), n)], rng.random(n) >= 0.15)


@pytest.fixture(scope="module")
def batches():
    out = {}
    for n in N_ROWS:
        rng = np.random.default_rng(1000 + n)
        b = OrderedDict((f"c{i}", pool_column(t, n, rng)) for i, t in enumerate(TYPES))
        b["row"] = OCol("Int64", np.arange(n))
        out[n] = b
    return out


@pytest.mark.parametrize("n", N_ROWS)
@pytest.mark.parametrize("n_keys", [1, 2, 3])
def test_sort_batch_against_python_sorted(batches, n_keys, n):
    """every type as the first key under all four (descending, nulls_first) placements; the second and third keys are other types
    under other placements"""
    b = batches[n]
    for i in range(len(TYPES)):
        for p, (desc, nf) in enumerate(PLACEMENTS):
            keys = [(f"c{(i + 7 * k) % len(TYPES)}", *PLACEMENTS[(p + k) % 4]) for k in range(n_keys)]
            assert keys[0][1:] == (desc, nf)
            got = check(b, keys)
            if n:                                                       # every column is gathered by the same order, bit for bit
                rows = got["row"].values
                for name, c in b.items():
                    assert np.array_equal(got[name].is_valid(), c.is_valid()[rows])
                    if c.dtype != "Utf8" and c.dtype != "Boolean":
                        ut = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[c.values.dtype.itemsize]
                        assert np.array_equal(got[name].values.view(ut), c.values[rows].view(ut))
                    else:
                        assert list(got[name].values) == list(c.values[rows])


@pytest.mark.parametrize("dtype", ["Float64", "Float32"])
def test_float_special_set(dtype):
    """the special set of the GPU tests (each pattern twice, octave-spread fillers, NULLs) under every placement, and the
    properties of the total order stated directly"""
    n = 300
    rng = np.random.default_rng(7)
    b = OrderedDict([("f", sort_cases.float_special_column(dtype, n, rng)), ("t", OCol("Int32", rng.integers(0, 4, n))),
                     ("row", OCol("Int64", np.arange(n)))])
    for desc, nf in PLACEMENTS:
        check(b, [("f", desc, nf)])
        check(b, [("f", desc, nf), ("t", True, True)])
    got = check(b, [("f", False, False)])
    n_valid = int(b["f"].is_valid().sum())
    assert n_valid < n and not got["f"].is_valid()[n_valid:].any() and got["f"].is_valid()[:n_valid].all()      # NULLS LAST
    wide = dtype == "Float64"
    bits = [int(x) for x in got["f"].values[:n_valid].view(np.uint64 if wide else np.uint32)]
    rows = [int(r) for r in got["row"].values[:n_valid]]
    sign, mag_mask = (1 << 63, (1 << 63) - 1) if wide else (1 << 31, (1 << 31) - 1)
    inf = 0x7FF0000000000000 if wide else 0x7F800000
    is_nan = [(x & mag_mask) > inf for x in bits]
    neg_nan = [x for x, nan in zip(bits, is_nan) if nan and x & sign]
    pos_nan = [x for x, nan in zip(bits, is_nan) if nan and not x & sign]
    assert len(set(neg_nan)) == 4 and len(set(pos_nan)) == 4             # (a NULL may have taken one copy of a pattern, never both here)
    # every sign-bit-set NaN first, by falling magnitude bits; every sign-bit-clear NaN last
    assert bits[:len(neg_nan)] == neg_nan and [x & mag_mask for x in neg_nan] == sorted((x & mag_mask for x in neg_nan), reverse=True)
    assert bits[-len(pos_nan):] == pos_nan and pos_nan == sorted(pos_nan)
    # -0.0 directly before +0.0
    n_neg0, n_pos0 = bits.count(sign), bits.count(0)
    assert n_neg0 >= 1 and n_pos0 >= 1
    z = bits.index(sign)
    assert bits[z:z + n_neg0 + n_pos0] == [sign] * n_neg0 + [0] * n_pos0
    # equal bit patterns keep input order
    ties = [k for k in range(1, n_valid) if bits[k] == bits[k - 1]]
    assert len(ties) >= 11 and all(rows[k] > rows[k - 1] for k in ties)
