"""Inputs shared by the sort-order tests (test_sort_order_cpu.py pins the oracle's order, test_sort_edges_gpu.py the device's on
every route): the floating-point values at which a sort key's order-preserving image can go wrong, as bit patterns."""
import numpy as np

from oracle.engine import OCol

# sign-bit-set patterns in the order an ascending sort must give them (falling magnitude); the positive mirror of each follows
F64_NEGATIVE = [
    0xFFFFFFFFFFFFFFFF,        # -NaN, every payload bit
    0xFFF8000000000001,        # -NaN, quiet, payload 1
    0xFFF8000000000000,        # -NaN, quiet
    0xFFF0000000000001,        # -NaN, signalling
    0xFFF0000000000000,        # -inf
    0xFFEFFFFFFFFFFFFF,        # -DBL_MAX
    0xBFF0000000000000,        # -1.0
    0x8010000000000000,        # -DBL_MIN
    0x800FFFFFFFFFFFFF,        # the largest negative subnormal
    0x8000000000000001,        # -5e-324
    0x8000000000000000,        # -0.0
]
F32_NEGATIVE = [0xFFFFFFFF, 0xFFC00001, 0xFFC00000, 0xFF800001, 0xFF800000, 0xFF7FFFFF, 0xBF800000, 0x80800000, 0x807FFFFF,
                0x80000001, 0x80000000]


# which patterns a batch too small for all of them takes first (indices into special_bits): the zeros, a NaN of either sign with a
# payload, the infinities, the outermost NaNs, the smallest subnormals, then the rest
SMALL_FIRST = [10, 11, 1, 20, 4, 17, 0, 21, 9, 12, 3, 18, 2, 19, 8, 13, 5, 16, 7, 14, 6, 15]


def special_bits(dtype):
    """all 22 patterns of `dtype` in ascending total order, as a uint64 / uint32 array"""
    neg, sign, ut = (F64_NEGATIVE, 1 << 63, np.uint64) if dtype == "Float64" else (F32_NEGATIVE, 1 << 31, np.uint32)
    return np.array(neg + [b ^ sign for b in reversed(neg)], dtype=ut)


def float_special_column(dtype, n, rng, null_share=0.05):
    """n rows of `dtype`: every special pattern twice (n < 176: the first n // 8 patterns of SMALL_FIRST, twice each, so that the
    specials stay within a quarter of the batch), the rest +-2^U(-300, 300) (Float32: +-2^U(-100, 100)) — spread
    over the octaves, so that a split on sign and exponent leaves a handful of rows per bin — permuted, null_share of the rows
    (at least two) NULL.  The values under the NULL rows are whatever the permutation left there: a sort that looks at them shows."""
    ft, span = (np.float64, 300) if dtype == "Float64" else (np.float32, 100)
    bits = special_bits(dtype)
    if 2 * len(bits) > n // 4:
        bits = np.sort(bits[SMALL_FIRST[:max(2, n // 8)]])
    special = np.concatenate([bits, bits]).view(ft)
    k = n - len(special)
    filler = (rng.choice([-1.0, 1.0], k) * np.exp2(rng.uniform(-span, span, k))).astype(ft)
    values = np.concatenate([special, filler])[rng.permutation(n)]
    valid = np.ones(n, bool)
    if null_share:
        valid[rng.choice(n, max(2, round(n * null_share)), replace=False)] = False
    return OCol(dtype, values, valid)
