"""The Python restatement of the code-point string functions and date_part, and the case lists of
tests/test_string_fns_cpu.py and tests/test_string_fns_gpu.py.

Nothing here reads the library.  The string functions work on Python `str`, whose index IS the code-point index; date_part is
datetime.date on a day count brought into datetime's years 1 .. 9999 by whole 400-year cycles (146 097 days, a multiple of 7: the
weekday, the day of the year, the month and the day do not change, the year moves by 400 per cycle)."""
import datetime

import numpy as np

I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1
WAVE_BYTES = 1024                      # STR_CONCAT_WAVE_BYTES (str_kernels.h)
NEGATIVE = "negative substring length not allowed"


class NegativeLength(ValueError):
    pass


# ---- the string functions ------------------------------------------------------------------------------------------------------

def substr(s, start, count=None):
    """the code points at positions [start, start + count) intersected with [1, len], positions 1-based"""
    if count is not None and count < 0:
        raise NegativeLength(NEGATIVE)
    lo = max(start, 1)
    hi = len(s) + 1 if count is None else min(start + count, len(s) + 1)          # (Python integers: no overflow to restate)
    return s[lo - 1:hi - 1] if hi > lo else ""


def left(s, n):
    return s[:n] if n >= 0 else s[:max(len(s) + n, 0)]


def right(s, n):
    if n >= 0:
        return s[len(s) - n:] if n < len(s) else s
    return s[-n:]


def char_length(s):
    return len(s)


def strpos(s, sub):
    return s.find(sub) + 1              # str.find: the code-point index, -1 when absent, 0 for an empty sub


def starts_with(s, prefix):
    return s.startswith(prefix)


STRING_FUNCTIONS = {"substr": substr, "left": left, "right": right, "char_length": char_length, "strpos": strpos, "starts_with": starts_with}

_BIG = "naïve€𝄞x"
PINNED_STRINGS = [
    ("substr", ("alphabet", 0, 3), "al"),
    ("substr", ("alphabet", 3), "phabet"),
    ("substr", (_BIG, 3, 4), "ïve€"),
    ("substr", ("alphabet", I64_MAX, I64_MAX), ""),
    ("substr", ("alphabet", I64_MIN, I64_MAX), ""),
    ("substr", ("alphabet", -2, I64_MAX), "alphabet"),
    ("substr", ("alphabet", 2, 0), ""),
    ("substr", ("", 1, 5), ""),
    ("left", ("abcde", -2), "abc"),
    ("right", ("abcde", -2), "cde"),
    ("left", ("ab", 5), "ab"),
    ("right", ("ab", 5), "ab"),
    ("left", ("ab", -5), ""),
    ("right", ("ab", I64_MIN), ""),
    ("left", (_BIG, 6), "naïve€"),
    ("right", (_BIG, 3), "€𝄞x"),
    ("char_length", ("€𝄞",), 2),
    ("char_length", ("",), 0),
    ("strpos", ("€𝄞x", "x"), 3),
    ("strpos", ("abc", ""), 1),
    ("strpos", ("", ""), 1),
    ("strpos", ("abc", "d"), 0),
    ("strpos", ("abc", "abcd"), 0),
    ("strpos", ("aab", "ab"), 2),
    ("starts_with", ("abc", ""), True),
    ("starts_with", ("abc", "ab"), True),
    ("starts_with", ("ab", "abc"), False),
    ("starts_with", ("€x", "€"), True),
]

ALPHABET = ["a", "b", "-", "1", "é", "ï", "ß", "€", "ஐ", "𝄞", "😀"]           # 1-, 2-, 3- and 4-byte code points


def random_string(rng, max_len=40):
    return "".join(ALPHABET[k] for k in rng.integers(0, len(ALPHABET), int(rng.integers(0, max_len + 1))))


def random_int(rng, n):
    """from {int64 min, -3 .. n + 3, int64 max}"""
    k = int(rng.integers(-4, n + 5))
    return I64_MIN if k == -4 else I64_MAX if k == n + 4 else k


def random_string_calls(count, seed):
    """(function, arguments) over strings of 0 .. 40 code points of mixed widths; a substr count may be negative"""
    rng = np.random.default_rng(seed)
    calls = []
    for i in range(count):
        s = random_string(rng)
        fn = ("substr", "substr3", "left", "right", "char_length", "strpos", "starts_with")[i % 7]
        if fn == "substr":
            calls.append(("substr", (s, random_int(rng, len(s)))))
        elif fn == "substr3":
            calls.append(("substr", (s, random_int(rng, len(s)), random_int(rng, len(s)))))
        elif fn in ("left", "right"):
            calls.append((fn, (s, random_int(rng, len(s)))))
        elif fn == "char_length":
            calls.append((fn, (s,)))
        else:
            if len(s) and rng.random() < 0.7:            # a piece of s (a prefix half the time), else an unrelated string
                a = 0 if rng.random() < 0.5 else int(rng.integers(0, len(s)))
                sub = s[a:a + int(rng.integers(0, 4))]
            else:
                sub = random_string(rng, 3)
            calls.append((fn, (s, sub)))
    return calls


def evaluate(fn, args):
    """the answer; the string NEGATIVE for a substr with a negative count"""
    try:
        return STRING_FUNCTIONS[fn](*args)
    except NegativeLength:
        return NEGATIVE


# ---- date_part -----------------------------------------------------------------------------------------------------------------

PARTS = ("year", "quarter", "month", "day", "dow", "doy", "hour", "minute", "second")
# type name -> (short name of the check program, units per day)
TEMPORAL = {"Date32": ("d32", 1), "Date64": ("d64", 86400 * 10**3), "Timestamp(Second)": ("s", 86400),
            "Timestamp(Millisecond)": ("ms", 86400 * 10**3), "Timestamp(Microsecond)": ("us", 86400 * 10**6),
            "Timestamp(Nanosecond)": ("ns", 86400 * 10**9)}
_EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()
_CYCLE_DAYS = 146097


def date_part(part, v, dtype):
    """one value in Python integers; None where the field does not fit Int32"""
    upd = TEMPORAL[dtype][1]
    days, rem = divmod(int(v), upd)                     # floors: an instant before 1970 belongs to the day before
    sod = rem * 86400 // upd                            # second of the day (0 for a Date32)
    if part == "hour":
        return sod // 3600
    if part == "minute":
        return sod // 60 % 60
    if part == "second":
        return sod % 60
    ordinal = days + _EPOCH_ORDINAL
    cycles = (ordinal - 400) // _CYCLE_DAYS             # into years 1 .. 9999, well inside
    d = datetime.date.fromordinal(ordinal - cycles * _CYCLE_DAYS)
    if part == "year":
        y = d.year + 400 * cycles
        return y if I32_MIN <= y <= I32_MAX else None
    if part == "quarter":
        return (d.month - 1) // 3 + 1
    if part == "month":
        return d.month
    if part == "day":
        return d.day
    if part == "dow":
        return d.isoweekday() % 7                       # 0 = Sunday
    return d.timetuple().tm_yday


def days_of(y, m, d):
    return datetime.date(y, m, d).toordinal() - _EPOCH_ORDINAL


PINNED_PARTS = [
    ("year", -1, "Date32", 1969),
    ("dow", 0, "Date32", 4),
    ("doy", days_of(2000, 12, 31), "Date32", 366),
    ("doy", days_of(1999, 12, 31), "Date32", 365),
    ("quarter", days_of(1999, 4, 1), "Date32", 2),
    ("quarter", days_of(1999, 3, 31), "Date32", 1),
    ("hour", 12345, "Date32", 0),
    ("second", -1, "Timestamp(Nanosecond)", 59),
    ("minute", -1, "Timestamp(Nanosecond)", 59),
    ("hour", -1, "Timestamp(Nanosecond)", 23),
    ("day", -1, "Timestamp(Nanosecond)", 31),
    ("month", -1, "Timestamp(Nanosecond)", 12),
    ("year", -1, "Timestamp(Nanosecond)", 1969),
    ("year", I64_MIN, "Timestamp(Second)", None),
    ("year", I64_MAX, "Timestamp(Second)", None),
    ("year", I64_MIN, "Timestamp(Nanosecond)", 1677),
    ("year", I64_MAX, "Timestamp(Nanosecond)", 2262),
    ("dow", days_of(2024, 2, 25) * 86400 * 10**3, "Date64", 0),
    ("second", 61500, "Timestamp(Millisecond)", 1),
    ("year", days_of(1, 1, 1) - 1, "Date32", 0),
    ("year", days_of(1, 1, 1) - 366 - 1, "Date32", -1),
]


def edge_values(dtype):
    """the days around each month end of a leap (2000, 2024) and a non-leap year (1900, 2023), +-1 unit around 0 and around
    each of those midnights, and the extremes of the storage type"""
    upd = TEMPORAL[dtype][1]
    out = [-1, 0, 1, -upd - 1, -upd, -upd + 1, upd - 1, upd, upd + 1]
    for y in (1900, 2000, 2023, 2024):
        for m in range(1, 13):
            first = days_of(y, m, 1)
            for day in (first - 2, first - 1, first, first + 1):
                out += [day * upd, day * upd - 1, day * upd + upd - 1] if upd > 1 else [day]
    lo, hi = (I32_MIN, I32_MAX) if dtype == "Date32" else (I64_MIN, I64_MAX)
    return out + [lo, lo + 1, hi - 1, hi]


def random_temporal(dtype, n, seed):
    """n values: most within a few centuries of 1970, some over the whole storage type"""
    rng = np.random.default_rng(seed)
    upd = TEMPORAL[dtype][1]
    lo, hi = (I32_MIN, I32_MAX) if dtype == "Date32" else (I64_MIN, I64_MAX)
    near = rng.integers(-100000, 100000, n) * upd + (rng.integers(0, upd, n) if upd > 1 else 0)       # (int64 nanoseconds end in 2262)
    wide = rng.integers(lo, hi, n, dtype=np.int64, endpoint=True)
    v = np.where(rng.random(n) < 0.8, near, wide)
    return np.clip(v, lo, hi).astype(np.int64)
