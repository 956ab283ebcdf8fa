"""The Python restatement of to_timestamp's grammar and date_trunc's arithmetic, and the case lists of
tests/test_temporal_fns_cpu.py and tests/test_scalar_fns_gpu.py.

Nothing here reads the library: the grammar is a regular expression plus datetime.date, the truncation is numpy's flooring
datetime64 `astype` (week: (days + 3) floor 7, 1970-01-01 being a Thursday), with a scalar version in Python integers beside it
for the values numpy cannot floor (the int64 minimum is its NaT, and its floor wraps just above it)."""
import datetime
import re

import numpy as np

I64_MIN, I64_MAX = -2**63, 2**63 - 1
UNITS = {"Timestamp(Second)": ("s", 1), "Timestamp(Millisecond)": ("ms", 10**3), "Timestamp(Microsecond)": ("us", 10**6),
         "Timestamp(Nanosecond)": ("ns", 10**9)}
GRANULARITIES = ("second", "minute", "hour", "day", "week", "month", "year")
_NUMPY_CODE = {"second": "s", "minute": "m", "hour": "h", "day": "D", "month": "M", "year": "Y"}
_EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()

_TEXT = re.compile(r"(\d{4})-(\d{2})-(\d{2})[T ](\d{2}):(\d{2}):(\d{2})(?:\.(\d{1,9}))?(?:[Zz]|([+-])(\d{2}):(\d{2}))?", re.ASCII)


def to_timestamp(text):
    """nanoseconds since 1970-01-01T00:00:00Z, None for a text outside the grammar or the range of int64 nanoseconds"""
    m = _TEXT.fullmatch(text)
    if not m:
        return None
    y, mo, d, hh, mi, ss = (int(x) for x in m.group(1, 2, 3, 4, 5, 6))
    try:
        days = datetime.date(y, mo, d).toordinal() - _EPOCH_ORDINAL       # (year 0000 raises too: it is far outside int64 nanoseconds)
    except ValueError:
        return None
    if hh > 23 or mi > 59 or ss > 59:
        return None
    frac = int(m.group(7).ljust(9, "0")) if m.group(7) else 0
    offset = 0
    if m.group(8):
        oh, om = int(m.group(9)), int(m.group(10))
        if oh > 23 or om > 59:
            return None
        offset = (oh * 3600 + om * 60) * (-1 if m.group(8) == "-" else 1)
    ns = (days * 86400 + hh * 3600 + mi * 60 + ss - offset) * 10**9 + frac
    return ns if I64_MIN <= ns <= I64_MAX else None


def date_trunc_one(g, v, unit):
    """one value in Python integers; None where the floor does not fit int64"""
    ups = UNITS[unit][1]
    if g in ("second", "minute", "hour", "day"):
        period = ups * {"second": 1, "minute": 60, "hour": 3600, "day": 86400}[g]
        r = v // period * period
    else:
        days = v // (ups * 86400)
        if g == "week":
            days = (days + 3) // 7 * 7 - 3
        else:
            d = datetime.date.fromordinal(days + _EPOCH_ORDINAL)
            days = (d.replace(day=1) if g == "month" else d.replace(month=1, day=1)).toordinal() - _EPOCH_ORDINAL
        r = days * ups * 86400
    return r if r >= I64_MIN else None


def date_trunc(g, values, unit):
    """a list: the floor of every value by numpy's datetime64 conversion, None where it does not fit int64"""
    code, ups = UNITS[unit]
    v = np.asarray(values, np.int64)
    t = v.view(f"datetime64[{code}]")
    if g == "week":
        days = t.astype("datetime64[D]").astype(np.int64)
        scaled = [int(x) * 86400 * ups for x in (days + 3) // 7 * 7 - 3]
    elif g in ("month", "year"):
        scaled = [int(x) * 86400 * ups for x in t.astype(f"datetime64[{_NUMPY_CODE[g]}]").astype("datetime64[D]").astype(np.int64)]
    else:
        scaled = [int(x) * ups for x in t.astype(f"datetime64[{_NUMPY_CODE[g]}]").astype("datetime64[s]").astype(np.int64)]
    out = [r if r >= I64_MIN else None for r in scaled]
    # numpy floors a negative value as (v - (period - 1)) / period, which wraps within one period of the int64 minimum, and the
    # minimum itself is its NaT: the values of the lowest 10^17 (three years of nanoseconds) take the scalar road
    for i in np.nonzero(v < I64_MIN + 10**17)[0]:
        out[i] = date_trunc_one(g, int(v[i]), unit)
    return out


# ---- the pinned literals of the contract ------------------------------------------------------------------------------------------
PINNED_TEXTS = [("1997-01-31T09:26:56.123", 854702816123000000), ("1997-01-31 09:26:56.123-05:00", 854720816123000000),
                ("2021-03-01T00:15:00+05:30", 1614537900000000000), ("1969-12-31T23:59:59.5Z", -500000000),
                ("2020-02-29T23:59:59.999999999z", 1583020799999999999), ("1677-09-21T00:12:43.145224192", I64_MIN),
                ("2262-04-11T23:47:16.854775807", I64_MAX)]

INVALID_TEXTS = [
    "1677-09-21T00:12:43.145224191", "2262-04-11T23:47:16.854775808",            # the two range ends moved outward by 1 ns
    "2021-02-29T00:00:00", "2021-13-01T00:00:00", "2021-03-01T24:00:00", "2021-03-01T00:60:00", "2021-03-01T00:00:60",
    "2021-03-01T00:00:00.1234567890", "2021-03-01T00:00:00.",                    # a 10-digit fraction, '.' and no digit
    "2021-03-01T00:00:00+24:00", "2021-03-01T00:00:00+00:60", "2021-03-01T00:00:00+0530", "2021-03-01T00:00:00+05:30Z",
    "2021-03-01", "12021-03-01T00:00:00",                                        # a date alone, a 5-digit year
    " 2021-03-01T00:00:00", "2021-03-01T00:00:00 ", "",                          # blanks around the value, the empty string
    "٢٠٢١-٠٣-٠١T٠٠:٠٠:٠٠", "2021-03-01T00:00:0٣",                                 # non-ASCII digits
    # more of the grammar's edges
    "2021-03-01t00:00:00", "2021-03-01T00:00:00.Z", "2021-03-01T00:00:00Zz", "2021-03-01T00:00:00+5:30", "2021-03-01T00:00:00-05:3",
    "2021-3-01T00:00:00", "2021-03-01T0:00:00", "2021-03-01T00:00", "2021/03/01T00:00:00", "2021-03-00T00:00:00", "2021-00-10T00:00:00",
    "1900-02-29T00:00:00", "2021-04-31T00:00:00", "2021-03-01T00:00:00.5 Z", "-021-03-01T00:00:00", "2021-03-01T00:00:00+05:30:00",
    "1677-09-20T23:59:59Z", "2262-04-12T00:00:00", "0000-01-01T00:00:00", "9999-12-31T23:59:59",
]

NS = "Timestamp(Nanosecond)"
TRUNC_OF_MINUS_HALF_SECOND = {"second": -1000000000, "minute": -60000000000, "hour": -3600000000000, "day": -86400000000000,
                              "week": -259200000000000, "month": -2678400000000000, "year": -31536000000000000}
# (granularity, nanoseconds in, nanoseconds out)
PINNED_TRUNC = [(g, -500000000, r) for g, r in TRUNC_OF_MINUS_HALF_SECOND.items()] + [
    ("week", 3 * 86400 * 10**9, -3 * 86400 * 10**9),                                    # 1970-01-04 -> 1969-12-29
    ("week", 4 * 86400 * 10**9 + 5, 4 * 86400 * 10**9),                                 # 1970-01-05 -> itself
    ("week", 1609632000000000000 + 86399 * 10**9, 1609113600000000000),                 # 2021-01-03 -> 2020-12-28
    ("week", 1709164800000000000 + 12345, 1708905600000000000),                         # 2024-02-29 -> 2024-02-26
    ("month", 1709164800000000000 + 12345, 1706745600000000000),                        # 2024-02-29 -> 2024-02-01
    ("year", I64_MIN, None), ("month", I64_MIN, None), ("week", I64_MIN, None), ("day", I64_MIN, None), ("second", I64_MIN, None),
    ("second", I64_MIN + 1, None), ("week", I64_MIN + 86400 * 10**9, None), ("day", I64_MIN + 86400 * 10**9, -9223286400000000000),
    ("second", I64_MAX, I64_MAX // 10**9 * 10**9), ("year", I64_MAX, 9214646400000000000),
]


def pinned_every_unit():
    """all seven granularities on each of the four units: the instants of PINNED_TRUNC that are whole in the unit, and -1"""
    out = []
    for unit, (_, ups) in UNITS.items():
        for v_ns in (-500000000, 1709164800000000000, 1609632000000000000, -1, 0, 951782400 * 10**9):
            v = v_ns // (10**9 // ups)
            out += [(unit, g, v) for g in GRANULARITIES]
    return out


def _civil_text(secs, frac, width, sep, offset, suffix):
    local = secs + offset
    days, rem = divmod(local, 86400)
    d = datetime.date.fromordinal(days + _EPOCH_ORDINAL)
    text = "%04d-%02d-%02d%s%02d:%02d:%02d" % (d.year, d.month, d.day, sep, rem // 3600, rem // 60 % 60, rem % 60)
    if width:
        text += "." + ("%09d" % frac)[:width]
    return text + suffix


def random_texts(n, seed):
    """[(text, nanoseconds)]: random instants of the whole int64 range written with a random fraction width (0 = none .. 9), either
    separator and no offset, Z, z or a random +-hh:mm"""
    rng = np.random.default_rng(seed)
    out = []
    for ns in rng.integers(I64_MIN + 10**9, I64_MAX, n, dtype=np.int64, endpoint=True):
        ns = int(ns)
        width = int(rng.integers(0, 10))
        ns -= ns % 10**(9 - width)
        kind = int(rng.integers(0, 5))
        offset, suffix = 0, ("", "Z", "z")[kind] if kind < 3 else ""
        if kind >= 3:
            oh, om = int(rng.integers(0, 24)), int(rng.integers(0, 60))
            sign = 1 if kind == 3 else -1
            offset, suffix = sign * (oh * 3600 + om * 60), "%s%02d:%02d" % ("+" if sign > 0 else "-", oh, om)
        secs, frac = divmod(ns, 10**9)
        out.append((_civil_text(secs, frac, width, "T" if rng.random() < 0.5 else " ", offset, suffix), ns))
    return out


_YEAR_1, _YEAR_10000 = -62135596800, 253402300800            # seconds of 0001-01-01 and of 10000-01-01


def random_values(unit, n, seed):
    """seconds, milliseconds and microseconds from years 0001-9999, nanoseconds from the whole int64 range"""
    rng = np.random.default_rng(seed)
    ups = UNITS[unit][1]
    if unit == NS:
        return rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    return rng.integers(_YEAR_1 * ups, _YEAR_10000 * ups, n, dtype=np.int64)
