"""CAST between Utf8 and the fixed-width types: a Python restatement of the table in DESIGN.md §3.2, and the case lists both test
tiers draw from (tests/test_cast_text_cpu.py, tests/test_cast_utf8_gpu.py).

The oracle's `_cast` has no Utf8 casts, and arrow-rs 4.0 is not available to pin against, so the expectations are restated here
from the table itself, with the standard library doing the arithmetic: `int()` behind a regex and a range test, `float()` for the
strings the exactness rule accepts (CPython's float() is correctly rounded), `np.float32(float(s))`, `datetime.date`."""
import datetime
import re
import struct

import numpy as np

DECLINED = "DECLINED"          # a float string outside the exact path: the batch fails with BHIP_ENOTIMPL (neither a value nor NULL)

INT_RANGE = {"Int8": (-2**7, 2**7 - 1), "Int16": (-2**15, 2**15 - 1), "Int32": (-2**31, 2**31 - 1), "Int64": (-2**63, 2**63 - 1),
             "UInt8": (0, 2**8 - 1), "UInt16": (0, 2**16 - 1), "UInt32": (0, 2**32 - 1), "UInt64": (0, 2**64 - 1)}
INT_TYPES = list(INT_RANGE)
PARSE_TYPES = INT_TYPES + ["Boolean", "Date32", "Float64", "Float32"]
FORMAT_TYPES = INT_TYPES + ["Boolean", "Date32"]

_SIGNED = re.compile(r"[+-]?[0-9]+")
_UNSIGNED = re.compile(r"[+]?[0-9]+")
_DATE = re.compile(r"([0-9]{4})-([0-9]{2})-([0-9]{2})")
_FLOAT = re.compile(r"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")
_TRUE, _FALSE = {"true", "t", "yes", "y", "on", "1"}, {"false", "f", "no", "n", "off", "0"}
_ASCII_LOWER = {c: c + 32 for c in range(ord("A"), ord("Z") + 1)}

EPOCH = datetime.date(1970, 1, 1)
DATE_MIN, DATE_MAX = -719528, 2932896          # 0000-01-01, 9999-12-31
_CYCLE = 146097                                # days in 400 years: datetime.date has no year 0, the calendar repeats


def days_of(y, m, d):
    """days since 1970-01-01 of a proleptic Gregorian date, year 0 included; None when there is no such day"""
    try:
        if y == 0:
            return (datetime.date(400, m, d) - EPOCH).days - _CYCLE
        return (datetime.date(y, m, d) - EPOCH).days
    except ValueError:
        return None


def date_text(days):
    if not DATE_MIN <= days <= DATE_MAX:
        return None
    if days < (datetime.date(1, 1, 1) - EPOCH).days:
        d = EPOCH + datetime.timedelta(days=days + _CYCLE)
        return f"{d.year - 400:04d}-{d.month:02d}-{d.day:02d}"
    d = EPOCH + datetime.timedelta(days=days)
    return f"{d.year:04d}-{d.month:02d}-{d.day:02d}"


def _float64(s):
    low = s.translate(_ASCII_LOWER)
    body = low[1:] if low[:1] in ("+", "-") else low
    if body in ("inf", "infinity", "nan"):
        return float(low)
    m = _FLOAT.fullmatch(s)
    if not m:
        return None
    sign, ip, fp, fp2, ex = m.groups()
    frac = fp2 if ip is None else (fp or "")
    digits = ((ip or "") + frac).lstrip("0")
    stripped = digits.rstrip("0")
    z = len(digits) - len(stripped)
    mant = int(stripped) if stripped else 0
    if mant == 0:
        return -0.0 if sign == "-" else 0.0
    e10 = int(ex or "0") + z - len(frac)
    if mant < 2**53 and -22 <= e10 <= 22:
        return float(s)
    return DECLINED


def _float32(s):
    d = _float64(s)
    if d is None or d is DECLINED:
        return d
    f = np.float32(d)
    if d == d and float(f) != d:
        # d is not a float: declined when it is exactly the midpoint of the two floats around it
        g = np.nextafter(f, np.float32(np.inf if d > float(f) else -np.inf), dtype=np.float32)
        if (float(f) + float(g)) / 2 == d:
            return DECLINED
    return f


def parse(s, to):
    """CAST(s AS to): the value, None for NULL, DECLINED"""
    if s is None:
        return None
    if to in INT_RANGE:
        if not (_UNSIGNED if to.startswith("U") else _SIGNED).fullmatch(s):
            return None
        v = int(s)
        lo, hi = INT_RANGE[to]
        return v if lo <= v <= hi else None
    if to == "Boolean":
        w = s.translate(_ASCII_LOWER)
        return True if w in _TRUE else False if w in _FALSE else None
    if to == "Date32":
        m = _DATE.fullmatch(s)
        return days_of(int(m.group(1)), int(m.group(2)), int(m.group(3))) if m and 1 <= int(m.group(2)) <= 12 and int(m.group(3)) >= 1 else None
    if to == "Float64":
        return _float64(s)
    if to == "Float32":
        return _float32(s)
    raise ValueError(to)


def format_value(v, frm):
    """CAST(v AS Utf8): the text, None for NULL"""
    if v is None:
        return None
    if frm in INT_RANGE:
        return str(int(v))
    if frm == "Boolean":
        return "1" if v else "0"
    if frm == "Date32":
        return date_text(int(v))
    raise ValueError(frm)


def bits(v, dtype):
    """the comparison key of a value: floats by bit pattern"""
    if v is None or v is DECLINED:
        return v
    if dtype == "Float64":
        return struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    if dtype == "Float32":
        return struct.unpack("<I", struct.pack("<f", np.float32(v)))[0]
    if dtype == "Boolean":
        return bool(v)
    if dtype == "Utf8":
        return str(v)
    return int(v)


# ---- the case list ------------------------------------------------------------------------------------------------------------

def integer_strings(t):
    lo, hi = INT_RANGE[t]
    fits = str(min(hi, 123))
    return [str(lo), str(hi), str(lo - 1), str(hi + 1), "+7", "-0", "007", "0" * 40 + fits, "", " 1", "1 ", "1.0", "-1", "٣", "12" * 150,
            "0", "+", "-", "+-1", "1e3", "0x10", "１", "-" + "0" * 25 + "1"]


BOOLEAN_STRINGS = ["true", "TRUE", "tRuE", "t", "T", "yes", "YeS", "y", "Y", "on", "oN", "1", "false", "FALSE", "fAlSe", "f", "F", "no", "No",
                   "n", "N", "off", "OfF", "0", "2", "tr", "", " true", "true ", "truee", "01", "yess", "ｏｎ"]
DATE_STRINGS = ["2000-02-29", "1900-02-29", "0000-01-01", "9999-12-31", "2001-13-01", "2001-1-01", "2001-01-1", "2001-01-0", "2001-01-011",
                "2001-00-10", "2001-04-31", "2001-04-30", "1970-01-01", "1969-12-31", "0000-02-29", "0100-02-29", "2400-02-29", "2001/01/01",
                "2001-01-32", "20010101", "", "+001-01-01", "2001-01-01 ", "1994-01-01", "1998-09-02", "٢٠٠١-01-01"]
DATE_DAYS = [DATE_MIN, DATE_MAX, DATE_MIN - 1, DATE_MAX + 1, 0, -1, 10471, -719163, -719162, 11016, 2**31 - 1, -2**31, 59, 60, 789, -25567]

FLOAT_ACCEPTED = ["0", "-0.0", ".5", "5.", "1e22", "1e-22", "9007199254740991", "1000000000000000000000", "1.50000000000000000000", "0e999999999999",
                  "inF", "-Infinity", "NaN", "+nan", "-nan", "+inf", "3.14159", "-2.5e-3", "1E5", "+.25e+1", "000123.4500", "0.000", "-0e-999999999999",
                  "123456789012345e7", "0.0000000000000000000001", "9007199254740991e22", "16777216", "0.1", "100e-24"]
FLOAT_DECLINED = ["1e23", "1e-23", "9007199254740993", "0.1234567890123456789", "1e400", "9007199254740992", "1e-400", "123456789012345678e5",
                  "1" + "0" * 23, "0." + "0" * 22 + "1"]
FLOAT_NULL = [".", "e5", "1e", "1e+", "--1", "1.2.3", "0x10", "", " 1", "1 ", "+", "-", "+.", "1e5.0", "in", "infinit", "nane", "1,5", "١.٥", "1_0", "-.e1", "infinityy"]
FLOAT32_DECLINED = ["16777217", "1.00000005960464477539", "33554434", "16777219"]
FLOAT32_ACCEPTED = ["16777218", "1.0000001", "16777216", "0.1", "3.4e22", "1e-22", "33554432", "33554436"]


def parse_cases():
    """(type, string) pairs: the whole CPU-tier list"""
    out = []
    for t in INT_TYPES:
        out += [(t, s) for s in integer_strings(t)]
    out += [("Boolean", s) for s in BOOLEAN_STRINGS]
    out += [("Date32", s) for s in DATE_STRINGS]
    for t in ("Float64", "Float32"):
        out += [(t, s) for s in FLOAT_ACCEPTED + FLOAT_DECLINED + FLOAT_NULL + FLOAT32_DECLINED + FLOAT32_ACCEPTED]
    return out


def format_cases():
    """(type, value) pairs"""
    out = []
    for t in INT_TYPES:
        lo, hi = INT_RANGE[t]
        out += [(t, v) for v in sorted({lo, hi, 0, 1, min(hi, 9), min(hi, 10), min(hi, 99), min(hi, 100), max(lo, -1), max(lo, -10), hi // 3, lo // 7})]
    out += [("Boolean", 0), ("Boolean", 1)]
    out += [("Date32", d) for d in DATE_DAYS]
    return out


def random_float_strings(n, seed=7):
    """repr() of random doubles and %.*f / %.*e renderings with 1-17 digits.  Short renderings of values of moderate magnitude
    dominate, so that most strings are on the exact path (the test asserts the share)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = i % 8
        x = float(rng.standard_normal() * 10.0 ** int(rng.integers(-6, 9)))
        if kind == 0:
            out.append(repr(float(rng.random())))                                   # 16-17 digits: mostly declined
        elif kind == 1:
            out.append(repr(round(x, int(rng.integers(0, 6)))))                      # a short repr
        elif kind < 5:
            out.append("%.*f" % (int(rng.integers(1, 18)), float(rng.standard_normal() * 10.0 ** int(rng.integers(-2, 5)))))
        else:
            out.append("%.*e" % (int(rng.integers(1, 18)), x))
    return out


def random_strings(t, n, seed):
    """inputs for the GPU tier: the case list of the type, then random values around it"""
    rng = np.random.default_rng(seed)
    if t in INT_RANGE:
        base = integer_strings(t)
        lo, hi = INT_RANGE[t]
        rnd = [str(int(v)) for v in rng.integers(max(lo, -2**62), min(hi, 2**62), n, dtype=np.int64, endpoint=True)]
        rnd = [("+" + s if i % 7 == 0 and not s.startswith("-") else "00" + s if i % 11 == 0 and not s.startswith("-") else s) for i, s in enumerate(rnd)]
    elif t == "Boolean":
        base, rnd = BOOLEAN_STRINGS, [BOOLEAN_STRINGS[k] for k in rng.integers(0, len(BOOLEAN_STRINGS), n)]
    elif t == "Date32":
        base = DATE_STRINGS
        rnd = [date_text(int(d)) for d in rng.integers(DATE_MIN, DATE_MAX, n, endpoint=True)]
        rnd = [s[:9] if i % 13 == 0 else s for i, s in enumerate(rnd)]
    else:
        base = FLOAT_ACCEPTED + FLOAT_NULL + FLOAT32_ACCEPTED
        rnd = [s for s in random_float_strings(3 * n + 64, seed) if parse(s, "Float64") is not DECLINED and parse(s, "Float32") is not DECLINED]
    vals = (base + rnd)[:n] if n <= len(base) else base + rnd[:n - len(base)]
    return vals


def random_values(t, n, seed):
    rng = np.random.default_rng(seed)
    base = [v for tt, v in format_cases() if tt == t]
    if t in INT_RANGE:
        lo, hi = INT_RANGE[t]
        rnd = [int(v) for v in rng.integers(max(lo, -2**62), min(hi, 2**62), n, dtype=np.int64, endpoint=True)]
    elif t == "Boolean":
        rnd = [int(v) for v in rng.integers(0, 2, n)]
    else:
        rnd = [int(v) for v in rng.integers(DATE_MIN - 1000, DATE_MAX + 1000, n)]
    return (base + rnd)[:n]
