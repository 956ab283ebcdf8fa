"""The value grammar of the text scans (text_convert in ballista_amd/csrc/text_device.h), as a case table: the strings a `.tbl` or
CSV field of a fixed-width column may hold, and the ones the scan refuses.  tests/test_text_values_gpu.py runs every case through
from_tbl and from_csv; tests/test_text_value_cases_cpu.py holds the table itself against Python.

The expectation is Python's: `int()`, `float()` (the correctly rounded conversion) and `datetime.date`.  The grammar is narrower
than Python's (no blanks, no exponent, no '_'), so a refused string is one that Python refuses too, or one outside the grammar below,
or, for "NotImplementedOnGpu", a decimal of the grammar that the one exact division cannot convert (M >= 2^53, more than 19
digits, more than 22 fraction digits)."""
import datetime
import re

EPOCH = datetime.date(1970, 1, 1)
INT_RANGE = {"Int32": (-2**31, 2**31 - 1), "Int64": (-2**63, 2**63 - 1)}
GRAMMAR = {"Int32": re.compile(r"[+-]?[0-9]+"), "Int64": re.compile(r"[+-]?[0-9]+"),
           "Float64": re.compile(r"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)"), "Date32": re.compile(r"[0-9]{4}-[0-9]{2}-[0-9]{2}")}

ACCEPTED = {
    "Int32": ["0", "-0", "+7", "007", "0000000000000000000001", "2147483647", "-2147483648"],
    "Int64": ["9223372036854775807", "-9223372036854775808"],
    "Float64": ["0", "-0", "-0.00", "+1.5", ".5", "5.", "123456.789012345", "9007199254740991", "0.0000000000000000001", "0.1", "0.07"],
    "Date32": ["1970-01-01", "0001-01-01", "9999-12-31", "2000-02-29", "1969-12-31"],
}
# the value every other row of a text holds
PLAIN = {"Int32": "42", "Int64": "42", "Float64": "2.25", "Date32": "1996-01-02"}

REFUSED = {
    "ExecutionError": {
        "Int32": ["2147483648", "-2147483649", "-", "+", "1.0", "1e3", "12a", " 1"],
        "Int64": ["9223372036854775808", "-9223372036854775809", "99999999999999999999"],
        "Float64": ["1e0", "1.2.3", "-", "abc"],
        "Date32": ["1996-13-02", "1996-00-10", "1996-01-00", "1996-01-32", "1996-1-02", "1996/01/02", "1996-01-0x"],
    },
    "NotImplementedOnGpu": {
        "Float64": ["9007199254740992", "0.12345678901234567890", "0.00000000000000000000001"],
    },
}


def expected(dtype, s):
    """the value of an accepted string: an int (Int32 / Int64, Date32 as days since 1970-01-01) or a float"""
    if dtype in INT_RANGE:
        v = int(s)
        lo, hi = INT_RANGE[dtype]
        if not lo <= v <= hi:
            raise ValueError(f"{s} is outside {dtype}")
        return v
    if dtype == "Float64":
        return float(s)
    return (datetime.date.fromisoformat(s) - EPOCH).days


def exactly_convertible(s):
    """a decimal of the grammar that M / 10^k converts: M < 2^53 read from at most 19 counted digits (leading zeros of the integer
    part are free), k <= 22"""
    body = s.lstrip("+-")
    ip, _, fp = body.partition(".")
    return len(ip.lstrip("0") + fp) <= 19 and len(fp) <= 22 and int((ip + fp) or "0") < 2**53


def accepted_cases():
    return [(dt, s) for dt, values in ACCEPTED.items() for s in values]


def refused_cases():
    return [(dt, s, error) for error, by_type in REFUSED.items() for dt, values in by_type.items() for s in values]
