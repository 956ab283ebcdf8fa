"""The value grammar of the text scans is one function (text_convert, ballista_amd/csrc/text_device.h) behind three walks:
tbl_parse_kernel, csv_parse_kernel<false> (a text without a quote) and csv_parse_kernel<true>.  Every case of
tests/text_value_cases.py goes through all three, which must agree with Python's int / float / datetime.date (floats bit for
bit) and so with each other.

Accepted values sit in row 0, in a row of the second tile and in the last row of 600 rows: two full tiles of 256 and a tail whose
last wave has no record.  The same rows with a ~300-byte filler field do not fit the LDS stage, so those tiles are walked in HBM."""
import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd import _lib

import text_value_cases as T

pytestmark = pytest.mark.gpu

N_ROWS = 600
AT = (0, 300, N_ROWS - 1)
FILLER = "f" * 300


def texts(values, dtype, filler):
    """the same rows as `.tbl`, as quote-free CSV and as CSV with the string fields quoted -> {reader name: (text, schema)}"""
    schema = [("id", E.INT32), ("v", dtype)] + ([("pad", E.UTF8)] if filler else []) + [("s", E.UTF8)]
    rows = [[str(i), v] + ([FILLER] if filler else []) + [f"s{i}"] for i, v in enumerate(values)]
    quote = lambda r: r[:2] + ['"' + c + '"' for c in r[2:]]
    return {"tbl": ("".join("|".join(r) + "|\n" for r in rows).encode(), schema),
            "csv": ("".join(",".join(r) + "\n" for r in rows).encode(), schema),
            "csv quoted": ("".join(",".join(quote(r)) + "\n" for r in rows).encode(), schema)}


def scan(ctx, reader, text, schema):
    if reader == "tbl":
        return ba.RecordBatch.from_tbl(ctx, text, schema)
    assert (b'"' in text) == (reader == "csv quoted")
    return ba.RecordBatch.from_csv(ctx, text, schema, has_header=False)


@pytest.mark.parametrize("filler", [False, True], ids=["lds", "hbm"])
@pytest.mark.parametrize("dtype,s", T.accepted_cases())
def test_accepted_value_reads_the_same_in_every_reader(ctx, dtype, s, filler):
    values = [T.PLAIN[dtype]] * N_ROWS
    for i in AT:
        values[i] = s
    want = [T.expected(dtype, v) for v in values]
    for reader, (text, schema) in texts(values, dtype, filler).items():
        rb = scan(ctx, reader, text, schema)
        assert rb.num_rows == N_ROWS, reader
        _, ids, valid = rb.column(0)
        assert valid is None and [int(x) for x in ids] == list(range(N_ROWS)), reader
        _, got, valid = rb.column(1)
        assert valid is None, reader
        if dtype == E.FLOAT64:
            got, exp = np.asarray(got, np.float64).view(np.uint64), np.asarray(want, np.float64).view(np.uint64)
            assert np.array_equal(got, exp), (reader, [hex(int(got[i])) for i in AT])       # bit for bit: -0.0 is not 0.0
        else:
            assert [int(x) for x in got] == want, (reader, [int(got[i]) for i in AT])
        _, strings, _ = rb.column(rb.num_columns - 1)
        assert list(strings) == [f"s{i}" for i in range(N_ROWS)], reader
        if filler:
            assert set(rb.column(2)[1]) == {FILLER}, reader


@pytest.mark.parametrize("dtype,s,error", T.refused_cases())
def test_refused_value_is_the_same_error_in_every_reader(ctx, dtype, s, error):
    values = [T.PLAIN[dtype], s, T.PLAIN[dtype]]
    for reader, (text, schema) in texts(values, dtype, False).items():
        with pytest.raises(getattr(_lib, error)):
            scan(ctx, reader, text, schema)
