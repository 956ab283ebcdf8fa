"""General CSV text -> device columns (ballista_amd/csrc/kernels_csv.hip, bhip_batch_from_csv): the scan leaf the reference
builds as CsvExec(schema, has_header, delimiter) for `--format csv` — rust/benchmarks/tpch/src/main.rs:129-150,
rust/core/src/serde/physical_plan/from_proto.rs:93-110.

Every parity case goes through RecordBatch.from_csv and is compared with two independent CPU readers: pyarrow.csv.read_csv
(explicit column_types, newlines_in_values) for values and NULLs, Python's csv module for strings and the record count.  The
two CPU readers are first asserted to agree with each other on the input: a text on which they disagree belongs to the
refusals (BHIP_ENOTIMPL), not here.  Floats are compared bit for bit; integers, dates, strings, row counts, validity exactly."""
import csv
import datetime
import io
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

import ballista_amd as ba
from ballista_amd import expr as E, tpch
from ballista_amd._lib import ExecutionError, NotImplementedOnGpu, PlanError

import helpers
import plan_nodes as N
import proto_encode as pe

pytestmark = pytest.mark.gpu
TBL = os.path.join(helpers.GOLDEN, "tbl")
CHUNK = 16384                     # bytes of text per workgroup in the record passes (TBL_CHUNK)

LINEITEM = [("l_orderkey", E.INT32), ("l_partkey", E.INT32), ("l_suppkey", E.INT32), ("l_linenumber", E.INT32),
            ("l_quantity", E.FLOAT64), ("l_extendedprice", E.FLOAT64), ("l_discount", E.FLOAT64), ("l_tax", E.FLOAT64),
            ("l_returnflag", E.UTF8), ("l_linestatus", E.UTF8), ("l_shipdate", E.DATE32), ("l_commitdate", E.DATE32),
            ("l_receiptdate", E.DATE32), ("l_shipinstruct", E.UTF8), ("l_shipmode", E.UTF8), ("l_comment", E.UTF8)]
ORDERS = [("o_orderkey", E.INT32), ("o_custkey", E.INT32), ("o_orderstatus", E.UTF8), ("o_totalprice", E.FLOAT64),
          ("o_orderdate", E.DATE32), ("o_orderpriority", E.UTF8), ("o_clerk", E.UTF8), ("o_shippriority", E.INT32), ("o_comment", E.UTF8)]
NATION = [("n_nationkey", E.INT32), ("n_name", E.UTF8), ("n_regionkey", E.INT32), ("n_comment", E.UTF8)]
PA_TYPE = {E.INT32: pa.int32(), E.INT64: pa.int64(), E.FLOAT64: pa.float64(), E.DATE32: pa.date32(), E.UTF8: pa.string(),
           E.BOOLEAN: pa.bool_()}
EPOCH = datetime.date(1970, 1, 1)


def py_bool(s):
    return {"true": True, "false": False}[s.lower()]


def cpu_readers(text, schema, delimiter, has_header, py_bools):
    """-> {name: list with None for NULL} from pyarrow, after asserting that Python's csv module reads the same records"""
    names = [f[0] for f in schema]
    types = {f[0]: (pa.string() if (f[1] == E.BOOLEAN and py_bools) else PA_TYPE[f[1]]) for f in schema}
    table = pacsv.read_csv(io.BytesIO(text),
                           read_options=pacsv.ReadOptions(column_names=None if has_header else names, use_threads=False),
                           parse_options=pacsv.ParseOptions(delimiter=delimiter, newlines_in_values=True),
                           convert_options=pacsv.ConvertOptions(column_types=types))
    assert table.column_names == names
    want = {n: table.column(n).to_pylist() for n in names}
    rows = list(csv.reader(io.StringIO(text.decode(), newline=""), delimiter=delimiter))
    if has_header:
        assert rows[0] == names
        rows = rows[1:]
    assert len(rows) == table.num_rows                                       # the two readers find the same records ...
    for k, (name, dtype, *_) in enumerate(schema):
        cells = [r[k] for r in rows]
        if dtype == E.UTF8:
            assert cells == want[name], name                                 # ... the same strings ...
            continue
        if dtype == E.BOOLEAN and py_bools:                                  # letter cases pyarrow does not know: Python's rule
            want[name] = [None if c == "" else py_bool(c) for c in cells]
            continue
        conv = {E.INT32: int, E.INT64: int, E.FLOAT64: float, E.DATE32: datetime.date.fromisoformat, E.BOOLEAN: py_bool}[dtype]
        mine = [None if c == "" else conv(c) for c in cells]                 # ... and the same values and NULLs
        if dtype == E.FLOAT64:
            assert [None if v is None else np.float64(v).view(np.uint64) for v in mine] == \
                   [None if v is None else np.float64(v).view(np.uint64) for v in want[name]], name
        else:
            assert mine == want[name], name
    return want, len(rows)


def check(ctx, text, schema, columns=None, delimiter=",", has_header=True, py_bools=False):
    want, n_rows = cpu_readers(text, schema, delimiter, has_header, py_bools)
    rb = ba.RecordBatch.from_csv(ctx, text, schema, columns, delimiter=delimiter, has_header=has_header)
    cols = columns or [f[0] for f in schema]
    assert rb.num_rows == n_rows
    assert [rb.column_info(i)[0] for i in range(rb.num_columns)] == cols
    for i, name in enumerate(cols):
        w = want[name]
        dtype, vals, valid = rb.column(i)
        nulls = [v is None for v in w]
        if any(nulls):
            assert valid is not None and [not v for v in valid] == nulls, name
        else:
            assert valid is None, name                                       # no NULL occurred: no validity buffer
        keep = [k for k, isnull in enumerate(nulls) if not isnull]
        got = [vals[k] for k in keep]
        exp = [w[k] for k in keep]
        if dtype == E.UTF8:
            assert got == exp, name
        elif dtype == E.FLOAT64:
            assert np.array_equal(np.asarray(got, np.float64).view(np.uint64), np.asarray(exp, np.float64).view(np.uint64)), name   # bit-exact
        elif dtype == E.DATE32:
            assert [int(v) for v in got] == [(d - EPOCH).days for d in exp], name
        elif dtype == E.BOOLEAN:
            assert [bool(v) for v in got] == exp, name
        else:
            assert [int(v) for v in got] == exp, name
    return rb


def tbl_as_csv(name, quoting, terminator="\n", header=True, schema=None):
    """a reference `.tbl` fixture rewritten as comma CSV"""
    lines = open(os.path.join(TBL, name + ".tbl"), "rb").read().decode().split("\n")
    out = io.StringIO(newline="")
    w = csv.writer(out, quoting=quoting, lineterminator=terminator)
    if header:
        w.writerow([f[0] for f in schema])
    for ln in lines:
        if ln:
            w.writerow(ln.split("|")[:-1])
    return out.getvalue().encode()


@pytest.mark.parametrize("name,schema", [("lineitem_partition0", LINEITEM), ("lineitem_partition1", LINEITEM), ("orders_orders", ORDERS),
                                         ("nation_nation", NATION)])
@pytest.mark.parametrize("quoting", [csv.QUOTE_MINIMAL, csv.QUOTE_ALL], ids=["minimal", "quote_all"])
def test_reference_fixtures_as_csv(ctx, name, schema, quoting):
    text = tbl_as_csv(name, quoting, schema=schema)
    check(ctx, text, schema)
    check(ctx, text, schema, [schema[-1][0], schema[0][0]])                                   # projection, reordered
    check(ctx, text.rstrip(b"\n"), schema, [schema[1][0]])                                    # unterminated last record
    check(ctx, tbl_as_csv(name, quoting, terminator="\r\n", schema=schema), schema)           # CRLF
    check(ctx, tbl_as_csv(name, quoting, header=False, schema=schema), schema, has_header=False)


GEN_SCHEMA = [("a", E.INT32, True), ("b", E.INT64, False), ("c", E.FLOAT64, False), ("d", E.FLOAT64, True), ("e", E.DATE32, True),
              ("f", E.UTF8, True), ("g", E.BOOLEAN, True), ("h", E.UTF8, False), ("k", E.BOOLEAN, False)]
_generated = {}


def generated_rows(n=50_000):
    """the awkward values of test_tbl_scan_gpu.test_generated_text_with_awkward_values, plus strings that hold every delimiter,
    quotes, line ends, and empty fields in the nullable columns.  Each cell: (text, must be quoted)"""
    if n in _generated:
        return _generated[n]
    rng = np.random.default_rng(0)
    pieces = [",", ";", "\t", "|", '"', '""', "\n", "\r\n", " ", "x,y", 'say "hi"', "a\nb"]
    bools = ["true", "false", "True", "FALSE", "tRuE", "fAlSe", "TRUE", "False"]
    rows = []
    for i in range(n):
        k = int(rng.integers(-2 ** 31, 2 ** 31 - 1))
        big = int(rng.integers(-2 ** 62, 2 ** 62))
        cents = int(rng.integers(0, 10 ** 9))
        dec = f"{'-' if rng.random() < 0.3 else ''}{cents // 100}.{cents % 100:02d}"
        frac = ["0.1", "0.07", "123456.789012345", "0", "-0.00", "9007199254740991", "1e0"][int(rng.integers(0, 6))]
        d = EPOCH + datetime.timedelta(days=int(rng.integers(-20000, 40000)))
        s = "".join(chr(int(c)) for c in rng.integers(97, 123, int(rng.integers(0, 40))))
        for _ in range(int(rng.integers(0, 3))):                       # up to two awkward pieces somewhere inside
            at = int(rng.integers(0, len(s) + 1))
            s = s[:at] + pieces[int(rng.integers(0, len(pieces)))] + s[at:]
        h = "".join(chr(int(c)) for c in rng.integers(97, 123, int(rng.integers(0, 8))))
        null = lambda p=0.1: rng.random() < p
        quote = lambda p=0.1: bool(rng.random() < p)                   # some cells are quoted without need, "" among them
        rows.append([("" if null() else str(k), quote()), (str(big), quote()), (dec, quote()), ("" if null() else frac, quote()),
                     ("" if null() else d.isoformat(), quote()), (s, quote(0.2)), ("" if null() else bools[int(rng.integers(0, 8))], quote()),
                     (h, quote()), (bools[int(rng.integers(0, 8))], False)])
    _generated[n] = rows
    return rows


def render(rows, delimiter, terminator="\n", header=None):
    def cell(s, q):
        if q or delimiter in s or '"' in s or "\n" in s or "\r" in s:
            return '"' + s.replace('"', '""') + '"'
        return s
    lines = ([delimiter.join(header)] if header else []) + [delimiter.join(cell(s, q) for s, q in r) for r in rows]
    return (terminator.join(lines) + terminator).encode()


@pytest.mark.parametrize("delimiter", [",", ";", "\t", "|"], ids=["comma", "semicolon", "tab", "pipe"])
def test_generated_records_with_quotes_nulls_and_awkward_values(ctx, delimiter):
    rows = generated_rows()
    names = [f[0] for f in GEN_SCHEMA]
    text = render(rows, delimiter, header=names)
    assert len(rows) >= 50_000 and text.count(b'"') > 10_000
    check(ctx, text, GEN_SCHEMA, delimiter=delimiter, py_bools=True)
    check(ctx, render(rows, delimiter, terminator="\r\n"), GEN_SCHEMA, ["f", "c", "e", "g", "a"], delimiter=delimiter, has_header=False,
          py_bools=True)


def test_booleans_pyarrow_knows_and_a_quote_free_text(ctx):
    """no '"' anywhere: the record passes take their quote-free shape; Booleans in the three spellings pyarrow reads"""
    rng = np.random.default_rng(3)
    spell = ["true", "True", "TRUE", "false", "False", "FALSE", ""]
    lines = ["n;t;x"] + [f"{i};{spell[int(rng.integers(0, 7))]};{i * 0.125}" for i in range(20_000)]
    text = ("\n".join(lines) + "\n").encode()
    schema = [("n", E.INT64, False), ("t", E.BOOLEAN, True), ("x", E.FLOAT64, False)]
    check(ctx, text, schema, delimiter=";")
    check(ctx, text[:-1], schema, ["t"], delimiter=";")


def filler(k, size):
    """one record `k,"xx..x",true` + '\n' of exactly `size` bytes"""
    head = f'{k},"'
    body = size - len(head) - len('",true\n')
    assert body >= 0
    return head + "x" * body + '",true\n'


EDGE_SCHEMA = [("n", E.INT32), ("s", E.UTF8), ("t", E.BOOLEAN)]


def text_with_field_at(offset_in_field, field, edge=CHUNK):
    """records such that byte `offset_in_field` of the quoted cell `field` (its opening quote is byte 0) lies at text offset `edge`;
    the cell sits in a record `7,<field>,false`"""
    want_start = edge - offset_in_field - len("7,")
    out, k = "", 0
    while want_start - len(out) > 200:
        out += filler(k, 100)
        k += 1
    rest = want_start - len(out)
    out += filler(k, rest - 20) + filler(k + 1, 20) if rest >= 40 else filler(k, rest)
    assert len(out) == want_start
    out += "7," + field + ",false\n"
    out += "".join(filler(100 + j, 50) for j in range(400))           # records behind it: a wrong parity would cut them up
    return out.encode()


def test_quoted_field_with_newlines_across_a_chunk_edge_and_thread_edges(ctx):
    inner = "".join(f"line{j}\n" if j % 3 else f'li""ne{j},\r\n' for j in range(40))      # ~300 bytes, line ends every 6-10 bytes
    field = '"' + inner + '"'
    for off in (1, 70, 150, len(field) - 2):
        text = text_with_field_at(off, field)
        assert text[CHUNK - off] == ord('"') and text[CHUNK - off + len(field) - 1] == ord('"')      # the cell straddles byte 16384
        assert b"\n" in text[CHUNK - off:CHUNK] or off < 6
        check(ctx, text, EDGE_SCHEMA, has_header=False)
        check(ctx, text, EDGE_SCHEMA, ["s"], has_header=False)


def test_escaped_quote_pair_split_by_a_chunk_edge(ctx):
    field = '"ab""cd\nef""""gh"'
    at = field.index('""') + 1                                          # the second quote of the first pair
    text = text_with_field_at(at, field)
    assert text[CHUNK - 1:CHUNK + 1] == b'""' and text[CHUNK - 2:CHUNK - 1] == b"b"
    check(ctx, text, EDGE_SCHEMA, has_header=False)
    at = field.index('""""') + 2                                        # between the two pairs
    text = text_with_field_at(at, field)
    assert text[CHUNK - 2:CHUNK + 2] == b'""""'
    check(ctx, text, EDGE_SCHEMA, has_header=False)
    # the closing quote is the chunk's last byte, the opening quote of the next record's cell its first-but-two
    text = text_with_field_at(len(field) - 1, field, edge=CHUNK - 1)
    assert text[CHUNK - 1:CHUNK] == b'"' and text[CHUNK:CHUNK + 1] == b","
    check(ctx, text, EDGE_SCHEMA, has_header=False)


def test_quoted_field_longer_than_a_chunk(ctx):
    rng = np.random.default_rng(9)
    parts = []
    while sum(map(len, parts)) < 40_000:
        parts.append(["\n", '""', ",", "\r\n", "word", "x" * 61][int(rng.integers(0, 6))])
    field = '"' + "".join(parts) + '"'
    text = ("n,s,t\n1,short,true\n2," + field + ",false\n3,\"\",TRUE\n" + "".join(filler(10 + j, 40) for j in range(600))).encode()
    assert len(field) > 2 * CHUNK
    check(ctx, text, EDGE_SCHEMA)
    check(ctx, text, EDGE_SCHEMA, ["t", "s"])


def test_a_file_that_is_one_quoted_record(ctx):
    schema = [("s", E.UTF8)]
    for text in (b'"a\nb,""c"""', b'"a\nb,""c"""\n', b'"only\r\nthis"\r\n', b'"' + b"x\n" * 20_000 + b'"'):
        check(ctx, text, schema, has_header=False)
    rb = ba.RecordBatch.from_csv(ctx, b"", schema)
    assert rb.num_rows == 0 and rb.num_columns == 1
    rb = ba.RecordBatch.from_csv(ctx, b"s\n", schema)                    # a header and nothing else
    assert rb.num_rows == 0


def test_long_records_walk_the_text_in_hbm(ctx):
    """256 records of ~300 bytes do not fit the 48 KB LDS stage of a workgroup: that tile is walked in HBM; long and short tiles
    alternate, and the long cells are quoted and hold line ends and "" pairs"""
    rng = np.random.default_rng(5)
    rows = []
    for i in range(3000):
        long_tile = (i // 256) % 2 == 1
        s = "".join(chr(int(c)) for c in rng.integers(97, 123, int(rng.integers(250, 400)) if long_tile else int(rng.integers(0, 20))))
        if long_tile:
            s = s[:50] + "\n" + s[50:120] + '"' + s[120:200] + ",\r\n" + s[200:]
        rows.append([(str(i), False), (s, i % 5 == 0), (f"{i * 0.25:.2f}", False), (s[::-1][:7], False), ("" if i % 7 == 0 else "true", False)])
    schema = [("a", E.INT32), ("s", E.UTF8), ("x", E.FLOAT64), ("t", E.UTF8), ("b", E.BOOLEAN, True)]
    text = render(rows, ",", header=[f[0] for f in schema])
    check(ctx, text, schema)
    check(ctx, text, schema, ["x", "t", "b"])


def test_what_readers_disagree_on_is_refused_not_guessed(ctx):
    schema = [("a", E.INT32), ("s", E.UTF8), ("b", E.INT32)]
    ba.RecordBatch.from_csv(ctx, b'1,"x",2\n', schema, has_header=False)
    for stray in (b'1,a"b"c,2\n',                  # quotes inside an unquoted field
                  b'1,"ab"c,2\n',                  # bytes behind a closing quote
                  b'1,ab"c,2\n',                   # ... and an odd number of quotes
                  b'1,"abc,2\n3,x,4\n',            # a quoted field that is never closed
                  b'1,a\rb,2\n'):                  # a carriage return that ends no record
        with pytest.raises(NotImplementedOnGpu):
            ba.RecordBatch.from_csv(ctx, stray, schema, has_header=False)


def test_malformed_text_is_reported(ctx):
    schema = [("a", E.INT32), ("x", E.FLOAT64, True), ("d", E.DATE32), ("t", E.BOOLEAN)]
    ba.RecordBatch.from_csv(ctx, b"1,2.5,1996-01-02,true\n", schema, has_header=False)
    ba.RecordBatch.from_csv(ctx, b"1,,1996-01-02,true\n", schema, has_header=False)           # x is nullable
    for bad in (b"1,2.5,1996-01-02\n",                       # a field is missing
                b'1,"2.5,1996-01-02,true"\n',                # ... because a quoted cell swallowed the others
                b"1,abc,1996-01-02,true\n",                  # not a number
                b"1,2.5,1996-13-02,true\n",                  # not a date
                b"1,2.5,1996-01-02,yes\n",                   # not a Boolean
                b'1,"2""5",1996-01-02,true\n',               # a quote inside a number
                b"99999999999,2.5,1996-01-02,true\n",        # out of Int32 range
                b",2.5,1996-01-02,true\n",                   # an empty field in a column that is not nullable
                b'1,2.5,"",true\n',                          # ... quoted
                b"1,2.5,1996-01-02,true\n\n2,1.0,1996-01-03,false\n"):   # blank line
        with pytest.raises(ExecutionError):
            ba.RecordBatch.from_csv(ctx, bad, schema, has_header=False)
    with pytest.raises(NotImplementedOnGpu):
        ba.RecordBatch.from_csv(ctx, b"1,0.12345678901234567890,1996-01-02,true\n", schema, has_header=False)
    for delimiter in (",,", "", '"', "\n", "\r"):
        with pytest.raises(PlanError):
            ba.RecordBatch.from_csv(ctx, b"1,2.5,1996-01-02,true\n", schema, delimiter=delimiter, has_header=False)


def test_q1_over_a_csv_scan_leaf_of_the_wire_plan_equals_golden(ctx, monkeypatch, tmp_path):
    """no resolver: a CsvScanExecNode with has_header = true, delimiter = "," over two CSV files written from the lineitem fixture
    is the library's own device CSV scan — Q1 above it on the wire, equal to the golden of the fixture"""
    files = []
    for p in range(2):
        fn = tmp_path / f"lineitem_partition{p}.csv"
        fn.write_bytes(tbl_as_csv(f"lineitem_partition{p}", csv.QUOTE_MINIMAL, schema=LINEITEM))
        files.append(str(fn))
    assert any(b'"' in open(f, "rb").read() for f in files)              # the comments hold commas: quoted cells
    type_name = {E.INT32: "Int32", E.FLOAT64: "Float64", E.UTF8: "Utf8", E.DATE32: "Date32"}
    file_schema = [(n, type_name[t]) for n, t in LINEITEM]
    proj = [0, 2, 4, 5, 6, 7, 8, 9, 10]
    body = (pe.f_str(1, str(tmp_path)) + pe.f_packed(2, proj) + pe.f_bytes(3, pe.schema([(n, t, False) for n, t in file_schema])) +
            pe.f_str(4, ".csv") + pe.f_varint(5, 1) + pe.f_varint(6, 32768) + pe.f_str(7, ",") + pe.f_str(8, files[0]) + pe.f_str(8, files[1]))
    scan_bytes = pe.f_bytes(2, body)
    scan = ba.ExecutionPlan.from_proto(ctx, scan_bytes)
    assert scan.as_any() == "CsvExec" and scan.output_partitioning().partition_count() == 2
    assert [n for n, _, _ in scan.schema()] == [file_schema[i][0] for i in proj]
    assert "delimiter=','" in scan.display() and "has_header=true" in scan.display()
    # Q1 above it, on the wire as well: encode the operators over a stand-in leaf, then splice the real scan bytes in
    li = N.MemoryExec([[helpers.lineitem_fixture()]])
    li.name = "mem://x"
    li._schema = [(file_schema[i][0], file_schema[i][1], False) for i in proj]
    monkeypatch.setattr(tpch, "P", N)
    q1 = tpch.q1_plan(li)
    monkeypatch.undo()
    orig = pe.plan

    def plan_with_scan(p):
        return scan_bytes if p is li else orig(p)
    monkeypatch.setattr(pe, "plan", plan_with_scan)
    data = orig(q1)
    monkeypatch.undo()
    got = helpers.concat([helpers.from_device(b) for b in ba.ExecutionPlan.from_proto(ctx, data).collect()])
    g = json.load(open(os.path.join(helpers.GOLDEN, "q1_fixture.json")))["rows"]
    assert list(zip(got["l_returnflag"].to_pylist(), got["l_linestatus"].to_pylist())) == [(r["l_returnflag"], r["l_linestatus"]) for r in g]
    assert got["count_order"].to_pylist() == [r["count_order"] for r in g]
    for k in ("sum_qty", "sum_base_price", "sum_disc_price", "sum_charge", "avg_qty", "avg_price", "avg_disc"):
        assert np.allclose(got[k].to_pylist(), [r[k] for r in g], rtol=1e-9, atol=0), k      # the bound of test_tbl_scan_gpu for this golden
