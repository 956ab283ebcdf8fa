"""`.tbl` and CSV files of any size through the device scan (ballista_amd/csrc/host/text_stream.cpp, bhip_plan_text_scan,
ballista_amd.CsvExec): the file is cut into slabs of `slab_bytes` of text wherever those fall, a slab yields the records that
end in it as one batch, and the rest is carried to the next slab on the device.

The oracle is the one-shot scan (RecordBatch.from_tbl / from_csv on the whole text), which tests/test_tbl_scan_gpu.py and
tests/test_csv_scan_gpu.py check against the reference's fixtures, pyarrow and Python's csv module: the concatenated batches of
a stream must equal it column by column — floats by their bit patterns, integers, dates, strings, booleans, row counts and NULL
positions exactly — for every slab size that holds the longest record."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E, tpch
from ballista_amd._lib import ExecutionError, NotImplementedOnGpu, PlanError

import helpers
import plan_nodes as N
import proto_encode as pe

pytestmark = pytest.mark.gpu
TBL = os.path.join(helpers.GOLDEN, "tbl")
KIB, MIB = 1 << 10, 1 << 20
SLABS = [16 * KIB, 48 * KIB, 1 * MIB]

LINEITEM = [("l_orderkey", E.INT32), ("l_partkey", E.INT32), ("l_suppkey", E.INT32), ("l_linenumber", E.INT32),
            ("l_quantity", E.FLOAT64), ("l_extendedprice", E.FLOAT64), ("l_discount", E.FLOAT64), ("l_tax", E.FLOAT64),
            ("l_returnflag", E.UTF8), ("l_linestatus", E.UTF8), ("l_shipdate", E.DATE32), ("l_commitdate", E.DATE32),
            ("l_receiptdate", E.DATE32), ("l_shipinstruct", E.UTF8), ("l_shipmode", E.UTF8), ("l_comment", E.UTF8)]
ORDERS = [("o_orderkey", E.INT32), ("o_custkey", E.INT32), ("o_orderstatus", E.UTF8), ("o_totalprice", E.FLOAT64),
          ("o_orderdate", E.DATE32), ("o_orderpriority", E.UTF8), ("o_clerk", E.UTF8), ("o_shippriority", E.INT32), ("o_comment", E.UTF8)]
NATION = [("n_nationkey", E.INT32), ("n_name", E.UTF8), ("n_regionkey", E.INT32), ("n_comment", E.UTF8)]

# every CSV feature of the scan in a handful of records: nullable Int32 / Float64 / Date32 / Boolean with NULLs, quoted strings
# with "" pairs, delimiters, '\r' and '\n' inside quotes
CSV_SCHEMA = [("a", E.INT32, True), ("b", E.INT64, False), ("c", E.FLOAT64, True), ("d", E.DATE32, True), ("s", E.UTF8, False),
              ("g", E.BOOLEAN, True), ("t", E.UTF8, False)]


def csv_body(delim, eol, quote_all=True):
    q = (lambda s: '"' + s.replace('"', '""') + '"') if quote_all else (lambda s: s)
    d = delim
    rows = [
        ["1", "-9000000000", "0.1", "1996-01-02", q("plain"), "true", q("x")],
        ["", "2", "2.5", "", q('say ""hi""' if not quote_all else 'say "hi"'), "", q("")],
        ["-3", "3", "", "1970-01-01", '"a%sb"' % d, "FALSE", '"line one\nline two"'],
        ["4", "4", "1234567.125", "2024-02-29", '"cr\rinside"', "True", '"""quoted"""'],
        ["2147483647", "5", "-0.0", "1969-12-31", '"mixed %s ""q"" \r\n end"' % d, "false", q("tail")],
        ["", "6", "", "", q("nulls before"), "", '"%s%s%s"' % (d, d, d)],
    ]
    if not quote_all:
        rows[1][4] = '"say ""hi"""'
    return "".join(d.join(r) + eol for r in rows).encode()


def csv_text(delim=",", eol="\n", header=True, reps=1, quote_all=True, terminated=True):
    head = (delim.join(f[0] for f in CSV_SCHEMA) + eol).encode() if header else b""
    text = head + csv_body(delim, eol, quote_all) * reps
    return text if terminated else text[:-len(eol)]


def repeat_to(text, n_bytes):
    return text * (n_bytes // len(text) + 1)


# ---- comparison -------------------------------------------------------------------------------------------------------------
def host_columns(rb):
    return [rb.column(i) for i in range(rb.num_columns)]


def assert_stream_equals(batches, whole):
    """the concatenation of `batches` is `whole`; a batch carries a validity buffer exactly when a NULL occurred in it"""
    want = host_columns(whole)
    assert sum(b.num_rows for b in batches) == whole.num_rows
    got = [host_columns(b) for b in batches]
    for i, (dtype, w_vals, w_valid) in enumerate(want):
        name = whole.column_info(i)[0]
        for b in batches:
            assert b.column_info(i)[:2] == whole.column_info(i)[:2]
        valid_parts = []
        for b, cols in zip(batches, got):
            v = cols[i][2]
            if v is not None:
                assert not v.all(), f"{name}: a validity buffer although no NULL occurred in the batch"
            valid_parts.append(np.ones(b.num_rows, np.bool_) if v is None else v)
        g_valid = np.concatenate(valid_parts) if valid_parts else np.ones(0, np.bool_)
        ww = np.ones(whole.num_rows, np.bool_) if w_valid is None else w_valid
        assert np.array_equal(g_valid, ww), f"{name}: NULL positions"
        if dtype == E.UTF8:
            g_vals = [s for cols in got for s in cols[i][1]]
            assert g_vals == list(w_vals), name
            continue
        g_vals = np.concatenate([cols[i][1] for cols in got]) if got else np.zeros(0, w_vals.dtype)
        assert g_vals.dtype == w_vals.dtype
        if dtype == E.FLOAT64:
            assert np.array_equal(g_vals.view(np.uint64)[ww], w_vals.view(np.uint64)[ww]), f"{name}: bit patterns"
        else:
            assert np.array_equal(g_vals[ww], w_vals[ww]), name


def one_shot(ctx, text, schema, columns, fmt):
    if fmt.get("tbl"):
        return ba.RecordBatch.from_tbl(ctx, text, [f[:2] for f in schema], columns)
    return ba.RecordBatch.from_csv(ctx, text, schema, columns, delimiter=fmt["delimiter"], has_header=fmt["has_header"])


def stream_batches(ctx, path, schema, columns, fmt, slab_bytes):
    plan = ba.CsvExec(ctx, [str(path)], schema, columns, slab_bytes=slab_bytes, **fmt)
    assert plan.as_any() == "CsvExec" and plan.output_partitioning().partition_count() == 1
    return list(plan.execute(0))


def check_all_slabs(ctx, tmp_path, text, schema, columns, fmt, slabs):
    path = tmp_path / "text.dat"
    path.write_bytes(text)
    whole = one_shot(ctx, text, schema, columns, fmt)
    for slab in slabs:
        batches = stream_batches(ctx, path, schema, columns, fmt, slab)
        print(f"slab {slab}: {len(batches)} batches, {whole.num_rows} rows")
        if len(text) > slab:
            assert len(batches) > 1
            assert len(batches) <= -(-len(text) // slab)             # at most one batch per slab
        else:
            assert len(batches) == 1
        assert_stream_equals(batches, whole)


TBL_FMT = dict(tbl=True)
BIG = 16 * MIB                     # larger than every text below


# ---- 1. equal to the one-shot scan ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,schema,proj", [("lineitem_partition0", LINEITEM, ["l_comment", "l_quantity", "l_shipdate", "l_returnflag"]),
                                              ("orders_orders", ORDERS, ["o_comment", "o_orderkey"]),
                                              ("nation_nation", NATION, ["n_name"])])
def test_tbl_goldens_streamed_equal_one_shot(ctx, tmp_path, name, schema, proj):
    unit = open(os.path.join(TBL, name + ".tbl"), "rb").read()
    text = repeat_to(unit, 5 * MIB)                                  # at least 5 slabs of the largest slab size
    assert len(text) >= 5 * max(SLABS)
    for columns in (None, proj):
        check_all_slabs(ctx, tmp_path, text, schema, columns, TBL_FMT, SLABS + [BIG])


@pytest.mark.parametrize("case", ["semicolon_header_quoted", "crlf", "unterminated", "no_header_minimal_quotes"])
def test_csv_texts_streamed_equal_one_shot(ctx, tmp_path, case):
    reps = 5 * MIB // len(csv_body(",", "\n", quote_all=case != "no_header_minimal_quotes")) + 1
    if case == "semicolon_header_quoted":
        text, fmt = csv_text(";", "\n", True, reps), dict(delimiter=";", has_header=True)
    elif case == "crlf":
        text, fmt = csv_text(",", "\r\n", True, reps), dict(delimiter=",", has_header=True)
    elif case == "unterminated":
        text, fmt = csv_text(",", "\n", True, reps, terminated=False), dict(delimiter=",", has_header=True)
    else:
        text, fmt = csv_text(",", "\n", False, reps, quote_all=False), dict(delimiter=",", has_header=False)
    assert len(text) >= 5 * max(SLABS)
    assert (case == "unterminated") == (not text.endswith(b"\n"))
    for columns in (None, ["t", "c", "g", "a"]):
        check_all_slabs(ctx, tmp_path, text, CSV_SCHEMA, columns, fmt, SLABS + [BIG])


def test_small_files_give_one_batch(ctx, tmp_path):
    """a file that fits one slab is one batch, identical to the one-shot scan; empty and header-only files are one batch of 0 rows"""
    for text, fmt, schema in ((open(os.path.join(TBL, "lineitem_partition0.tbl"), "rb").read(), TBL_FMT, LINEITEM),
                              (csv_text(), dict(delimiter=",", has_header=True), CSV_SCHEMA),
                              (b"", TBL_FMT, LINEITEM), (b"", dict(delimiter=",", has_header=True), CSV_SCHEMA),
                              (csv_text(reps=0), dict(delimiter=",", has_header=True), CSV_SCHEMA),
                              (csv_text(reps=0, terminated=False), dict(delimiter=",", has_header=True), CSV_SCHEMA)):
        path = tmp_path / "small.dat"
        path.write_bytes(text)
        for slab in (0, 16 * KIB):                                   # 0: the default size
            batches = stream_batches(ctx, path, schema, None, fmt, slab)
            assert len(batches) == 1
            assert_stream_equals(batches, one_shot(ctx, text, schema, None, fmt))
            if len(text) < 100:
                assert batches[0].num_rows == 0
    # a text of exactly one slab
    unit = csv_body(",", "\n")
    text = (unit * (16 * KIB // len(unit) + 1))[:16 * KIB - 1] + b"\n"
    text = text[:text.rfind(b"\n1,")] + b"\n"                      # cut at a record start, then pad the last string
    pad = 16 * KIB - len(text) - len(b'1,2,,,"",,""\n')
    text += b'1,2,,,"' + b"p" * pad + b'",,""\n'
    assert len(text) == 16 * KIB
    path = tmp_path / "exact.csv"
    path.write_bytes(text)
    fmt = dict(delimiter=",", has_header=False)
    batches = stream_batches(ctx, path, CSV_SCHEMA, None, fmt, 16 * KIB)
    assert len(batches) == 1
    assert_stream_equals(batches, one_shot(ctx, text, CSV_SCHEMA, None, fmt))


def test_a_record_longer_than_the_carry_room_but_not_than_the_slab(ctx, tmp_path):
    """carries of more than 1 MiB take the path that joins carry and slab in a buffer of their own"""
    fmt = dict(delimiter=",", has_header=True)
    long_record = b'7,8,1.5,2001-01-01,"' + b"L" * (3 * MIB // 2) + b'",true,"after ""it"""\n'
    unit = csv_body(",", "\n")
    text = csv_text(reps=3000) + long_record + unit * 9000 + long_record + unit * 3
    check_all_slabs(ctx, tmp_path, text, CSV_SCHEMA, None, fmt, [2 * MIB, BIG])


# ---- 2. boundary sweep ------------------------------------------------------------------------------------------------------
FEATURES = ["record_end", "cr_of_crlf", "newline_in_quotes", "first_quote_of_pair", "opening_quote", "delimiter", "header_newline"]


def text_with_byte_at(feature, where):
    """a CSV text (header, ',') in which the chosen byte of `feature` sits at offset `where`: one Utf8 field before it is padded"""
    eol = "\r\n" if feature == "cr_of_crlf" else "\n"
    head = csv_text(",", eol, True, 0)
    unit = csv_body(",", eol)
    tail = unit * (2 * 16 * KIB // len(unit) + 2)
    if feature == "header_newline":
        # the header is not compared with the schema: its last name is padded
        head = head[:-len(eol)]
        head += b"x" * (where - len(head)) + eol.encode()
        assert head.index(b"\n") == where
        return head + tail
    record = {"record_end": b'1,2,0.5,1999-12-31,"s",true,"t"' + eol.encode(),
              "cr_of_crlf": b'1,2,0.5,1999-12-31,"s",true,"t"\r\n',
              "newline_in_quotes": b'1,2,0.5,1999-12-31,"s",true,"t\nu"\n',
              "first_quote_of_pair": b'1,2,0.5,1999-12-31,"s",true,"t""u"\n',
              "opening_quote": b'1,2,0.5,1999-12-31,"s",true,"t"\n',
              "delimiter": b'1,2,0.5,1999-12-31,"s",true,"t"\n'}[feature]
    at = {"record_end": lambda: record.rindex(b"\n"), "cr_of_crlf": lambda: record.rindex(b"\r"),
          "newline_in_quotes": lambda: record.index(b"\n"), "first_quote_of_pair": lambda: record.index(b'""'),
          "opening_quote": lambda: record.rindex(b',"') + 1, "delimiter": lambda: record.rindex(b',"')}[feature]()
    front = head + unit * 20
    pad_record = b'9,9,,,"%s",,"pad"' + eol.encode()
    n_pad = where - at - len(front) - (len(pad_record) - 2)
    assert n_pad >= 0
    text = front + pad_record % (b"p" * n_pad) + record
    assert len(text) - len(record) + at == where
    return text + tail


@pytest.mark.parametrize("feature", FEATURES)
def test_boundary_sweep(ctx, tmp_path, feature):
    slab = 16 * KIB
    fmt = dict(delimiter=",", has_header=True)
    for d in (-2, -1, 0, 1, 2):
        text = text_with_byte_at(feature, slab + d)
        want = {"record_end": b"\n", "cr_of_crlf": b"\r", "newline_in_quotes": b"\n", "first_quote_of_pair": b'"',
                "opening_quote": b'"', "delimiter": b",", "header_newline": b"\n"}[feature]
        assert text[slab + d:slab + d + 1] == want
        if feature == "first_quote_of_pair":
            assert text[slab + d + 1:slab + d + 2] == b'"'
        assert len(text) > 2 * slab
        path = tmp_path / f"sweep_{d + 2}.csv"
        path.write_bytes(text)
        whole = one_shot(ctx, text, CSV_SCHEMA, None, fmt)
        batches = stream_batches(ctx, path, CSV_SCHEMA, None, fmt, slab)
        assert len(batches) > 1
        assert_stream_equals(batches, whole)


# ---- 3. errors --------------------------------------------------------------------------------------------------------------
def fresh_scan_is_correct(ctx, tmp_path):
    text = csv_text(reps=400)
    path = tmp_path / "fresh.csv"
    path.write_bytes(text)
    fmt = dict(delimiter=",", has_header=True)
    assert_stream_equals(stream_batches(ctx, path, CSV_SCHEMA, None, fmt, 16 * KIB), one_shot(ctx, text, CSV_SCHEMA, None, fmt))


def test_malformed_value_in_the_third_slab(ctx, tmp_path):
    slab = 16 * KIB
    unit = csv_body(",", "\n")
    good = csv_text(reps=1) + unit * (2 * slab // len(unit) + 2)
    assert 2 * slab < len(good) < 3 * slab - 200
    text = good + b'12x,2,0.5,1999-12-31,"s",true,"t"\n' + unit * (3 * slab // len(unit))
    path = tmp_path / "malformed.csv"
    path.write_bytes(text)
    stream = ba.CsvExec(ctx, [str(path)], CSV_SCHEMA, slab_bytes=slab).execute(0)
    first, second = next(stream), next(stream)
    assert first.num_rows > 0 and second.num_rows > 0
    with pytest.raises(ExecutionError, match="malformed.csv") as err:
        next(stream)
    assert "not a value of its column's type" in str(err.value) and str(2 * slab) in str(err.value)
    # the two batches that arrived are the first rows of the text
    whole_rows = one_shot(ctx, good, CSV_SCHEMA, None, dict(delimiter=",", has_header=True))
    n = first.num_rows + second.num_rows
    assert [int(v) for v in np.concatenate([first.column(1)[1], second.column(1)[1]])] == [int(v) for v in whole_rows.column(1)[1][:n]]
    del stream
    fresh_scan_is_correct(ctx, tmp_path)


def test_records_that_do_not_end(ctx, tmp_path):
    slab = 16 * KIB
    unit = csv_body(",", "\n")
    # a record of two and a half slabs
    text = csv_text(reps=10) + b'1,2,0.5,1999-12-31,"' + b"w" * (5 * slab // 2) + b'",true,"t"\n' + unit * 10
    path = tmp_path / "long_record.csv"
    path.write_bytes(text)
    with pytest.raises(NotImplementedOnGpu, match="longer than the slab") as err:
        list(ba.CsvExec(ctx, [str(path)], CSV_SCHEMA, slab_bytes=slab).execute(0))
    assert "long_record.csv" in str(err.value) and "not closed" in str(err.value)
    fresh_scan_is_correct(ctx, tmp_path)
    # the same file is fine once a slab holds the record
    fmt = dict(delimiter=",", has_header=True)
    assert_stream_equals(stream_batches(ctx, path, CSV_SCHEMA, None, fmt, 48 * KIB), one_shot(ctx, text, CSV_SCHEMA, None, fmt))
    # a quote opened in the first slab and never closed
    text = csv_text(reps=10) + b'1,2,0.5,1999-12-31,"open' + unit * (4 * slab // len(unit))
    path = tmp_path / "open_quote.csv"
    path.write_bytes(text)
    with pytest.raises(NotImplementedOnGpu, match="open_quote.csv"):
        list(ba.CsvExec(ctx, [str(path)], CSV_SCHEMA, slab_bytes=slab).execute(0))
    fresh_scan_is_correct(ctx, tmp_path)
    # ... and in a `.tbl` file, a line longer than the slab
    line = open(os.path.join(TBL, "nation_nation.tbl"), "rb").read()
    text = line + b"99|" + b"n" * (3 * slab) + b"|1|comment|\n" + line
    path = tmp_path / "long_line.tbl"
    path.write_bytes(text)
    with pytest.raises(NotImplementedOnGpu, match="long_line.tbl"):
        list(ba.CsvExec(ctx, [str(path)], NATION, tbl=True, slab_bytes=slab).execute(0))
    fresh_scan_is_correct(ctx, tmp_path)


def test_bad_arguments(ctx, tmp_path):
    path = tmp_path / "x.csv"
    path.write_bytes(csv_text())
    for slab in (1000, 3 << 30, 16 * KIB + 512, -16 * KIB):
        with pytest.raises(PlanError):
            ba.CsvExec(ctx, [str(path)], CSV_SCHEMA, slab_bytes=slab)
    for delimiter in (",,", "", '"', "\n", "\r"):
        with pytest.raises(PlanError):
            ba.CsvExec(ctx, [str(path)], CSV_SCHEMA, delimiter=delimiter)
    with pytest.raises(ExecutionError, match="cannot open"):
        next(ba.CsvExec(ctx, [str(tmp_path / "missing.csv")], CSV_SCHEMA).execute(0))
    fresh_scan_is_correct(ctx, tmp_path)


# ---- 4. early release -------------------------------------------------------------------------------------------------------
def test_early_release_and_interleaved_streams(ctx, tmp_path):
    slab = 16 * KIB
    fmt = dict(delimiter=",", has_header=True)
    unit = csv_body(",", "\n")
    text = csv_text(reps=(6 * slab - 600) // len(unit))
    assert 5 * slab < len(text) <= 6 * slab
    path = tmp_path / "six_slabs.csv"
    path.write_bytes(text)
    whole = one_shot(ctx, text, CSV_SCHEMA, None, fmt)
    ctx.synchronize()
    before = ctx.memory()[0]
    stream = ba.CsvExec(ctx, [str(path)], CSV_SCHEMA, slab_bytes=slab).execute(0)
    first = next(stream)
    assert 0 < first.num_rows < whole.num_rows
    assert ctx.memory()[0] > before
    del stream                                                       # stops the reader, frees the slabs
    fresh_scan_is_correct(ctx, tmp_path)
    n = first.num_rows
    assert list(first.column(4)[1]) == list(whole.column(4)[1][:n])
    del first
    assert ctx.memory()[0] == before
    # two streams over different files, pulled in turn from one thread
    other = open(os.path.join(TBL, "orders_orders.tbl"), "rb").read()
    other = other * (5 * slab // len(other))
    other_path = tmp_path / "orders.tbl"
    other_path.write_bytes(other)
    s1 = ba.CsvExec(ctx, [str(path)], CSV_SCHEMA, slab_bytes=slab).execute(0)
    s2 = ba.CsvExec(ctx, [str(other_path)], ORDERS, tbl=True, slab_bytes=slab).execute(0)
    got1, got2 = [], []
    while True:
        b1, b2 = next(s1, None), next(s2, None)
        if b1 is None and b2 is None:
            break
        if b1 is not None:
            got1.append(b1)
        if b2 is not None:
            got2.append(b2)
    assert len(got1) > 1 and len(got2) > 1
    assert_stream_equals(got1, whole)
    assert_stream_equals(got2, one_shot(ctx, other, ORDERS, None, TBL_FMT))


def test_several_files_are_several_partitions(ctx, tmp_path):
    texts = [open(os.path.join(TBL, f"lineitem_partition{p}.tbl"), "rb").read() * 40 for p in range(2)]
    paths = []
    for p, t in enumerate(texts):
        paths.append(str(tmp_path / f"part{p}.tbl"))
        open(paths[-1], "wb").write(t)
    plan = ba.CsvExec(ctx, paths, LINEITEM, ["l_orderkey", "l_comment"], tbl=True, slab_bytes=16 * KIB)
    assert plan.output_partitioning().partition_count() == 2
    assert [n for n, _, _ in plan.schema()] == ["l_orderkey", "l_comment"]
    assert "device scan" in plan.display() and "batch_size is not used" in plan.display()
    for p, t in enumerate(texts):
        assert_stream_equals(list(plan.execute(p)), one_shot(ctx, t, LINEITEM, ["l_orderkey", "l_comment"], TBL_FMT))
    got = plan.collect()
    assert sum(b.num_rows for b in got) == 2 * 40 * 10


# ---- 5. the wire plan -------------------------------------------------------------------------------------------------------
WIRE_TYPE = {E.INT32: "Int32", E.FLOAT64: "Float64", E.UTF8: "Utf8", E.DATE32: "Date32"}
Q1_PROJ = [0, 2, 4, 5, 6, 7, 8, 9, 10]


def tbl_scan_node(directory, files, proj, batch_size=32768):
    """a CsvScanExecNode over '|'-separated header-less files (rust/core/proto/ballista.proto)"""
    body = (pe.f_str(1, directory) + pe.f_packed(2, proj) + pe.f_bytes(3, pe.schema([(n, WIRE_TYPE[t], False) for n, t in LINEITEM])) +
            pe.f_str(4, ".tbl") + pe.f_varint(6, batch_size) + pe.f_str(7, "|"))
    for f in files:
        body += pe.f_str(8, f)
    return pe.f_bytes(2, body)


def splice(monkeypatch, build, scan_bytes, schema):
    """the operators of build(leaf) on the wire with `scan_bytes` where the leaf stands"""
    leaf = N.MemoryExec([[helpers.lineitem_fixture()]])
    leaf.name = "mem://x"
    leaf._schema = schema
    monkeypatch.setattr(tpch, "P", N)
    tree = build(leaf)
    monkeypatch.undo()
    orig = pe.plan
    monkeypatch.setattr(pe, "plan", lambda p: scan_bytes if p is leaf else orig(p))
    data = orig(tree)
    monkeypatch.undo()
    return data


def q1_partial_merge_final(leaf):
    """Partial aggregate -> Merge -> Final aggregate, the shape of Q1 without its projection and sort"""
    P = tpch.P
    q = tpch.q1_parts(tpch._schema_of(leaf))
    partial = P.HashAggregateExec(P.PARTIAL, q["group"], q["aggs"], P.FilterExec(q["predicate"], leaf))
    group = [(E.col("l_returnflag"), "l_returnflag"), (E.col("l_linestatus"), "l_linestatus")]
    return P.HashAggregateExec(P.FINAL, group, tpch.q1_final_aggs(), P.MergeExec(partial))


CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import ballista_amd as ba
import helpers
ctx = ba.Context(0)
plan = ba.ExecutionPlan.from_proto(ctx, open(sys.argv[2], "rb").read())
assert "one batch per slab of 16384 bytes" in plan.display(), plan.display()
leaf = ba.ExecutionPlan.from_proto(ctx, open(sys.argv[3], "rb").read())
batches = [sum(1 for _ in leaf.execute(p)) for p in range(leaf.output_partitioning().partition_count())]
got = helpers.concat([helpers.from_device(b) for b in plan.collect()])
json.dump(dict(batches=batches, cols={k: v.to_pylist() for k, v in got.items()}), open(sys.argv[4], "w"))
"""


def test_q1_shaped_wire_plan_over_the_streamed_leaf(ctx, tmp_path, monkeypatch):
    """a CsvScanExecNode over a directory of two `.tbl` files, no resolver: two partitions, each streamed in 16 KiB slabs (the
    slab size comes from the environment, which the library reads when it is loaded: a child process), under Partial
    aggregate -> Merge -> Final aggregate; equal to the same plan over a MemoryExec of the one-shot batches"""
    import json
    data_dir = tmp_path / "lineitem"
    data_dir.mkdir()
    texts = []
    for p in range(2):
        unit = open(os.path.join(TBL, f"lineitem_partition{p}.tbl"), "rb").read()
        texts.append(unit * (5 * 16 * KIB // len(unit) + 1 + p))
        (data_dir / f"part-{p}.tbl").write_bytes(texts[-1])
    scan_bytes = tbl_scan_node(str(data_dir), [], Q1_PROJ)          # no filenames: the directory is listed
    scan = ba.ExecutionPlan.from_proto(ctx, scan_bytes)
    assert scan.as_any() == "CsvExec" and scan.output_partitioning().partition_count() == 2
    schema = [(LINEITEM[i][0], WIRE_TYPE[LINEITEM[i][1]], False) for i in Q1_PROJ]
    data = splice(monkeypatch, q1_partial_merge_final, scan_bytes, schema)
    (tmp_path / "plan.bin").write_bytes(data)
    (tmp_path / "leaf.bin").write_bytes(scan_bytes)
    env = dict(os.environ, BHIP_TEXT_SLAB_MB=str(16 / 1024))
    out = tmp_path / "out.json"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, helpers.ROOT, str(tmp_path / "plan.bin"),
                        str(tmp_path / "leaf.bin"), str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    child = json.load(open(out))
    assert all(n >= 5 for n in child["batches"]), child["batches"]          # the leaf really streamed
    got = child["cols"]
    # the same operators over the one-shot batches
    cols = [LINEITEM[i][0] for i in Q1_PROJ]
    mem = ba.MemoryExec([[ba.RecordBatch.from_tbl(ctx, t, LINEITEM, cols)] for t in texts], ctx)
    want = helpers.concat(helpers.collect_product(q1_partial_merge_final(mem)))
    assert set(got) == set(want.keys())
    key = lambda c: sorted(range(len(c["l_returnflag"])), key=lambda i: (c["l_returnflag"][i], c["l_linestatus"][i]))
    want = {k: v.to_pylist() for k, v in want.items()}
    go, wo = key(got), key(want)
    assert len(go) == len(wo) > 1
    for k in want:
        g, w = [got[k][i] for i in go], [want[k][i] for i in wo]
        if k in ("l_returnflag", "l_linestatus", "count_order"):
            assert g == w, k                                         # groups and counts exactly
        else:
            assert np.allclose(g, w, rtol=1e-6, atol=0), k           # RTOL of tests/test_q1_q6_gpu.py


# ---- 6. beyond 4 GiB --------------------------------------------------------------------------------------------------------
BIG_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import ballista_amd as ba
import helpers
ctx = ba.Context(0)
plan = ba.ExecutionPlan.from_proto(ctx, open(sys.argv[2], "rb").read())
leaf = ba.ExecutionPlan.from_proto(ctx, open(sys.argv[3], "rb").read())
got = helpers.concat([helpers.from_device(b) for b in plan.collect()])
peak = ctx.memory()[1]
stats = leaf.execute(0).drain()
json.dump(dict(peak=peak, cols={k: v.to_pylist() for k, v in got.items()}, rows=stats["num_rows"], batches=stats["num_batches"]),
          open(sys.argv[4], "w"))
"""


def test_a_file_beyond_4_gib_through_the_wire_plan(ctx, tmp_path, monkeypatch):
    """lineitem_partition0.tbl repeated to 4.25 GiB, scanned with the default slab size through bhip_plan_from_proto with no
    resolver: the row count, SUM(l_quantity) (exact in doubles: the quantities are small integers), MIN / MAX(l_shipdate), and
    the peak of device memory, which stays below the projected columns plus four slabs"""
    import json
    need = 6 << 30
    free = shutil.disk_usage(tmp_path).free
    if free < need:
        pytest.skip(f"the filesystem of tmp_path has {free / 2**30:.1f} GiB free, the 4.25 GiB file of this test needs 6 GiB")
    unit = open(os.path.join(TBL, "lineitem_partition0.tbl"), "rb").read()
    rows = [ln.split("|") for ln in unit.decode().splitlines()]
    block = unit * 4096
    reps_of_block = (17 << 28) // len(block) + 1                      # 4.25 GiB
    reps = reps_of_block * 4096
    path = tmp_path / "lineitem.tbl"
    with open(path, "wb") as f:
        for _ in range(reps_of_block):
            f.write(block)
    assert os.path.getsize(path) >= 17 << 28
    proj = [4, 10, 8]                                                # l_quantity, l_shipdate, l_returnflag
    scan_bytes = tbl_scan_node(str(path), [str(path)], proj)
    schema = [(LINEITEM[i][0], WIRE_TYPE[LINEITEM[i][1]], False) for i in proj]

    def aggregate(leaf):
        P = tpch.P
        aggs = [E.Sum(E.col("l_quantity"), "sum_qty"), E.Min(E.col("l_shipdate"), "min_ship"), E.Max(E.col("l_shipdate"), "max_ship"),
                E.Count(E.lit(1, E.UINT8), "n")]
        partial = P.HashAggregateExec(P.PARTIAL, [], aggs, leaf)
        final = [E.AggregateExpr(f, E.col(f"{n}[{f.lower()}]"), n) for f, n in (("SUM", "sum_qty"), ("MIN", "min_ship"), ("MAX", "max_ship"), ("COUNT", "n"))]
        return P.HashAggregateExec(P.FINAL, [], final, P.MergeExec(partial))
    data = splice(monkeypatch, aggregate, scan_bytes, schema)
    (tmp_path / "plan.bin").write_bytes(data)
    (tmp_path / "leaf.bin").write_bytes(scan_bytes)
    out = tmp_path / "out.json"
    env = {k: v for k, v in os.environ.items() if k != "BHIP_TEXT_SLAB_MB"}       # the default slab size
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-c", BIG_CHILD, helpers.ROOT, str(tmp_path / "plan.bin"),
                        str(tmp_path / "leaf.bin"), str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.load(open(out))
    n_rows = reps * len(rows)
    print("rows", got["rows"], "batches", got["batches"], "peak", got["peak"], got["cols"])
    assert got["rows"] == n_rows and got["cols"]["n"] == [n_rows]
    default_slab = ba.plan.TEXT_SLAB_DEFAULT
    assert got["batches"] == -(-os.path.getsize(path) // default_slab)
    assert got["cols"]["sum_qty"] == [float(reps * sum(int(r[4]) for r in rows))]
    days = [helpers._days(r[10]) for r in rows]
    assert got["cols"]["min_ship"] == [min(days)] and got["cols"]["max_ship"] == [max(days)]
    # l_quantity 8 bytes, l_shipdate 4, l_returnflag 4 (offset) + 1 (value) per row, + the (n + 1)-th offset of every batch
    projected = n_rows * 17 + 4 * got["batches"]
    assert got["peak"] < projected + 4 * default_slab, (got["peak"], projected)
