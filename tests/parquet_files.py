"""Parquet files at the page, run and NULL edges a default writer never produces — shared by the CPU tier
(test_parquet_decode_cpu.py) and the GPU tier (test_parquet_edges_gpu.py).  No GPU and no library import in here.

a. pages(path, row_group, column): the page headers of one column chunk, so that every case ASSERTS the structure it is
   about (a pyarrow that writes other pages must fail the case, not turn it into a repeat of the older tests);
b. write_hand(...): a minimal writer for files pyarrow cannot produce — one flat column, one PLAIN dictionary page, data pages
   V1 / V2 whose bodies are explicit lists of RLE and bit-packed runs, data-page encoding id 2 or 8, UNCOMPRESSED or SNAPPY
   (a literal-only stream).  Every hand-written file is read back with pyarrow and must hold the intended values;
c. CASES: (name, writer(tmp_dir) -> [paths], kwargs for ParquetExec).

The expected value of every check is pyarrow reading the same file: canonical_text() is that read in the text form
tests/c/parquet_decode_check.cpp prints."""
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq

PLAIN, PLAIN_DICT, RLE_DICT = 0, 2, 8
DATA_V1, DICT_PAGE, DATA_V2 = 0, 2, 3


# ---- a. page-header reader ----------------------------------------------------------------------------------------------------
def _varint(b, p):
    v = s = 0
    while True:
        v |= (b[p] & 0x7F) << s
        s += 7
        p += 1
        if not b[p - 1] & 0x80:
            return v, p


def _zigzag(v):
    return (v >> 1) ^ -(v & 1)


def _value(b, p, ty):
    if ty in (1, 2):
        return ty == 1, p
    if ty == 3:
        return b[p], p + 1
    if ty in (4, 5, 6):
        v, p = _varint(b, p)
        return _zigzag(v), p
    if ty == 7:
        return struct.unpack_from("<d", b, p)[0], p + 8
    if ty == 8:
        n, p = _varint(b, p)
        return bytes(b[p:p + n]), p + n
    if ty in (9, 10):
        n, et = b[p] >> 4, b[p] & 15
        p += 1
        if n == 15:
            n, p = _varint(b, p)
        items = []
        for _ in range(n):
            if et in (1, 2):
                v, p = b[p] == 1, p + 1
            else:
                v, p = _value(b, p, et)
            items.append(v)
        return items, p
    if ty == 12:
        return _struct(b, p)
    raise ValueError(f"thrift type {ty}")


def _struct(b, p):
    """one compact-Thrift struct at b[p:] -> ({field id: value}, position behind it)"""
    out, fid = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        if h >> 4:
            fid += h >> 4
        else:
            v, p = _varint(b, p)
            fid = _zigzag(v)
        out[fid], p = _value(b, p, h & 15)


def _count_set(b, n):
    """set values among the first n of an RLE / bit-packed hybrid of width 1 (definition levels of a flat column)"""
    p = out = ones = 0
    while out < n:
        h, p = _varint(b, p)
        if h & 1:
            for byte in b[p:p + (h >> 1)]:
                k = min(8, n - out)
                ones += bin(byte & ((1 << k) - 1)).count("1")
                out += k
            p += h >> 1
        else:
            k = min(h >> 1, n - out)
            ones += k * (b[p] & 1)
            out += k
            p += 1
    return ones


def _inflate(body, size):
    return pa.Codec("snappy").decompress(body, decompressed_size=size).to_pybytes() if size else b""


def pages(path, row_group, column):
    """[(page_type, n_values, encoding, n_nulls_or_None, index_bit_width_or_None)] of one column chunk, dictionary page included
    (n_nulls is None for it; the bit width is None for a page that is not dictionary-encoded)"""
    f = pq.ParquetFile(path)
    cm = f.metadata.row_group(row_group).column(column)
    optional = f.schema.column(column).max_definition_level > 0
    start = cm.data_page_offset
    if cm.dictionary_page_offset and cm.dictionary_page_offset < start:
        start = cm.dictionary_page_offset
    with open(path, "rb") as fh:
        fh.seek(start)
        raw = fh.read(cm.total_compressed_size)
    snappy = cm.compression == "SNAPPY"
    out, p, seen = [], 0, 0
    while seen < cm.num_values:
        h, p = _struct(raw, p)
        body = raw[p:p + h[3]]
        p += h[3]
        if 7 in h:
            out.append((DICT_PAGE, h[7][1], h[7][2], None, None))
            continue
        if 5 in h:
            n, enc, nulls = h[5][1], h[5][2], 0
            if snappy:
                body = _inflate(body, h[2])
            if optional:
                dl = struct.unpack_from("<I", body)[0]
                nulls = n - _count_set(body[4:4 + dl], n)
                body = body[4 + dl:]
        elif 8 in h:
            d = h[8]
            n, nulls, enc = d[1], d[2], d[4]
            levels = d[5] + d.get(6, 0)
            body = body[levels:]
            if snappy and d.get(7, True):
                body = _inflate(body, h[2] - levels)
        else:
            continue
        seen += n
        out.append((h[1], n, enc, nulls, body[0] if enc in (PLAIN_DICT, RLE_DICT) and body else None))
    return out


def data_pages(path, row_group, column):
    return [pg for pg in pages(path, row_group, column) if pg[0] != DICT_PAGE]


# ---- b. the hand-writer -------------------------------------------------------------------------------------------------------
def _uv(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _zv(v):
    return _uv((v << 1) ^ (v >> 63))


BOOL, I32, I64, BIN, LIST, STRUCT = 1, 5, 6, 8, 9, 12


def _tvalue(ty, v):
    if ty == BOOL:
        return b""
    if ty in (I32, I64):
        return _zv(v)
    if ty == BIN:
        return _uv(len(v)) + v
    if ty == STRUCT:
        return _tstruct(v)
    et, items = v                                              # LIST
    head = bytes([(len(items) << 4) | et]) if len(items) < 15 else bytes([0xF0 | et]) + _uv(len(items))
    return head + b"".join(_tvalue(et, x) for x in items)


def _tstruct(fields):
    """[(field id, type, value)] in ascending id order -> compact-Thrift struct"""
    out, last = bytearray(), 0
    for fid, ty, v in fields:
        t = (1 if v else 2) if ty == BOOL else ty
        out += bytes([((fid - last) << 4) | t]) if 0 < fid - last <= 15 else bytes([t]) + _zv(fid)
        out += _tvalue(ty, v)
        last = fid
    return bytes(out) + b"\0"


def rle(value, count, bw):
    return _uv(count << 1) + value.to_bytes((bw + 7) // 8, "little")


def packed(values, bw):
    vals = list(values) + [0] * (-len(values) % 8)             # whole groups of 8
    bits = 0
    for i, v in enumerate(vals):
        bits |= v << (i * bw)
    return _uv((len(vals) // 8) << 1 | 1) + bits.to_bytes(len(vals) * bw // 8, "little")


def snappy_literal(data):
    """a valid Snappy stream with no copy element: varint length + literal chunks"""
    out = bytearray(_uv(len(data)))
    for i in range(0, len(data), 60):
        c = data[i:i + 60]
        out += bytes([(len(c) - 1) << 2]) + c
    return bytes(out)


PHYS = {"INT32": (1, "<i"), "INT64": (2, "<q"), "DOUBLE": (5, "<d"), "BYTE_ARRAY": (6, None)}
ARROW = {"INT32": pa.int32(), "INT64": pa.int64(), "DOUBLE": pa.float64(), "BYTE_ARRAY": pa.string()}


def _plain(phys, values):
    fmt = PHYS[phys][1]
    if fmt:
        return b"".join(struct.pack(fmt, v) for v in values)
    return b"".join(struct.pack("<I", len(v)) + v for v in (s.encode() for s in values))


def _levels(valid, as_packed):
    if as_packed:
        return packed([int(v) for v in valid], 1)
    out, i = b"", 0
    while i < len(valid):
        j = i
        while j < len(valid) and valid[j] == valid[i]:
            j += 1
        out += rle(int(valid[i]), j - i, 1)
        i = j
    return out


def write_hand(path, phys, dictionary, page_list, optional=False, snappy=False, dict_encoding=PLAIN):
    """One flat column `c`.  A page is a dict:
         bw      index bit width
         runs    [("rle", index, count) | ("packed", [indices])] — written exactly as listed
         n_valid values the page takes from its runs (default: all of them; fewer = a clipped last run)
         valid   per-row validity of an OPTIONAL column (default: every row valid); packed_levels=True writes it bit-packed
         v2, enc (RLE_DICT), compressed (True; V2 only: False leaves the values uncompressed inside a SNAPPY chunk)
    Returns the values the file holds; pyarrow must read exactly those."""
    comp = snappy_literal if snappy else (lambda b: b)
    n_rows, expect, enc_ids = 0, [], {dict_encoding, 3}

    def page_header(ptype, usize, csize, sub_id, sub):
        return _tstruct([(1, I32, ptype), (2, I32, usize), (3, I32, csize), (sub_id, STRUCT, sub)])

    dbody = _plain(phys, dictionary)
    blob = page_header(DICT_PAGE, len(dbody), len(comp(dbody)), 7, [(1, I32, len(dictionary)), (2, I32, dict_encoding)]) + comp(dbody)
    usize_total = len(blob) - len(comp(dbody)) + len(dbody)
    data_off = 4 + len(blob)
    for pg in page_list:
        bw, enc = pg["bw"], pg.get("enc", RLE_DICT)
        idx = []
        body = bytes([bw])
        for r in pg["runs"]:
            if r[0] == "rle":
                body += rle(r[1], r[2], bw)
                idx += [r[1]] * r[2]
            else:
                body += packed(r[1], bw)
                idx += list(r[1]) + [0] * (-len(r[1]) % 8)
        n_valid = pg.get("n_valid", sum(r[2] if r[0] == "rle" else len(r[1]) for r in pg["runs"]))
        assert n_valid <= len(idx)
        valid = pg.get("valid") or [True] * n_valid
        assert sum(valid) == n_valid and (optional or all(valid))
        n = len(valid)
        it = iter(idx)
        expect += [dictionary[next(it)] if v else None for v in valid]
        levels = _levels(valid, pg.get("packed_levels", False)) if optional else b""
        enc_ids.add(enc)
        if pg.get("v2"):
            compressed = pg.get("compressed", True)
            cbody = comp(body) if compressed else body
            sub = [(1, I32, n), (2, I32, n - n_valid), (3, I32, n), (4, I32, enc), (5, I32, len(levels)), (6, I32, 0), (7, BOOL, compressed)]
            page = page_header(DATA_V2, len(levels) + len(body), len(levels) + len(cbody), 8, sub) + levels + cbody
            usize_total += len(page) - len(cbody) + len(body)
        else:
            payload = (struct.pack("<I", len(levels)) + levels if optional else b"") + body
            page = page_header(DATA_V1, len(payload), len(comp(payload)), 5, [(1, I32, n), (2, I32, enc), (3, I32, 3), (4, I32, 3)]) + comp(payload)
            usize_total += len(page) - len(comp(payload)) + len(payload)
        blob += page
        n_rows += n
    column = [(1, I32, PHYS[phys][0]), (3, I32, 1 if optional else 0), (4, BIN, b"c")] + ([(6, I32, 0)] if phys == "BYTE_ARRAY" else [])
    meta = [(1, I32, PHYS[phys][0]), (2, LIST, (I32, sorted(enc_ids))), (3, LIST, (BIN, [b"c"])), (4, I32, 1 if snappy else 0), (5, I64, n_rows),
            (6, I64, usize_total), (7, I64, len(blob)), (9, I64, data_off), (11, I64, 4)]
    group = [(1, LIST, (STRUCT, [[(2, I64, 4), (3, STRUCT, meta)]])), (2, I64, usize_total), (3, I64, n_rows)]
    footer = _tstruct([(1, I32, 1), (2, LIST, (STRUCT, [[(4, BIN, b"schema"), (5, I32, 1)], column])), (3, I64, n_rows), (4, LIST, (STRUCT, [group])),
                       (6, BIN, b"tests/parquet_files.py")])
    with open(path, "wb") as f:
        f.write(b"PAR1" + blob + footer + struct.pack("<I", len(footer)) + b"PAR1")
    got = pq.read_table(path).column("c")
    assert got.type == ARROW[phys] and got.to_pylist() == expect, f"{path}: pyarrow does not read what was written"
    return expect


# ---- the text both tiers compare ----------------------------------------------------------------------------------------------
def canonical_text(paths):
    """what tests/c/parquet_decode_check.cpp prints for `paths`, from pyarrow's read of them"""
    out = []
    for path in paths:
        f = pq.ParquetFile(path)
        for g in range(f.metadata.num_row_groups):
            t = f.read_row_group(g)
            if t.num_rows == 0:
                continue
            for name in t.schema.names:
                a = t[name].combine_chunks()
                out.append(f"# {os.path.basename(path)} group {g} column {name} rows {len(a)}")
                ty = a.type
                valid = a.is_valid().to_numpy(zero_copy_only=False)
                if pa.types.is_string(ty) or pa.types.is_binary(ty):
                    vals = [v.hex() if v is not None else None for v in a.cast(pa.binary()).to_pylist()]
                elif pa.types.is_boolean(ty):
                    vals = [None if v is None else str(int(v)) for v in a.to_pylist()]
                else:
                    if pa.types.is_floating(ty) or pa.types.is_temporal(ty):
                        a = a.view({4: pa.uint32() if pa.types.is_floating(ty) else pa.int32(), 8: pa.uint64() if pa.types.is_floating(ty) else pa.int64()}[ty.bit_width // 8])
                    raw = pc.fill_null(a, 0).to_numpy(zero_copy_only=False)
                    if pa.types.is_floating(ty):
                        vals = [format(int(v), "08x" if ty.bit_width == 32 else "016x") for v in raw]
                    else:
                        vals = [str(int(v)) for v in raw]
                out += [v if ok else "NULL" for v, ok in zip(vals, valid)]
    return "\n".join(out) + "\n"


# ---- c. the cases -------------------------------------------------------------------------------------------------------------
def _masked(values, ty, mask):
    return pa.array(values, type=ty, mask=mask)


def mixed_table(n, null_frac, seed, nullable=True):
    """every column type the scan supports; `low` and `s` of low cardinality, `u` and `f64` unique values (their dictionaries overflow
    a small dictionary_pagesize_limit in the middle of the chunk)"""
    rng = np.random.default_rng(seed)

    def m():
        return (rng.random(n) < null_frac) if null_frac else None
    words = ["", "a", "MAIL", "SHIP", "REG AIR", "a longer string with spaces", "é日本"]
    cols = [("low", pa.int32(), rng.integers(0, 7, n).astype(np.int32)),
            ("i64", pa.int64(), rng.integers(-2 ** 62, 2 ** 62, n)),
            ("f64", pa.float64(), rng.random(n) * 1e5),
            ("f32", pa.float32(), rng.normal(0, 100, n).astype(np.float32)),
            ("b", pa.bool_(), rng.random(n) > 0.5),
            ("d32", pa.date32(), rng.integers(8000, 11000, n).astype(np.int32)),
            ("tus", pa.timestamp("us"), rng.integers(0, 2 ** 51, n)),
            ("i8", pa.int8(), rng.integers(-128, 128, n).astype(np.int8)),
            ("u16", pa.uint16(), rng.integers(0, 2 ** 16, n).astype(np.uint16)),
            ("s", pa.string(), [words[k] for k in rng.integers(0, len(words), n)]),
            ("u", pa.string(), [f"unique-{i}-{'z' * int(k)}" for i, k in enumerate(rng.integers(0, 9, n))])]
    if not nullable:                                           # required_fields: the remaining supported types as well
        cols += [("tms", pa.timestamp("ms"), rng.integers(0, 2 ** 41, n)),
                 ("u8", pa.uint8(), rng.integers(0, 256, n).astype(np.uint8)),
                 ("i16", pa.int16(), rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16)),
                 ("u32", pa.uint32(), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)),
                 ("u64", pa.uint64(), rng.integers(0, 2 ** 63, n, dtype=np.uint64) * 2 + 1)]
    arrays = [_masked(list(v) if isinstance(v, list) else v, ty, m()) for _, ty, v in cols]
    return pa.Table.from_arrays(arrays, schema=pa.schema([pa.field(name, ty, nullable) for name, ty, _ in cols]))


def _chunks(path):
    md = pq.ParquetFile(path).metadata
    return [(g, c, md.schema.column(c).name) for g in range(md.num_row_groups) for c in range(md.num_columns)]


def unaligned_pages(version, compression, dictionary, null_frac):
    def write(d):
        path = os.path.join(d, "unaligned.parquet")
        pq.write_table(mixed_table(3000, null_frac, 7), path, write_batch_size=37, data_page_size=64, row_group_size=1500, dictionary_pagesize_limit=300,
                       data_page_version=version, compression=compression, use_dictionary=dictionary)
        for g, c, name in _chunks(path):
            pgs = data_pages(path, g, c)
            if name == "b":                                    # Boolean pages do get concatenated; V1 closes them far less often
                assert len(pgs) >= (2 if version == "2.0" or null_frac else 3), (name, len(pgs))
                continue
            assert len(pgs) >= 20, (name, len(pgs))
            assert any(pg[1] % 64 for pg in pgs[:-1]), name
            if dictionary and name in ("u", "f64"):
                encs = {pg[2] for pg in pgs}
                assert PLAIN in encs and encs & {PLAIN_DICT, RLE_DICT}, (name, encs)
        return [path]
    return write


def one_row_pages(version):
    def write(d):
        path = os.path.join(d, "one_row.parquet")
        pq.write_table(mixed_table(200, 0.5, 11), path, write_batch_size=1, data_page_size=1, data_page_version=version)
        for g, c, name in _chunks(path):
            pgs = data_pages(path, g, c)
            if not (name == "b" and version == "1.0"):         # (a PLAIN Boolean page of V1 is not closed while it holds NULLs alone)
                assert any(pg[1] == pg[3] for pg in pgs), name                # a page with 0 valid values
            assert any(pg[1] == 1 and pg[3] == 0 for pg in pgs), name         # one row, one valid value
        return [path]
    return write


WORD_ROWS = 256
NULL_PATTERNS = {"first": [0], "last": [WORD_ROWS - 1], "straddle": [63, 64], "lastpage": [WORD_ROWS - 20],
                 "all_but_one": [i for i in range(WORD_ROWS) if i != 100]}


def word_boundaries(page_rows, dictionary):
    def write(d):
        path = os.path.join(d, f"words{page_rows}.parquet")
        cols = {}
        for pat, rows in NULL_PATTERNS.items():
            mask = np.zeros(WORD_ROWS, bool)
            mask[rows] = True
            cols["l_" + pat] = pa.array(np.arange(WORD_ROWS) * 10 ** 10 + 1, pa.int64(), mask=mask)
            cols["s_" + pat] = pa.array([f"row-{i:04d}" for i in range(WORD_ROWS)], pa.string(), mask=mask)
            cols["b_" + pat] = pa.array((np.arange(WORD_ROWS) % 3 == 0), pa.bool_(), mask=mask)
        pq.write_table(pa.table(cols), path, write_batch_size=page_rows, data_page_size=1, use_dictionary=dictionary, data_page_version="2.0")
        for g, c, name in _chunks(path):
            rows = [pg[1] for pg in data_pages(path, g, c)]
            if name.endswith("all_but_one") and not dictionary:    # a PLAIN page of NULLs alone holds no byte and is not closed: whole batches still
                assert len(rows) > 1 and all(r % page_rows == 0 for r in rows), (name, rows)
            else:
                assert rows == [page_rows] * (WORD_ROWS // page_rows), (name, rows)
        return [path]
    return write


def required_fields(version, dictionary):
    def write(d):
        path = os.path.join(d, "required.parquet")
        pq.write_table(mixed_table(500, 0, 3, nullable=False), path, write_batch_size=37, data_page_size=64, dictionary_pagesize_limit=300,
                       data_page_version=version, use_dictionary=dictionary)
        f = pq.ParquetFile(path)
        for g, c, name in _chunks(path):
            assert f.schema.column(c).max_definition_level == 0, name
            assert name == "b" or len(data_pages(path, g, c)) > 1, name
        return [path]
    return write


def all_null(dictionary):
    def write(d):
        path = os.path.join(d, "all_null.parquet")
        t = pa.table({"l": pa.array([None] * 100 + list(range(100)), pa.int64()), "s": pa.array([None] * 100 + [f"v{i % 9}" for i in range(100)], pa.string())})
        pq.write_table(t, path, row_group_size=100, use_dictionary=dictionary)
        for c in (0, 1):
            pgs = pages(path, 0, c)
            assert all(pg[1] == pg[3] for pg in pgs if pg[0] != DICT_PAGE)
            if dictionary:
                assert pgs[0][0] == DICT_PAGE and pgs[0][1] == 0, pgs
        return [path]
    return write


def wide_dictionary(d):
    path = os.path.join(d, "wide.parquet")
    rng = np.random.default_rng(19)
    n = 300_000
    strings = np.array([f"s{k:05d}" for k in range(70_000)], dtype=object)
    t = pa.table({"perm": pa.array(rng.permutation(n).astype(np.int32)),
                  "s": pa.array(strings[rng.integers(0, len(strings), n)], pa.string(), mask=rng.random(n) < 0.2)})
    pq.write_table(t, path, dictionary_pagesize_limit=1 << 26, data_page_size=1 << 16)
    pgs = data_pages(path, 0, 0)
    assert len(pgs) > 1 and all(pg[2] in (PLAIN_DICT, RLE_DICT) for pg in pgs) and pgs[-1][4] == 19, pgs
    assert all(pg[2] in (PLAIN_DICT, RLE_DICT) for pg in data_pages(path, 0, 1))
    return [path]


F64_BITS = [0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001, 0x7FF80000DEADBEEF, 0xFFF8000000000005,
            0x0000000000000001, 0x8000000000000001, 0x3FF8000000000000]
F32_BITS = [0x0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7FC0BEEF, 0xFFC00005, 0x00000001, 0x80000001, 0x3FC00000]


def float_bits(dictionary):
    def write(d):
        path = os.path.join(d, "float_bits.parquet")
        rng = np.random.default_rng(2)
        n = 300
        f64 = np.array(F64_BITS, np.uint64)[rng.integers(0, len(F64_BITS), n)].view(np.float64)
        f32 = np.array(F32_BITS, np.uint32)[rng.integers(0, len(F32_BITS), n)].view(np.float32)
        mask = rng.random(n) < 0.2
        t = pa.table({"f64": pa.array(f64), "f32": pa.array(f32), "f64n": pa.array(f64, mask=mask), "f32n": pa.array(f32, mask=mask)})
        pq.write_table(t, path, use_dictionary=dictionary, write_batch_size=37, data_page_size=64)
        return [path]
    return write


def string_sizes(dictionary, nulls):
    def write(d):
        path = os.path.join(d, "strings.parquet")
        short = ["", "a", "seven77", "eight888", "nine99999"]
        long_ = ["L" * 300, "M" * 3000, "n" * 299 + "é"]
        vals = []
        for block in range(6):                                 # 64-row groups: short ones total < 2,048 bytes, the others far more
            for i in range(64):
                vals.append(short[(i + block) % 5] if block % 2 == 0 else (long_[i % 3] if i % 4 == 0 else short[i % 5]))
        vals += ["tail", "M" * 3000, ""]                       # a last, partial group of 64
        mask = (np.arange(len(vals)) % 5 == 2) if nulls else None
        pq.write_table(pa.table({"s": pa.array(vals, pa.string(), mask=mask)}), path, use_dictionary=dictionary, write_batch_size=50, data_page_size=4096)
        encs = {pg[2] for pg in data_pages(path, 0, 0)}
        assert encs == ({RLE_DICT} if dictionary else {PLAIN}), encs
        return [path]
    return write


def five_files(d):
    paths = []
    for i, n in enumerate([700, 1001, 0, 300, 450]):
        rng = np.random.default_rng(40 + i)
        mask = (rng.random(n) < 0.3) if i in (1, 4) else None  # `x` has NULLs in two of the files only
        t = pa.table({"x": pa.array(rng.integers(0, 50, n), pa.int64(), mask=mask), "s": pa.array([f"f{i}-{k % 11}" for k in range(n)], pa.string()),
                      "f": pa.array(rng.random(n))})
        paths.append(os.path.join(d, f"part-{i}.parquet"))
        pq.write_table(t, paths[-1], row_group_size=1000 if i == 1 else 256)   # file 1: a 1-row row group behind 1,000 rows
    assert pq.ParquetFile(paths[2]).metadata.num_rows == 0
    md = pq.ParquetFile(paths[1]).metadata
    assert md.row_group(md.num_row_groups - 1).num_rows == 1
    return paths


# ---- hand-written ----
INTS = [100, -7, 2 ** 31 - 1, -2 ** 31, 42]
WIDTHS = [1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32]


def _some_nulls(n_valid, every=4):
    """validity with n_valid set rows and a NULL in front of every `every`-th of them"""
    out = []
    for k in range(n_valid):
        if k % every == 1:
            out.append(False)
        out.append(True)
    return out + [False]


def hand_widths(optional):
    def write(d):
        paths = []
        big = list(range(-5, 65_536))                          # 65,541 entries: indices that need a 17th bit
        for bw in WIDTHS:
            top = min(len(INTS), 1 << bw)
            a, b = [(3 * i + 1) % top for i in range(16)], [(i * 2) % top for i in range(8)]
            if bw % 2:
                assert {(i * bw) & 7 for i in range(16)} == set(range(8))    # a value starts at every bit offset of a byte
            pg = dict(bw=bw, runs=[("packed", a), ("rle", top - 1, 5), ("packed", b), ("rle", 0, 1)])
            if optional:
                pg["valid"] = _some_nulls(30)
            paths.append(os.path.join(d, f"width{bw:02d}.parquet"))
            write_hand(paths[-1], "INT32", INTS, [pg], optional=optional)
            assert pages(paths[-1], 0, 0)[1][4] == bw
        for bw in (17, 24, 25, 31, 32):                        # index values above 2^16: the upper bits of the mask, 3 value bytes of an RLE run
            hi = [65_540 - 7 * i for i in range(16)]
            pg = dict(bw=bw, runs=[("rle", 65_540, 3), ("packed", hi), ("rle", 65_536, 2), ("packed", hi[:8])])
            if optional:
                pg["valid"] = _some_nulls(29, 3)
            paths.append(os.path.join(d, f"wide{bw:02d}.parquet"))
            write_hand(paths[-1], "INT32", big, [pg], optional=optional)
        return paths
    return write


def hand_rle_bytes(optional):
    """RLE runs whose value takes 1, 2, 3 and 4 bytes (widths 8, 16, 24, 32), with the second value byte in use (a 300-entry dictionary);
    hand_widths has the third.  A non-zero fourth byte would need a dictionary of 2^24 entries."""
    def write(d):
        words = [f"w{i}" for i in range(300)]
        paths = []
        for bw in (8, 16, 24, 32):
            v = 299 if bw > 8 else 255
            pg = dict(bw=bw, runs=[("rle", v, 9), ("rle", 256 if bw > 8 else 1, 70), ("rle", 7, 1)])
            if optional:
                pg["valid"] = _some_nulls(80, 7)
            paths.append(os.path.join(d, f"rle{bw}.parquet"))
            write_hand(paths[-1], "BYTE_ARRAY", words, [pg], optional=optional)
        return paths
    return write


RUN_MIX = dict(bw=3, runs=[("packed", [0, 1, 2, 3, 4, 3, 2, 1]), ("rle", 4, 3), ("packed", [4, 4, 0, 0, 1, 2, 3, 4, 1, 1, 1, 1, 2, 2, 2, 2]), ("rle", 2, 1),
                           ("packed", [3, 0, 3, 0, 3, 0, 3, 0]), ("rle", 0, 130), ("rle", 1, 1), ("packed", [1, 2, 3, 4, 0, 1, 2, 3])])


def hand_run_mix(optional, name="run_mix.parquet"):
    def write(d):
        path = os.path.join(d, name)
        pg = dict(RUN_MIX)
        if optional:
            pg["valid"] = _some_nulls(175, 5)
        write_hand(path, "BYTE_ARRAY", ["", "a", "bc", "def", "é日本"], [pg], optional=optional)
        return [path]
    return write


def hand_clipped(optional):
    def write(d):
        path = os.path.join(d, "clipped.parquet")
        p1 = dict(bw=5, runs=[("packed", list(range(16)))], n_valid=13)                       # 5 of the last group's 8 values are needed
        p2 = dict(bw=5, runs=[("rle", 17, 100)], n_valid=10)                                  # an RLE count beyond the page
        p3 = dict(bw=5, runs=[("packed", [19, 18, 17, 16, 15, 14, 13, 12]), ("rle", 3, 1000)], n_valid=20, v2=True)
        p4 = dict(bw=12, runs=[("rle", 1, 2), ("packed", [9, 8, 7, 6, 5, 4, 3, 2])], n_valid=3)  # one value of a whole group
        pgs = [p1, p2, p3, p4]
        if optional:
            for pg in pgs:
                pg["valid"] = _some_nulls(pg["n_valid"], 3)
        write_hand(path, "INT64", [10 ** 12 + i for i in range(20)], pgs, optional=optional)
        return [path]
    return write


def hand_staging(optional):
    """three pages of one NULL-free chunk at widths 1, 9 and 20: the staged-dictionary route (each run carries its width, offsets re-based)"""
    def write(d):
        path = os.path.join(d, "staging.parquet")
        pgs = [dict(bw=1, runs=[("packed", [1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1]), ("rle", 1, 4)], n_valid=15),
               dict(bw=9, runs=[("rle", 299, 2), ("packed", [299 - 13 * i for i in range(16)]), ("rle", 256, 3)]),
               dict(bw=20, runs=[("packed", [7 * i for i in range(24)]), ("rle", 298, 6), ("packed", [255, 256, 257])], n_valid=33, v2=True)]
        write_hand(path, "DOUBLE", [i / 8 - 3 for i in range(300)], pgs, optional=optional)
        return [path]
    return write


def hand_legacy(optional):
    def write(d):
        paths = [os.path.join(d, "legacy_s.parquet"), os.path.join(d, "legacy_i.parquet")]
        pg = dict(RUN_MIX, enc=PLAIN_DICT)
        pg2 = dict(bw=2, runs=[("rle", 3, 40), ("packed", [0, 1, 2, 3] * 4)], enc=PLAIN_DICT)
        if optional:
            pg["valid"], pg2["valid"] = _some_nulls(175, 6), _some_nulls(56, 2)
        write_hand(paths[0], "BYTE_ARRAY", ["", "a", "bc", "def", "é日本"], [pg, pg2], optional=optional, dict_encoding=PLAIN_DICT)
        write_hand(paths[1], "BYTE_ARRAY", ["p", "q", "rs", "t" * 9], [pg2, pg2], optional=optional, dict_encoding=PLAIN_DICT, snappy=True)
        assert [p[2] for p in pages(paths[0], 0, 0)] == [PLAIN_DICT] * 3
        return paths
    return write


def hand_v2_uncompressed(optional):
    def write(d):
        path = os.path.join(d, "v2_uncompressed.parquet")
        pgs = [dict(bw=4, runs=[("packed", list(range(16))), ("rle", 9, 30)], v2=True, compressed=False),
               dict(bw=4, runs=[("rle", 2, 11), ("packed", [15 - i for i in range(16)])], v2=True, compressed=True),
               dict(bw=6, runs=[("packed", [3 * i for i in range(8)]), ("rle", 19, 1)], v2=True, compressed=False)]
        if optional:
            for k, pg in enumerate(pgs):
                pg["valid"] = _some_nulls(sum(r[2] if r[0] == "rle" else len(r[1]) for r in pg["runs"]), 3 + k)
        write_hand(path, "INT64", [-(10 ** 15) + 3 * i for i in range(24)], pgs, optional=optional, snappy=True)
        return [path]
    return write


def hand_packed_levels(d):
    """bit-packed definition levels over a page of 70 rows (9 groups of levels, the last cut by the row count), V1 and V2"""
    path = os.path.join(d, "packed_levels.parquet")
    valid = [i % 3 != 1 and i != 64 for i in range(70)]
    nv = sum(valid)
    pgs = [dict(bw=3, runs=[("packed", [i % 5 for i in range(nv)])], valid=valid, packed_levels=True),
           dict(bw=3, runs=[("rle", 4, nv)], valid=valid[::-1], packed_levels=True, v2=True)]
    write_hand(path, "BYTE_ARRAY", ["", "a", "bc", "def", "é日本"], pgs, optional=True)
    return [path]


CASES = []
for _v in ("1.0", "2.0"):
    for _c in ("NONE", "SNAPPY"):
        for _d in (True, False):
            for _nf in (0.3, 0):
                CASES.append((f"unaligned_pages-v{_v[0]}-{_c.lower()}-{'dict' if _d else 'plain'}-{'nulls' if _nf else 'nonull'}", unaligned_pages(_v, _c, _d, _nf), {}))
CASES += [(f"one_row_pages-v{_v[0]}", one_row_pages(_v), {}) for _v in ("1.0", "2.0")]
CASES += [(f"word_boundaries-{_n}-{'dict' if _d else 'plain'}", word_boundaries(_n, _d), {}) for _n in (64, 128) for _d in (True, False)]
CASES += [(f"required_fields-v{_v[0]}-{'dict' if _d else 'plain'}", required_fields(_v, _d), {}) for _v in ("1.0", "2.0") for _d in (True, False)]
CASES += [(f"all_null-{'dict' if _d else 'plain'}", all_null(_d), {}) for _d in (True, False)]
CASES += [("wide_dictionary", wide_dictionary, {})]
CASES += [(f"float_bits-{'dict' if _d else 'plain'}", float_bits(_d), {}) for _d in (True, False)]
CASES += [(f"string_sizes-{'dict' if _d else 'plain'}-{'nulls' if _n else 'nonull'}", string_sizes(_d, _n), {}) for _d in (True, False) for _n in (True, False)]
CASES += [(f"files_and_partitions-{_p}", five_files, dict(num_partitions=_p, projection=[2, 0, 1])) for _p in (1, 2, 7)]
for _o in (False, True):
    _s = "optional" if _o else "required"
    CASES += [(f"hand_widths-{_s}", hand_widths(_o), {}), (f"hand_rle_bytes-{_s}", hand_rle_bytes(_o), {}), (f"hand_run_mix-{_s}", hand_run_mix(_o), {}),
              (f"hand_clipped-{_s}", hand_clipped(_o), {}), (f"hand_staging-{_s}", hand_staging(_o), {}), (f"hand_legacy-{_s}", hand_legacy(_o), {}),
              (f"hand_v2_uncompressed-{_s}", hand_v2_uncompressed(_o), {})]
CASES += [("hand_packed_levels", hand_packed_levels, {})]
CASE_IDS = [c[0] for c in CASES]

# which cases feed the checks below the Arrow export (COUNT / IS NOT NULL) and the page-at-a-time child process of the GPU tier
VALIDITY_CASES = [c for c in CASES if c[0].split("-")[0] in ("unaligned_pages", "one_row_pages", "word_boundaries", "all_null") and "nonull" not in c[0]]
PER_PAGE_CASES = [c for c in CASES if (c[0].startswith("unaligned_pages") and "nonull" in c[0]) or c[0].startswith("required_fields") or c[0].startswith("hand_staging")]
