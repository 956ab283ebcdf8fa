"""Columns as a caller may hand them to bhip_batch_from_device: every Arrow buffer of a batch laid into one byte arena at a chosen
residue of its address mod 16, in exactly its Arrow size (bitmaps: whole 64-bit words, what the library reads), with nothing but
poison around it.

A kernel that lets a byte beyond a column's end into a result gives different answers over the 0x00 and the 0xFF arena; a
dispatch that sends an unaligned column to a wide-load kernel shows in the route the library reports.  MARGIN bytes of poison lie
before the first buffer, between any two and after the last: a condition, not a measurement — no over-read of a few bytes leaves
the allocation, so these inputs cannot fault.

arena() and decode() are pure numpy (test_offset_columns_cpu.py); borrow() needs a device."""
from collections import OrderedDict

import numpy as np

from oracle.engine import NP_TYPES, OCol, batch_len

MARGIN = 256
ROLES = ("data", "offsets", "validity")

# bytes past a 16-byte boundary at which the GPU tier places buffers, by the width of what they hold
SHIFTS_8 = (0, 8)
SHIFTS_4 = (0, 4, 8, 12)               # 4-byte values and Utf8 offsets
SHIFTS_2 = (0, 2, 14)
SHIFTS_1 = (0, 1, 15)                  # 1-byte values and Utf8 bytes
SHIFTS_BITMAP = (0, 8)


def shift_of(shifts, name, role):
    """shifts: {(column, role): s} before {column: s} (its data buffer only) before {role: s}; 0 where nothing is said"""
    if (name, role) in shifts:
        return shifts[(name, role)]
    if role == "data" and name in shifts:
        return shifts[name]
    return shifts.get(role, 0)


def bitmap_words(bits, tail_bits):
    """a bool array as an Arrow bitmap (least significant bit first) of whole 64-bit words; the bits past its length are tail_bits"""
    n = len(bits)
    padded = np.full((n + 63) // 64 * 64, bool(tail_bits))
    padded[:n] = bits
    return np.packbits(padded, bitorder="little")


def column_buffers(c: OCol, tail_bits=0):
    """{role: bytes as a uint8 array} of one oracle column, each in its Arrow size"""
    out = OrderedDict()
    if c.dtype == "Utf8":
        enc = [s.encode() for s in c.values]
        off = np.zeros(len(enc) + 1, np.int32)
        off[1:] = np.cumsum([len(b) for b in enc])
        out["data"] = np.frombuffer(b"".join(enc), np.uint8)
        out["offsets"] = off.view(np.uint8)
    elif c.dtype == "Boolean":
        out["data"] = bitmap_words(c.values, tail_bits)
    else:
        out["data"] = np.ascontiguousarray(c.values, NP_TYPES[c.dtype]).view(np.uint8)
    if c.valid is not None:
        out["validity"] = bitmap_words(c.valid, tail_bits)
    return out


def arena(batch, shifts, poison, tail_bits=0, base=0):
    """-> (uint8 array, {column: {role: (byte offset, byte length)}}).  Byte `offset` of the array will live at an address that is
    base + offset (mod 16): each buffer starts where that is its shift."""
    assert poison in (0x00, 0xFF) and tail_bits in (0, 1)
    placed, layout, at = [], OrderedDict(), MARGIN
    for name, c in batch.items():
        layout[name] = {}
        for role, raw in column_buffers(c, tail_bits).items():
            s = shift_of(shifts, name, role)
            assert 0 <= s < 16
            at += (s - base - at) % 16
            placed.append((at, raw))
            layout[name][role] = (at, len(raw))
            at += len(raw) + MARGIN
    out = np.full(at, poison, np.uint8)
    for off, raw in placed:
        out[off:off + len(raw)] = raw
    return out, layout


def decode(arr, layout, schema, n):
    """the batch an arena holds: schema = [(name, dtype)], n rows"""
    out = OrderedDict()
    for name, dtype in schema:
        where = layout[name]
        piece = lambda role: arr[where[role][0]:where[role][0] + where[role][1]]
        valid = np.unpackbits(piece("validity"), bitorder="little")[:n].astype(bool) if "validity" in where else None
        if dtype == "Utf8":
            off = piece("offsets").copy().view(np.int32)
            raw = piece("data").tobytes()
            values = [raw[off[i]:off[i + 1]].decode() for i in range(n)]
        elif dtype == "Boolean":
            values = np.unpackbits(piece("data"), bitorder="little")[:n].astype(bool)
        else:
            values = piece("data").copy().view(NP_TYPES[dtype])
        out[name] = OCol(dtype, values, valid)
    return out


def buffer_mask(arr, layout):
    """True at every byte of the arena that belongs to a buffer"""
    m = np.zeros(len(arr), bool)
    for where in layout.values():
        for off, size in where.values():
            m[off:off + size] = True
    return m


# ---- partition slices: the scatter route of a hash repartition hands out columns that start first[p] * width bytes into a buffer ---------

SLICE_ROWS, SLICE_PARTS = 1500, 3


def slice_table(seed):
    """fixed-width and NULL-free, one Int32 key: the input the scatter route takes.  About three quarters of the rows carry a key of
    partition 2, so that this slice is a batch of more than 1024 rows: beyond the plain sort of small batches, where a limit over a
    sort selects"""
    import repartition_cases as rc
    rng = np.random.default_rng(seed)
    n = SLICE_ROWS
    keys = np.arange(-500, 500)
    pid = rc.pid_of_ints(keys.astype(np.int64).view(np.uint64), SLICE_PARTS)
    want = rng.choice(SLICE_PARTS, n, p=[0.1, 0.15, 0.75])
    k = np.array([rng.choice(keys[pid == p]) for p in want])
    return OrderedDict([("k", OCol("Int32", k)),
                        ("i8", OCol("Int8", np.concatenate([rng.integers(-128, 128, n - 2), [-128, 127]]))),
                        ("i16", OCol("Int16", np.concatenate([rng.integers(-2 ** 15, 2 ** 15, n - 2), [-2 ** 15, 2 ** 15 - 1]]))),
                        ("f32", OCol("Float32", rng.normal(0, 100, n).astype(np.float32))),
                        ("f64", OCol("Float64", np.round(rng.uniform(0.0, 0.11, n), 2))),
                        ("d", OCol("Date32", rng.integers(8500, 10500, n))),
                        ("p", OCol("Int32", np.arange(n)))])


def slice_first(table):
    """first row of every partition within the scattered columns, from the oracle's restated row hash"""
    import repartition_cases as rc
    from ballista_amd.expr import col
    pid = rc.restated_pid(table, [col("k")], SLICE_PARTS)
    return np.concatenate([[0], np.cumsum(np.bincount(pid, minlength=SLICE_PARTS))])


def slice_seed():
    """the first seed whose partitions 1 and 2 start at an odd row — an odd address for 1-byte values, 8 mod 16 for 8-byte ones, 4 or
    12 mod 16 for 4-byte ones — and whose partition 2 holds more than 1024 rows"""
    for seed in range(1000):
        first = slice_first(slice_table(seed))
        if first[1] % 2 == 1 and first[2] % 2 == 1 and first[3] - first[2] > 1024:
            return seed
    raise AssertionError("no seed found")


# ---- the device side ------------------------------------------------------------------------------------------------------------------

def upload(ctx, batch, shifts, poison, tail_bits=0):
    """the arena as an owning one-column UInt8 batch -> (that batch, its device address, layout).  The allocator's blocks start on
    256 bytes; were one not to, the arena is laid out again for the residue its address has"""
    import ballista_amd as ba
    base = 0
    for _ in range(2):
        arr, layout = arena(batch, shifts, poison, tail_bits, base)
        own = ba.RecordBatch.from_columns(ctx, [("arena", "UInt8", arr, None)])
        addr = own.column_device(0)[0]
        if addr % 16 == base:
            return own, addr, layout
        base = addr % 16
    raise AssertionError("the arena's address changes its residue mod 16 from one upload to the next")


def borrow_batch(ctx, batch, shifts, poison, tail_bits=0):
    """the device RecordBatch that borrows `batch`'s buffers out of an uploaded arena (which it keeps alive)"""
    import ctypes as C
    import ballista_amd as ba
    from ballista_amd import _lib as L
    from ballista_amd.plan import DTYPE_ID
    own, addr, layout = upload(ctx, batch, shifts, poison, tail_bits)
    n = batch_len(batch)
    for name, where in layout.items():
        for role, (off, _) in where.items():
            assert (addr + off) % 16 == shift_of(shifts, name, role), (name, role)
    if batch and all(c.dtype not in ("Utf8", "Boolean") and c.valid is None for c in batch.values()):
        cols = [(name, c.dtype, addr + layout[name]["data"][0]) for name, c in batch.items()]
        return ba.RecordBatch.from_device_pointers(ctx, cols, n, keep=own)
    descs, keep = [], []
    for name, c in batch.items():
        where = layout[name]
        at = lambda role: addr + where[role][0] if role in where else None
        d = L.ColumnDesc()
        nb = name.encode()
        keep.append(nb)
        d.name, d.dtype, d.nullable = nb, DTYPE_ID[c.dtype], 1 if c.valid is not None else 0
        d.data, d.offsets, d.validity = at("data"), at("offsets"), at("validity")
        d.data_bytes = where["data"][1] if c.dtype == "Utf8" else 0
        descs.append(d)
    arr = (L.ColumnDesc * max(1, len(descs)))(*descs)
    h = C.c_void_p()
    L.check(L.lib().bhip_batch_from_device(ctx._h, len(descs), arr, n, C.byref(h)))
    rb = ba.RecordBatch(h, ctx)
    rb._owner = own
    return rb


def borrow(ctx, batch, shifts, poison, tail_bits=0):
    """a one-partition MemoryExec over the borrowed batch; the oracle evaluates plans above it over `batch` itself"""
    import ballista_amd as ba
    src = ba.MemoryExec([[borrow_batch(ctx, batch, shifts, poison, tail_bits)]], ctx)
    src._oracle_partitions = [[batch]]
    return src
