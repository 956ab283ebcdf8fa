"""TEST INFRASTRUCTURE shared by test_wide_agg_cases_cpu.py (no GPU) and test_wide_agg_edges_gpu.py: the inputs of the tests of
HashAggregateExec's wide-key route (host/ops_agg_wide.cpp run_wide, kernels_hash.hip wide_key_assign_kernel / wide_keys_equal) and a
SECOND statement of what that route computes.

Nothing here touches a device.  A case is (name, partitions of batches, group expressions, aggregates, facts); `facts` holds what the
case claims of itself — "wide": the route it must take (True: wide_key_assign runs, False: it does not, None: not asserted),
"n_groups", and per family the slots, capacities and boundary lengths — and test_wide_agg_cases_cpu.py proves each claim.

The route, restated (`group_by_representatives`): every row has a 64-bit row hash (repartition_cases.restated_hash, which the
repartitioning tests have checked against the device), its slot is mix64(hash) & (capacity - 1) with capacity =
join_route_cases.table_capacity(rows), and walking the rows in order each one probes linearly from its slot, wrapping at the table's
end, and takes the first occupant whose key is EQUAL as its representative, or the first empty slot for itself.  Equality is pluggable:
RIGHT is wide_keys_equal's (validity first; then Utf8 by length and bytes, Boolean by value, everything else by bits — a float by the
bits of the double it equals), and WRONG names the mistakes the cases are built against.  A case discriminates when a wrong equality
changes its number of groups."""
import functools
import itertools
import math
import os
import re
from collections import OrderedDict, namedtuple

import numpy as np

from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og
from oracle.engine import OCol

import join_route_cases as RC
import repartition_cases as RP

ROOT = RC.ROOT
Case = namedtuple("Case", "name partitions group aggs facts")
NULL_BITS = RP.NULL_BITS
LONG = "a partner column of forty bytes in all.."          # 40 bytes: no share of the packed key holds it
assert len(LONG.encode()) == 40


def fn(name, *args):
    return E.ScalarFunctionExpr(name, list(args))


def keys_of(case):
    return [n for _, n in case.group]


def table_of(case):
    """every row of the case as one batch"""
    live = [b for part in case.partitions for b in part if og.batch_len(b)]
    return og.concat_batches(live) if live else case.partitions[0][0]


def n_rows(case):
    return sum(og.batch_len(b) for part in case.partitions for b in part)


def cut(batch, rows):
    at = np.concatenate([[0], np.cumsum(rows)])
    assert at[-1] == og.batch_len(batch)
    return [OrderedDict((k, c.take(np.arange(int(a), int(b)))) for k, c in batch.items()) for a, b in zip(at, at[1:])]


# ---- columns -----------------------------------------------------------------------------------------------------------------------------

FLOAT_BITS = {"Float64": np.uint64, "Float32": np.uint32}


def column(dtype, vals):
    """a column from Python values, None = NULL (stored as 0 / "" / False).  A float is given by its BIT PATTERN, so that a NaN's
    payload and a zero's sign arrive as written"""
    valid = [v is not None for v in vals]
    if dtype == "Utf8":
        return OCol(dtype, ["" if v is None else v for v in vals], valid)
    if dtype == "Boolean":
        return OCol(dtype, np.array([bool(v) for v in vals], np.bool_), valid)
    if dtype in FLOAT_BITS:
        bits = np.array([0 if v is None else v for v in vals], dtype=FLOAT_BITS[dtype])
        return OCol(dtype, bits.view(og.NP_TYPES[dtype]), valid)
    nt = og.NP_TYPES[dtype]
    return OCol(dtype, np.array([0 if v is None else v for v in vals], dtype=object).astype(np.uint64 if dtype.startswith("UInt") else np.int64).astype(nt),
                valid)


def eighths(rn, nulls=True):
    """a Float64 column of multiples of 1/8 between -4 and 4 (every partial sum of fewer than 2^48 of them is exact, in any order),
    NULL in every fifth row"""
    rn = np.asarray(rn, np.int64)
    return OCol("Float64", ((rn * 7) % 64 - 32) / 8.0, (rn % 5 != 3) if nulls else None)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------

def row_hashes(table, names):
    return RP.restated_hash([table[n] for n in names])


def slots_of(hashes, capacity):
    """the slot wide_key_assign_kernel tries first: mix64(row hash) & mask"""
    return (RP.mix64(hashes) & np.uint64(capacity - 1)).astype(np.int64)


Cells = namedtuple("Cells", "kinds cols hashes")


def cells_of(table, names):
    """the key columns as Python values: per column a list of (valid, stored value) — the value a NULL row STORES included — with a
    Utf8 value as its bytes and a float as the bits of the double it equals (dt_load widens a Float32)"""
    kinds, cols = [], []
    for n in names:
        c = table[n]
        ok = c.is_valid().tolist()
        if c.dtype == "Utf8":
            kinds.append("utf8")
            vals = [s.encode("utf-8") for s in c.values]
        elif c.dtype == "Boolean":
            kinds.append("bool")
            vals = [bool(v) for v in c.values]
        elif c.dtype in og.FLOAT_TYPES:
            kinds.append("float")
            with np.errstate(invalid="ignore"):
                vals = np.ascontiguousarray(c.values.astype(np.float64)).view(np.uint64).tolist()
        else:
            kinds.append("int")
            vals = [int(v) for v in c.values]
        cols.append(list(zip(ok, vals)))
    return Cells(kinds, cols, row_hashes(table, names).tolist())


def _is_nan(bits):
    return (bits & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000


def _is_zero(bits):
    return (bits & 0x7FFFFFFFFFFFFFFF) == 0


def _columnwise(value_equal, validity=True, skip=()):
    def equal(K, a, b):
        for kind, c in zip(K.kinds, K.cols):
            if kind in skip:
                continue
            (va, xa), (vb, xb) = c[a], c[b]
            if validity:
                if va != vb:
                    return False
                if not va:
                    continue
            if not value_equal(kind, xa, xb):
                return False
        return True
    return equal


def _plain(kind, x, y):
    return x == y


RIGHT = _columnwise(_plain)


def _concatenated(K, a, b):
    """the Utf8 columns compared as ONE string (their validities apart), the other columns rightly"""
    if not _columnwise(_plain, skip=("utf8",))(K, a, b):
        return False
    sa = [c[a] for kind, c in zip(K.kinds, K.cols) if kind == "utf8"]
    sb = [c[b] for kind, c in zip(K.kinds, K.cols) if kind == "utf8"]
    return [v for v, _ in sa] == [v for v, _ in sb] and b"".join(x for v, x in sa if v) == b"".join(x for v, x in sb if v)


WRONG = OrderedDict([
    # the stored values alone: a NULL is whatever lies under it
    ("validity_ignored", _columnwise(_plain, validity=False)),
    # NULL == NULL only where the bytes under the two NULLs agree
    ("null_payload_compared", lambda K, a, b: RIGHT(K, a, b) and _columnwise(_plain, validity=False)(K, a, b)),
    ("utf8_length_ignored", _columnwise(lambda k, x, y: x[:min(len(x), len(y))] == y[:min(len(x), len(y))] if k == "utf8" else x == y)),
    ("utf8_first_15_bytes", _columnwise(lambda k, x, y: x[:15] == y[:15] if k == "utf8" else x == y)),
    ("utf8_concatenated", _concatenated),
    ("zeros_equal", _columnwise(lambda k, x, y: x == y or (k == "float" and _is_zero(x) and _is_zero(y)))),
    ("nans_equal", _columnwise(lambda k, x, y: x == y or (k == "float" and _is_nan(x) and _is_nan(y)))),
    ("boolean_ignored", _columnwise(_plain, skip=("bool",))),
    ("equal_hash_is_equal_key", lambda K, a, b: K.hashes[a] == K.hashes[b]),
])


def group_by_representatives(K, capacity, equal=RIGHT, wrap=True):
    """rep[row] for every row, walking the rows in order.  wrap=False restates a probe loop that forgets the mask: a row whose chain
    runs off the table's end finds nothing there and stands for itself"""
    slots = slots_of(np.array(K.hashes, np.uint64), capacity).tolist()
    table = [None] * capacity
    rep = []
    for row, slot in enumerate(slots):
        while True:
            if slot >= capacity:
                rep.append(row)
                break
            o = table[slot]
            if o is None:
                table[slot] = row
                rep.append(row)
                break
            if equal(K, o, row):
                rep.append(o)
                break
            slot = (slot + 1) % capacity if wrap else slot + 1
    return rep, table


def restated_group_count(case, equal=RIGHT, wrap=True):
    t = table_of(case)
    K = cells_of(t, keys_of(case))
    rep, _ = group_by_representatives(K, RC.table_capacity(og.batch_len(t)), equal, wrap)
    return len(set(rep))


def oracle_group_count(case):
    return og.batch_len(og.hash_aggregate(table_of(case), "Partial", case.group, case.aggs))


# ---- the layout rule of the packed key (ProgramBuilder::finish, host/expr.cpp) -----------------------------------------------------------------

LAYOUT_SOURCE = ["if (!hash_only_ && (fixed > 16 || (n_utf8 > 0 && (16 - fixed) / n_utf8 < 2)))",
                 "const int utf8_width = n_utf8 ? (16 - fixed) / n_utf8 : 0;"]
TOO_LONG_SOURCE = "if (len > width - 1) { err |= SCAN_ERR_KEY_TOO_LONG; len = width - 1; }"           # vm_device.h: one byte of a part is its length
FIXED_WIDTH = {"Boolean": 1, "Int8": 1, "UInt8": 1, "Int16": 2, "UInt16": 2, "Int32": 4, "UInt32": 4, "Date32": 4, "Float32": 8,      # (add_key: a
               "Int64": 8, "UInt64": 8, "Float64": 8, "Date64": 8, "Timestamp(Microsecond)": 8}       # Float32 part holds the double's bits)


def packed_layout(parts):
    """parts: [(dtype, nullable)] -> (fits the packed key at all, the longest Utf8 value a part holds).  Fixed parts take their width
    and one byte more when nullable; the Utf8 parts share the rest of 16 bytes equally, one byte of each being the length"""
    fixed = sum(FIXED_WIDTH[t] + (1 if nullable else 0) for t, nullable in parts if t != "Utf8")
    n_utf8 = sum(1 for t, _ in parts if t == "Utf8")
    if fixed > 16 or (n_utf8 > 0 and (16 - fixed) // n_utf8 < 2):
        return False, None
    return True, ((16 - fixed) // n_utf8 - 1 if n_utf8 else None)


def key_parts(case):
    t = table_of(case)
    return [(t[e.name].dtype, t[e.name].valid is not None) for e, _ in case.group]


# ---- A. equality, column by column ---------------------------------------------------------------------------------------------------------------

def _int_values(bits, signed):
    if signed:
        return [0, 1, -1, -(1 << (bits - 1)), (1 << (bits - 1)) - 1, 1 << (bits - 2), None]       # lowest bit, sign, highest bits
    return [0, 1, (1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1, None]


# +0.0, -0.0, +inf, -inf, the smallest subnormal, three quiet NaNs (the patterns of test_agg_edges_gpu.float_specials), 1.0
F64_VALUES = [0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000, 1, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123,
              0x3FF0000000000000, None]
F32_VALUES = [0, 0x80000000, 0x7F800000, 0xFF800000, 1, 0x7FC00000, 0xFFC00000, 0x7FC00123, 0x3F800000, None]
S40 = "forty bytes that end in one of two: ...A"
assert len(S40) == 40
# "" and NULL; a, a + NUL, ab; 40 bytes differing in the last byte and in the first; é (C3 A9) beside ê (C3 AA) and ĩ (C4 A9)
UTF8_VALUES = ["", None, "a", "a\x00", "ab", S40, S40[:-1] + "B", "g" + S40[1:], "é", "ê", "ĩ"]
UTF8_PAIRS = [(("ab", "c"), ("a", "bc")), (("", "x"), ("x", ""))]
VALUES = OrderedDict([
    ("Int8", _int_values(8, True)), ("Int16", _int_values(16, True)), ("Int32", _int_values(32, True)), ("Int64", _int_values(64, True)),
    ("UInt8", _int_values(8, False)), ("UInt16", _int_values(16, False)), ("UInt32", _int_values(32, False)), ("UInt64", _int_values(64, False)),
    ("Date32", _int_values(32, True)), ("Date64", _int_values(64, True)), ("Timestamp(Microsecond)", _int_values(64, True)),
    ("Float32", F32_VALUES), ("Float64", F64_VALUES), ("Boolean", [True, False, None]), ("Utf8", UTF8_VALUES)])
BASE = {"Boolean": True, "Utf8": "x", "Float32": 0x40A00000, "Float64": 0x4014000000000000}          # 5.0; integers: 5
EIGHT_BYTES = ("Int64", "UInt64", "Date64", "Timestamp(Microsecond)", "Float64")


def equality_pairs(dtype):
    """pairs of (k1, k2) keys that differ in ONE column by one step: every two values of the type in column 1 beside the base value in
    column 2, and the other way round; (NULL, base) against (base, NULL); for Utf8 the pairs that agree once concatenated"""
    vals, base = VALUES[dtype], BASE.get(dtype, 5)
    pairs = []
    for u, v in itertools.combinations(vals, 2):
        pairs += [((u, base), (v, base)), ((base, u), (base, v))]
    pairs.append(((None, base), (base, None)))
    if dtype == "Utf8":
        pairs += UTF8_PAIRS
    return pairs


def spread_rows(n_groups, seed, least=4, period=3):
    """group i in least + i % period rows (neighbouring groups differ in their COUNT too), shuffled"""
    g = np.concatenate([np.full(least + i % period, i) for i in range(n_groups)])
    return np.random.default_rng(seed).permutation(g)


# (no aggregate shares a name with a key column: a Final's result would hold two columns of one name)
RN_AGGS = [E.Sum(col("rn"), "rn_sum"), E.Count(col("rn"), "rn_count"), E.Min(col("rn"), "rn_min"), E.Max(col("rn"), "rn_max")]


def shared_slot_salts(prefix, capacity):
    """prefix: the row hashes of the leading key columns of the keys 2j and 2j + 1 of pair j.  -> one Int64 per pair which, as the LAST
    key column of both, sends the two to the same slot of `capacity`; no two pairs get the same one"""
    out = []
    for j in range(len(prefix) // 2):
        lo = (j + 1) << 24
        while True:
            cand = np.arange(lo, lo + 8192, dtype=np.int64)
            sx, sy = (slots_of(RP.mix64(np.uint64(prefix[2 * j + k]) ^ cand.view(np.uint64)), capacity) for k in (0, 1))
            hit = np.nonzero(sx == sy)[0]
            if len(hit):
                out.append(int(cand[hit[0]]))
                break
            lo += 8192
    return out


@functools.lru_cache(maxsize=None)
def equality_case(dtype):
    """keys (k1, k2[, p], salt).  wide_keys_equal only ever compares two rows that meet in one probe chain, so the two keys of a pair
    share a `salt` (an Int64, the last key column) searched so that both start at the SAME slot: whichever comes second is compared with
    the first.  An 8-byte type has three 8-byte columns (wide by layout); every other type has the 40-byte p beside it (wide by value)"""
    pairs = equality_pairs(dtype)
    keys = [k for pair in pairs for k in pair]
    g = spread_rows(len(keys), len(dtype), least=3, period=2)
    n = len(g)
    lead = OrderedDict([("k1", column(dtype, [k[0] for k in keys])), ("k2", column(dtype, [k[1] for k in keys]))])
    if dtype not in EIGHT_BYTES:
        lead["p"] = OCol("Utf8", [LONG] * len(keys))
    capacity = RC.table_capacity(n)
    salts = shared_slot_salts(RP.restated_hash(list(lead.values())), capacity)
    t = OrderedDict((name, c.take(g)) for name, c in lead.items())
    t["salt"] = OCol("Int64", np.array(salts, np.int64)[g // 2])
    t["rn"] = OCol("Int64", np.arange(n))
    group = [(col(k), k) for k in t if k != "rn"]
    return Case("equality_" + dtype, [[t]], group, RN_AGGS, {"wide": True, "n_groups": len(keys), "capacity": capacity, "pairs": len(pairs)})


EQUALITY_CASES = [equality_case(t) for t in VALUES]

ARROW_START, ARROW_ROWS = 3, 77                            # a slice at bit 3 of its buffers, over more than one bitmap word


@functools.lru_cache(maxsize=None)
def arrow_slice_case():
    """-> (the pyarrow record batch, sliced; the Case with the same rows as OCols).  Keys a: Int32, b: Boolean, s: Utf8, p: a long Utf8.
    The arrays are made from raw buffers: the NULL rows of a and s hold row-dependent nonsense, so two NULL keys never store the same
    bytes"""
    import pyarrow as pa
    n = ARROW_START + ARROW_ROWS + 5
    i = np.arange(n)
    a_valid, s_valid, b_valid = i % 4 != 1, i % 3 != 2, i % 5 != 0
    a = np.where(a_valid, i % 2, 1000 + i).astype(np.int32)                      # valid: 0 / 1; NULL: nonsense
    b = (i % 7) < 3
    s = [("é" if k % 2 else "") if ok else "junk%d" % k for k, ok in zip(i.tolist(), s_valid.tolist())]
    bitmap = lambda m: pa.py_buffer(np.packbits(m, bitorder="little").tobytes())
    enc = [x.encode() for x in s]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.int32)
    arrays = [pa.Array.from_buffers(pa.int32(), n, [bitmap(a_valid), pa.py_buffer(a.tobytes())], null_count=-1),
              pa.Array.from_buffers(pa.bool_(), n, [bitmap(b_valid), bitmap(b)], null_count=-1),
              pa.Array.from_buffers(pa.string(), n, [bitmap(s_valid), pa.py_buffer(offs.tobytes()), pa.py_buffer(b"".join(enc))], null_count=-1),
              pa.array([LONG] * n, pa.string()), pa.array(i, pa.int64())]
    rb = pa.record_batch(arrays, names=["a", "b", "s", "p", "rn"]).slice(ARROW_START, ARROW_ROWS)
    w = slice(ARROW_START, ARROW_START + ARROW_ROWS)
    t = OrderedDict([("a", OCol("Int32", a[w], a_valid[w])), ("b", OCol("Boolean", b[w], b_valid[w])), ("s", OCol("Utf8", s[w], s_valid[w])),
                     ("p", OCol("Utf8", [LONG] * ARROW_ROWS)), ("rn", OCol("Int64", i[w]))])
    group = [(col(k), k) for k in ("a", "b", "s", "p")]
    n_groups = len(set(zip(*[t[k].to_pylist() for k in ("a", "b", "s")])))
    return rb, Case("arrow_slice", [[t]], group, RN_AGGS, {"wide": True, "n_groups": n_groups})


# ---- B. collisions ----------------------------------------------------------------------------------------------------------------------------

COLLISION_DRAW, COLLISION_KEYS, COLLISION_CAPACITY = 1 << 17, 72, 1024
ABC = [(col(k), k) for k in ("a", "b", "c")]


@functools.lru_cache(maxsize=None)
def collision_draw():
    """2^17 seeded Int64 triples and the slot of each in a table of 1024"""
    tri = np.random.default_rng(1022).integers(-2 ** 63, 2 ** 63 - 1, (COLLISION_DRAW, 3), endpoint=True)
    h = RP.restated_hash([OCol("Int64", tri[:, j]) for j in range(3)])
    return tri, slots_of(h, COLLISION_CAPACITY)


def _abc_case(name, first, keys, seed, facts):
    g = spread_rows(len(keys), seed)
    t = OrderedDict([("a", first([keys[i][0] for i in g])), ("b", OCol("Int64", [keys[i][1] for i in g])), ("c", OCol("Int64", [keys[i][2] for i in g])),
                     ("rn", OCol("Int64", np.arange(len(g))))])
    assert len(g) < 512                                    # table_capacity: 1024 slots
    return Case(name, [[t]], ABC, RN_AGGS, dict(facts, wide=True, n_groups=len(keys), capacity=COLLISION_CAPACITY))


@functools.lru_cache(maxsize=None)
def slot_collision_case():
    """72 distinct keys of three Int64 columns whose slots are 1022 or 1023 of 1024, 4 to 6 rows each, shuffled: one chain that wraps
    past slot 0 and on to about slot 70"""
    tri, slot = collision_draw()
    hits = np.nonzero(slot >= COLLISION_CAPACITY - 2)[0][:COLLISION_KEYS]
    keys = [tuple(int(x) for x in tri[i]) for i in hits]
    return _abc_case("slot_collisions", lambda v: OCol("Int64", v), keys, 5, {"slots": (COLLISION_CAPACITY - 2, COLLISION_CAPACITY - 1)})


B, C_ = 4242, -99                                          # the b and c of the equal-hash pairs


@functools.lru_cache(maxsize=None)
def equal_hash_cases():
    """rows whose 64-bit row hashes are equal while their keys differ: hash_row folds -0.0 onto +0.0 and hashes a NULL as the Int64
    "nullnull"; a third group differs from each pair in b alone"""
    pz, nz, one = 0, 1 << 63, 0x3FF0000000000000
    zero = _abc_case("equal_hash_zeros", lambda v: column("Float64", v), [(pz, B, C_), (nz, B, C_), (one, B, C_), (pz, B + 1, C_), (nz, B + 1, C_)], 7,
                     {})
    # (the NULL rows STORE the "nullnull" bits too: the pair is equal in everything but validity)
    under_null = lambda v: OCol("Int64", [NULL_BITS if x is None else x for x in v], [x is not None for x in v])
    null = _abc_case("equal_hash_null", under_null, [(None, B, C_), (NULL_BITS, B, C_), (0, B, C_), (None, B + 1, C_), (NULL_BITS, B + 1, C_)], 8,
                     {})
    return [zero, null]


def key_list(case):
    """the distinct keys of a case in first-appearance order, as tuples of cells"""
    t = table_of(case)
    K = cells_of(t, keys_of(case))
    return list(OrderedDict.fromkeys(tuple(c[r] for c in K.cols) for r in range(og.batch_len(t))))


# ---- C. sizes and contention ----------------------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097]
SHAPES = ["one_group", "all_distinct", "two_alternating", "sqrt_groups"]
BIG = 70_000
VALUE_AGGS = [E.Sum(col("v"), "v_sum"), E.Count(col("v"), "v_count"), E.Min(col("v"), "v_min"), E.Max(col("v"), "v_max"), E.Avg(col("v"), "v_avg")]


def shape_groups(shape, n):
    rn = np.arange(n, dtype=np.int64)
    if shape == "one_group":
        return np.zeros(n, np.int64)
    if shape == "all_distinct":
        return rn
    if shape == "two_alternating":
        return rn % 2
    return np.random.default_rng(n).permutation(n) % max(1, math.isqrt(n))


@functools.lru_cache(maxsize=None)
def size_case(shape, n):
    """keys (a, b, c): three NULL-free Int64 columns (24 bytes: wide by layout), a a scramble of the group number; the input as three
    batches, the middle one empty"""
    g = shape_groups(shape, n)
    t = OrderedDict([("a", OCol("Int64", RP.mix64(g.astype(np.uint64)).view(np.int64))), ("b", OCol("Int64", g)), ("c", OCol("Int64", np.full(n, 7))),
                     ("v", eighths(np.arange(n)))])
    n_groups = len(np.unique(g))
    return Case("%s_%d" % (shape, n), [cut(t, [n // 2, 0, n - n // 2])], ABC, VALUE_AGGS, {"wide": True, "n_groups": n_groups, "hash_inner": n >= HINT_ROWS})


HINT_SOURCE = "if (n >= 4096) inner->path_hint_.store(-1);"
HINT_ROWS = 4096

# ---- D. the fall-over ---------------------------------------------------------------------------------------------------------------------------

LAYOUTS = OrderedDict([("utf8", ["s"]), ("utf8_int32", ["s", "i"]), ("two_utf8", ["s", "t"])])
LAYOUT_PARTS = {"utf8": [("Utf8", False)], "utf8_int32": [("Utf8", False), ("Int32", False)], "two_utf8": [("Utf8", False), ("Utf8", False)]}
FALLOVER_ROWS = 300
FALLOVER_AGGS = [E.Sum(col("rn"), "rn_sum"), E.Count(col("rn"), "rn_count"), E.Avg(col("v"), "v_avg"), E.Sum(col("v"), "v_sum")]
KEEP = col("f") > lit(0.5)


def fits(layout):
    ok, longest = packed_layout(LAYOUT_PARTS[layout])
    assert ok
    return longest


def fallover_table(layout, n=FALLOVER_ROWS, long_at=None, rn0=0):
    """s: three short values and one of exactly the longest length the layout's share holds; the row `long_at` holds that value and one
    byte more (a key cut to its share would merge the two).  f is 0 in that row alone: FilterExec(KEEP) removes it"""
    fit = "F" * fits(layout)
    rn = np.arange(rn0, rn0 + n)
    s = [("A", "BB", "", fit)[k % 4] for k in range(n)]
    f = np.ones(n)
    if long_at is not None:
        s[long_at] = fit + "!"
        f[long_at] = 0.0
    return OrderedDict([("s", OCol("Utf8", s)), ("i", OCol("Int32", (rn % 3).astype(np.int32))), ("t", OCol("Utf8", [("u", "vv")[k % 2] for k in rn.tolist()])),
                        ("f", OCol("Float64", f)), ("v", eighths(rn)), ("rn", OCol("Int64", rn))])


def fallover_case(layout, where):
    """where: "fits", "row_0", "last_row" (of the last of three batches), "filtered" (the case's plan puts FilterExec(KEEP) below),
    "partition_1" (of two), "after_hint" (partition 0: 3000 short rows in three groups, partition 1 holds the value)"""
    n = FALLOVER_ROWS
    group = [(col(k), k) for k in LAYOUTS[layout]]
    wide = {"fits": False, "filtered": None}.get(where, True)
    if where in ("fits", "row_0", "last_row", "filtered"):
        t = fallover_table(layout, long_at={"fits": None, "row_0": 0, "last_row": n - 1, "filtered": n // 2}[where])
        parts = [cut(t, [n // 3, n // 3, n - 2 * (n // 3)])]
    elif where == "partition_1":
        parts = [[fallover_table(layout)], [fallover_table(layout, long_at=n // 2, rn0=n)]]
    else:
        short = fallover_table(layout, 3000)
        short["s"] = OCol("Utf8", [("A", "BB", "C")[k % 3] for k in range(3000)])
        short["t"] = OCol("Utf8", ["u"] * 3000)
        parts = [[short], [fallover_table(layout, long_at=n - 1, rn0=3000)]]
    return Case("fallover_%s_%s" % (layout, where), parts, group, FALLOVER_AGGS, {"wide": wide, "fits": fits(layout), "filtered": where == "filtered"})


FALLOVER_WHERE = ["fits", "row_0", "last_row", "filtered", "partition_1", "after_hint"]
HEAD_ROWS, HEAD_SAMPLE = (1 << 17) + 1, 32768
HEAD_SOURCE = ["if (hint == 0 && gmax > 0 && !group_.empty() && !use_lean && (!mid_sized || (gmax == 4 && total_in >= (1 << 17)))) {",
               "head->n_rows = std::min<int64_t>(head->n_rows, 32768);",
               "if (hint == 0 && gmax == 4 && mid_sized && !wide_acc && n_acc <= 4 && !use_lean) gmax = 8;"]
HEAD_AGGS = [E.Sum(col("v"), "v_sum"), E.Count(col("v"), "v_count"), E.Min(col("v"), "v_min"), E.Max(col("v"), "v_max"), E.Min(col("rn"), "rn_min"), E.Max(col("rn"), "rn_max")]


@functools.lru_cache(maxsize=None)
def head_sample_case():
    """2^17 + 1 rows in ONE batch, six accumulators, three one-byte keys — and in the last row alone, far behind the 32 768-row head the
    ladder samples, a 16-byte one"""
    n = HEAD_ROWS
    rn = np.arange(n)
    s = np.array(["A", "B", "C"], dtype=object)[rn % 3]
    s[n - 1] = "F" * 16
    t = OrderedDict([("s", OCol("Utf8", s)), ("v", eighths(rn)), ("rn", OCol("Int64", rn))])
    return Case("fallover_behind_the_head_sample", [[t]], [(col("s"), "s")], HEAD_AGGS, {"wide": True, "n_groups": 4, "accumulators": 6})


# ---- E. modes ----------------------------------------------------------------------------------------------------------------------------------

MODE_GROUPS, MODE_ROWS, NULL_GROUP = 8, 400, 3
MODE_KEYS = [(col("s"), "s"), (col("i"), "i")]
MODE_AGGS = [E.Avg(col("x"), "ax"), E.Avg(col("y"), "ay"), E.Avg(col("z"), "az"), E.Sum(col("z"), "sz"), E.Count(col("z"), "cz"), E.Sum(col("x"), "sx")]
MODE_STRING_AGGS = MODE_AGGS + [E.Min(col("m"), "mm")]


@functools.lru_cache(maxsize=None)
def mode_table():
    """keys (s, i): a string with the group number, too long for the packed key, and an Int32; arguments x: Int32, y: Float32, z: Float64,
    each NULL in some rows and in EVERY row of group 3; m: a Utf8 column for MIN"""
    n = MODE_ROWS
    rn = np.arange(n)
    g = np.random.default_rng(12).integers(0, MODE_GROUPS, n)
    g[:MODE_GROUPS] = np.arange(MODE_GROUPS)
    live = g != NULL_GROUP
    z = eighths(rn)
    return OrderedDict([("s", OCol("Utf8", ["a group key of the wide kind, number %02d" % k for k in g])), ("i", OCol("Int32", (g % 3).astype(np.int32), rn % 97 != 5)),
                        ("x", OCol("Int32", (rn % 23 - 11).astype(np.int32), live & (rn % 7 != 1))), ("y", OCol("Float32", z.values.astype(np.float32), live & (rn % 4 != 2))),
                        ("z", OCol("Float64", z.values, live & z.is_valid())), ("m", OCol("Utf8", ["m%d" % (k % 11) for k in rn], rn % 6 != 0))])


def mode_partitions(n_parts):
    t = mode_table()
    n = MODE_ROWS
    return [cut(t, [n])] if n_parts == 1 else [[b] for b in cut(t, [n // 2, n - n // 2])]


ELISION_SOURCE = ["if (!pa || !below || pa->mode_ != BHIP_AGG_PARTIAL || pa->output_partitioning().count != 1 || pa->strings_) return false;",
                  "// wide keys: the Partial's state batch, then AVG = [sum] / [count] as a projection"]

# ---- F. strings on top ----------------------------------------------------------------------------------------------------------------------------

STRING_GROUPS = [[None, None, None], ["same", "same", "same", None], ["", "a", None], ["", ""], ["z", "é", "\x7f", "ÿ"], ["\U0001f600", "zz", "￿"],
                 ["ab", "a", "abc"], ["only"]]
STRING_AGGS = [E.Min(col("m"), "m_min"), E.Max(col("m"), "m_max"), E.Count(col("m"), "m_count"), E.Sum(col("rn"), "rn_sum")]


@functools.lru_cache(maxsize=None)
def string_minmax_table():
    """MIN / MAX over m, grouped by (s, i) with s too long for the packed key: a group with only NULL strings, equal strings in several
    rows, "" alone and beside others, bytes >= 0x80"""
    gs, ms = [], []
    for rep in range(6):
        for g, vals in enumerate(STRING_GROUPS):
            gs += [g] * len(vals)
            ms += vals
    order = np.random.default_rng(3).permutation(len(gs))
    gs, ms = [gs[k] for k in order], [ms[k] for k in order]
    return OrderedDict([("s", OCol("Utf8", ["the group of strings number %02d" % g for g in gs])), ("i", OCol("Int32", [g % 2 for g in gs])), ("m", column("Utf8", ms)),
                        ("rn", OCol("Int64", np.arange(len(gs))))])


EXPR_ROWS = 240


@functools.lru_cache(maxsize=None)
def string_expr_table():
    """a, b: ASCII strings in mixed case with blanks at their ends, a NULL in some rows; cc: concat(a, b) worked out here with Python's str
    (SQL ||: NULL where either argument is), for the oracle, which has no concat of its own"""
    rn = np.arange(EXPR_ROWS)
    a = ["  A Mixed-Case Key, Number %d  " % (k % 5) for k in rn]
    b = ["\tand a Second Part %d " % (k % 3) for k in rn]
    av, bv = rn % 11 != 4, rn % 13 != 6
    cc = [x + y for x, y in zip(a, b)]
    return OrderedDict([("a", OCol("Utf8", a, av)), ("b", OCol("Utf8", b, bv)), ("cc", OCol("Utf8", cc, av & bv)), ("v", eighths(rn)), ("rn", OCol("Int64", rn))])


# name -> (the device's group expressions, the oracle's over the same table)
STRING_EXPR_KEYS = OrderedDict([
    ("lower", ([(fn("lower", col("a")), "k")],) * 2),
    ("trim", ([(fn("trim", col("b")), "k")],) * 2),
    ("lower_trim", ([(fn("lower", fn("trim", col("a"))), "k"), (fn("trim", col("b")), "k2")],) * 2),
    ("concat", ([(fn("concat", col("a"), col("b")), "k")], [(col("cc"), "k")])),
])

# ---- G. limits ----------------------------------------------------------------------------------------------------------------------------------

MAX_GROUP_EXPRS = 16
MESSAGES = {"too_many": "more than 16 group expressions", "reserved": "column name '__group_rep' is reserved",
            "layout": "key columns do not fit the 16-byte packed key", "value": "a Utf8 key value is longer than the packed-key path supports",
            "key_parts": "more than 8 key columns"}


@functools.lru_cache(maxsize=None)
def many_keys_table(n_keys):
    """k0 .. : Int32 columns holding single bits of the group number, the last one the number itself (40 groups).  The first eight hold
    its low three bits only: groups that agree in them differ in columns past the eighth alone, which the row hash takes in a second pass"""
    n = 400
    g = np.random.default_rng(16).integers(0, 40, n)
    t = OrderedDict(("k%d" % j, OCol("Int32", ((g >> (j % 3 if j < 8 else j % 6)) & 1).astype(np.int32) if j < n_keys - 1 else g.astype(np.int32), ((g % 8 if j < 8 else g) + j) % 9 != 0)) for j in range(n_keys))
    t["rn"] = OCol("Int64", np.arange(n))
    return t


def many_keys_case(n_keys):
    t = many_keys_table(n_keys)
    group = [(col("k%d" % j), "k%d" % j) for j in range(n_keys)]
    n_groups = len(set(zip(*[t[n].to_pylist() for _, n in group])))
    return Case("%d_group_expressions" % n_keys, [cut(t, [150, 250])], group, RN_AGGS, {"wide": True, "n_groups": n_groups})


# ---- which case each wrong equality is built against ----------------------------------------------------------------------------------------------

def discrimination():
    """wrong equality (or "no_wrap") -> the cases whose number of groups it changes"""
    eq = {c.name: c for c in EQUALITY_CASES}
    arrow = arrow_slice_case()[1]
    zero, null = equal_hash_cases()
    return OrderedDict([
        ("validity_ignored", [eq["equality_" + t] for t in VALUES] + [null]),             # 0 / "" / False beside NULL in every type
        ("null_payload_compared", [arrow]),
        ("utf8_length_ignored", [eq["equality_Utf8"]]),
        ("utf8_first_15_bytes", [eq["equality_Utf8"]]),
        ("utf8_concatenated", [eq["equality_Utf8"]]),
        ("zeros_equal", [eq["equality_Float32"], eq["equality_Float64"], zero]),
        ("nans_equal", [eq["equality_Float32"], eq["equality_Float64"]]),
        ("boolean_ignored", [eq["equality_Boolean"]]),
        ("equal_hash_is_equal_key", [zero, null]),
        ("no_wrap", [slot_collision_case()]),
    ])


def source_text(rel):
    return open(os.path.join(RC.CSRC, rel)).read()


def tests_file_text(name):
    return open(os.path.join(ROOT, "tests", name)).read()
