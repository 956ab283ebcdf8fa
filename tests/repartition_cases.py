"""TEST INFRASTRUCTURE shared by test_repartition_cases_cpu.py (no GPU) and test_repartition_edges_gpu.py: the inputs of the hash
repartitioning tests and a SECOND statement of the partition id.

Nothing here touches a device.  A case is a named table (an OrderedDict of OCols, each with an `rn` Int64 row number), the key
expressions, the partition counts it is split into and the device route it must take ("scatter": partition_hist / partition_scatter
of kernels_sort.hip; "sort": hash_row + hash_to_pid + radix_sort_pairs + partition_bounds + one gather per partition).

The partition id is restated here without oracle.engine.row_hash (DESIGN.md "Row hash"): per key column the value's 64 bits — an
integer sign- or zero-extended, a Boolean as 0 / 1, a float as the bits of the double it equals with -0.0 folded onto +0.0, FNV-1a-64
of a string's bytes, "nullnull" for NULL — folded by h = mix64(h ^ bits) from h = 0, then h % n_parts.  Fixed-width columns are
numpy uint64 arithmetic (which wraps), strings a plain loop.  The skew cases (all rows in one partition, chosen partitions empty, all
256 live) are built by SEARCHING key values with this restatement, not by trying seeds; test_repartition_cases_cpu.py checks that
every case is what its name says and that the oracle's own statement gives the same ids row for row."""
from collections import OrderedDict
from functools import lru_cache

import numpy as np

from ballista_amd import expr as E
from ballista_amd.expr import col
from oracle import engine as og
from oracle.engine import OCol

import sort_cases

# ---- the restated hash -----------------------------------------------------------------------------------------------------------------

NULL_BITS = 0x6E756C6C6E756C6C                       # the bytes "nullnull"
FNV_BASIS = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
_MASK = (1 << 64) - 1


def mix64(z):
    """splitmix64's output function over a uint64 array (or one integer): the increment, two xor-shift-multiplies, an xor-shift"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fnv1a(data: bytes) -> int:
    h = FNV_BASIS
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & _MASK
    return h


def value_bits(c: OCol):
    """the 64 bits of every row of one key column, as a uint64 array"""
    n = len(c)
    if c.dtype == "Utf8":
        bits = np.array([fnv1a(s.encode("utf-8")) for s in c.values], dtype=np.uint64).reshape(n)
    elif c.dtype in og.FLOAT_TYPES:
        with np.errstate(invalid="ignore"):           # (widening a signalling NaN quiets it and raises the flag)
            d = c.values.astype(np.float64)           # exact for a Float32: it hashes as the double it equals
        d = np.where(d == 0.0, np.float64(0.0), d)    # -0.0 == +0.0, so both become +0.0
        bits = np.ascontiguousarray(d).view(np.uint64)
    elif c.dtype == "Boolean" or c.dtype in og.UNSIGNED_TYPES:
        bits = c.values.astype(np.uint64)             # zero-extended
    else:
        bits = c.values.astype(np.int64).view(np.uint64)   # sign-extended
    return np.where(c.is_valid(), bits, np.uint64(NULL_BITS))


def restated_hash(cols):
    h = np.zeros(len(cols[0]), np.uint64)
    for c in cols:
        h = mix64(h ^ value_bits(c))
    return h


def restated_pid(batch, exprs, n_parts):
    """partition id of every row (int64 array).  A key expression is evaluated by the oracle's expression evaluator; the hash of its
    values is this module's"""
    if og.batch_len(batch) == 0:
        return np.zeros(0, np.int64)
    h = restated_hash([og.evaluate(e, batch) for e in exprs])
    return (h % np.uint64(n_parts)).astype(np.int64)


def restated_partitions(batch, exprs, n_parts):
    pid = restated_pid(batch, exprs, n_parts)
    return [OrderedDict((k, c.take(np.nonzero(pid == p)[0])) for k, c in batch.items()) for p in range(n_parts)]


def pid_of_ints(values, n_parts):
    """partition id of 64-bit key images given as a uint64 array (one NULL-free integer key column)"""
    return (mix64(np.asarray(values, np.uint64)) % np.uint64(n_parts)).astype(np.int64)


def search_keys(n_parts, wanted, count, start=1, step=1):
    """the first `count` integers of start, start + step, ... whose partition (as an Int64 key) is in `wanted`"""
    out, lo = [], start
    wanted = np.asarray(sorted(wanted))
    while len(out) < count:
        cand = lo + step * np.arange(65536, dtype=np.int64)
        hit = cand[np.isin(pid_of_ints(cand.view(np.uint64), n_parts), wanted)]
        out.extend(hit[:count - len(out)].tolist())
        lo += step * 65536
    return np.array(out, np.int64)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, batch, exprs, n_parts, route, bit_exact=False):
        self.name, self.batch, self.exprs, self.n_parts, self.route, self.bit_exact = name, batch, exprs, list(n_parts), route, bit_exact

    @property
    def n(self):
        return og.batch_len(self.batch)

    def __repr__(self):
        return self.name


K = [col("k")]
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2 ** 31, 2 ** 31 - 1, -2 ** 63, 2 ** 63 - 1
KEY_TYPES = ["Int32", "Date32", "Int64", "UInt64"]                          # the key types of the scatter pass
EXTREMES = {"Int32": [I32_MIN, -1, 0, I32_MAX], "Date32": [I32_MIN, -1, 0, I32_MAX],
            "Int64": [I32_MIN, -1, 0, I32_MAX, I64_MIN, I64_MAX, I32_MAX + 1, I32_MIN - 1],
            "UInt64": [0, I32_MAX, I64_MAX, 2 ** 63, 2 ** 64 - 1, 2 ** 63 + 1, 2 ** 32, 2 ** 64 - 2 ** 31]}

# ---- 1. the scatter pass: sizes x partition counts x key types under payload columns of every width -----------------------------------------

SCATTER_SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]       # wave, sub-tile (256) and workgroup chunk (4096) edges
SCATTER_NPARTS = [1, 2, 3, 7, 255, 256]
_OTHER = [1, 2, 7, 255]
# every size at 3 and 256 partitions; every size with one of the other counts, each of which also meets a size of three workgroups
SCATTER_PAIRS = ([(p, n) for p in (3, 256) for n in SCATTER_SIZES] + [(_OTHER[i % 4], n) for i, n in enumerate(SCATTER_SIZES)] +
                 [(1, 8193), (2, 8193), (255, 4097), (255, 8193)])
PAYLOADS = [("p_i8", "Int8"), ("p_u8", "UInt8"), ("p_i16", "Int16"), ("p_u16", "UInt16"), ("p_i32", "Int32"), ("p_f32", "Float32"),
            ("p_d32", "Date32"), ("p_i64", "Int64"), ("p_u64", "UInt64"), ("p_f64", "Float64"), ("p_ts", "Timestamp(Microsecond)")]


def scatter_keys(dtype, n):
    """row i, by i % 4: one of the type's extremes; a dense small value (0 .. 36, so every one repeats); a key that differs from its
    neighbours only above bit 32 (the 32-bit types: only in the upper half word); a value of the whole range"""
    i = np.arange(n, dtype=np.uint64)
    q = i // np.uint64(4)
    wide = dtype in ("Int64", "UInt64")
    ext = np.array([v & _MASK for v in EXTREMES[dtype]], dtype=np.uint64)[(q % np.uint64(len(EXTREMES[dtype]))).astype(np.int64)]
    dense = q % np.uint64(37)
    high = (q << np.uint64(32 if wide else 16)) | np.uint64(7)
    with np.errstate(over="ignore"):
        spread = mix64(i * np.uint64(0xD1B54A32D192ED03))
    v = np.select([i % np.uint64(4) == 0, i % np.uint64(4) == 1, i % np.uint64(4) == 2], [ext, dense, high], spread)
    if not wide:
        v = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return OCol(dtype, v.view(np.int64) if dtype == "Int64" else v)


def payload_columns(n):
    """a column of every fixed width, each value a function of the row number that differs between neighbouring rows in every byte
    it has: a copy of the wrong width, or from the wrong row, shows.  The float columns hold arbitrary bit patterns (NaNs with
    payloads and both zeros among them), so these tables are compared bit for bit"""
    rn = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        w = (rn + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    out = OrderedDict()
    for j, (name, dtype) in enumerate(PAYLOADS):
        x = w ^ (w >> np.uint64(7 + j))
        nt = og.NP_TYPES[dtype]
        size = np.dtype(nt).itemsize
        narrow = (x >> np.uint64(64 - 8 * size)).astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[size])
        out[name] = OCol(dtype, narrow.view(nt))
    if n > 1:
        out["p_f64"].values[:2] = [-0.0, 0.0]
        out["p_f32"].values[:2] = [0.0, -0.0]
    return out


@lru_cache(maxsize=None)
def scatter_table(dtype, n):
    t = OrderedDict([("k", scatter_keys(dtype, n)), ("rn", OCol("Int64", np.arange(n)))])
    t.update(payload_columns(n))
    return t


def scatter_case(dtype, n_parts, n):
    return Case(f"scatter_{dtype}_{n}_rows", scatter_table(dtype, n), K, [n_parts], "scatter", bit_exact=True)


# ---- 2. the route switch: 32 columns, 33 columns, 257 partitions ----------------------------------------------------------------------------

SWITCH_ROWS = 1500


@lru_cache(maxsize=None)
def wide_table(n_cols):
    """k, rn and n_cols - 2 NULL-free Int32 / Int16 columns"""
    n = SWITCH_ROWS
    t = OrderedDict([("k", scatter_keys("Int64", n)), ("rn", OCol("Int64", np.arange(n)))])
    for j in range(n_cols - 2):
        t[f"c{j}"] = OCol("Int16", (np.arange(n) * (j + 3)).astype(np.int16)) if j % 2 else OCol("Int32", np.arange(n, dtype=np.int32) * 1000 + j)
    return t


SWITCH_CASES = [Case("switch_32_columns", wide_table(32), K, [256], "scatter"),
                Case("switch_33_columns", wide_table(33), K, [256], "sort"),
                Case("switch_257_partitions", wide_table(32), K, [257], "sort"),
                Case("switch_33_columns_257_partitions", wide_table(33), K, [257], "sort")]

# ---- 3. skew and emptiness: keys found by searching with the restatement ------------------------------------------------------------------------

SKEW_ROWS = 4097 + 300                                # two workgroups, the second one partly filled


def _skew(name, keys, n_parts):
    n = len(keys)
    t = OrderedDict([("k", OCol("Int64", keys)), ("rn", OCol("Int64", np.arange(n))), ("v", OCol("Int16", (np.arange(n) * 3).astype(np.int16)))])
    return Case(name, t, K, [n_parts], "scatter")


def _cycle(keys, n):
    return np.asarray(keys, np.int64)[np.arange(n) % len(keys)]


def skew_cases():
    out = []
    # distinct keys that all hash to partition 4 of 7 (and to the only live one of 256): every ballot of every wave has one digit
    out.append(_skew("one_partition", search_keys(7, [4], SKEW_ROWS), 7))
    out.append(_skew("one_partition_of_256", search_keys(256, [255], SKEW_ROWS, start=-10 ** 9), 256))
    out.append(_skew("all_equal", np.full(SKEW_ROWS, I64_MIN, np.int64), 255))
    a, b = int(search_keys(3, [0], 1)[0]), int(search_keys(3, [2], 1)[0])
    out.append(_skew("two_alternating", _cycle([a, b], SKEW_ROWS), 3))
    out.append(_skew("first_empty", search_keys(5, [1, 2, 3, 4], SKEW_ROWS), 5))
    out.append(_skew("last_empty", search_keys(5, [0, 1, 2, 3], SKEW_ROWS), 5))
    out.append(_skew("interior_empty", search_keys(7, [0, 1, 5, 6], SKEW_ROWS), 7))
    live = np.concatenate([search_keys(256, [p], 3, start=2 ** 40) for p in range(256)])
    out.append(_skew("all_256_live", live[(np.arange(len(live)) * 7) % len(live)], 256))          # 768 rows, 7 is coprime: a permutation
    out.append(_skew("single_row", np.array([I64_MAX]), 256))
    out.append(_skew("single_row_one_partition", np.array([-1]), 1))
    few = [int(search_keys(256, [p], 1, start=-5, step=-1)[0]) for p in (255, 0, 100, 101, 0)]     # first and last live, 251 empty
    out.append(_skew("more_partitions_than_rows", np.array(few, np.int64), 256))
    return out


SKEW_CASES = skew_cases()
EMPTY_PARTITIONS = {"first_empty": [0], "last_empty": [4], "interior_empty": [2, 3, 4]}

# ---- 4. the sort pass -----------------------------------------------------------------------------------------------------------------------

SORT_SIZES = [1, 2, 1023, 1024, 1025, 4097]          # 1024: the last size of the one-workgroup sort
SORT_NPARTS = [1, 2, 3, 255, 256, 257, 1000]         # from 257 the partition ids differ in two bytes: two LSD passes
# every size at 3 and 257 partitions; the other counts at one small-sort size and one radix size each
SORT_PAIRS = ([(p, n) for p in (3, 257) for n in SORT_SIZES] +
              [(1, 1024), (1, 1025), (2, 2), (2, 4097), (255, 1023), (255, 1025), (256, 1024), (256, 4097), (1000, 1023), (1000, 1025)])
LONG = "long-" + "0123456789abcdef" * 18 + "-tail"    # 298 bytes, then a suffix per row: about 300
STRINGS = ["", "a", "b", "ab", "ba", "é", "é", "日本語", "日本", "𝄞 clef", "ß-ü", "Customer#000000001", " ", "\t", LONG + "x", LONG + "y",
           "x" + LONG, "ñandú" * 60]


def utf8_values(n, nulls=True):
    """'' and NULL both present (NULL rows hold a non-empty stored value), 300-byte strings that differ in their last byte, multi-byte UTF-8"""
    vals = [STRINGS[(i * 5 + i // 18) % len(STRINGS)] for i in range(n)]
    valid = np.array([i % 11 != 3 for i in range(n)]) if nulls else None
    if n > 1:
        vals[0], vals[1] = "", "stored under a NULL"
        if nulls:
            valid[0], valid[1] = True, False
    return OCol("Utf8", vals, valid)


@lru_cache(maxsize=None)
def two_key_table(n):
    """a: Int64 with NULLs; s: Utf8 with NULLs; rows with a NULL in a only, in s only, and in both"""
    rng = np.random.default_rng(n)
    a = rng.integers(-5, 6, n) * (2 ** 33 + 1)
    va = np.arange(n) % 7 != 2
    s = utf8_values(n)
    if n > 4:
        va[1] = False                                  # both NULL (utf8_values makes row 1 NULL)
        va[2], va[3] = False, True                     # a only
    return OrderedDict([("a", OCol("Int64", a, va)), ("s", s), ("rn", OCol("Int64", np.arange(n))),
                        ("x", OCol("Float64", np.arange(n) * 0.5))])


def sort_size_case(n_parts, n):
    return Case(f"sort_{n}_rows", two_key_table(n), [col("a"), col("s")], [n_parts], "sort")


KEY_ROWS = 1300                                       # beyond the one-workgroup sort


def _key_table(name, key_cols, exprs, n_parts, n=KEY_ROWS, bit_exact=False, extra=()):
    t = OrderedDict(key_cols)
    t["rn"] = OCol("Int64", np.arange(n))
    t.update(extra)
    return Case(name, t, exprs, n_parts, "sort", bit_exact)


def float_key(dtype, n):
    """the specials of sort_cases (NaNs of both signs with payloads, infinities, subnormals, both zeros, NULLs) and, in rows 0 and
    1, -0.0 and +0.0"""
    c = sort_cases.float_special_column(dtype, n, np.random.default_rng(11))
    c.values[0], c.values[1] = -0.0, 0.0
    valid = c.is_valid().copy()
    valid[:2] = True
    return OCol(dtype, c.values, valid)


def key_cases():
    n = KEY_ROWS
    rng = np.random.default_rng(4)
    t2 = two_key_table(n)
    out = [Case("keys_int64_utf8", t2, [col("a"), col("s")], [7, 300], "sort"),
           Case("keys_utf8_int64", t2, [col("s"), col("a")], [7, 300], "sort"),
           _key_table("key_utf8", [("k", utf8_values(n))], K, [7, 257]),
           _key_table("key_boolean", [("k", OCol("Boolean", np.arange(n) % 3 == 0, np.arange(n) % 5 != 1))], K, [2, 5]),
           _key_table("key_float64", [("k", float_key("Float64", n))], K, [7], bit_exact=True),
           _key_table("key_float32", [("k", float_key("Float32", n))], K, [7], bit_exact=True)]
    a = rng.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int32)
    b = rng.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int32)
    a[:4], b[:4] = [I32_MAX, I32_MIN, -1, 0], [1, -1, 1, 0]                  # the sum wraps
    ab = [("a", OCol("Int32", a)), ("b", OCol("Int32", b))]
    out.append(_key_table("key_sum_of_columns", ab, [E.BinaryExpr(col("a"), "Plus", col("b"))], [7]))
    w = rng.integers(-2 ** 33, 2 ** 33, n)
    w[:4] = [I32_MAX, I32_MAX + 1, I32_MIN, I32_MIN - 1]                     # a cast the target cannot hold is NULL
    out.append(_key_table("key_cast_narrowing", [("a", OCol("Int64", w))], [E.CastExpr(col("a"), "Int32")], [7]))
    out.append(_key_table("key_cast_to_float", ab, [E.CastExpr(col("a"), "Float64")], [7]))
    out.append(_key_table("key_all_null", [("k", OCol("Int32", np.arange(n, dtype=np.int32), np.zeros(n, bool)))], K, [7, 257]))
    out.append(_key_table("key_all_equal", [("k", OCol("Int64", np.full(n, 42))), ("s", utf8_values(n))], K, [7, 257]))
    out.append(_key_table("more_partitions_than_rows_sorted", [("k", utf8_values(300))], K, [1000], n=300))
    return out


KEY_CASES = key_cases()

# ---- 5. the empty batch ------------------------------------------------------------------------------------------------------------------

EMPTY_CASES = [Case("empty_fixed_width", scatter_table("Int64", 0), K, [1, 3, 256, 257], "none", bit_exact=True),
               Case("empty_with_utf8", OrderedDict([("k", OCol("Int32", np.zeros(0, np.int32))), ("rn", OCol("Int64", np.zeros(0, np.int64))),
                                                    ("s", OCol("Utf8", []))]), K, [1, 3, 257], "none")]

# ---- 6. agreement between the routes and between the types ----------------------------------------------------------------------------------

AGREE_ROWS = 2000
AGREE_NPARTS = 13


def agreement_values(dtype):
    rng = np.random.default_rng(21)
    nt = og.NP_TYPES[dtype]
    info = np.iinfo(nt)
    v = rng.integers(info.min, info.max, AGREE_ROWS, dtype=np.uint64 if dtype == "UInt64" else np.int64, endpoint=True).astype(nt)
    ext = np.array([x & _MASK for x in EXTREMES[dtype]], np.uint64).astype(nt) if dtype == "UInt64" else np.array(EXTREMES[dtype], nt)
    v[:2 * len(ext)] = np.concatenate([ext, ext])
    return v


def route_agreement_tables(dtype):
    """the same key values three times: {"lone": k and rn, NULL-free (the scatter pass); "utf8": beside a Utf8 payload (the sort
    pass); "bitmap": one row longer, that last row's key NULL — the GPU test cuts it off, which leaves a validity bitmap over rows
    none of which is NULL (the sort pass)}"""
    v = agreement_values(dtype)
    n = len(v)
    rn = OCol("Int64", np.arange(n))
    longer = OrderedDict([("k", OCol(dtype, np.concatenate([v, v[:1]]), np.arange(n + 1) < n)), ("rn", OCol("Int64", np.arange(n + 1)))])
    return {"lone": OrderedDict([("k", OCol(dtype, v)), ("rn", rn)]),
            "utf8": OrderedDict([("k", OCol(dtype, v)), ("rn", rn), ("s", OCol("Utf8", [f"row {i}" for i in range(n)]))]),
            "bitmap": longer}


# one list of values per group, held as every type of the group: all of them must go to the same partitions
_I8 = np.concatenate([[-128, -1, 0, 1, 127], np.arange(-128, 128), np.random.default_rng(5).integers(-128, 128, 1039)])
_U32 = np.concatenate([[0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.random.default_rng(6).integers(0, 2 ** 32, 1295)])      # half of them >= 2^31
_D32 = np.concatenate([[I32_MIN, -1, 0, I32_MAX], np.random.default_rng(7).integers(I32_MIN, I32_MAX, 1296)])
_F32 = np.concatenate([np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4028235e38, 1.17549435e-38], np.float32),
                       np.random.default_rng(8).normal(0, 1e3, 1289).astype(np.float32)])
TYPE_GROUPS = {"signed_widths": (_I8, ["Int8", "Int16", "Int32", "Int64"]), "unsigned_as_int64": (_U32, ["UInt32", "Int64"]),
               "date_as_int32": (_D32, ["Date32", "Int32"]), "float_widths": (_F32, ["Float32", "Float64"])}
# (a lone NULL-free Int32 / Int64 / Date32 key takes the scatter pass, every other type the sort pass)
TYPE_ROUTE = {"Int32": "scatter", "Int64": "scatter", "Date32": "scatter", "UInt64": "scatter"}


def type_table(group, dtype):
    v = TYPE_GROUPS[group][0]
    return OrderedDict([("k", OCol(dtype, v.astype(og.NP_TYPES[dtype]))), ("rn", OCol("Int64", np.arange(len(v))))])


# ---- 7. RepartitionExec over batches that alternate between the routes ----------------------------------------------------------------------

REPART_NPARTS = 5
REPART_SCHEMA = [("k", "Int64"), ("v", "Int32"), ("rn", "Int64")]


def repartition_stream():
    """two input partitions of batches of one (nullable-key) schema: "fixed" = no NULL (no validity buffer: the scatter pass), "nulls" =
    NULL keys (the sort pass), "empty" = no rows.  -> [[(kind, batch)]], row numbers running on through the whole stream"""
    layout = [[("empty", 0), ("fixed", 4097), ("nulls", 1025), ("fixed", 300), ("empty", 0)], [("nulls", 700), ("empty", 0), ("fixed", 1), ("nulls", 4097)]]
    rng = np.random.default_rng(31)
    out, rn0 = [], 0
    for part in layout:
        batches = []
        for kind, n in part:
            k = rng.integers(-2 ** 40, 2 ** 40, n)
            valid = (np.arange(n) % 9 != 4) if kind == "nulls" else None
            batches.append((kind, OrderedDict([("k", OCol("Int64", k, valid)), ("v", OCol("Int32", rng.integers(0, 1000, n))),
                                               ("rn", OCol("Int64", np.arange(rn0, rn0 + n)))])))
            rn0 += n
        out.append(batches)
    return out


# ---- 8. the streaming shuffle -------------------------------------------------------------------------------------------------------------

SHUFFLE_WORLD = 3
SHUFFLE_SIZES = [5000, 9001, 4096]                    # rank 0: every row to rank 1


def shuffle_batch(rank, key):
    """rank `rank`'s input under key "k" (UInt64, every value >= 2^63) or "d" (Date32, every value negative); all of rank 0's rows
    hash to rank 1 under the key in use (values found by search), the other ranks' rows spread"""
    n = SHUFFLE_SIZES[rank]
    rng = np.random.default_rng(40 + rank)
    if rank == 0:
        hit = search_keys(SHUFFLE_WORLD, [1], 40, start=-3, step=-1)                       # negative: as UInt64 at or above 2^63
        pick = hit[np.arange(n) % len(hit)]
        k, d = (pick.view(np.uint64), -rng.integers(1, 10 ** 6, n)) if key == "k" else (rng.integers(2 ** 63, 2 ** 64, n, dtype=np.uint64), pick)
    else:
        k, d = rng.integers(2 ** 63, 2 ** 64, n, dtype=np.uint64), -rng.integers(1, 2 ** 31, n, endpoint=True)
        k[:2] = [2 ** 63, 2 ** 64 - 1]
        d[:2] = [I32_MIN, -1]
    return OrderedDict([("k", OCol("UInt64", k)), ("d", OCol("Date32", d.astype(np.int32))), ("src", OCol("Int32", np.full(n, rank, np.int32))),
                        ("rn", OCol("Int64", np.arange(n))), ("x", OCol("Float64", rng.random(n)))])


def all_cases():
    """every (case, n_parts) the GPU file splits with ba.plan.hash_partition"""
    cases = [scatter_case(t, p, n) for p, n in SCATTER_PAIRS for t in KEY_TYPES] + SWITCH_CASES + SKEW_CASES
    cases += [sort_size_case(p, n) for p, n in SORT_PAIRS] + KEY_CASES + EMPTY_CASES
    return [(c, p) for c in cases for p in c.n_parts]
