"""TEST INFRASTRUCTURE shared by test_join_route_cases_cpu.py (CPU), test_join_routes_gpu.py and join_routes_gpu_child.py: the inputs
and the EXPECTED rows of HashJoinExec's single-key ("narrow") build and probe routes, at the places where each route's arithmetic
turns over (host/ops_join.cpp try_narrow, kernels_join.hip, kernels_hash.hip join_build_narrow[64] / join_key_present[64]).

The expectation is a plain equi-join: a dict from key value to build rows, NULL keys never matching, which yields (li, ri) pairs;
join_filter_cases.from_pairs turns the pairs into the rows of Inner / Left / Right / Full.  test_join_route_cases_cpu.py checks that
derivation against the CPU oracle's join, and that every case lies on the side of its limit that its name says.  Rows compare as
multisets keyed by the row ids li / ri, floats by bit pattern: nothing here has a tolerance.

A case is (name, key dtype, build keys, build validity, probe keys, probe validity, expected route).  Routes:
  tiny         tiny_rank_build alone (<= TINY_BUILD_ROWS rows spanning < TINY_BUILD_WINDOW values, unique)
  rank_sorted  join_key_stats -> rank_bits_sorted -> rank_pack (strictly increasing, no NULL: rank = row)
  rank_any     join_key_stats -> rank_bits_any -> rank_pack -> rank_perm
  table        join_build_narrow[64] (window_ok false: sparse keys, or no key at all)
  packed/<r>   a duplicate key, found on route <r>: the join ends on the general table (join_key_form() == "packed")"""
import functools
import os
import re
from collections import OrderedDict, namedtuple

import numpy as np

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og
from oracle.engine import OCol

import helpers
import join_filter_cases as JF
import join_types_cases as JT
import nljoin_cases as NC

ROOT = helpers.ROOT
CSRC = os.path.join(ROOT, "ballista_amd", "csrc")
TYPES = [JF.INNER, JF.LEFT, JF.RIGHT, JT.FULL]
ON = [("lk", "rk")]


# ---- constants, read from the sources -----------------------------------------------------------------------------------------------------

def source_text(rel):
    return open(os.path.join(CSRC, rel)).read()


def source_constant(rel, name):
    """a `constexpr <type> NAME = <integer expression>;` of a source file"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, source_text(rel))
    assert m, name
    return int(eval(re.sub(r"(\d)(?:ull|u)\b", r"\1", m.group(1)), {}))


TINY_BUILD_ROWS = source_constant("kernels_join.hip", "TINY_BUILD_ROWS")            # 1024
TINY_BUILD_WINDOW = source_constant("kernels_join.hip", "TINY_BUILD_WINDOW")        # 2^16: the tiny build takes range < this
SEL_TILE = source_constant("kernels.h", "SEL_TILE")                                  # 1024
JOIN_FILTER_MAX = source_constant("host/hash_kernels.h", "JOIN_FILTER_MAX")          # 3
_WINDOW_OK = re.search(r"window_ok = any_key && range <= \(1ull << window_log2\) && range / (\d+) <= \(uint64_t\)n \+ (\d+);", source_text("host/ops_join.cpp"))
assert _WINDOW_OK, "try_narrow's window_ok has changed: restate it here"
WINDOW_DIV, WINDOW_SLACK = int(_WINDOW_OK.group(1)), int(_WINDOW_OK.group(2))        # 4096, 256
RANK_WINDOW_LOG2 = 36                    # try_narrow: env_int("BHIP_RANK_WINDOW_LOG2", 36)
PRESENT_MIN_ROWS, PRESENT_MAX_RANGE = 1 << 18, 1 << 30      # try_narrow: `range <= (1ull << 30) && n >= (1 << 18)` in front of the CAS table
TABLE_CAPACITY_SOURCE = "inline uint64_t table_capacity(uint64_t rows) { uint64_t cap = 1024; while (cap < 2 * rows) cap <<= 1; return cap; }"
MIX64_SOURCE = ["z += 0x9E3779B97F4A7C15ull;", "z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;", "z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;",
                "return z ^ (z >> 31);"]
M64 = (1 << 64) - 1


def table_capacity(rows):
    """host/core.hpp table_capacity (TABLE_CAPACITY_SOURCE, which the CPU tier looks up there)"""
    cap = 1024
    while cap < 2 * rows:
        cap <<= 1
    return cap


def mix64(z):
    """vm_device.h mix64 (MIX64_SOURCE); the 4-byte table hashes the key's 32 bits zero-extended, the 8-byte table its 64 bits"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def window_ok(rng_, n, log2=RANK_WINDOW_LOG2):
    """try_narrow's choice of the rank map for n build rows whose valid keys span rng_ = kmax - kmin (None: no valid key)"""
    return rng_ is not None and rng_ <= (1 << log2) and rng_ // WINDOW_DIV <= n + WINDOW_SLACK


def window_limit(n):
    """the largest range the rank map takes for n build rows"""
    return WINDOW_DIV * (n + WINDOW_SLACK) + WINDOW_DIV - 1


# ---- key types -----------------------------------------------------------------------------------------------------------------------------
# HashJoinExec::narrow_key_width: Int32 / Date32 (4 bytes), Int64 / UInt64 (8 bytes); the plan refuses a key pair of two different types
# ("join keys .. have different types"), so each type joins itself.  Keys are generated as SIGNED integers of the width (the order join_key_stats compares in: key ^ sign bit as unsigned); a UInt64 column
# holds the same 64 bits

DTYPES = ["Int32", "Date32", "Int64", "UInt64"]
WIDTH = {"Int32": 4, "Date32": 4, "Int64": 8, "UInt64": 8}


def domain(width):
    return (-(1 << 31), (1 << 31) - 1) if width == 4 else (-(1 << 63), (1 << 63) - 1)


def as_column_values(dtype, signed):
    signed = np.asarray(signed, np.int64)
    return signed.astype(np.int32) if WIDTH[dtype] == 4 else signed.view(np.uint64) if dtype == "UInt64" else signed


def signed_view(dtype, values):
    values = np.asarray(values)
    return values.view(np.int64) if dtype == "UInt64" else values.astype(np.int64)


def home_slot(dtype, signed_key, cap):
    """the slot join_build_narrow[64] tries first"""
    return mix64(signed_key & (0xFFFFFFFF if WIDTH[dtype] == 4 else M64)) & (cap - 1)


Case = namedtuple("Case", "name dtype bkeys bvalid pkeys pvalid route")


def key_stats(case):
    """(n, kmin, kmax) over the valid build keys, signed Python integers (None, None: no valid key)"""
    k = signed_view(case.dtype, case.bkeys)
    if case.bvalid is not None:
        k = k[case.bvalid]
    return (len(case.bkeys), None, None) if len(k) == 0 else (len(case.bkeys), int(k.min()), int(k.max()))


def is_sorted(case):
    """join_key_stats' "strictly increasing and no NULL-able column" """
    k = signed_view(case.dtype, case.bkeys)
    return case.bvalid is None and bool(np.all(k[1:] > k[:-1]))


def has_duplicates(case):
    k = signed_view(case.dtype, case.bkeys)
    if case.bvalid is not None:
        k = k[case.bvalid]
    return len(np.unique(k)) != len(k)


# ---- the probe side of a build case ----------------------------------------------------------------------------------------------------------
# one stream of batches around the wave (64), one pass of a wave (FP_CHUNK = 256) and the selection tile (SEL_TILE): the last-tile EDGE
# variant, interior tiles, the prefetch past the final tile; then a batch in which no row matches and one in which every row does (the
# rank probe's LDS strip of 192 entries flushes at more than 128)
PROBE_BATCHES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
N_MAIN = sum(PROBE_BATCHES)
N_NONE = N_ALL = 300
BATCH_ROWS = PROBE_BATCHES + [N_NONE, N_ALL]
N_PROBE = sum(BATCH_ROWS)
BIG_BATCH_AT = sum(PROBE_BATCHES[:-1])                                    # first row of the 2049-row batch
NULL_ROWS = sorted({0, 63, 64, 1023, 1024, N_PROBE - 1} | {BIG_BATCH_AT + r for r in (0, 63, 64, 1023, 1024, 2048)})


def uniform(rng, lo, hi, size):
    """integers of [lo, hi] (Python integers up to the whole 64-bit domain) as int64"""
    r = rng.integers(0, hi - lo, size, dtype=np.uint64, endpoint=True)
    return (r + np.uint64(lo & M64)).view(np.int64)


def edge_keys(width, kmin, kmax, some_present):
    """the probe keys at which the window arithmetic turns over, for a build side spanning [kmin, kmax]"""
    span = kmax - kmin
    last_bit = kmin + 64 * ((span >> 6) + 1) - 1             # the last bit of the last map word
    e = [kmin - 1, kmin, kmax, kmax + 1, last_bit, last_bit + 1]
    lo, hi = domain(width)
    e += [lo, hi, lo + 1, hi - 1]
    if width == 4:
        e += [kmin - 1 - k for k in (0, 31, 32)]             # 32-bit offsets that wrap to just under 2^32: the dropped-row word of MAPBUF / BITS
    else:
        e += [kmin + (1 << 32), kmin + (1 << 34) - 1, kmin + (1 << 34), kmin + (1 << 63), kmin - 1, kmin - 1 - 31, kmin - 1 - 32]
        for k in some_present:                                # the low 32 bits of a present key's offset, 2^32 and 2^34 further on
            e += [k + (1 << 32), k + (1 << 34), k - (1 << 32)]
    return [k for k in e if lo <= k <= hi]


EXTRA_ROW = 2                             # a probe row that is never NULL and never an edge key's: a case's own extra probe key


def make_probe(rng, width, valid_keys, extra=None):
    """-> (signed probe keys, validity): about half of the random rows match; the edge keys sit on rows that are never NULL"""
    lo, hi = domain(width)
    present = set(valid_keys.tolist())
    if present:
        kmin, kmax = min(present), max(present)
        near = uniform(rng, max(lo, kmin - 64), min(hi, kmax + 64), N_MAIN)
        dense = float(np.isin(near, valid_keys).mean())       # a dense window: some of the rows drawn from around it match too
        picked = rng.random(N_MAIN) < max(0.0, (0.5 - dense) / (1.0 - dense + 1e-9))
        keys = np.where(picked, valid_keys[rng.integers(0, len(valid_keys), N_MAIN)], near)
        edges = edge_keys(width, kmin, kmax, [int(valid_keys[i]) for i in (0, len(valid_keys) // 2, len(valid_keys) - 1)])
    else:
        kmin = kmax = 0
        keys = uniform(rng, -1000, 1000, N_MAIN)
        edges = edge_keys(width, 0, 0, [])
    free = np.setdiff1d(np.arange(N_MAIN), NULL_ROWS + [EXTRA_ROW])
    keys[rng.choice(free, len(edges), replace=False)] = np.array(edges, np.int64)
    if extra is not None:
        keys[EXTRA_ROW] = extra
    # absent keys: the nearest above the window, then below it, then anywhere
    cand = [k for k in list(range(kmax + 1, kmax + 1 + 2 * N_NONE)) + list(range(kmin - 1, kmin - 1 - 2 * N_NONE, -1)) if lo <= k <= hi and k not in present]
    cand += [int(k) for k in uniform(rng, lo, hi, 4 * N_NONE) if int(k) not in present]
    none = np.array(cand[:N_NONE], np.int64)
    assert len(none) == N_NONE
    every = valid_keys[rng.integers(0, len(valid_keys), N_ALL)] if present else uniform(rng, -1000, 1000, N_ALL)
    valid = np.ones(N_PROBE, np.bool_)
    valid[NULL_ROWS] = False
    return np.concatenate([keys, none, every]), valid


# ---- the build cases -------------------------------------------------------------------------------------------------------------------------

def offsets(rng, n, span):
    """n distinct sorted offsets of [0, span) that include 0 and span - 1"""
    if n == 1:
        assert span == 1
        return np.zeros(1, np.int64)
    assert span >= n
    inner_n, pool = n - 2, span - 2
    if pool <= 8 * inner_n + 16:
        inner = rng.permutation(pool)[:inner_n] + 1
    else:
        draw = np.unique(uniform(rng, 1, span - 2, 2 * inner_n + 16))
        assert len(draw) >= inner_n
        inner = rng.permutation(draw)[:inner_n]
    return np.sort(np.concatenate([[0, span - 1], inner]).astype(np.int64))


def null_rows(n):
    """NULL build keys at rows 0, 63, 64 and n - 1 — but a build side of two rows keeps its second, so that it has a key at all (one
    row: the all-NULL build side, a case of its own)"""
    return [r for r in ((0,) if n <= 2 else (0, 63, 64, n - 1)) if r < n]


PIECE_RUNS = [1, 31, 32, 33, 5, 64, 2, 30, 3, 63, 17]         # keys per run of consecutive key values; a gap of >= one 32-bit piece between runs
N_PIECES = 1061                                              # rows of the piece-logic case: not a multiple of 64, the last run ends on the last row


def piece_offsets():
    """rank_bits_sorted's piece logic: sorted offsets whose runs fill one 32-bit piece with 1, 31 and 32 keys, run over a piece's end
    (33, 63, 64), and — because the run lengths do not divide 64 — start, end and straddle at every lane of a wave"""
    out, at, i = [], 0, 0
    while len(out) < N_PIECES:
        run = min(PIECE_RUNS[i % len(PIECE_RUNS)], N_PIECES - len(out))
        out += list(range(at, at + run))
        at = ((at + run + 31) // 32 + 1) * 32               # the next run starts on a piece boundary, one empty piece further on
        i += 1
    return np.array(out, np.int64)


def collision_keys(dtype, cap, n_keys=6):
    """small positive keys whose home slot is cap - 1 or cap - 2 (linear probing wraps to slot 0), and one more with such a home that
    the build side does not get: its probe walks the whole cluster to an empty slot"""
    found, k = [], 1
    while len(found) < n_keys + 1:
        if home_slot(dtype, k, cap) >= cap - 2:
            found.append(k)
        k += 1
    return found[:n_keys], found[n_keys]


BASES = {4: [1000, -40_000, -5, 100_003], 8: [10 ** 11 + 3, -(1 << 40), -5, 7_000_000_123]}


@functools.lru_cache(maxsize=None)
def build_cases(dtype):
    """the build-route cases of one key type, each with its probe side"""
    width = WIDTH[dtype]
    lo, hi = domain(width)
    out = []

    def add(name, signed, nulls, route, shuffle=False, extra=None):
        rng = np.random.default_rng(len(out) * 101 + DTYPES.index(dtype) * 7 + 11)
        signed = np.asarray(signed, np.int64)
        if shuffle:
            signed = rng.permutation(signed)
            if np.all(signed[1:] > signed[:-1]):            # (two rows: half of the permutations are the sorted one)
                signed = signed[::-1].copy()
        bvalid = None
        if nulls:
            bvalid = np.ones(len(signed), np.bool_)
            bvalid[nulls] = False
        pk, pv = make_probe(rng, width, signed if bvalid is None else signed[bvalid], extra)
        out.append(Case(name, dtype, as_column_values(dtype, signed), bvalid, as_column_values(dtype, pk), pv, route))

    def dense(n, span, base_index):
        rng = np.random.default_rng(n * 13 + span % 1009 + base_index)
        return offsets(rng, n, span) + BASES[width][base_index % 4]

    # ---- tiny -------------------------------------------------------------------------------------------------------------------------------
    for i, n in enumerate([1, 2, 64, 1023, 1024]):
        keys = dense(n, 1 if n == 1 else 3 * n + 5, i)
        add("tiny/sorted_n%d" % n, keys, None, "tiny")
        add("tiny/shuffled_n%d" % n, keys, None, "tiny", shuffle=True)
        # (one row and it is NULL: no key at all — no map, an empty CAS table)
        add("tiny/nulls_n%d" % n, keys, null_rows(n), "table" if n == 1 else "tiny")
    # (range = kmax - kmin; the tiny build takes range < TINY_BUILD_WINDOW)
    add("tiny/range_65534", dense(25, TINY_BUILD_WINDOW - 1, 1), None, "tiny")
    add("tiny/range_65535", dense(25, TINY_BUILD_WINDOW, 2), None, "tiny")                        # the last the LDS key set holds
    add("tiny/range_65535_shuffled_n1024", dense(1024, TINY_BUILD_WINDOW, 3), None, "tiny", shuffle=True)
    add("tiny/range_65536", dense(25, TINY_BUILD_WINDOW + 1, 3), None, "rank_sorted")             # declined: the general rank map
    add("tiny/range_65536_shuffled_n1024", dense(1024, TINY_BUILD_WINDOW + 1, 0), None, "rank_any", shuffle=True)
    dup = dense(700, 3000, 1)
    dup[350] = dup[349]
    add("tiny/duplicate", dup, None, "packed/tiny")
    add("tiny/n1025", dense(TINY_BUILD_ROWS + 1, 5000, 2), None, "rank_sorted")

    # ---- rank map -----------------------------------------------------------------------------------------------------------------------------
    for i, n in enumerate([1025, 4097]):
        add("rank/sorted_n%d" % n, dense(n, 4 * n + 3, i), None, "rank_sorted")
        add("rank/shuffled_n%d" % n, dense(n, 4 * n + 3, i + 1), None, "rank_any", shuffle=True)
        add("rank/nulls_n%d" % n, dense(n, 4 * n + 3, i + 2), null_rows(n), "rank_any")
        add("rank/window_limit_n%d" % n, dense(n, window_limit(n) + 1, i + 3), None, "rank_sorted")
        add("rank/window_limit_shuffled_n%d" % n, dense(n, window_limit(n) + 1, i), None, "rank_any", shuffle=True)
        add("rank/window_limit_plus_1_n%d" % n, dense(n, window_limit(n) + 2, i + 1), None, "table")
    add("rank/pieces", piece_offsets() + BASES[width][0], None, "rank_sorted")
    add("rank/pieces_across_zero", piece_offsets() - 1500, None, "rank_sorted")                  # the sign bias of join_key_stats: kmin < 0 < kmax
    add("rank/at_type_min", dense(1025, 5000, 0) - BASES[width][0] + lo, None, "rank_sorted")    # kmin - 1 does not exist
    add("rank/at_type_max", dense(1025, 5000, 0) - BASES[width][0] + hi - 4999, None, "rank_sorted")
    add("rank/at_type_max_shuffled", dense(1025, 5000, 1) - BASES[width][1] + hi - 4999, None, "rank_any", shuffle=True)
    dup = dense(1500, 6000, 3)
    dup[10] = dup[1400]
    add("rank/duplicate_unsorted", dup, None, "packed/rank", shuffle=True)
    dup = dense(1500, 6000, 0)
    dup[701] = dup[700]                                                                          # sorted but for `nb <= b` at one row
    add("rank/duplicate_sorted", dup, None, "packed/rank")

    # ---- CAS table: sparse by the data alone -----------------------------------------------------------------------------------------------------
    def sparse(n, seed, fixed=()):
        rng = np.random.default_rng(seed)
        fill = np.unique(uniform(rng, lo, hi, 2 * n + 64))
        fill = rng.permutation(fill[~np.isin(fill, np.array(fixed, np.int64))])[: n - len(fixed)]
        return np.concatenate([np.array(fixed, np.int64), fill])

    # (a single key spans nothing: window_ok holds for every n = 1, so ONE row reaches the CAS table only under BHIP_JOIN_TABLE=1 —
    # join_routes_gpu_child.py; by the data alone the smallest table has two rows)
    add("table/n1", np.array([BASES[width][2]], np.int64), None, "tiny")
    add("table/n2", np.array([lo + 5, hi - 7], np.int64), None, "table")
    for n in (300, 5000):
        add("table/n%d" % n, sparse(n, n), None, "table")
    add("table/nulls_n300", sparse(300, 4), null_rows(300), "table")
    ends = [lo, -1, 0, 1, hi] if width == 4 else [lo, -1, 0, hi]
    add("table/type_ends", sparse(300, 5, ends), None, "table", shuffle=True)
    add("table/key_0_at_row_0", sparse(300, 6, [0]), None, "table")                              # 4-byte slot word: 0 | (0 + 1) << 32
    cluster, absent = collision_keys(dtype, table_capacity(300))
    add("table/collisions", sparse(300, 7, cluster), None, "table", shuffle=True, extra=absent)
    dup = sparse(300, 8)
    dup[200] = dup[17]
    add("table/duplicate", dup, None, "packed/table")
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return [c for t in DTYPES for c in build_cases(t)]


def cases(prefix=None, dtype=None):
    return [c for c in all_cases() if (prefix is None or c.name.startswith(prefix)) and (dtype is None or c.dtype == dtype)]


def case_id(c):
    return "%s-%s" % (c.dtype, c.name)


def find(dtype, name):
    return next(c for c in all_cases() if c.dtype == dtype and c.name == name)


# ---- the two sides and the expected rows ------------------------------------------------------------------------------------------------------

SPECIAL_FLOATS = [float("nan"), -0.0, float("inf"), -float("inf"), 5e-324]


def payload(rng, n, prefix):
    x = rng.integers(0, 1000, n) / 8.0
    x[::97] = np.resize(SPECIAL_FLOATS, len(x[::97]))
    return [(prefix + "x", OCol("Float64", x)), (prefix + "s", OCol("Utf8", ["%s%d" % (prefix, i % 13) + "-" * (i % 5) for i in range(n)]))]


_SIDES = {}


def sides(case, probe_nulls):
    """-> (left, right): lk, lx (Float64), ls (Utf8), li / rk, rx, rs, ri.  One object per (case, probe_nulls): never modified"""
    key = (case.dtype, case.name, bool(probe_nulls))
    if key not in _SIDES:
        rng = np.random.default_rng(len(case.bkeys) + 3)
        nl, nr = len(case.bkeys), len(case.pkeys)
        left = JT.with_ids("l", nl, [("lk", OCol(case.dtype, case.bkeys, case.bvalid))] + payload(rng, nl, "l"))
        right = JT.with_ids("r", nr, [("rk", OCol(case.dtype, case.pkeys, case.pvalid if probe_nulls else None))] + payload(rng, nr, "r"))
        _SIDES[key] = (left, right)
    return _SIDES[key]


def reference_pairs(left, right, on=ON):
    """the equi-join by its definition: a dict from key to build rows; a NULL in any key part matches nothing.  -> (li, ri) row numbers"""
    lcols, rcols = [left[a].to_pylist() for a, _ in on], [right[b].to_pylist() for _, b in on]
    table = {}
    for i, k in enumerate(zip(*lcols)):
        if None not in k:
            table.setdefault(k, []).append(i)
    li, ri = [], []
    for j, k in enumerate(zip(*rcols)):
        if None not in k:
            for i in table.get(k, ()):
                li.append(i)
                ri.append(j)
    return np.array(li, np.int64), np.array(ri, np.int64)


_PAIRS = {}


def pairs(left, right, on=ON):
    key = (id(left), id(right), tuple(on))
    if key not in _PAIRS:
        _PAIRS[key] = (left, right) + reference_pairs(left, right, on)
    return _PAIRS[key][2:]


def expected(jt, left, right, on=ON):
    li, ri = pairs(left, right, on)
    return JF.from_pairs(jt, left, right, on, li, ri)


assert_same_rows = NC.assert_same_rows


# ---- plans and route assertions -----------------------------------------------------------------------------------------------------------------

def cut(batch, rows):
    at = np.concatenate([[0], np.cumsum(rows)])
    assert at[-1] == og.batch_len(batch)
    return [helpers.slice_batch(batch, int(a), int(b)) for a, b in zip(at, at[1:])]


def build_exec(ctx, left):
    """the build rows in one partition of two batches (join_key_stats and the rank kernels see their concatenation)"""
    n = og.batch_len(left)
    return helpers.memory_exec(ctx, [cut(left, [n // 3, n - n // 3]) if n > 1 else [left]])


def probe_exec(ctx, right, rows=None):
    """ONE partition (Left and Full answer for the build side), the batches of BATCH_ROWS in one stream"""
    return helpers.memory_exec(ctx, [cut(right, rows or BATCH_ROWS)])


def timing_context():
    """a context that records every launch under its name (BHIP_KERNEL_TIMING is read when a context is made)"""
    old = os.environ.get("BHIP_KERNEL_TIMING")
    os.environ["BHIP_KERNEL_TIMING"] = "2"
    try:
        return ba.Context(0)
    finally:
        if old is None:
            del os.environ["BHIP_KERNEL_TIMING"]
        else:
            os.environ["BHIP_KERNEL_TIMING"] = old


BUILD_KERNELS = {"tiny_rank_build", "join_key_stats", "rank_bits_sorted", "rank_bits_any", "rank_pack", "rank_perm", "join_build_narrow",
                 "join_key_present", "join_key_present64"}
# route -> (the kernels that ran, the kernels that did not)
ROUTE_KERNELS = {
    "tiny": ({"tiny_rank_build"}, BUILD_KERNELS - {"tiny_rank_build"}),
    "rank_sorted": ({"join_key_stats", "rank_bits_sorted", "rank_pack"}, {"rank_bits_any", "rank_perm", "join_build_narrow"}),
    "rank_any": ({"join_key_stats", "rank_bits_any", "rank_pack", "rank_perm"}, {"rank_bits_sorted", "join_build_narrow"}),
    "table": ({"join_key_stats", "join_build_narrow"}, {"rank_bits_sorted", "rank_bits_any", "rank_pack", "rank_perm"}),
    "packed/tiny": ({"tiny_rank_build", "join_key_stats", "rank_bits_any"}, {"rank_bits_sorted", "rank_perm", "join_build_narrow"}),
    "packed/rank": ({"join_key_stats", "rank_bits_any"}, {"rank_bits_sorted", "rank_perm", "join_build_narrow", "tiny_rank_build"}),
    "packed/table": ({"join_key_stats", "join_build_narrow"}, {"rank_bits_sorted", "rank_bits_any", "rank_perm"}),
}


def assert_route(names, route, n, forced_table=False):
    ran, not_ran = ROUTE_KERNELS[route]
    if forced_table:                                        # BHIP_JOIN_TABLE=1 skips the tiny build and still reads the statistics
        ran, not_ran = ran - {"tiny_rank_build"}, not_ran | {"tiny_rank_build"}
    assert ran <= names, (route, sorted(ran - names), sorted(names))
    assert not (not_ran & names), (route, sorted(not_ran & names))
    if n > TINY_BUILD_ROWS:
        assert "tiny_rank_build" not in names


def rank_probe_form(perm=False, resid=False, bits=False, width=4, mode=None):
    """the name launch_join_filter_probe gives the one-read kernel's variant (every map of these tests fits a buffer descriptor)"""
    kind = "flat" if mode == "flat" else "bits" if bits and not perm and not resid and mode != "nobits" else "mapbuf"
    return "rank/" + kind + ("+perm" if perm else "") + ("+resid" if resid else "") + \
        ("+rows8" if mode == "rows8" and width == 4 and not perm else "") + ("+gather" if mode == "noscalar" and kind != "flat" else "")


def run_case(ctx, case, jt, probe_nulls, route=None, mode=None, left=None, forbid=()):
    """one join of a build case: the rows against the reference; with `route`, the kernels by name (ctx: a timing context) and the probe
    variant.  `left`: the build rows to use in place of the case's own (a shuffled copy: the expectation is the same)"""
    own, right = sides(case, probe_nulls)
    plan = ba.HashJoinExec(build_exec(ctx, own if left is None else left), probe_exec(ctx, right), ON, jt)
    if route is not None:
        ctx.kernel_stats(reset=True)
    got = JF.rows(plan)
    assert_same_rows(got, expected(jt, own, right))
    if route is None:
        return got
    names = set(ctx.kernel_stats(reset=True))
    n = len(case.bkeys)
    assert_route(names, route, n, forced_table=mode == "table")
    assert not names & set(forbid), sorted(names & set(forbid))
    packed = route.startswith("packed/")
    assert ctx.join_key_form() == ("packed" if packed else "narrow")
    if packed:
        assert not names & {"join_rank_probe", "join_filter_probe"}, sorted(names)
        return got
    ranked = route != "table"
    perm = route == "rank_any" or (route == "tiny" and not is_sorted(case))
    direct_last = ranked and jt == JF.INNER and not probe_nulls
    if direct_last:                                          # every batch through the one-read kernel
        assert "join_rank_probe" in names and "join_filter_probe" not in names, sorted(names)
        assert ctx.join_probe_form() == rank_probe_form(perm, width=WIDTH[case.dtype], mode=mode), ctx.join_probe_form()
    else:                                                    # NULL probe keys, an outer join or the CAS table: the general kernel (the last batch has a NULL)
        assert "join_filter_probe" in names, sorted(names)
        assert ("join_rank_probe" in names) == (ranked and jt == JF.INNER), sorted(names)      # the batches without a NULL
        assert ctx.join_probe_form() == ("filter/map" if ranked else "filter/table"), ctx.join_probe_form()
    return got


# ---- probe shapes: one rank-map build each, sorted and shuffled ------------------------------------------------------------------------------

SHAPE_NL, SHAPE_NR = 1025, 2 * SEL_TILE + 257
SHAPE_BATCHES = [SEL_TILE + 1, SHAPE_NR - SEL_TILE - 1]
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
# name -> the terms (column, lo, hi): lo <= column <= hi
FILTERS = OrderedDict([
    ("one_term", [("ra", 10, 79)]),
    ("one_term_empty", [("ra", 80, 10)]),
    ("one_term_int32_ends", [("ra", I32_MIN, I32_MAX)]),
    ("three_terms", [("ra", 10, 79), ("rb", 9100, I32_MAX), ("rc", I32_MIN, 20)]),
    ("three_terms_one_empty", [("ra", 10, 79), ("rb", 9300, 9100), ("rc", -50, 50)]),
    ("three_terms_all_pass", [("ra", I32_MIN, I32_MAX), ("rb", 0, I32_MAX), ("rc", I32_MIN, I32_MAX)]),
])
SHAPE_SCHEMA = {"rk": "Int32", "ra": "Int32", "rb": "Date32", "rc": "Int32", "rx": "Float64", "rs": "Utf8", "ri": "Int64"}


@functools.lru_cache(maxsize=None)
def shape_sides(order, build="rank"):
    """1025 unique Int32 build keys (rank: over 4100 values; table: sparse), sorted or shuffled, with a second key column lb; a probe side
    with the range columns ra / rb / rc (ra and rc hold the Int32 ends) and a second key column that agrees with the build row's on most
    matches.  The same build rows in both orders, row ids and all"""
    rng = np.random.default_rng(77 if build == "rank" else 78)
    if build == "rank":
        lk = offsets(rng, SHAPE_NL, 4 * SHAPE_NL) + 2000
    else:
        lk = np.sort(np.unique(uniform(rng, I32_MIN, I32_MAX, 2 * SHAPE_NL))[rng.permutation(2 * SHAPE_NL - 8)[:SHAPE_NL]])
    lb = rng.integers(9000, 9012, SHAPE_NL)
    left = JT.with_ids("l", SHAPE_NL, [("lk", OCol("Int32", lk.astype(np.int32))), ("lb", OCol("Date32", lb.astype(np.int32)))] + payload(rng, SHAPE_NL, "l"))
    rk = np.where(rng.random(SHAPE_NR) < 0.5, lk[rng.integers(0, SHAPE_NL, SHAPE_NR)], uniform(rng, int(lk.min()) - 40, int(lk.max()) + 40, SHAPE_NR))
    rk[5:9] = [lk.min() - 1, lk.min(), lk.max(), lk.max() + 1]
    second = dict(zip(lk.tolist(), lb.tolist()))
    rb2 = np.where(rng.random(SHAPE_NR) < 0.7, np.array([second.get(int(k), 9000) for k in rk]), rng.integers(8998, 9014, SHAPE_NR))
    ra, rc = rng.integers(0, 100, SHAPE_NR), rng.integers(-50, 50, SHAPE_NR)
    ra[[3, SEL_TILE, SHAPE_NR - 1]] = [I32_MIN, I32_MAX, I32_MIN]
    rc[[4, SEL_TILE + 1, SHAPE_NR - 2]] = [I32_MAX, I32_MIN, I32_MAX]
    right = JT.with_ids("r", SHAPE_NR, [("rk", OCol("Int32", rk.astype(np.int32))), ("ra", OCol("Int32", ra.astype(np.int32))),
                                        ("rb", OCol("Date32", rng.integers(9000, 9400, SHAPE_NR).astype(np.int32))), ("rc", OCol("Int32", rc.astype(np.int32))),
                                        ("rb2", OCol("Date32", rb2.astype(np.int32)))] + payload(rng, SHAPE_NR, "r"))
    if order == "shuffled":
        perm = np.random.default_rng(5).permutation(SHAPE_NL)
        left = OrderedDict((k, c.take(perm)) for k, c in left.items())
    return left, right


def filter_expr(name):
    e = None
    for c, lo_, hi_ in FILTERS[name]:
        t = (col(c) >= lit(lo_, SHAPE_SCHEMA[c])).and_(col(c) <= lit(hi_, SHAPE_SCHEMA[c]))
        e = t if e is None else e.and_(t)
    return E.coerce(e, dict(SHAPE_SCHEMA, rb2="Date32"))


def filter_keep(name, right):
    """the rows the terms keep, in numpy"""
    keep = np.ones(og.batch_len(right), np.bool_)
    for c, lo_, hi_ in FILTERS[name]:
        v = right[c].values.astype(np.int64)
        keep &= (v >= lo_) & (v <= hi_)
    return keep


_KEPT = {}


def kept_side(name, right):
    key = (name, id(right))
    if key not in _KEPT:
        _KEPT[key] = (right, JT.rows_where(right, filter_keep(name, right)))
    return _KEPT[key][1]


def probe_bytes(names, width):
    """the filter terms the probe kernels were launched with, from their algorithmic bytes: rows * (key width + 4 * terms) + rows / 8 per
    batch (ops_join.cpp probe_narrow)"""
    total = sum(names[k][2] for k in ("join_rank_probe", "join_filter_probe") if k in names)
    plain = sum(n * width + n // 8 for n in SHAPE_BATCHES)
    assert (total - plain) % (4 * SHAPE_NR) == 0, (total, plain)
    return (total - plain) // (4 * SHAPE_NR)


def run_filter_shape(ctx, order, name, jt, mode=None):
    """a FilterExec of range terms below the probe side: fused into the probe kernel (NF = 1 and NF = JOIN_FILTER_MAX)"""
    left, right = shape_sides(order)
    probe = ba.FilterExec(filter_expr(name), probe_exec(ctx, right, SHAPE_BATCHES))
    ctx.kernel_stats(reset=True)
    got = JF.rows(ba.HashJoinExec(build_exec(ctx, left), probe, ON, jt))
    assert_same_rows(got, expected(jt, left, kept_side(name, right)))
    stats = ctx.kernel_stats(reset=True)
    if any(lo_ > hi_ for _, lo_, hi_ in FILTERS[name]):
        # an empty range is not fused (sop.cpp build_sop "empty range: leave it to the VM"): the filter runs first, no row is left to probe
        assert not {"join_rank_probe", "join_filter_probe"} & set(stats), sorted(stats)
        return got
    kernel = "join_rank_probe" if jt == JF.INNER else "join_filter_probe"
    assert kernel in stats and not ({"join_rank_probe", "join_filter_probe"} - {kernel}) & set(stats), sorted(stats)
    assert probe_bytes(stats, 4) == len(FILTERS[name]), (probe_bytes(stats, 4), name)              # the terms went into the probe
    assert len(FILTERS[name]) in (1, JOIN_FILTER_MAX)
    want = rank_probe_form(order == "shuffled", mode=mode) if jt == JF.INNER else "filter/map"
    assert ctx.join_probe_form() == want, (ctx.join_probe_form(), want)
    return got


PAIR_ON = [("lk", "rk"), ("lb", "rb2")]


@functools.lru_cache(maxsize=None)
def pair_sides(form, build, order):
    """ON (lk, lb) = (rk, rb2).  first_column: the build side is unique on lk alone, lb rides along (RESID); pairs: unique as pairs only —
    both columns packed into one 8-byte key: a rank map when the first column holds ONE value (the packed keys then span the second
    column's few values), a CAS table when it holds several (2^32 packed values apart)"""
    left, right = shape_sides(order, build)
    if form == "first_column":
        return left, right
    rng = np.random.default_rng(91)
    n = SHAPE_NL
    a = np.full(n, 7) if build == "rank" else rng.integers(-3, 4, n)
    b = offsets(rng, n, 4 * n) + 9000 if build == "rank" else rng.permutation(4 * n)[:n] + 9000
    if order == "shuffled" or build == "table":
        b = rng.permutation(b)
    left = JT.with_ids("l", n, [("lk", OCol("Int32", a.astype(np.int32))), ("lb", OCol("Date32", b.astype(np.int32)))] + payload(rng, n, "l"))
    nr = SHAPE_NR
    pick = rng.integers(0, n, nr)
    hit = rng.random(nr) < 0.5
    ra_ = np.where(hit | (rng.random(nr) < 0.5), a[pick], rng.integers(-4, 9, nr))
    rb_ = np.where(hit, b[pick], rng.integers(8990, 9000 + 4 * n + 10, nr))
    right = JT.with_ids("r", nr, [("rk", OCol("Int32", ra_.astype(np.int32))), ("rb2", OCol("Date32", rb_.astype(np.int32)))] + payload(rng, nr, "r"))
    return left, right


def run_pair_shape(ctx, form, build, order, jt, mode=None):
    left, right = pair_sides(form, build, order)
    ctx.kernel_stats(reset=True)
    got = JF.rows(ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right, SHAPE_BATCHES), PAIR_ON, jt))
    assert_same_rows(got, expected(jt, left, right, PAIR_ON))
    names = set(ctx.kernel_stats(reset=True))
    assert ctx.join_key_form() == "narrow"
    assert ("pack_key_pair" in names) == (form == "pairs"), sorted(names)
    ranked = build == "rank" and mode not in ("table", "window10")
    if build == "rank" and mode != "window10":
        assert ("join_build_narrow" in names) == (mode == "table")
    else:
        # (pairs: the first column alone was tried first, on the rank map, and declined for its duplicates)
        assert "join_build_narrow" in names and (form == "pairs" or not names & {"rank_bits_sorted", "rank_bits_any"}), sorted(names)
    resid = form == "first_column"
    if ranked and jt == JF.INNER:
        want = rank_probe_form(order == "shuffled", resid, width=4 if resid else 8, mode=mode)
    else:
        want = ("filter/map" if ranked else "filter/table") + ("+resid" if resid else "")
    assert ctx.join_probe_form() == want, (ctx.join_probe_form(), want)
    return got


SEMI_EXPRS = [(col("rk"), "rk"), (col("rx"), "rx"), (col("ri"), "ri")]


def run_semi_shape(ctx, order, mode=None):
    """a parent projection that reads no build column over an Inner join on a one-column build: nothing is staged; sorted: the key-set
    words alone (BITS), shuffled: the packed map"""
    left, right = shape_sides(order)
    plan = ba.ProjectionExec(SEMI_EXPRS, ba.HashJoinExec(build_exec(ctx, left), probe_exec(ctx, right, SHAPE_BATCHES), ON, JF.INNER))
    got = JF.rows(plan)
    assert_same_rows(got, og.project(expected(JF.INNER, left, right), SEMI_EXPRS))
    want = rank_probe_form(order == "shuffled", bits=True, mode=mode)
    assert ctx.join_probe_form() == want, (ctx.join_probe_form(), want)
    return got


def shape_runs():
    """(function, arguments) of every probe-shape case: what test_join_routes_gpu.py runs in process and the child under the probe switches"""
    out = []
    for order in ("sorted", "shuffled"):
        for name in FILTERS:
            for jt in (JF.INNER, JF.LEFT):
                out.append((run_filter_shape, (order, name, jt)))
        for form in ("first_column", "pairs"):
            for build in ("rank", "table"):
                for jt in (JF.INNER, JF.RIGHT):
                    out.append((run_pair_shape, (form, build, order, jt)))
        out.append((run_semi_shape, (order,)))
    return out


# ---- the key-set bitmap in front of the CAS table (BHIP_JOIN_TABLE=1: no data reaches it) --------------------------------------------------------

def present_sides(dtype, n):
    """n unique build keys spanning < 2^30 values, shuffled; 5000 probe rows with the window-edge keys, in two batches"""
    width = WIDTH[dtype]
    rng = np.random.default_rng(n + width)
    span = PRESENT_MAX_RANGE - 5
    lk = rng.permutation(offsets(rng, n, span)) + (-(1 << 29) + 11 if width == 4 else 10 ** 12 + 1)
    valid = np.ones(n, np.bool_)
    valid[null_rows(n)] = False
    live = lk[valid]
    kmin, kmax = int(live.min()), int(live.max())
    nr = 5000
    rk = np.where(rng.random(nr) < 0.5, live[rng.integers(0, len(live), nr)], uniform(rng, kmin - 64, kmax + 64, nr))
    edges = edge_keys(width, kmin, kmax, [int(live[0]), int(live[len(live) // 2])])
    rk[100:100 + len(edges)] = edges
    rv = np.ones(nr, np.bool_)
    rv[[0, 63, 64, 1023, 1024, nr - 1]] = False
    left = JT.with_ids("l", n, [("lk", OCol(dtype, as_column_values(dtype, lk), valid)), ("lx", OCol("Float64", rng.integers(0, 1000, n) / 8.0))])
    right = JT.with_ids("r", nr, [("rk", OCol(dtype, as_column_values(dtype, rk), rv))] + payload(rng, nr, "r"))
    return left, right, kmax - kmin
