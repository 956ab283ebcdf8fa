"""TEST INFRASTRUCTURE shared by test_scan_cases_cpu.py (CPU) and test_scan_forms_gpu.py: inputs and EXPECTED values on each side of
the limits at which the device prefix scan changes its launch form (kernels_util.hip exclusive_scan_t and launch_rank_pack):

  none    n == 0: two memsets
  one     n <= SCAN_ONE_LAUNCH_MAX: one workgroup walks the chunks with a running carry
  two     up to SCAN_TWO_LAUNCH_CHUNKS chunks: chunk sums, then every workgroup adds up the raw sums before its own
  three   more chunks: chunk sums, their scan by one workgroup, the apply launch

The limits are read from the source, so a changed constant moves the cases with it.  Three users of the scan are driven through plans:

  cast    u32 -> i32 with the total written behind the last offset (utf8_from_lengths): CAST(Int32 AS Utf8); the expected offsets are
          the exclusive cumulative sum of the digit counts, in numpy
  probe   u32 -> u64 without the total (the general join table's count -> scan -> emit): an Inner join on a build side with duplicate
          keys; the expected pairs are a dict join (key -> build rows), expanded over the probe rows in numpy
  rank    the rank map (launch_rank_pack) of a unique integer build side, by its granule count

Nothing here has a tolerance: offsets and bytes compare exactly, pairs as multisets of row ids."""
import functools
import re
from collections import OrderedDict, namedtuple

import numpy as np

from oracle.engine import OCol

import join_route_cases as RC


def source_constants(rel, names):
    """`constexpr <type> NAME = <integer expression>;` of a source file, each in terms of the ones before it"""
    text, env = RC.source_text(rel), {}
    for name in names:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, name
        expr = re.sub(r"(\d)(?:ull|u)\b", r"\1", re.sub(r"\(\s*\w+_t\s*\)", "", m.group(1)))
        env[name] = int(eval(expr, {}, env))
    return env


_K = source_constants("kernels_util.hip", ["SCAN_BLOCK", "SCAN_ITEMS", "SCAN_CHUNK", "SCAN_TWO_LAUNCH_CHUNKS", "SCAN_ONE_LAUNCH_MAX", "RP_ROUND",
                                           "RP_ROUNDS", "RP_CHUNK"])
C = SCAN_CHUNK = _K["SCAN_CHUNK"]                                   # 4096
SCAN_ONE_LAUNCH_MAX = _K["SCAN_ONE_LAUNCH_MAX"]                     # 8 chunks
SCAN_TWO_LAUNCH_CHUNKS = _K["SCAN_TWO_LAUNCH_CHUNKS"]               # 2048
RP_CHUNK = _K["RP_CHUNK"]                                           # 16384 granules
# the ladder itself, as both launchers state it (the CPU tier looks these lines up)
LADDER_SOURCE = ["if (n <= SCAN_ONE_LAUNCH_MAX) {", "if (n_chunks <= SCAN_TWO_LAUNCH_CHUNKS) {"]
N_GRAN_SOURCE = "const int64_t n_words = (int64_t)(range >> 6) + 1, n_gran = 2 * n_words;"          # host/ops_join.cpp try_narrow


def launch_form(n, chunk=SCAN_CHUNK):
    if n <= 0:
        return "none"
    if n <= SCAN_ONE_LAUNCH_MAX:
        return "one"
    return "two" if (n + chunk - 1) // chunk <= SCAN_TWO_LAUNCH_CHUNKS else "three"


TWO = SCAN_TWO_LAUNCH_CHUNKS * C                                    # about 8.39 M: the last size of the two-launch form
# (name, n, the form the name says)
SIZES = [("0", 0, "none"), ("1", 1, "one"), ("chunk_minus_1", C - 1, "one"), ("chunk", C, "one"), ("chunk_plus_1", C + 1, "one"),
         ("one_launch_max", SCAN_ONE_LAUNCH_MAX, "one"), ("one_launch_max_plus_1", SCAN_ONE_LAUNCH_MAX + 1, "two"),
         ("two_launch_chunks", TWO, "two"), ("two_launch_chunks_plus_1", TWO + 1, "three"),
         ("two_launch_chunks_plus_chunk_plus_1", TWO + C + 1, "three")]
SIZE_IDS = [s[0] for s in SIZES]
N_MAX = max(n for _, n, _ in SIZES)
SMALL_MAX = SCAN_ONE_LAUNCH_MAX + 1                                 # up to here every row's bytes and pairs are looked at one by one


def chunk_boundaries(n, chunk=C):
    """the first rows of the chunks after the first"""
    return np.arange(chunk, n, chunk, dtype=np.int64)


def windows(n):
    """the row windows whose value bytes are compared at the large sizes: the first and the last 2 * C rows and the 2 * C rows around
    the last chunk boundary (all rows when the windows cover them)"""
    if n <= SMALL_MAX:
        return [(0, n)]
    last = (n - 1) // C * C
    return [(0, 2 * C), (last - C, min(n, last + C)), (n - 2 * C, n)]


def _hash(n):
    return (np.arange(n, dtype=np.int64) * 2654435761) & 0xFFFFFFFF


# ---- cast: CAST(Int32 AS Utf8) ---------------------------------------------------------------------------------------------------------
I32_MIN = -(1 << 31)
EDGE_VALUES = [0, -1, 9, 10, -9, -10, 99999, -100000, (1 << 31) - 1, -(1 << 31) + 1, I32_MIN, 1000000000, -999999999]


@functools.lru_cache(maxsize=None)
def _cast_values_max():
    """N_MAX Int32 values whose texts are 1 to 11 bytes long: 1 to 10 digits, half of them negative, the type's ends among them;
    row B - 1 holds a one-byte and row B an eleven-byte value at every chunk boundary B"""
    n = N_MAX
    h = _hash(n)
    digits = (h >> 8) % 10 + 1
    p10 = 10 ** np.arange(11, dtype=np.int64)
    lo = np.where(digits == 1, 0, p10[digits - 1])
    span = np.where(digits == 1, 10, np.where(digits == 10, (1 << 31) - 10 ** 9, 9 * p10[digits - 1]))
    v = lo + (h * 40503 + 12345) % span
    v = np.where((h >> 4) & 1, -v, v)
    at = np.arange(5, n, 23)
    v[at] = np.resize(np.array(EDGE_VALUES, np.int64), len(at))
    b = chunk_boundaries(n)
    v[b - 1] = 7
    v[b] = I32_MIN
    assert v.min() == I32_MIN and v.max() == (1 << 31) - 1
    v = v.astype(np.int32)
    v.setflags(write=False)
    return v


def cast_values(n):
    """the first n of them: every size shares one array (a view, read-only)"""
    return _cast_values_max()[:n]


def digit_counts(v):
    """bytes of the decimal text of each Int32: its digits and the sign"""
    a = np.abs(v.astype(np.int64))
    nd = np.ones(len(v), np.int64)
    for k in range(1, 10):
        nd += a >= 10 ** k
    return nd + (v < 0)


@functools.lru_cache(maxsize=None)
def _cast_offsets_max():
    off = np.concatenate([[0], np.cumsum(digit_counts(_cast_values_max()))])
    off.setflags(write=False)
    return off


def cast_offsets(n):
    """the n + 1 expected offsets (int64; the last is the total)"""
    return _cast_offsets_max()[:n + 1]


def cast_text(v):
    return "".join(map(str, v.tolist())).encode()


# ---- probe: an Inner join on the general table ---------------------------------------------------------------------------------------------
BUILD_KEYS = [3, 1, 2, 3, 2, 3, 9, 9]                               # key k of 1 .. 3 has k rows; 0 has none; 9 is never probed


@functools.lru_cache(maxsize=None)
def _probe_keys_max():
    """N_MAX probe keys of 0 .. 3 (as many partners each); rows B - 1 and B differ at every chunk boundary B, by a number that changes
    from boundary to boundary"""
    n = N_MAX
    k = (_hash(n) >> 11) % 4
    b = chunk_boundaries(n)
    k[b - 1] = (b // C) % 4
    k[b] = (b // C + 1 + (b // C // 4) % 3) % 4
    k = k.astype(np.int32)
    k.setflags(write=False)
    return k


def probe_keys(n):
    return _probe_keys_max()[:n]


def id_side(prefix, keys):
    """a key column and the row ids, both Int32"""
    keys = np.asarray(keys, np.int32)
    return OrderedDict([(prefix + "k", OCol("Int32", keys)), (prefix + "i", OCol("Int32", np.arange(len(keys), dtype=np.int32)))])


def dict_join(bkeys, pkeys):
    """the equi-join by its definition, a dict from key to build rows (join_route_cases.reference_pairs), with the walk over the probe
    rows done in numpy: one lookup per distinct probe key.  -> (li, ri) in probe order, a probe row's partners in build order"""
    table = {}
    for i, k in enumerate(np.asarray(bkeys).tolist()):
        table.setdefault(k, []).append(i)
    uniq, inv = np.unique(np.asarray(pkeys), return_inverse=True)
    lists = [table.get(k, []) for k in uniq.tolist()]
    cnt_u = np.array([len(x) for x in lists], np.int64)
    start_u = np.concatenate([[0], np.cumsum(cnt_u)])[:-1] if len(lists) else np.zeros(0, np.int64)
    flat = np.array([i for x in lists for i in x], np.int64)
    cnt = cnt_u[inv] if len(pkeys) else np.zeros(0, np.int64)
    ri = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1] if len(cnt) else np.zeros(0, np.int64)
    li = flat[start_u[inv[ri]] + (np.arange(len(ri), dtype=np.int64) - first[ri])] if len(ri) else np.zeros(0, np.int64)
    return li, ri


@functools.lru_cache(maxsize=None)
def _probe_pairs_max():
    li, ri = dict_join(BUILD_KEYS, _probe_keys_max())
    return li, ri


def probe_pairs(n):
    """the pairs of the first n probe rows: those of all N_MAX rows come in probe order, so a size's pairs are a prefix"""
    li, ri = _probe_pairs_max()
    m = int(np.searchsorted(ri, n))
    return li[:m], ri[:m]


def pair_codes(li, ri, n_build):
    """one sorted integer per pair: equal arrays are equal multisets"""
    return np.sort(np.asarray(ri, np.int64) * n_build + np.asarray(li, np.int64))


# ---- rank: the rank map by its granule count ---------------------------------------------------------------------------------------------
RANK_KMIN = -500_000_000
RankCase = namedtuple("RankCase", "name n_gran form order bkeys pkeys")
# (name, granules, the form the name says); granule counts are even (two per 64-bit word of the key set)
RANK_SIZES = [("one_launch_max", SCAN_ONE_LAUNCH_MAX, "one"), ("one_launch_max_plus_2", SCAN_ONE_LAUNCH_MAX + 2, "two"),
              ("three_chunks", 3 * RP_CHUNK, "two"), ("three_chunks_plus_2", 3 * RP_CHUNK + 2, "two"),
              ("two_launch_chunks_plus_2", SCAN_TWO_LAUNCH_CHUNKS * RP_CHUNK + 2, "three")]
RANK_IDS = ["%s-%s" % (s[0], o) for s in RANK_SIZES for o in ("sorted", "shuffled")]


def granules(key_range):
    """try_narrow's n_gran (N_GRAN_SOURCE) for build keys spanning key_range = kmax - kmin"""
    return 2 * ((key_range >> 6) + 1)


def rank_form(n_gran):
    return launch_form(n_gran, SCAN_CHUNK if n_gran <= SCAN_ONE_LAUNCH_MAX else RP_CHUNK)


@functools.lru_cache(maxsize=None)
def rank_case(name, order):
    """unique Int32 build keys that span exactly the window of n_gran granules, as few rows as try_narrow's window rule takes (and more
    than the tiny build does), with a key in the first and in the last granule of every chunk — the first and the last value of each —
    and in both granules of the last word; probed by every build key and by absent keys next to those"""
    n_gran = dict((s[0], s[1]) for s in RANK_SIZES)[name]
    key_range = n_gran // 2 * 64 - 1
    assert granules(key_range) == n_gran
    n = max(key_range // RC.WINDOW_DIV - RC.WINDOW_SLACK, RC.TINY_BUILD_ROWS) + 1500
    rng = np.random.default_rng(n_gran % 100003)
    chunk = SCAN_CHUNK if n_gran <= SCAN_ONE_LAUNCH_MAX else RP_CHUNK
    b = chunk_boundaries(n_gran, chunk) * 32                         # the first value of each chunk after the first
    edge = np.concatenate([[0, 31, 32, key_range - 63, key_range - 32, key_range - 31, key_range], b - 32, b - 1, b, b + 31])
    edge = np.unique(edge[(edge >= 0) & (edge <= key_range)])
    fill = np.unique(RC.uniform(rng, 0, key_range, n))
    fill = rng.permutation(fill[~np.isin(fill, edge)])[:n - len(edge)]
    offs = np.sort(np.concatenate([edge, fill]))
    assert len(offs) == n == len(np.unique(offs)) and RC.window_ok(key_range, n) and n > RC.TINY_BUILD_ROWS
    bkeys = offs + RANK_KMIN
    absent = np.setdiff1d(np.concatenate([edge + 1, edge - 1, [-1, key_range + 1]]), offs) + RANK_KMIN
    pkeys = rng.permutation(np.concatenate([bkeys, absent]))
    if order == "shuffled":
        bkeys = rng.permutation(bkeys)
    return RankCase(name, n_gran, rank_form(n_gran), order, bkeys.astype(np.int32), pkeys.astype(np.int32))


def rank_cases():
    return [rank_case(s[0], o) for s in RANK_SIZES for o in ("sorted", "shuffled")]


def route_case_granules():
    """{granule count: launch form} of the rank maps the join-route cases build (join_route_cases.py): what was reached before"""
    out = {}
    for c in RC.all_cases():
        if c.route in ("rank_sorted", "rank_any"):
            n, kmin, kmax = RC.key_stats(c)
            out[granules(kmax - kmin)] = rank_form(granules(kmax - kmin))
    return out
