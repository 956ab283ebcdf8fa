"""TEST INFRASTRUCTURE shared by test_hash_table_cases_cpu.py (no GPU) and test_hash_collisions_gpu.py: inputs whose keys COLLIDE BY
CONSTRUCTION in the open-addressing tables behind HashJoinExec's general table and HashAggregateExec's hash path, and a SECOND statement
of those tables.

The tables (all: start at `hash & mask`, walk `(slot + 1) & mask`, identity by a key comparison):
  general join table   kernels_hash.hip join_upsert / join_find / join_owner_walk over PackedKeys and WideKeys.  Slot word =
                       (owner row + 1) | (high half of the hash) << 32; a prober compares keys only where that tag matches.
                       Packed: hash = hash_key(16-byte image).  Wide: slot and tag come from the row hash itself (WideKeys::hash returns
                       the hash side_keys' scan_keys launch stored: hash_row, restated by repartition_cases.restated_hash) — the wide
                       AGGREGATE table mixes once more (mix64(hash) & mask), the wide JOIN table does not.
  aggregate row table  table_upsert under scan_agg_hash_kernel: 32-bit owners, no tag, table_capacity(rows) slots
  aggregate run table  table_upsert under run_claim_kernel ("run_groups"): the same over the head rows of runs of equal keys
  merge table          merge_assign_kernel: MERGE_SLOTS slots in LDS over the per-workgroup partials of the register path

hash_key(k) = mix64(mix64(k.k0) ^ k.k1) and the row hash h = mix64(h ^ bits) per column are chains of a BIJECTION (mix64 is splitmix64's
finaliser: an addition, two xor-shift-multiplies by odd constants, an xor-shift), so for any wanted 64-bit hash H a key with exactly that
hash is SOLVED for (`unmix64`, `key_with_hash`) instead of searched or hoped for:
  packed1_dup  (v)          v = unmix64(unmix64(H))                       image (v, 0): widen_key / a force_not_null key part
  packed2      (a, b)       b = unmix64(H) ^ mix64(a)                     image (a, b): join keys carry no validity byte
  wide3        (a, b, c)    c = unmix64(H) ^ mix64(mix64(a) ^ b)          three Int64 columns do not fit 16 bytes: wide on their own

Families (functions of (capacity, form) -> Family(cluster keys, absent keys with the same homes, facts)):
  wrap_cluster          12 keys whose home slot is cap - 1 or cap - 2: the chain runs past slot 0; 3 absent keys walk all of it
  equal_tag_neighbours  8 keys of ONE 32-bit tag at homes s, s, s + 1, s + 1, ...: every comparison along the chain is a tag hit on a
                        different key (the hashes differ only below bit 32)
  equal_hash            6 keys (and 3 absent ones) of ONE 64-bit hash — not for packed1_dup: the hash of one word is a bijection
  k1_only               pairs that share their leading column(s) and differ in the last, and the reverse, each pair at one home and
                        tag so that the two ARE compared — not for packed1_dup: its second word is always 0
  capacity_turnover     wrap_cluster at 512 build rows (capacity 1024) and 513 (capacity 2048), filler keys far from the cluster

Nothing here touches a device.  test_hash_table_cases_cpu.py proves every claim under the restatement, pins the restated layout to the
source text, and shows that each `mistake` of `Table` changes the result of at least one named case (`discrimination`)."""
import functools
import re
from collections import OrderedDict, namedtuple

import numpy as np

from ballista_amd import expr as E
from ballista_amd.expr import col, lit
from oracle import engine as og
from oracle.engine import OCol

import helpers
import join_filter_cases as JF
import join_types_cases as JT
import join_route_cases as RC
import nljoin_cases as NC
import repartition_cases as RP
import wide_agg_cases as W

M64 = RC.M64
mix64 = RC.mix64
table_capacity = RC.table_capacity
ALL_TYPES = JF.ALL_TYPES                                   # Inner, Left, Right, Full, Semi, Anti, RightSemi, RightAnti

# ---- constants and texts, read from the sources ------------------------------------------------------------------------------------------

MERGE_SLOTS = RC.source_constant("kernels_agg.hip", "MERGE_SLOTS")                  # 2048
SEL_TILE = RC.SEL_TILE                                                             # 1024
# rows per lane and pass of join_owner_walk, per key form: {"Packed": 4, "Wide": 1}
PROBE_ROWS = {k: int(v) for k, v in re.findall(r"struct (Packed|Wide)Keys \{.*?static constexpr int PROBE_ROWS = (\d+);", RC.source_text("kernels_hash.hip"), re.S)}

# restatement -> (file, the text it restates); a change of any of them must send the reader back to the restatement named
PINNED = OrderedDict([
    ("hash_key", ("vm_device.h", "__device__ inline uint64_t hash_key(const Key128& k) { return mix64(mix64(k.k0) ^ k.k1); }")),
    ("packed_key (key_put)", ("vm_device.h", """__device__ inline void key_put(Key128& k, int pos, uint64_t v, int width) {
    // little-endian insert of the low `width` bytes of v at byte position pos
    if (width < 8) v &= ((1ull << (8 * width)) - 1ull);
    if (pos < 8) {
        k.k0 |= v << (8 * pos);
        if (pos + width > 8) k.k1 |= v >> (8 * (8 - pos));
    } else {
        k.k1 |= v << (8 * (pos - 8));
    }
}""")),
    ("packed_key (Key128 layout)", ("vm_device.h", """// A key tuple packs into 16 bytes (k0 = bytes 0-7, k1 = bytes 8-15, little-endian).
// Parts are laid out in order; a nullable part is preceded by one byte (0 = NULL, 1 = valid,
// value bytes zeroed when NULL); a Utf8 part is [len][bytes...] padded with zeros.""")),
    ("packed_key (nullable part)", ("vm_device.h", "if (kp.nullable) { key_put(k, pos, valid ? 1 : 0, 1); pos += 1; width -= 1; }\n            if (valid) key_put(k, pos, L.vals[kp.src * TILE + idx], width);")),
    ("packed1_dup image (widen_key_kernel)", ("kernels_util.hip", "k.x = sizeof(T) == 4 ? (uint64_t)(uint32_t)src[i] : (uint64_t)src[i];\n        k.y = 0;")),
    ("join keys carry no validity byte (side_keys)", ("host/ops_join.cpp", "for (auto& c : cols) pb.add_key(make_column(c), true);")),
    ("join keys carry no validity byte (add_key)", ("host/expr.hpp", "void add_key(const ExprPtr& e, bool force_not_null = false);")),
    ("Table (slot word)", ("kernels_hash.hip", "// JoinTable slot word = (claiming row + 1) | (high half of the key's hash) << 32, claimed by ONE 64-bit CAS.")),
    ("Table (join_upsert's want)", ("kernels_hash.hip", "const unsigned long long want = (unsigned long long)(row + 1u) | (tag << 32);")),
    ("Table (the tagged comparison)", ("kernels_hash.hip", "if ((o >> 32) == tag && keys.equal(T, (uint32_t)o - 1u, key)) return (uint32_t)slot;")),
    ("wide_hash (WideKeys::hash)", ("kernels_hash.hip", "__device__ uint64_t hash(const Key& k) const { return k.hash; }")),
    ("wide_hash (hash_row)", ("kernels_scan.hip", "h = mix64(h ^ bits);")),
    ("owner_table (table_upsert)", ("kernels_hash.hip", "if (k[0] == key.k0 && k[1] == key.k1) return (uint32_t)slot;\n        slot = (slot + 1) & mask;")),
    ("merge_table (MERGE_SLOTS)", ("kernels_agg.hip", "constexpr int MERGE_SLOTS = 2048;")),
    ("merge_table (the probe)", ("kernels_agg.hip", "uint32_t slot = (uint32_t)(hash_key(k) & (MERGE_SLOTS - 1));")),
    ("MERGE_GROUP_LIMIT", ("kernels_agg.hip", "if ((int)gi >= cap || gi >= MERGE_SLOTS / 2) {")),
    ("MERGE_GROUP_LIMIT (the caller's cap)", ("host/ops_agg.cpp", "const int cap = 1024;")),
    ("REGISTER_GROUPS", ("host/ops_agg.cpp", "gmax = (gmax == 4 && !wide_acc) ? 8 : -1;       // more groups than the register path holds: widen, then hash")),
    ("RUN_MIN_ROWS", ("host/ops_agg_hash.cpp", "if (!no_runs && P0.pred_slot < 0 && total_rows >= 4096 && clustered_hint->load() >= 0) {")),
    ("run table capacity", ("host/ops_agg_hash.cpp", "const uint64_t tcap = table_capacity((uint64_t)total_rows);")),
    ("row table capacity", ("host/ops_agg_hash.cpp", "cap = table_capacity((uint64_t)total_rows);         // (every row could be its own group)")),
    ("table_capacity", ("host/core.hpp", RC.TABLE_CAPACITY_SOURCE)),
])
REGISTER_GROUPS = 8                        # groups per WORKGROUP of the widest register kernel (scan_agg_lowcard_g8); more: the hash table
MERGE_GROUP_LIMIT = min(1024, MERGE_SLOTS // 2)            # groups merge_assign holds: the caller's cap and half of its slots
RUN_MIN_ROWS = 4096                        # hash_aggregate looks for runs from this many rows on

# ---- mix64 and its inverse ----------------------------------------------------------------------------------------------------------------------

_INV1 = pow(0xBF58476D1CE4E5B9, -1, 1 << 64)
_INV2 = pow(0x94D049BB133111EB, -1, 1 << 64)


def _unxorshift(z, s):
    """x with x ^ (x >> s) == z: the top s bits of x are z's, every further s bits follow from the ones above"""
    x = z
    for _ in range(64 // s + 1):
        x = z ^ (x >> s)
    return x


def unmix64(h):
    """the inverse of mix64: its four lines undone from the last to the first"""
    z = _unxorshift(h, 31)
    z = (z * _INV2) & M64
    z = _unxorshift(z, 27)
    z = (z * _INV1) & M64
    z = _unxorshift(z, 30)
    return (z - 0x9E3779B97F4A7C15) & M64


def signed(x):
    return x - (1 << 64) if x >> 63 else x


def u64(x):
    return x & M64


# ---- the key image and the hashes -------------------------------------------------------------------------------------------------------------------

def packed_key(cells):
    """cells: [(dtype, value or None, nullable)] -> (k0, k1), the 16-byte image as pack_key / key_put build it: parts in order,
    little-endian; a nullable part preceded by one byte (1 valid, 0 NULL with the value bytes zero)"""
    k = 0
    pos = 0
    for dtype, v, nullable in cells:
        width = W.FIXED_WIDTH[dtype]
        if nullable:
            k |= (0 if v is None else 1) << (8 * pos)
            pos += 1
        if v is not None:
            k |= (int(v) & ((1 << (8 * width)) - 1)) << (8 * pos)
        pos += width
    assert pos <= 16, "the parts do not fit the packed key"
    return k & M64, k >> 64


def hash_key(k0, k1):
    return mix64(mix64(k0) ^ k1)


def wide_hash(key):
    """the row hash of a NULL-free tuple of Int64 values (repartition_cases.restated_hash, one row, in Python integers)"""
    h = 0
    for v in key:
        h = mix64(h ^ u64(v))
    return h


FORMS = OrderedDict([("packed2", 2), ("packed1_dup", 1), ("wide3", 3)])           # form -> Int64 key columns on each side
TABLE_FORM = {"packed2": "packed", "packed1_dup": "packed", "wide3": "wide"}      # what ctx.join_key_form() reports


def image(form, key):
    return packed_key([("Int64", v, False) for v in key])


def key_hash(form, key):
    """the 64-bit hash whose low bits are the slot and whose high half is the tag of `key` in the general join table"""
    return wide_hash(key) if form == "wide3" else hash_key(*image(form, key))


def key_first(form, key):
    """what a comparison of the FIRST WORD alone sees: k0 of the image; the first column of a wide key"""
    return u64(key[0])


def key_with_hash(form, h, free=()):
    """the key of `form` whose hash is exactly h; free: its leading columns (packed1_dup: none, packed2: one, wide3: two)"""
    t = unmix64(h)
    if form == "packed1_dup":
        assert not free
        return (signed(unmix64(t)),)
    if form == "packed2":
        (a,) = free
        return (a, signed(t ^ mix64(u64(a))))
    a, b = free
    return (a, b, signed(t ^ mix64(mix64(u64(a)) ^ u64(b))))


def key_with_hash_and_tail(form, h, tail):
    """the reverse: the key whose LAST columns are `tail` and whose hash is h — its first column is solved for"""
    t = unmix64(h)
    if form == "packed2":
        (b,) = tail
        return (signed(unmix64(t ^ u64(b))), b)
    b, c = tail
    return (signed(unmix64(unmix64(t ^ u64(c)) ^ u64(b))), b, c)


def make_hash(cap, home, tag, mid):
    """tag << 32 | mid << log2(cap) | home: `mid` fills the bits between the slot bits and bit 32"""
    bits = cap.bit_length() - 1
    assert 0 <= home < cap and 0 <= tag < 1 << 32 and 0 <= mid < 1 << (32 - bits)
    return (tag << 32) | (mid << bits) | home


def home_of(form, key, cap):
    return key_hash(form, key) & (cap - 1)


def tag_of(form, key):
    return key_hash(form, key) >> 32


# ---- the tables, restated ------------------------------------------------------------------------------------------------------------------------------

MISTAKES = [None, "tag_is_key", "k0_only", "no_wrap", "stop_at_foreign_tag", "hash_is_key"]


class Table:
    """an open-addressing table over opaque keys: `hash_fn(key)` gives the 64-bit hash, `first_fn(key)` the first word.  tagged: the
    general join table (a slot holds (tag, owner row); keys are compared only where the tag matches); untagged: table_upsert and
    merge_assign (a slot holds the owner alone, every occupied slot is compared).  mistake:
      tag_is_key           a tag match is taken as equality
      k0_only              the first word alone is compared
      no_wrap              the probe forgets the mask: a chain that runs off the table's end finds nothing there — a row that builds
                           is lost, a row that probes misses
      stop_at_foreign_tag  a FIND ends at the first occupied slot whose tag differs (the build still walks on: it needs a slot)
      hash_is_key          equal 64-bit hashes are taken as equality"""

    def __init__(self, cap, hash_fn, first_fn, tagged=True, mistake=None):
        assert mistake in MISTAKES and (tagged or mistake not in ("tag_is_key", "stop_at_foreign_tag"))
        self.cap, self.hash_fn, self.first_fn, self.tagged, self.mistake = cap, hash_fn, first_fn, tagged, mistake
        self.owner = [None] * cap                          # slot -> (tag, owner row, owner's key)
        self.chain = {}                                    # slot -> the rows that ended on it (head / next)

    def _equal(self, theirs, key, h):
        if self.mistake == "tag_is_key":
            return True
        if self.mistake == "k0_only":
            return self.first_fn(theirs) == self.first_fn(key)
        if self.mistake == "hash_is_key":
            return self.hash_fn(theirs) == h
        return theirs == key

    def _walk(self, key, claim=None):
        h = self.hash_fn(key)
        tag = h >> 32 if self.tagged else 0
        slot = h & (self.cap - 1)
        while True:
            if slot >= self.cap:
                return None
            o = self.owner[slot]
            if o is None:
                if claim is None:
                    return None
                self.owner[slot] = (tag, claim, key)
                return slot
            if o[0] == tag:
                if self._equal(o[2], key, h):
                    return slot
            elif self.mistake == "stop_at_foreign_tag" and claim is None:
                return None
            slot = slot + 1 if self.mistake == "no_wrap" else (slot + 1) & (self.cap - 1)

    def upsert(self, row, key):
        slot = self._walk(key, row)
        if slot is not None:
            self.chain.setdefault(slot, []).append(row)
        return slot

    def find(self, key):
        return self._walk(key)

    def rows(self, key):
        slot = self.find(key)
        return [] if slot is None else self.chain[slot]

    def occupied(self):
        return [s for s, o in enumerate(self.owner) if o is not None]


def join_table(form, n_build, mistake=None):
    return Table(table_capacity(n_build), lambda k: key_hash(form, k), lambda k: key_first(form, k), True, mistake)


def owner_table(cap, mistake=None):
    """table_upsert's table over 16-byte images (k0, k1)"""
    return Table(cap, lambda k: hash_key(*k), lambda k: k[0], False, mistake)


def merge_table(mistake=None):
    """merge_assign_kernel's: MERGE_SLOTS slots over the images of the partial records"""
    return owner_table(MERGE_SLOTS, mistake)


def restated_pairs(form, build_keys, probe_keys, mistake=None):
    """the (build row, probe row) pairs of the general table, restated: build_keys / probe_keys hold one key tuple per row, None for a
    row with a NULL key part (which neither builds nor probes)"""
    t = join_table(form, len(build_keys), mistake)
    for i, k in enumerate(build_keys):
        if k is not None:
            t.upsert(i, k)
    return sorted((i, j) for j, k in enumerate(probe_keys) if k is not None for i in t.rows(k)), t


# ---- families ----------------------------------------------------------------------------------------------------------------------------------------

Family = namedtuple("Family", "name cap form cluster absent facts")
N_CLUSTER, N_ABSENT = 12, 3
FILLER_HOME0 = 32                          # filler key i has the home FILLER_HOME0 + i: no two share one, none is near a cluster


def _rng(name, cap, form):
    return np.random.default_rng(sum(name.encode()) * 31 + cap + 7 * list(FORMS).index(form))


def _word(rng):
    return int(rng.integers(-(1 << 62), 1 << 62))


def _free(rng, form):
    return tuple(_word(rng) for _ in range(FORMS[form] - 1))


def _tag(rng):
    return int(rng.integers(0, 1 << 32))


def _mid(rng, cap):
    return int(rng.integers(0, 1 << (32 - (cap.bit_length() - 1))))


def filler_keys(form, cap, n, seed=0):
    assert FILLER_HOME0 + n <= cap - 256
    rng = np.random.default_rng(1000 + seed + cap)
    return [key_with_hash(form, make_hash(cap, FILLER_HOME0 + i, _tag(rng), _mid(rng, cap)), _free(rng, form)) for i in range(n)]


def wrap_cluster(cap, form):
    rng = _rng("wrap_cluster", cap, form)
    homes = [cap - 1 - i % 2 for i in range(N_CLUSTER + N_ABSENT)]
    keys = [key_with_hash(form, make_hash(cap, h, _tag(rng), _mid(rng, cap)), _free(rng, form)) for h in homes]
    return Family("wrap_cluster", cap, form, keys[:N_CLUSTER], keys[N_CLUSTER:], {"homes": (cap - 2, cap - 1), "crosses_zero": True})


def equal_tag_neighbours(cap, form):
    rng = _rng("equal_tag_neighbours", cap, form)
    tag, s = _tag(rng), cap - 200
    build = [key_with_hash(form, make_hash(cap, s + i // 2, tag, 1 + i), _free(rng, form)) for i in range(8)]
    absent = [key_with_hash(form, make_hash(cap, s + i, tag, 100 + i), _free(rng, form)) for i in range(N_ABSENT)]
    return Family("equal_tag_neighbours", cap, form, build, absent, {"tag": tag, "first_home": s, "crosses_zero": False})


def equal_hash(cap, form):
    assert form != "packed1_dup"
    rng = _rng("equal_hash", cap, form)
    h = make_hash(cap, cap - 300, _tag(rng), _mid(rng, cap))
    free = [_free(rng, form) for _ in range(6 + N_ABSENT)]
    if form == "wide3":                                    # two keys share their first column, two their second
        free[1] = (free[0][0], free[1][1])
        free[3] = (free[3][0], free[2][1])
    keys = [key_with_hash(form, h, f) for f in free]
    return Family("equal_hash", cap, form, keys[:6], keys[6:], {"hash": h, "crosses_zero": False})


def k1_only(cap, form):
    """two pairs that share everything but the LAST column, two that share everything but the FIRST; per pair one absent key of the
    same kind.  The members of a pair (and its absent key) have one home and one tag, so the table compares them"""
    assert form != "packed1_dup"
    rng = _rng("k1_only", cap, form)
    build, absent, pairs = [], [], []
    for p in range(4):
        tag, home = _tag(rng), cap - 400 + 10 * p
        hs = [make_hash(cap, home, tag, 1 + j) for j in range(3)]
        if p < 2:
            lead = _free(rng, form)
            trio = [key_with_hash(form, h, lead) for h in hs]
        else:
            tail = _free(rng, form)
            trio = [key_with_hash_and_tail(form, h, tail) for h in hs]
        pairs.append((trio[0], trio[1], "last" if p < 2 else "first"))
        build += trio[:2]
        absent.append(trio[2])
    return Family("k1_only", cap, form, build, absent, {"pairs": pairs, "crosses_zero": False})


FAMILIES = OrderedDict([("wrap_cluster", wrap_cluster), ("equal_tag_neighbours", equal_tag_neighbours), ("equal_hash", equal_hash), ("k1_only", k1_only)])
# family id -> (family, build rows; None: the cluster and N_FILLERS filler keys)
FAMILY_IDS = OrderedDict([("wrap_cluster", ("wrap_cluster", None)), ("equal_tag_neighbours", ("equal_tag_neighbours", None)), ("equal_hash", ("equal_hash", None)),
                          ("k1_only", ("k1_only", None)), ("capacity_turnover_512", ("wrap_cluster", 512)), ("capacity_turnover_513", ("wrap_cluster", 513))])
# what cannot be built, left out of every parametrisation
LEFT_OUT = {
    ("equal_hash", "packed1_dup"): "the hash of ONE word is a bijection: no two different keys share their 64 bits",
    ("k1_only", "packed1_dup"): "the second word of a one-column key's image is always 0",
}
N_FILLERS = 40
VARIATIONS = ["unique", "duplicates"]


def multiplicities(n_keys, variation, form):
    """rows per build key.  unique: one each — but packed1_dup holds ONE duplicate, of its last filler key (a unique single Int64 column
    would stay on the narrow routes), so its build side is never `unique` to the probe: the join_probe_match route is packed2's and
    wide3's.  duplicates: 1 to 4"""
    if variation == "duplicates":
        return [1 + (5 * i + 2) % 4 for i in range(n_keys)]
    m = [1] * n_keys
    if form == "packed1_dup":
        m[-1] = 2
    return m


def build_key_list(family_id, form, variation):
    """-> (family, the distinct build keys [cluster first], rows per key)"""
    name, n_rows = FAMILY_IDS[family_id]
    if n_rows is None:
        n_keys = len(FAMILIES[name](1024, form).cluster) + N_FILLERS
        mult = multiplicities(n_keys, variation, form)
    else:                                                  # as many filler keys as fill exactly n_rows rows
        n_cluster = N_CLUSTER
        n_keys = n_cluster
        while sum(multiplicities(n_keys, variation, form)) < n_rows:
            n_keys += 1
        mult = multiplicities(n_keys, variation, form)
        over = sum(mult) - n_rows
        for i in range(n_keys - 2, n_cluster, -1):         # shorten filler keys that have a row to spare (not the last: packed1_dup's duplicate)
            if over and mult[i] > 1:
                mult[i] -= 1
                over -= 1
        assert over == 0
    total = sum(mult)
    fam = FAMILIES[name](table_capacity(total), form)
    keys = fam.cluster + filler_keys(form, fam.cap, n_keys - len(fam.cluster))
    return fam, keys, mult


PROBE_BATCHES = [1, 63, 64, 65, 255, 256, 257, 1025]       # either side of 64 * PROBE_ROWS rows (a wave pass: 256 packed, 64 wide) and of SEL_TILE
N_PROBE = sum(PROBE_BATCHES)                               # 1986
ON = {form: [("lk%d" % j, "rk%d" % j) for j in range(n)] for form, n in FORMS.items()}


def _key_columns(prefix, keys, n_cols, valid=None):
    """keys: one tuple per row; valid: per column a bool array or None"""
    return [("%sk%d" % (prefix, j), OCol("Int64", np.array([k[j] for k in keys], np.int64), None if valid is None else valid[j])) for j in range(n_cols)]


def stranger_keys(form, cap, n):
    rng = np.random.default_rng(4321 + cap)
    return [key_with_hash(form, int(rng.integers(0, 1 << 64, dtype=np.uint64)), _free(rng, form)) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def join_sides(family_id, form, variation, nulls=False):
    """-> (left, right, family, the distinct build keys).  left: lk0.., lx, li; right: rk0.., ry, ri.  One object per argument list:
    never modified.  nulls: both sides gain rows that STORE a cluster key under a NULL in one key column; they neither build nor match"""
    fam, keys, mult = build_key_list(family_id, form, variation)
    n_cols = FORMS[form]
    rng = np.random.default_rng(len(keys) + 13 * len(family_id) + n_cols)
    rows = [k for k, m in zip(keys, mult) for _ in range(m)]
    lvalid = None
    if nulls:
        extra = [fam.cluster[i % len(fam.cluster)] for i in range(8)]
        lvalid = [np.concatenate([np.ones(len(rows), np.bool_), np.array([i % n_cols != j for i in range(8)])]) for j in range(n_cols)]
        rows = rows + extra
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    if lvalid is not None:
        lvalid = [v[order] for v in lvalid]
    nl = len(rows)
    left = JT.with_ids("l", nl, _key_columns("l", rows, n_cols, lvalid) + [("lx", OCol("Float64", rng.integers(0, 1000, nl) / 8.0))])
    fillers = keys[len(fam.cluster):]
    pool = fam.cluster + fam.absent + fillers[:20] + fillers[-5:] + stranger_keys(form, fam.cap, 20)
    picks = np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), N_PROBE - len(pool))])
    # the cluster and its absent keys: more often than the rest
    heavy = rng.random(N_PROBE) < 0.4
    picks = np.where(heavy, rng.integers(0, len(fam.cluster) + len(fam.absent), N_PROBE), picks)
    picks[:len(pool)] = np.arange(len(pool))
    picks = rng.permutation(picks)
    prows = [pool[i] for i in picks]
    rvalid = None
    if nulls:
        rvalid = [np.ones(N_PROBE, np.bool_) for _ in range(n_cols)]
        for i, r in enumerate((0, 63, 64, 255, 256, 1023, 1024, N_PROBE - 1) + tuple(range(300, 330))):
            prows[r] = fam.cluster[i % len(fam.cluster)]
            rvalid[i % n_cols][r] = False
    right = JT.with_ids("r", N_PROBE, _key_columns("r", prows, n_cols, rvalid) + [("ry", OCol("Int64", rng.integers(0, 10 ** 6, N_PROBE)))])
    return left, right, fam, keys


def row_keys(batch, prefix, form):
    """one key tuple per row, None where a key part is NULL"""
    cols = [batch["%sk%d" % (prefix, j)].to_pylist() for j in range(FORMS[form])]
    return [None if None in k else k for k in zip(*cols)]


def expected_pairs(left, right, form):
    """the equi-join by its definition (join_route_cases.reference_pairs: a dict from key tuple to build rows, NULL keys never match)"""
    return RC.pairs(left, right, ON[form])


def expected_rows(jt, left, right, form):
    li, ri = expected_pairs(left, right, form)
    return JF.from_pairs(jt, left, right, ON[form], li, ri)


JOIN_CASES = [(f, form, v) for f in FAMILY_IDS for form in FORMS if (FAMILY_IDS[f][0], form) not in LEFT_OUT for v in VARIATIONS]


def join_case_id(c):
    return "-".join(c)


# the residual filter ri % 3 != 0, spelled with the truncating integer division the expression language has (it has no modulus)
def residual_filter(left, right, form):
    e = (col("ri") - col("ri") / lit(3) * lit(3)).ne(lit(0))
    return E.coerce(e, dict(JF.inner_schema(left, right, ON[form])))


def filtered_rows(jt, left, right, form):
    li, ri = expected_pairs(left, right, form)
    keep = right["ri"].values[ri] % 3 != 0
    return JF.from_pairs(jt, left, right, ON[form], li[keep], ri[keep])


FILTER_TYPES = [JF.INNER, JF.LEFT, JT.SEMI, JT.RIGHT_ANTI]


def build_exec(ctx, left):
    return NC.build_exec(ctx, left)                        # two partitions


def probe_exec(ctx, right, jt):
    """the batches of PROBE_BATCHES in two partitions — in one for the types whose build rows answer for every probe row (Left, Full,
    Semi, Anti)"""
    return NC.probe_exec(ctx, right, jt, PROBE_BATCHES)


# ---- aggregates ---------------------------------------------------------------------------------------------------------------------------------------

AggCase = namedtuple("AggCase", "name partitions group aggs facts")
AB = [(col("a"), "a"), (col("b"), "b")]
AGGS = [E.Count(lit(1, E.UINT8), "n"), E.Sum(col("rn"), "s"), E.Min(col("rn"), "mn"), E.Max(col("rn"), "mx")]
AGG_FAMILIES = ["wrap_cluster", "equal_hash", "k1_only"]
AGG_FORM = "packed2"                                       # two NULL-free Int64 group columns: the image (a, b), hash_key of it


def _ab_table(keys_per_row):
    n = len(keys_per_row)
    return OrderedDict([("a", OCol("Int64", np.array([k[0] for k in keys_per_row], np.int64))), ("b", OCol("Int64", np.array([k[1] for k in keys_per_row], np.int64))),
                        ("rn", OCol("Int64", np.arange(n, dtype=np.int64)))])


def _fill_rows(n_cluster, n_rows):
    """(number of keys, rows per key 1..4) summing to exactly n_rows"""
    n_keys = n_cluster
    mult = lambda k: [1 + (5 * i + 2) % 4 for i in range(k)]
    while sum(mult(n_keys)) < n_rows:
        n_keys += 1
    m = mult(n_keys)
    over = sum(m) - n_rows
    assert over < 4 and n_keys > n_cluster + 4
    for i in range(n_keys - 1, n_keys - 1 - 4, -1):        # shorten filler keys that have a row to spare
        if over and m[i] > 1:
            m[i] -= 1
            over -= 1
    assert over == 0 and sum(m) == n_rows
    return n_keys, m


@functools.lru_cache(maxsize=None)
def agg_rows_case(family, n_rows=None):
    """shuffled rows, more groups than a register kernel holds: the ROW table (scan_agg_hash over table_upsert), table_capacity(rows)"""
    n_cluster = len(FAMILIES[family](1024, AGG_FORM).cluster)
    if n_rows is None:
        n_keys = n_cluster + 30
        mult = [1 + (5 * i + 2) % 4 for i in range(n_keys)]
    else:
        n_keys, mult = _fill_rows(n_cluster, n_rows)
    total = sum(mult)
    cap = table_capacity(total)
    fam = FAMILIES[family](cap, AGG_FORM)
    keys = fam.cluster + filler_keys(AGG_FORM, cap, n_keys - n_cluster)
    rows = [k for k, m in zip(keys, mult) for _ in range(m)]
    rows = [rows[i] for i in np.random.default_rng(total).permutation(total)]
    t = _ab_table(rows)
    name = "rows/%s%s" % (family if n_rows is None else "capacity_turnover", "" if n_rows is None else "_%d" % n_rows)
    return AggCase(name, [[t]], AB, AGGS, {"route": "rows", "family": fam, "capacity": cap, "n_groups": n_keys, "n_rows": total})


def _run_lengths(target):
    """runs of 3 to 5 rows summing to exactly target"""
    r = target // 4
    lengths = [4] * r
    for i in range(r // 3):
        lengths[2 * i], lengths[2 * i + 1] = 3, 5
    for i in range(target - 4 * r):
        lengths[2 * i] += 1                                # a 3 becomes a 4
    assert sum(lengths) == target and 3 <= min(lengths) and max(lengths) <= 5
    return lengths


@functools.lru_cache(maxsize=None)
def agg_runs_case(family, n_rows=4200):
    """rows clustered into runs of 3 to 5 equal keys, every key in (at least) two runs, the runs in no order: the RUN table
    ("run_groups": table_upsert over the head rows of the runs), table_capacity(rows)"""
    assert n_rows >= RUN_MIN_ROWS
    lengths = _run_lengths(n_rows)
    n_runs = len(lengths)
    n_keys = n_runs // 2
    cap = table_capacity(n_rows)
    fam = FAMILIES[family](cap, AGG_FORM)
    keys = fam.cluster + filler_keys(AGG_FORM, cap, n_keys - len(fam.cluster))
    rng = np.random.default_rng(n_rows)
    first, second = rng.permutation(n_keys), rng.permutation(n_keys)
    if first[-1] == second[0]:
        second = second[::-1]
    run_keys = list(first) + list(second) + ([int(first[0])] if n_runs % 2 else [])
    assert len(run_keys) == n_runs
    rows = [keys[k] for k, ln in zip(run_keys, lengths) for _ in range(ln)]
    name = "runs/%s" % (family if n_rows == 4200 else "capacity_turnover_%d" % n_rows)
    return AggCase(name, [[_ab_table(rows)]], AB, AGGS, {"route": "runs", "family": fam, "capacity": cap, "n_groups": n_keys, "n_rows": n_rows, "n_runs": n_runs})


@functools.lru_cache(maxsize=None)
def agg_merge_case(family):
    """few enough groups PER BATCH for the register path (each batch is scanned by workgroups of its own: at most REGISTER_GROUPS
    groups each), several batches: their partials meet in merge_assign's MERGE_SLOTS-slot table.  wrap_cluster: 12 keys whose homes are
    2046 and 2047, each batch holding 8 of them — 12 colliding keys where one workgroup alone could bring 8"""
    fam = FAMILIES[family](MERGE_SLOTS, AGG_FORM)
    keys = fam.cluster
    if len(keys) <= REGISTER_GROUPS:
        subsets = [list(range(len(keys)))] * 3
    else:
        subsets = [[(2 * j + i) % len(keys) for i in range(REGISTER_GROUPS)] for j in range(len(keys) // 2)]
    rng = np.random.default_rng(len(keys))
    rows, cuts = [], []
    for s in subsets:
        batch = [keys[k] for k in s for _ in range(2 + k % 3)]
        batch = [batch[i] for i in rng.permutation(len(batch))]
        rows += batch
        cuts.append(len(batch))
    t = _ab_table(rows)
    return AggCase("merge/%s" % family, [W.cut(t, cuts)], AB, AGGS,
                   {"route": "merge", "family": fam, "capacity": MERGE_SLOTS, "n_groups": len(keys), "n_rows": len(rows), "groups_per_batch": [len(set(s)) for s in subsets]})


SPILL_GROUPS = 12


@functools.lru_cache(maxsize=None)
def agg_nullable_case():
    """GROUP BY one NULLABLE Int64 column: the image is k0 = 1 | v << 8, k1 = v >> 56.  The valid keys share their low 56 bits, so
    their k0 are equal and they differ in k1 — the byte that spills over — alone; the low bits are searched (256 candidates per try) so
    that at least three of them share one home slot: those ARE compared.  Beside them the NULL group (image (0, 0)) and the valid key
    0 (image (1, 0)).  Shuffled, more than REGISTER_GROUPS groups: the row table"""
    mult = [2 + i % 3 for i in range(SPILL_GROUPS + 2)]
    total = sum(mult)
    cap = table_capacity(total)
    low = 1
    while True:
        homes = {}
        for top in range(256):
            v = signed((top << 56) | low)
            homes.setdefault(hash_key(*packed_key([("Int64", v, True)])) & (cap - 1), []).append(top)
        shared = max(homes.values(), key=len)
        if len(shared) >= 3:
            break
        low += 1
    tops = shared[:3] + [t for t in (0, 1, 0x7F, 0x80, 0xFF, 2, 3, 0x40, 0xC0, 5, 6, 7) if t not in shared[:3]][:SPILL_GROUPS - 3]
    values = [signed((t << 56) | low) for t in tops] + [0, None]
    rows = [v for v, m in zip(values, mult) for _ in range(m)]
    rows = [rows[i] for i in np.random.default_rng(7).permutation(total)]
    t = OrderedDict([("k", W.column("Int64", rows)), ("rn", OCol("Int64", np.arange(total, dtype=np.int64)))])
    return AggCase("rows/nullable_spill_byte", [[t]], [(col("k"), "k")], AGGS,
                   {"route": "rows", "capacity": cap, "n_groups": len(values), "n_rows": total, "low": low, "shared_home": [signed((t << 56) | low) for t in shared[:3]]})


def agg_cases():
    out = [agg_rows_case(f) for f in AGG_FAMILIES] + [agg_rows_case("wrap_cluster", 512), agg_rows_case("wrap_cluster", 513)]
    # (hash_aggregate looks for runs from RUN_MIN_ROWS rows on, so the run table's capacity turns over at 4096 / 4097 rows)
    out += [agg_runs_case(f) for f in AGG_FAMILIES] + [agg_runs_case("wrap_cluster", 4096), agg_runs_case("wrap_cluster", 4097)]
    out += [agg_merge_case(f) for f in AGG_FAMILIES]
    return out + [agg_nullable_case()]


# the merge table has ONE capacity: capacity_turnover does not exist for it
AGG_LEFT_OUT = {("merge", "capacity_turnover"): "merge_assign's table always has MERGE_SLOTS slots"}


def find_agg(name):
    return next(c for c in agg_cases() if c.name == name)


def agg_table(case):
    return W.table_of(case)


def agg_key_names(case):
    return [n for _, n in case.group]


def agg_images(case):
    """the 16-byte image of every row's group key"""
    t = agg_table(case)
    names = agg_key_names(case)
    nullable = [t[n].valid is not None for n in names]
    return [packed_key([("Int64", v, nb) for v, nb in zip(k, nullable)]) for k in zip(*[t[n].to_pylist() for n in names])]


def expected_groups(case):
    """the Partial aggregate by its definition: a dict from key tuple to the group's row numbers -> the key columns and COUNT(*)
    [UInt64], SUM / MIN / MAX of rn [Int64].  Integers: exact in any order"""
    t = agg_table(case)
    names = agg_key_names(case)
    groups = OrderedDict()
    for k, rn in zip(zip(*[t[n].to_pylist() for n in names]), t["rn"].values.tolist()):
        groups.setdefault(k, []).append(rn)
    out = OrderedDict()
    for j, n in enumerate(names):
        out[n] = W.column("Int64", [k[j] for k in groups])
    out["n[count]"] = OCol("UInt64", np.array([len(v) for v in groups.values()], np.uint64))
    out["s[sum]"] = OCol("Int64", np.array([sum(v) for v in groups.values()], np.int64))
    out["mn[min]"] = OCol("Int64", np.array([min(v) for v in groups.values()], np.int64))
    out["mx[max]"] = OCol("Int64", np.array([max(v) for v in groups.values()], np.int64))
    return out


def restated_group_count(case, mistake=None):
    """the number of groups the case's table finds, restated.  rows: every row upserts its image; runs: the head row of every run;
    merge: per batch the distinct keys in order of appearance (what a workgroup's partial holds).  A row lost off the table's end
    (no_wrap) stands for itself"""
    images = agg_images(case)
    route = case.facts["route"]
    if route == "rows":
        entries = images
    elif route == "runs":
        entries = [k for i, k in enumerate(images) if i == 0 or images[i - 1] != k]
    else:
        entries, at = [], 0
        for b in case.partitions[0]:
            n = og.batch_len(b)
            entries += list(OrderedDict.fromkeys(images[at:at + n]))
            at += n
    t = owner_table(case.facts["capacity"], mistake)
    reps = set()
    for i, k in enumerate(entries):
        slot = t.upsert(i, k)
        reps.add(("lost", i) if slot is None else slot)
    return len(reps), t


# kernel names of a BHIP_KERNEL_TIMING=2 context (the TIMED_LAUNCH sites of host/ops_agg_hash.cpp and host/ops_agg.cpp):
# route -> (ran, did not run)
AGG_ROUTE_KERNELS = {
    "rows": ({"scan_agg_hash", "hash_agg_flags", "hash_agg_compact"}, {"run_heads", "run_slots", "run_groups"}),
    "runs": ({"run_heads", "run_slots", "run_groups", "scan_agg_hash", "hash_agg_compact"}, {"run_tail_resolve", "run_tail_remap", "run_compact", "emit_slots"}),
    "merge": ({"scan_agg_lowcard_g8_batches", "merge_partials"}, {"scan_agg_hash", "run_heads", "hash_agg_compact"}),
}
AGG_ROUTE_SOURCE = [("host/ops_agg_hash.cpp", 'TIMED_LAUNCH_N(ex, "%s"' % k) for k in ("scan_agg_hash", "hash_agg_flags", "hash_agg_compact", "run_heads", "run_slots", "run_groups",
                                                                                         "run_tail_resolve", "run_tail_remap", "run_compact")] + \
                   [("host/ops_agg.cpp", 'TIMED_LAUNCH(ex, "merge_partials"'), ("host/ops_agg.cpp", '"scan_agg_lowcard_g8_batches"'), ("host/ops_agg.cpp", 'TIMED_LAUNCH_N(ex, "emit_slots"')]


def assert_agg_route(names, route):
    ran, not_ran = AGG_ROUTE_KERNELS[route]
    assert ran <= names, (route, sorted(ran - names), sorted(names))
    assert not (not_ran & names), (route, sorted(not_ran & names))


# ---- which case each mistake is built against ------------------------------------------------------------------------------------------------------------

def discrimination():
    """mistake -> the cases whose restated result it changes: ("join", family id, form, variation) — a missing or an extra pair — or
    ("agg", case name) — another number of groups"""
    joins = lambda fams, forms: [("join", f, form, v) for f in fams for form in forms if (FAMILY_IDS[f][0], form) not in LEFT_OUT for v in VARIATIONS]
    wraps = ["wrap_cluster", "capacity_turnover_512", "capacity_turnover_513"]
    return OrderedDict([
        ("tag_is_key", joins(["equal_tag_neighbours", "equal_hash"], FORMS)),
        ("k0_only", joins(["k1_only"], FORMS) + [("agg", "rows/k1_only"), ("agg", "runs/k1_only"), ("agg", "merge/k1_only"), ("agg", "rows/nullable_spill_byte")]),
        ("no_wrap", joins(wraps, FORMS) + [("agg", n) for n in ("rows/wrap_cluster", "rows/capacity_turnover_512", "rows/capacity_turnover_513", "runs/wrap_cluster",
                                                                  "runs/capacity_turnover_4096", "runs/capacity_turnover_4097", "merge/wrap_cluster")]),
        ("stop_at_foreign_tag", joins(wraps, FORMS)),
        ("hash_is_key", joins(["equal_hash"], FORMS) + [("agg", "rows/equal_hash"), ("agg", "runs/equal_hash"), ("agg", "merge/equal_hash")]),
    ])
