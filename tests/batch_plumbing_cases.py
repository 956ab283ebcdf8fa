"""TEST INFRASTRUCTURE shared by test_batch_plumbing_cpu.py (no GPU) and test_batch_plumbing_gpu.py: the inputs and the EXPECTED values
of the code between operators — concat_batches (host/ops_basic.cpp) with its bitmap copy and offset rebase, the zero-copy head slice
of LimitExec, and CoalesceBatchesExec / LimitExec / MergeExec as operators over streams of batches.

Nothing here touches a device.  Expected values are numpy concatenation and slicing of OCols (helpers.concat, helpers.slice_batch) and
the few lines of Python below; every comparison the GPU file makes with them is bit for bit.

A part of a concat is a `Part`: per column (dtype, values, valid) where `valid` is a bool array of the part's length or None.  The
import (batch_from_host) keeps a validity buffer only if some bit is clear: None and an all-true array both give a column WITHOUT a
buffer (the bitmap copy then writes ones; `src == nullptr`), the array makes the schema nullable all the same.  A buffer whose bits are
all ones over the rows of the part exists only in a head slice: the slice keeps the longer batch's buffer, and the clear bits lie past
the cut (the `head` parts below; pattern last_zero makes every kept bit a one)."""
from collections import OrderedDict

import numpy as np

from oracle import engine as og
from oracle.engine import OCol

import helpers
from test_types_gpu import FIXED, values_of

# ---- 1. concat ---------------------------------------------------------------------------------------------------------------------------

LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 1025]
EDGES = (0, 1, 31, 32, 33, 63)                       # bit positions inside a 64-bit bitmap word at which a copy can go wrong
PATTERNS = ("ones", "zeros", "alternating", "edge_zero", "edge_one", "last_zero", "random")
UTF8_MODES = ("mixed", "empty", "all_null", "multibyte")
HEAD_CUTS = (1, 63, 64, 65)
TYPES = list(FIXED) + ["Boolean", "Utf8", "Utf8"]    # c0 .. c15 fixed width (1, 2, 4 and 8 bytes), c16 Boolean, c17 and c18 Utf8
NAMES = ["c%d" % i for i in range(len(TYPES))]
WORDS = ["", "a", "alpha", "Beta ", "é", "日本語", "x" * 40, "𝄞 clef", "ß-ü", "tail\t"]
MULTIBYTE = ["é", "日本語", "𝄞", "ñandú", "ж", "€uro"]
FLOAT_SPECIALS = [np.nan, -0.0, np.inf, -np.inf, 0.0]


def bits(pattern, n, rng):
    """n bits that make a shifted, dropped or repeated copy visible"""
    if pattern == "ones":
        return np.ones(n, bool)
    if pattern == "zeros":
        return np.zeros(n, bool)
    if pattern == "alternating":
        return np.arange(n) % 2 == 0
    if pattern in ("edge_zero", "edge_one"):         # a single 0 (1) at the part's first and last row
        b = np.full(n, pattern == "edge_zero")
        if n:
            b[0] = b[-1] = pattern != "edge_zero"
        return b
    if pattern == "last_zero":                       # under a head cut: a buffer whose kept bits are all ones
        b = np.ones(n, bool)
        b[-1:] = False
        return b
    assert pattern == "random"
    return rng.random(n) > 0.5


class Part:
    """one input batch of a concat.  cols: name -> (dtype, values, valid-or-None), `rows` rows each.  head: the device batch is
    LocalLimitExec(head) over these columns (a zero-copy slice: buffers of `rows` rows, n_rows = head); kept() is what it holds"""

    def __init__(self, cols, head=None):
        self.cols, self.head = cols, head
        self.rows = len(next(iter(cols.values()))[1])

    @property
    def n(self):
        return self.rows if self.head is None else min(self.head, self.rows)

    def columns(self):
        """what RecordBatch.from_columns takes, for ALL the rows (before a head cut)"""
        return [(k, t, list(v) if t == "Utf8" else v, valid) for k, (t, v, valid) in self.cols.items()]

    def kept(self):
        return OrderedDict((k, OCol(t, v[:self.n], None if valid is None else valid[:self.n])) for k, (t, v, valid) in self.cols.items())

    def has_buffer(self, name):
        """the device column has a validity buffer: some row — of ALL the rows, a head slice keeps the buffer — is NULL"""
        valid = self.cols[name][2]
        return valid is not None and not valid.all()

    def nullable(self, name):
        return self.cols[name][2] is not None


def make_part(n, seed, nullable=True, pattern="random", utf8="mixed", head=None):
    """n rows of every type.  pattern: the validity of every column (rotated by one pattern for the Boolean VALUES, so a case shows two);
    nullable False: no column has a validity buffer.  Floats carry NaN, -0.0 and both infinities, UInt64 values above 2^63, in the
    first rows and again in the last ones, so that short parts have them too and both ends of a long one do."""
    rng = np.random.default_rng(seed)
    cols = OrderedDict()
    for name, t in zip(NAMES, TYPES):
        valid = bits(pattern, n, rng) if nullable else None
        if t == "Utf8":
            mode = "mixed" if name == NAMES[-2] and utf8 != "all_null" else utf8          # c17 keeps ordinary strings unless all NULL
            pool = {"mixed": WORDS, "empty": [""], "all_null": WORDS, "multibyte": MULTIBYTE}[mode]
            v = np.array([pool[int(i)] for i in rng.integers(0, len(pool), n)], dtype=object)
            if mode == "all_null":
                valid = np.zeros(n, bool)
        elif t == "Boolean":
            v = bits(PATTERNS[(PATTERNS.index(pattern) + 1) % len(PATTERNS)], n, rng)
        else:
            v = values_of(t, n, rng)
            if t in ("Float32", "Float64"):
                for j, s in enumerate(FLOAT_SPECIALS[:n]):
                    v[j] = s
                    v[n - 1 - j] = s
            elif t == "UInt64" and n:
                v[0] = v[n - 1] = 2 ** 63 + 12345 + n
        cols[name] = (t, v, valid)
    return Part(cols, head)


class ConcatCase:
    def __init__(self, name, parts):
        self.name, self.parts = name, parts

    def lengths(self):
        return [p.n for p in self.parts]

    def expected(self):
        return helpers.concat([p.kept() for p in self.parts])

    def expected_data_bytes(self, name):
        """the value bytes of a Utf8 column of the result: every kept row's, the ones under a NULL included"""
        return sum(len(s.encode()) for p in self.parts for s in p.kept()[name].values)

    def __repr__(self):
        return self.name


# part lengths, chosen so that destination offsets and lengths meet EDGES (test_batch_plumbing_cpu.py proves it on the list below)
LENGTH_LISTS = [
    [1, 31, 32, 63, 1, 64, 33, 31, 65],             # offsets mod 64: 0 1 32 0 63 0 0 33 0
    [31, 33, 63, 1, 128, 32, 127, 1, 129, 2],       # 0 31 0 63 0 0 32 31 32 33
    [33, 1000, 1025, 65, 2, 127, 2, 64, 1],         # the long parts: many whole words between two partial ones
    [2, 1, 2, 31, 1, 1, 33],                        # parts strictly inside one word: 1 row at offset 2, 2 at 3, 31 at 5, 1 at 36, 1 at 37
    [63, 129, 1000, 128, 1025],                     # offset 63 into a long part; 1000 rows at offset 0 (192)
]


def _case(name, specs, **common):
    """specs: per part (n, overrides) or n"""
    parts = []
    for i, s in enumerate(specs):
        n, kw = (s, {}) if isinstance(s, int) else s
        parts.append(make_part(n, seed=1000 * len(name) + 7 * i + n, **{**common, **kw}))
    return ConcatCase(name, parts)


def concat_cases():
    out = []
    for li, lens in enumerate(LENGTH_LISTS):
        for nullable in (True, False):
            # every pattern appears on every list: the pattern changes from part to part
            specs = [(n, dict(pattern=PATTERNS[(i + li) % len(PATTERNS)])) for i, n in enumerate(lens)]
            out.append(_case("lengths%d_%s" % (li, "nullable" if nullable else "not_null"), specs, nullable=nullable))
    for pattern in PATTERNS:                          # one pattern on every part, at the offsets of the first two lists
        out.append(_case("pattern_" + pattern, LENGTH_LISTS[0] + LENGTH_LISTS[1], pattern=pattern))
    out.append(_case("200_parts_of_one_row", [(1, dict(pattern=PATTERNS[i % 3 + 2])) for i in range(200)]))
    out.append(_case("200_parts_of_one_row_not_null", [1] * 200, nullable=False))
    out.append(_case("zero_rows_first_last_middle_adjacent", [0, 33, 0, 0, 65, 1, 0, 31, 0]))
    out.append(_case("zero_rows_not_null", [0, 0, 2, 0, 64, 0], nullable=False))
    out.append(_case("every_part_zero_rows", [0, 0, 0]))
    out.append(_case("single_part", [129]))
    out.append(_case("single_part_zero_rows", [0]))
    # only some parts carry a validity buffer: the buffer-less part first, last, between two others, and several of them
    for where, specs in [("first", [(33, dict(nullable=False)), 65, 31]), ("last", [31, 65, (33, dict(nullable=False))]),
                         ("middle", [31, (70, dict(nullable=False)), 64, 2]),
                         ("inside_a_word", [(5, dict(pattern="zeros")), (3, dict(nullable=False)), (40, dict(pattern="zeros"))]),
                         ("several", [(1, dict(nullable=False)), (63, dict(pattern="zeros")), (64, dict(nullable=False)),
                                      (1, dict(pattern="zeros")), (129, dict(nullable=False)), (2, dict(pattern="edge_one"))])]:
        out.append(_case("no_buffer_" + where, specs, pattern="random"))
    for mode in UTF8_MODES[1:]:
        out.append(_case("utf8_" + mode, [33, (64, dict(utf8=mode)), 2, (31, dict(utf8=mode))]))
        out.append(_case("utf8_%s_every_part" % mode, [1, 64, 33], utf8=mode))
    out.append(_case("utf8_empty_first_and_last", [(2, dict(utf8="empty")), 65, (1, dict(utf8="empty"))], nullable=False))
    for cut in HEAD_CUTS:                             # a head slice of a longer batch as a part: first, in the middle, last
        out.append(_case("head_%d" % cut, [(130, dict(head=cut)), 31, (200, dict(head=cut, utf8="multibyte")), 2, (66, dict(head=cut))]))
    out.append(_case("head_all_valid_with_buffer", [(130, dict(head=1, pattern="last_zero")), (31, dict(pattern="zeros")),
                                                    (130, dict(head=63, pattern="last_zero")), (33, dict(pattern="zeros")),
                                                    (130, dict(head=64, pattern="last_zero")), (2, dict(pattern="zeros")),
                                                    (130, dict(head=65, pattern="last_zero"))]))
    out.append(_case("head_not_null", [(130, dict(head=63)), (100, dict(head=65)), 1], nullable=False))
    return out


def dest_offsets(lengths):
    """(rows before the part) mod 64, per part with rows"""
    out, row = [], 0
    for n in lengths:
        if n:
            out.append((row % 64, n))
        row += n
    return out


# ---- 2. the bits after a head slice --------------------------------------------------------------------------------------------------------

SLICE_ROWS = 1100
SLICE_KS = (1, 63, 64, 65, 127, 1000)
VARIANTS = ("A", "B")                                # A: the rows past the cut are all valid and true (stale ones); B: all NULL and false
TAIL_V = {"A": 10 ** 6, "B": -10 ** 6}


def slice_source(variant, k, seed=5):
    """1100 rows: c0 .. c18 as above, plus rn (the row number, never NULL), key (nullable Int64, 40 values: sort / join / hash key),
    v (nullable Int32 in -50 .. 50: SUM / MIN / MAX), x (nullable Float64, eighths: the range predicate).  Rows < k: scattered NULLs.
    Rows >= k: variant A all valid, Boolean true; B all NULL, Boolean false; v there is +-10^6, a value a MIN / MAX / SUM that read
    past the cut could not hide."""
    n = SLICE_ROWS
    rng = np.random.default_rng(seed)
    part = make_part(n, seed=seed + 1, pattern="random")
    b = OrderedDict()
    tail = np.arange(n) >= k

    def valid():
        return np.where(tail, variant == "A", rng.random(n) > 0.2)
    b["rn"] = OCol("Int64", np.arange(n, dtype=np.int64))
    b["key"] = OCol("Int64", rng.integers(0, 40, n) * 1000003 - 7, valid())
    b["v"] = OCol("Int32", np.where(tail, TAIL_V[variant], rng.integers(-50, 51, n)), valid())
    b["x"] = OCol("Float64", rng.integers(-400, 400, n) / 8.0, valid())
    for name, (t, v, _) in part.cols.items():
        if t == "Boolean":
            v = np.where(tail, variant == "A", rng.random(n) > 0.5)
        b[name] = OCol(t, v, valid())
    return b


# ---- 3. streams of batches -----------------------------------------------------------------------------------------------------------------

def coalesce_sizes(sizes, target):
    """the sizes of the batches CoalesceBatchesExec(target) makes of one partition's batches of `sizes` rows.

    The rule, as DataFusion's CoalesceBatchesStream::poll_next states it (physical_plan/coalesce_batches.rs of the revision the reference
    pins in rust/core/Cargo.toml:26, rev 46161d2 — an external dependency whose text is not part of the reference tree; the reference only builds the
    operator with its target, rust/core/src/serde/physical_plan/from_proto.rs:122-132, and prints it, rust/core/src/utils.rs:140-144):
    a batch of at least `target` rows passes as it is when nothing is buffered; an empty batch is dropped; any other batch is buffered,
    and once the buffered rows reach `target` (>=) they leave as one batch; what is left leaves at the end of the input."""
    out, pending = [], 0
    for n in sizes:
        if n >= target and pending == 0:
            out.append(n)
        elif n:
            pending += n
            if pending >= target:
                out.append(pending)
                pending = 0
    return out + ([pending] if pending else [])


T = 100                                              # the target of the sequences below
COALESCE_SEQUENCES = {                               # name -> (target, one list of batch sizes per partition)
    "pending_exactly_target": (T, [[40, 60, 30]]),
    "pending_target_minus_one_then_one": (T, [[40, 59, 1, 7]]),
    "pending_target_minus_one_at_the_end": (T, [[40, 59]]),
    "pending_target_plus_one": (T, [[40, 61, 5]]),
    "large_without_pending": (T, [[250, 100, 30]]),
    "large_with_pending": (T, [[30, 250, 100, 99, 100]]),
    "empty_between": (T, [[0, 50, 0, 0, 50, 0, 20, 0]]),
    "target_one": (1, [[1, 0, 3, 1]]),
    "target_above_all_input": (10 ** 6, [[30, 250, 1]]),
    "only_empty_batches": (T, [[0, 0]]),
    "two_partitions": (T, [[99, 1, 100, 5], [100, 5, 0, 95, 101]]),
}

COALESCE_SEQUENCES["empty_input"] = (T, [[], [5]])   # a partition without a batch, next to one with

LIMIT_BATCHES = [300, 200, 129]                      # one partition's batches: boundaries at 300 and 500 rows, 629 in all
LIMIT_PARTITIONS = [LIMIT_BATCHES, [], [129, 0, 300, 7]]
LIMITS = [0, 1, 150, 300, 301, 500, 629, 630, 10 ** 6]


def limit_sizes(sizes, limit):
    """the sizes of the batches a limit lets through of one stream: whole batches while they fit (an empty one among them passes),
    the head of the first that does not, nothing after the limit is reached"""
    out, left = [], limit
    for n in sizes:
        if left <= 0:
            break
        out.append(min(n, left))
        left -= out[-1]
    return out


def stream_batch(n, seed):
    """a narrow batch for the stream operators: rn-like id, a nullable Int32, a Boolean and a Utf8 column"""
    rng = np.random.default_rng(seed)
    return OrderedDict([("id", OCol("Int64", seed * 10 ** 6 + np.arange(n, dtype=np.int64))),
                        ("v", OCol("Int32", rng.integers(-9, 9, n), bits("random", n, rng))),
                        ("b", OCol("Boolean", bits("random", n, rng), bits("alternating", n, rng))),
                        ("s", OCol("Utf8", [WORDS[int(i)] for i in rng.integers(0, len(WORDS), n)], bits("edge_zero", n, rng)))])


def split_by_sizes(batches, sizes):
    """the concatenation of `batches`, cut into consecutive batches of `sizes` rows"""
    whole, out, lo = helpers.concat(batches), [], 0
    for n in sizes:
        out.append(helpers.slice_batch(whole, lo, lo + n))
        lo += n
    assert lo == og.batch_len(whole)
    return out
