"""Inputs for the hash aggregate's row-order Float64 sums (ballista_amd/csrc/kernels_dagg.hip) and a plain reference of what
DESIGN.md §3.4 promises about them.  Python and numpy only: nothing of the product is imported here.

A Case is the ordered rows of ONE partition: an Int64 key `k`, Float64 (or Float32) arguments x0 .. x{m-1} with optional
validity, an optional Int32 `keep` column (the predicate is keep = 1) and a list of batch cuts.

The reference (`reference`) works on the concatenated rows.  A RUN is a maximal stretch of consecutive kept rows with one key
that does not cross a multiple of 1024 rows.  Per group: the row count, the non-NULL count per argument, and per argument the
LEFT FOLD of the run sums in first-row order (total = r0; total = total + r1; ... in Python floats).  A NULL argument adds
+0.0 to its run.  SUM is NULL where the group has no non-NULL value, AVG is SUM / non-NULL count.

What happens INSIDE a run is not restated (the kernel adds a run's rows in a fixed tree over 64-row chunks).  Three value
families make that unnecessary:

  1  exact             multiples of 1/8, |v| <= 2^20, some negative, -0.0 and +0.0: every partial sum of every association is
                       exact, so the expected bits depend on no tree; a lost, doubled or misattributed row, run or carry
                       changes the result.  `check_family1` asserts the premise on the case itself.
  2  order-pinning     every multi-row stretch holds family-1 values and lies inside one tile (its sum is exact); the
                       ill-conditioned values sit in single-row runs: [1, 2^53, 1, .., 1, -2^52] (row-order fold 2^52) or seeded
                       draws from +-{2^53, 2^52, 1, 3}, redrawn until, for every group with at least 3 runs, the reverse fold,
                       the fold with the first run moved last and the fold with the last run moved first all differ in bits
                       from the row-order fold.  `check_family2` asserts that; a case that misses it is an error, not a skip.
  3  ill-conditioned   +-m * 2^e, e in 0..60, inside multi-row runs that straddle chunks and tiles: here the tree matters, so
                       the gate is the bound that holds for ANY order of addition, |got - exact| <= gamma_{n-1} * sum|x| with
                       gamma_k = k u / (1 - k u), u = 2^-53, n = the group's rows (NULLs included), exact by Fraction.

Keeping the aggregate on the hash table: every case that has room for them holds at least 12 groups (filler groups around the
watched ones).  A one-row or one-key case cannot, so every plan the tests build ALSO carries `primer(case)` as partition 0
— 13 groups in 39 rows — which is executed first and leaves the operator on the hash path for the case (partition 1).
"""
from __future__ import annotations

import struct
from collections import OrderedDict
from fractions import Fraction

import numpy as np

TILE = 1024                 # DS_TILE of kernels_dagg.hip
CHUNK = 64
LIST_MAX = 16               # DET_LIST_MAX of host/hash_kernels.h: more runs per group -> the sorted combine
PASS_ACCS = 4               # DS_MAX: Float64 sums per pass of the segment kernel
MAX_ACCS = 16               # VM_MAX_ACC of vm_isa.h
RUN_ROWS = 4096             # rows from which clustered input takes the run paths (ops_agg_hash.cpp)
N_FILLERS = 13
FILLER0 = 1000              # round-robin filler keys FILLER0 .. FILLER0 + 12
FRESH0 = 100000             # keys of filler blocks that are groups of their own
U = 2.0 ** -53
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096, 4097]
CUTS = (1, 63, 64, 64, 1000, 2053)        # 64 twice: an empty batch between two cuts


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


class Case:
    def __init__(self, name, family, k, xs, valids=None, keep=None, x_dtype="Float64", route=None, cuts=None):
        n = len(k)
        self.name, self.family = name, family
        self.k = np.asarray(k, dtype=np.int64)
        self.x_dtype = x_dtype
        self.xs = [np.asarray(x, dtype=np.float32 if x_dtype == "Float32" else np.float64) for x in xs]
        self.valids = [None] * len(xs) if valids is None else [None if v is None else np.asarray(v, dtype=np.bool_) for v in valids]
        self.keep = None if keep is None else np.asarray(keep, dtype=np.int32)
        self.route = route                    # None | "distinct" | "two" | "table": the run path a clustered case claims
        self.cuts = sorted(c for c in CUTS if c < n) if cuts is None else list(cuts)
        assert all(len(x) == n for x in self.xs) and all(v is None or len(v) == n for v in self.valids)
        assert self.keep is None or len(self.keep) == n
        assert all(0 <= a <= b <= n for a, b in zip([0] + self.cuts, self.cuts + [n]))
        self._ref = self._exact = None

    def __repr__(self):
        return f"Case({self.name}, family {self.family}, {self.n} rows, m = {self.m})"

    @property
    def n(self):
        return len(self.k)

    @property
    def m(self):
        return len(self.xs)

    def kept(self):
        return np.ones(self.n, np.bool_) if self.keep is None else self.keep == 1

    def valid(self, j):
        return np.ones(self.n, np.bool_) if self.valids[j] is None else self.valids[j]

    def batches(self, cut):
        """row ranges of the batches: one batch, or the case's cuts"""
        edges = [0] + (self.cuts if cut else []) + [self.n]
        return list(zip(edges[:-1], edges[1:]))

    def columns(self, lo, hi, m=None):
        """rows lo .. hi-1 as name -> (Arrow type, values, validity or None)"""
        out = OrderedDict([("k", ("Int64", self.k[lo:hi], None))])
        for j in range(self.m if m is None else m):
            out[f"x{j}"] = (self.x_dtype, self.xs[j][lo:hi], None if self.valids[j] is None else self.valids[j][lo:hi])
        if self.keep is not None:
            out["keep"] = ("Int32", self.keep[lo:hi], None)
        return out

    def with_args(self, m):
        """the same rows with the first m arguments only"""
        return Case(f"{self.name}[m={m}]", self.family, self.k, self.xs[:m], self.valids[:m], self.keep, self.x_dtype, self.route, self.cuts)


# ---- the reference ------------------------------------------------------------------------------------------------------------

def stretches(case):
    """maximal stretches of consecutive kept rows with one key: [(key, lo, hi)]"""
    out, kept, k = [], case.kept(), case.k
    i, n = 0, case.n
    while i < n:
        if not kept[i]:
            i += 1
            continue
        j = i + 1
        while j < n and kept[j] and k[j] == k[i]:
            j += 1
        out.append((int(k[i]), i, j))
        i = j
    return out


def runs(case):
    """stretches cut at every multiple of 1024 rows: [(key, lo, hi)] in row order"""
    out = []
    for key, lo, hi in stretches(case):
        while lo < hi:
            end = min(hi, (lo // TILE + 1) * TILE)
            out.append((key, lo, end))
            lo = end
    return out


def runs_per_group(case):
    cnt = OrderedDict()
    for key, _, _ in runs(case):
        cnt[key] = cnt.get(key, 0) + 1
    return cnt


def max_runs(case):
    return max(runs_per_group(case).values(), default=0)


def fold(values):
    total = values[0]
    for v in values[1:]:
        total = total + v
    return total


def addends(case, j, lo, hi):
    """the Python floats rows lo .. hi-1 add for argument j (NULL: +0.0)"""
    x, ok = case.xs[j], case.valid(j)
    return [float(x[i]) if ok[i] else 0.0 for i in range(lo, hi)]


class Ref:
    """keys in first-row order; per key: rows, nonnull[j], run_sums[j] (first-row order), sums[j] (None = NULL)"""

    def __init__(self):
        self.keys, self.rows, self.nonnull, self.run_sums, self.sums = [], {}, {}, {}, {}


def reference(case):
    if case._ref is not None:
        return case._ref
    r = Ref()
    for key, lo, hi in runs(case):
        if key not in r.rows:
            r.keys.append(key)
            r.rows[key] = 0
            r.nonnull[key] = [0] * case.m
            r.run_sums[key] = [[] for _ in range(case.m)]
        r.rows[key] += hi - lo
        for j in range(case.m):
            r.nonnull[key][j] += int(np.count_nonzero(case.valid(j)[lo:hi]))
            r.run_sums[key][j].append(fold(addends(case, j, lo, hi)))
    for key in r.keys:
        r.sums[key] = [fold(r.run_sums[key][j]) if r.nonnull[key][j] else None for j in range(case.m)]
    case._ref = r
    return r


def exact(case):
    """per key and argument: (the exact sum, the exact sum of magnitudes) as Fractions, over the kept non-NULL rows"""
    if case._exact is not None:
        return case._exact
    out = {}
    for key, lo, hi in runs(case):
        e = out.setdefault(key, [[Fraction(0), Fraction(0)] for _ in range(case.m)])
        for j in range(case.m):
            for v in addends(case, j, lo, hi):
                e[j][0] += Fraction(v)
                e[j][1] += abs(Fraction(v))
    case._exact = out
    return out


def gamma_bound(n_rows, abs_sum):
    """the bound on |computed - exact| of ANY order of adding n_rows values: gamma_{n-1} * sum|x|, as a Fraction"""
    ku = Fraction(max(n_rows - 1, 0)) * Fraction(U)
    return ku / (1 - ku) * abs_sum


def alternative_folds(run_sums):
    """three other orders of the same run sums: reversed, the first run last, the last run first"""
    rs = list(run_sums)
    return [fold(rs[::-1]), fold(rs[1:] + rs[:1]), fold(rs[-1:] + rs[:-1])]


def pins_the_order(run_sums):
    want = bits(fold(list(run_sums)))
    return all(bits(a) != want for a in alternative_folds(run_sums))


# ---- conditions a case asserts on itself -----------------------------------------------------------------------------------------

def check_family1(case):
    """every value is a multiple of 1/8 with |v| <= 2^20 and every group's sum of |v| * 8 stays below 2^53: all partial sums of all
    associations are exact"""
    for j in range(case.m):
        v = case.xs[j].astype(np.float64)
        assert np.all(np.abs(v) <= 2.0 ** 20) and np.all(v * 8 == np.round(v * 8)), (case.name, j)
    for key, e in exact(case).items():
        for j in range(case.m):
            assert e[j][1] * 8 < 2 ** 53, (case.name, key, j)


def check_family2(case):
    """multi-row stretches lie inside one tile and add up exactly; every group with >= 3 runs pins the order of its runs"""
    for key, lo, hi in stretches(case):
        if hi - lo > 1:
            assert lo // TILE == (hi - 1) // TILE, (case.name, key, lo, hi)
            for j in range(case.m):
                a = addends(case, j, lo, hi)
                assert Fraction(fold(a)) == sum(Fraction(v) for v in a), (case.name, key, lo, hi, j)
    ref = reference(case)
    pinned = 0
    for key in ref.keys:
        if len(ref.run_sums[key][0]) >= 3:
            for j in range(case.m):
                assert pins_the_order(ref.run_sums[key][j]), (case.name, key, j)
            pinned += 1
    return pinned


# ---- expected output ----------------------------------------------------------------------------------------------------------------

def agg_spec(m, avg_of=0, count_of=None):
    """SUM(x0) .. SUM(x{m-1}), COUNT(*), AVG(x{avg_of}) [, COUNT(x{count_of})] as (function, argument) pairs"""
    spec = [("sum", j) for j in range(m)] + [("rows", None), ("avg", avg_of)]
    return spec + ([("count", count_of)] if count_of is not None else [])


def agg_name(fun, j):
    return "n" if fun == "rows" else {"sum": "s", "avg": "a", "count": "c"}[fun] + str(j)


def _sum_cast(case, fun, v):
    if fun == "sum" and case.x_dtype == "Float32":
        return float(np.float32(v))           # (family 1: the exact sum, rounded once)
    return v


def expected(cases, spec, mode):
    """the output of HashAggregateExec(mode, [k], spec) over the union of `cases` (disjoint keys), sorted by key:
    name -> (Arrow type, values, validity); and the names of the Float sum / average columns"""
    rows = []
    for case in cases:
        ref = reference(case)
        for key in ref.keys:
            rows.append((key, case, ref))
    rows.sort(key=lambda r: r[0])
    assert len({r[0] for r in rows}) == len(rows)
    out = OrderedDict([("k", ("Int64", np.array([r[0] for r in rows], np.int64), None))])
    float_cols = []
    x_dtype = cases[0].x_dtype

    def col(name, dtype, vals):
        ok = np.array([v is not None for v in vals], np.bool_)
        arr = np.array([0 if v is None else v for v in vals], {"UInt64": np.uint64, "Float64": np.float64, "Float32": np.float32}[dtype])
        out[name] = (dtype, arr, ok)
        if dtype != "UInt64":
            float_cols.append(name)

    for fun, j in spec:
        name = agg_name(fun, j)
        if fun == "rows":
            col(name + ("[count]" if mode == "Partial" else ""), "UInt64", [ref.rows[key] for key, _, ref in rows])
        elif fun == "count":
            col(name + ("[count]" if mode == "Partial" else ""), "UInt64", [ref.nonnull[key][j] for key, _, ref in rows])
        elif fun == "sum":
            col(name + ("[sum]" if mode == "Partial" else ""), x_dtype,
                [None if ref.sums[key][j] is None else _sum_cast(c, fun, ref.sums[key][j]) for key, c, ref in rows])
        elif mode == "Partial":
            col(name + "[count]", "UInt64", [ref.nonnull[key][j] for key, _, ref in rows])
            col(name + "[sum]", "Float64", [ref.sums[key][j] for key, _, ref in rows])
        else:
            col(name, "Float64", [None if ref.sums[key][j] is None else ref.sums[key][j] / ref.nonnull[key][j] for key, _, ref in rows])
    return out, float_cols


def aggregates(E, spec):
    """the spec as aggregate expressions; E: ballista_amd.expr, handed in by the caller"""
    out = []
    for fun, j in spec:
        name = agg_name(fun, j)
        if fun == "rows":
            out.append(E.Count(E.lit(1, E.UINT8), name))
        else:
            out.append({"sum": E.Sum, "avg": E.Avg, "count": E.Count}[fun](E.col(f"x{j}"), name))
    return out


def plan(P, E, source, case, spec, mode="Partial"):
    """HashAggregateExec(Partial) over `source`, FilterExec(keep = 1) directly under it where the case has a predicate; mode
    "Final": Partial -> MergeExec -> Final.  P: the module of plan classes (ballista_amd or tests/plan_nodes.py)"""
    if case.keep is not None:
        source = P.FilterExec(E.coerce(E.col("keep").eq(E.lit(1)), {"keep": "Int32"}), source)
    group = [(E.col("k"), "k")]
    part = P.HashAggregateExec("Partial", group, aggregates(E, spec), source)
    if mode == "Partial":
        return part
    return P.HashAggregateExec("Final", group, aggregates(E, spec), P.MergeExec(part))


def host_batches(case, cut, OCol, m=None):
    """the case's batches as oracle-style batches (name -> OCol)"""
    return [OrderedDict((name, OCol(t, v, ok)) for name, (t, v, ok) in case.columns(lo, hi, m).items()) for lo, hi in case.batches(cut)]


def sorted_by_key(batch):
    idx = np.argsort(batch["k"].values, kind="stable")
    return OrderedDict((name, c.take(idx)) for name, c in batch.items())


def check_result(got, cases, spec, mode, helpers, gate="bits"):
    """`got` (an oracle-style batch, any row order) against the reference over `cases`.  Keys, counts and validity: bit for bit.
    The sums, gate "bits": bit for bit, except that an exactly zero sum may carry either sign; gate "gamma": within the bound
    for any order of addition around the exact sum (Partial states only)"""
    want_cols, float_cols = expected(cases, spec, mode)
    want = OrderedDict((name, helpers.OCol(t, v, ok)) for name, (t, v, ok) in want_cols.items())
    if not got or len(got["k"]) == 0:
        assert len(want["k"]) == 0, (len(want["k"]), "groups expected, none returned")
        return
    got = sorted_by_key(got)
    helpers.assert_same_schema(got, want)
    plain = [name for name in want if name not in float_cols]
    helpers.assert_bit_exact(OrderedDict((n, got[n]) for n in plain), OrderedDict((n, want[n]) for n in plain))
    for name in float_cols:
        assert np.array_equal(got[name].is_valid(), want[name].is_valid()), f"{name}: validity differs"
    if gate == "bits":
        helpers.assert_rows_equal(got, want, ordered=True, float_rtol=0.0, zero_sign_cols=tuple(float_cols))
        return
    assert mode == "Partial" and len(cases) == 1
    case = cases[0]
    ex, ref = exact(case), reference(case)
    for name in float_cols:
        j = int(name.split("[")[0][1:])
        for key, v, ok in zip(want["k"].values, got[name].values, got[name].is_valid()):
            if ok:
                e, a = ex[int(key)][j]
                assert abs(Fraction(float(v)) - e) <= gamma_bound(ref.rows[int(key)], a), (case.name, name, int(key), float(v), float(e))


# ---- values---------------------------------------------------------------------------------------------------------------------------

def f1_values(rng, n):
    v = rng.integers(-2 ** 23, 2 ** 23 + 1, n).astype(np.float64) / 8.0
    z = rng.random(n)
    v[z < 0.04] = -0.0
    v[z > 0.96] = 0.0
    return v


def f3_values(rng, n):
    return rng.integers(1, 2 ** 20, n).astype(np.float64) * np.exp2(rng.integers(0, 61, n)) * rng.choice([-1.0, 1.0], n)


PATTERN_DRAWS = np.array([2.0 ** 53, 2.0 ** 52, 1.0, 3.0, -2.0 ** 53, -2.0 ** 52, -1.0, -3.0])


def fixed_pattern(r, scale=1.0):
    """[1, 2^53, 1, .., 1, -2^52] * scale: the row-order fold is 2^52 * scale"""
    assert r >= 3
    p = [1.0, 2.0 ** 53] + [1.0] * (r - 3) + [-2.0 ** 52]
    assert fold(p) == 2.0 ** 52
    return [v * scale for v in p]


def f2_fill(rng, case_k, keep, j, fixed):
    """argument j of a family-2 case: family-1 values everywhere, then the single-row runs of every group with >= 3 runs hold
    the fixed pattern (all runs single rows, `fixed`) or seeded draws, redrawn until the group pins its order"""
    n = len(case_k)
    x = f1_values(rng, n)
    probe = Case("probe", 2, case_k, [x], keep=keep)
    by_key = OrderedDict()
    for key, lo, hi in runs(probe):
        by_key.setdefault(key, []).append((lo, hi))
    for gi, (key, rs) in enumerate(by_key.items()):
        if len(rs) < 3:
            continue
        singles = [q for q, (lo, hi) in enumerate(rs) if hi - lo == 1]
        sums = [fold([float(v) for v in x[lo:hi]]) for lo, hi in rs]
        if fixed and len(singles) == len(rs):
            vals = fixed_pattern(len(rs), 2.0 ** (gi % 7))
            assert pins_the_order(vals)
        else:
            assert len(singles) >= 2, (key, "too few single-row runs to pin the order")
            for _ in range(20000):
                draw = rng.choice(PATTERN_DRAWS, len(singles))
                vals = list(sums)
                for q, v in zip(singles, draw):
                    vals[q] = float(v)
                if pins_the_order(vals):
                    break
            else:
                raise AssertionError(f"group {key}: no draw pins the order")
        for q in singles:
            x[rs[q][0]] = vals[q]
    return x


def make_case(name, family, k, m=2, keep=None, null_rows=None, seed=None, x_dtype="Float64", route=None, null_rate=0.0):
    """values of the family over a key layout.  null_rows: {argument: rows that are NULL}; null_rate: random NULLs on the odd
    arguments (families 1 and 3)"""
    rng = np.random.default_rng(sum(map(ord, name)) * 7 + family if seed is None else seed)
    n = len(k)
    xs, valids = [], []
    for j in range(m):
        if family == 1:
            xs.append(f1_values(rng, n))
        elif family == 2:
            xs.append(f2_fill(rng, k, keep, j, fixed=(j == 0)))
        else:
            xs.append(f3_values(rng, n))
        v = None
        if null_rows and j in null_rows:
            v = np.ones(n, np.bool_)
            v[list(null_rows[j])] = False
        elif null_rate and j % 2 == 1 and family != 2:
            v = rng.random(n) >= null_rate
        valids.append(v)
    return Case(name, family, k, xs, valids, keep, x_dtype, route)


# ---- key layouts ------------------------------------------------------------------------------------------------------------------------

def layout(n, placed, filler, split_fresh_at_tiles=False):
    """n rows: the (key, lo, hi) stretches of `placed`, filler keys everywhere else.  filler "rr": 13 keys round-robin, every
    filler row a run of its own (hundreds of runs per group: the sorted combine); "fresh": blocks of up to 41 rows (7 in a small case), each block a
    group of its own (one run, two where it crosses a tile end — never with split_fresh_at_tiles — so no list grows long)"""
    k = np.full(n, -1, np.int64)
    for key, lo, hi in placed:
        assert 0 <= lo < hi <= n and np.all(k[lo:hi] == -1), (key, lo, hi)
        k[lo:hi] = key
    free = k == -1
    if filler == "rr":
        k[free] = FILLER0 + np.arange(n)[free] % N_FILLERS
    else:
        nxt, i, block = FRESH0, 0, 41 if n >= 600 else 7
        while i < n:
            if not free[i]:
                i += 1
                continue
            j = i
            while j < n and free[j] and j - i < block and not (split_fresh_at_tiles and j > i and j % TILE == 0):
                j += 1
            k[i:j] = nxt
            nxt += 1
            i = j
    for key, lo, hi in placed:                       # a placed stretch is a stretch: its neighbours hold other keys
        assert (lo == 0 or k[lo - 1] != key) and (hi == n or k[hi] != key), (key, lo, hi)
    return k


def size_layout(n, kind, rng):
    if kind == "round_robin":
        return FILLER0 + np.arange(n, dtype=np.int64) % N_FILLERS
    if kind == "one_key":
        return np.full(n, 7, np.int64)
    return FILLER0 + rng.integers(0, N_FILLERS, n).astype(np.int64)


# one watched group (key 7) with a single stretch; what the placement is there for
BOUNDARIES = OrderedDict([
    ("ends_on_lane_62", (62, 63)),
    ("ends_on_lane_63", (63, 64)),
    ("carry_into_lane_0", (63, 65)),
    ("exactly_one_chunk", (64, 128)),
    ("carry_through_two_chunks", (10, 200)),
    ("tile_end_closes_the_chunk", (1000, 1024)),
    ("tile_end_closes_the_carry", (1000, 1025)),
    ("two_rows_across_the_tile_end", (1023, 1025)),
    ("four_runs", (500, 3100)),
])


def boundary_case(name, filler):
    lo, hi = BOUNDARIES[name]
    n = hi + 70 if hi % CHUNK else hi + 64 + 6
    k = layout(n, [(7, lo, hi)], filler)
    return make_case(f"boundary_{name}_{filler}", 1, k, m=2, null_rate=0.1)


def carry_then_closes_case(filler):
    """key 7 ends on lane 63 of chunk 1 (rows 70 .. 127: it is the carry), key 8 starts on lane 0 of chunk 2 and closes inside
    it together with further runs: emit_carry and the chunk's own closes in one step.  The last chunk is partial and its final run
    (key 9) ends on the last row"""
    n = 3 * CHUNK + 37
    k = layout(n, [(7, 70, 128), (8, 128, 140), (7, 150, 160), (9, n - 9, n)], filler)
    return make_case(f"carry_then_closes_{filler}", 1, k, m=2, null_rate=0.1)


def spread(groups, pad, split):
    """groups: [(key, single-row runs)].  The rows of all groups spread evenly over each other, a fresh-key block of
    pad[i % len(pad)] rows between neighbours: several tiles, every listed row a run of its own"""
    rows = sorted(((q + 0.5) / r + 1e-4 * gi, key) for gi, (key, r) in enumerate(groups) for q in range(r))
    seq = []
    for i, (_, key) in enumerate(rows):
        seq.append((key, 1))
        seq.append((None, pad[i % len(pad)]))
    n = sum(length for _, length in seq)
    placed, at = [], 0
    for key, length in seq:
        if key is not None:
            placed.append((key, at, at + 1))
        at += length
    k = layout(n, placed, "fresh", split_fresh_at_tiles=split)
    got = Case("probe", 1, k, [np.zeros(n)])
    rp = runs_per_group(got)
    assert all(rp[key] == r for key, r in groups), [(key, rp[key], r) for key, r in groups]
    return k


MANY_RUNS = [(1, 1), (2, 2), (3, 15), (4, 16), (5, 17), (6, 40)] + [(7 + i, 3 + i) for i in range(8)]
FEW_RUNS = [(1, 1), (2, 2), (3, 3), (4, 15), (5, 16), (6, 16)] + [(7 + i, 3 + i) for i in range(8)]
PADS = (0, 31, 17, 0, 40, 9, 23, 64, 5)


def runs_case(which, family):
    groups = MANY_RUNS if which == "with_17_and_40" else FEW_RUNS
    k = spread(groups, PADS, split=family == 2)
    c = make_case(f"runs_per_group_{which}_f{family}", family, k, m=2)
    assert (max_runs(c) > LIST_MAX) == (which == "with_17_and_40") and c.n > 2 * TILE
    return c


def mixed_layout(n, rng, max_len, split, extra=()):
    """random stretches of 1 .. max_len rows over 14 keys (1 .. 14), neighbours differing; split: cut at tile ends by changing
    the key there.  extra: (key, rows) single rows planted afterwards"""
    k = np.zeros(n, np.int64)
    i, prev = 0, 0
    while i < n:
        key = int(rng.integers(1, 15))
        if key == prev:
            key = key % 14 + 1
        length = int(rng.integers(1, max_len + 1))
        j = min(n, i + length)
        if split:
            j = min(j, (i // TILE + 1) * TILE)
        k[i:j] = key
        i, prev = j, key
    for key, rows in extra:
        for r in rows:
            k[r] = key
            assert k[r - 1] != key and (r + 1 == n or k[r + 1] != key)
    return k


def acc_layout():
    """runs that straddle chunks and tiles over 14 keys, and key 50 in 17 single-row runs"""
    rng = np.random.default_rng(4242)
    n = 2500
    k = mixed_layout(n, rng, 150, split=False, extra=[(50, range(40, 40 + 17 * 140, 140))])
    probe = Case("probe", 1, k, [np.zeros(n)])
    assert runs_per_group(probe)[50] == 17
    assert any(lo < b < hi for _, lo, hi in stretches(probe) for b in (TILE, 2 * TILE))
    return k


ACC_M = (1, 4, 5, 8, 9)


def acc_case(family=1):
    """nine arguments; the tests aggregate the first m of them (with_args)"""
    c = make_case(f"accumulators_f{family}", family, acc_layout(), m=max(ACC_M), null_rate=0.15)
    assert max(ACC_M) + 2 <= MAX_ACCS
    return c


def nulls_case(filler):
    """x0: NULL on lane 0, on lane 63 and on the row behind it; on a tile's last row and the first of the next; a run of NULLs
    only inside a group that has values elsewhere (key 8); a group of NULLs only in two runs (key 9)"""
    n = 1200
    placed = [(7, 0, 70), (8, 200, 210), (8, 230, 240), (9, 300, 305), (9, 400, 401), (7, 1000, 1030)]
    k = layout(n, placed, filler)
    null0 = [0, 63, 64, 1023, 1024] + list(range(200, 210)) + list(range(300, 305)) + [400]
    c = make_case(f"nulls_{filler}", 1, k, m=2, null_rows={0: null0, 1: [5, 1023]})
    ref = reference(c)
    assert ref.sums[9][0] is None and ref.rows[9] == 6 and ref.sums[9][1] is not None and ref.sums[8][0] is not None
    return c


def predicate_case(runs_of_11, filler):
    """keep = 0: inside a run (key 7), on lane 63 (key 8), on row 1023 (key 9), a whole chunk (key 10), every 3rd row of key 11
    (runs_of_11 runs of two rows), every row of key 12 (the group does not exist) and some filler rows"""
    n = 1300
    placed = [(7, 10, 40), (8, 50, 100), (10, 128, 320), (9, 1000, 1050), (11, 1100, 1100 + 3 * runs_of_11 - 1), (12, 1200, 1230)]
    k = layout(n, placed, filler)
    keep = np.ones(n, np.int32)
    keep[[25, 63, 1023]] = 0
    keep[192:256] = 0
    keep[1102:1100 + 3 * runs_of_11 - 1:3] = 0
    keep[1200:1230] = 0
    keep[np.flatnonzero(k >= FILLER0)[::11]] = 0
    c = make_case(f"predicate_{runs_of_11}_runs_{filler}", 1, k, m=2, keep=keep, null_rate=0.1)
    rp = runs_per_group(c)
    assert rp[7] == 2 and rp[8] == 2 and rp[9] == 2 and rp[10] == 2 and rp[11] == runs_of_11 and 12 not in rp
    return c


def predicate_single_rows_case():
    """family 2 behind the predicate: every other row of keys 7 (17 kept rows) and 8 (16) dropped, so each kept row is a run"""
    n = 1100
    k = layout(n, [(7, 20, 53), (8, 1000, 1031)], "rr")
    keep = np.ones(n, np.int32)
    keep[21:53:2] = 0
    keep[1001:1031:2] = 0
    c = make_case("predicate_single_row_runs_f2", 2, k, m=2, keep=keep)
    rp = runs_per_group(c)
    assert rp[7] == 17 and rp[8] == 16
    return c


def predicate_drops_everything_case():
    n = 300
    k = layout(n, [(7, 10, 40)], "rr")
    return make_case("predicate_drops_every_row", 1, k, m=2, keep=np.zeros(n, np.int32))


def clustered_lengths(n, rng):
    """stretch lengths 2 .. 9 adding up to n, none ending on row 1024, 2048 or 3072"""
    out, at = [], 0
    while at < n:
        length = int(rng.integers(2, 10))
        if at + length in (TILE, 2 * TILE, 3 * TILE):
            length += 1
        length = min(length, n - at)
        out.append(length)
        at += length
    if out[-1] == 1 and len(out) > 1:                 # (keep runs <= rows / 2 comfortably)
        out[-2] += 1
        out.pop()
    return out


def n_breaks(k):
    return int(np.count_nonzero(k[1:] < k[:-1]))


def run_path_case(n, form):
    """clustered input: ascending keys (every run a group), one descent (two ascending stretches; the second holds keys of the
    first and new ones), a key that comes back twice (the run table).  Stretches straddle rows 1024, 2048 and 3072"""
    rng = np.random.default_rng(n * 3 + len(form))
    lengths = clustered_lengths(n, rng)
    s = len(lengths)
    keys = np.arange(s, dtype=np.int64) * 3 + 10
    if form == "one_descent":
        cut = s * 2 // 3
        tail = np.sort(np.concatenate([keys[5:cut:4][:(s - cut) // 2], keys[7:cut:4] + 1]))[:s - cut]
        tail = np.unique(tail)
        keys = np.concatenate([keys[:cut], tail, keys[-1] + 3 * np.arange(1, s - cut - len(tail) + 1)])
    elif form == "comes_back":
        keys[s // 3] = keys[20]
        keys[2 * s // 3] = keys[20]
    k = np.repeat(keys, lengths)
    assert len(k) == n and n_breaks(k) == {"ascending": 0, "one_descent": 1, "comes_back": 2}[form]
    route = None if n < RUN_ROWS else {"ascending": "distinct", "one_descent": "two", "comes_back": "table"}[form]
    c = make_case(f"run_path_{form}_{n}", 1, k, m=2, route=route, null_rate=0.1)
    st = stretches(c)
    assert 2 * len(st) <= n and all(any(lo < b < hi for _, lo, hi in st) for b in (TILE, 2 * TILE, 3 * TILE))
    if form == "one_descent":
        first, second = set(k[:np.flatnonzero(k[1:] < k[:-1])[0] + 1]), set(k[np.flatnonzero(k[1:] < k[:-1])[0] + 1:])
        assert first & second and second - first
    if form == "comes_back":
        assert runs_per_group(c)[int(keys[20])] >= 3
    return c


RUN_FORMS = ("ascending", "one_descent", "comes_back")
RUN_SIZES = (4095, 4096, 4097)


def run_table_f2_case():
    """family 2 on the run table: 4096 clustered rows whose stretches end at every tile end, and key 5 coming back as 17 single
    rows, key 6 as 3"""
    rng = np.random.default_rng(77)
    n = 4096
    lengths = []
    for _ in range(4):
        part = clustered_lengths(TILE, rng)
        lengths += part
    s = len(lengths)
    keys = np.arange(s, dtype=np.int64) * 3 + 10
    lengths = np.array(lengths)
    ones = np.flatnonzero(lengths >= 3)[5::9]
    assert len(ones) >= 20
    k = np.repeat(keys, lengths)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    for q, si in enumerate(ones[:20]):
        k[starts[si] + 1] = 5 if q < 17 else 6                # a single row inside a stretch: it splits the stretch, too
    c = make_case("run_table_f2", 2, k, m=2, route="table")
    rp = runs_per_group(c)
    assert rp[5] == 17 and rp[6] == 3 and 2 * len(stretches(c)) <= n and n_breaks(k) > 1
    return c


def ill_conditioned_case():
    rng = np.random.default_rng(9)
    k = mixed_layout(3000, rng, 120, split=False)
    c = make_case("ill_conditioned_inside_runs", 3, k, m=2, null_rate=0.1)
    assert any(lo < b < hi for _, lo, hi in stretches(c) for b in (TILE, 2 * TILE))
    return c


def float32_case():
    rng = np.random.default_rng(32)
    k = mixed_layout(1100, rng, 90, split=False, extra=[(50, range(30, 30 + 17 * 60, 60))])
    return make_case("float32_argument", 1, k, m=2, x_dtype="Float32", null_rate=0.1)


def size_cases():
    out = []
    for n in SIZES:
        for kind in ("round_robin", "one_key", "random"):
            rng = np.random.default_rng(n)
            route = "distinct" if kind == "one_key" and n >= RUN_ROWS else None          # one run: clustered, and ascending
            out.append(make_case(f"size_{n}_{kind}", 1, size_layout(n, kind, rng), m=2, null_rate=0.1, route=route))
    return out


def derived_route(case):
    """the run path ops_agg_hash.cpp takes for the case's rows, read off the keys: none below 4096 rows, behind a predicate or
    with more than half as many stretches of equal keys as rows; else by the places where the key descends"""
    k = case.k
    if case.keep is not None or case.n < RUN_ROWS or 2 * (1 + int(np.count_nonzero(k[1:] != k[:-1]))) > case.n:
        return None
    return ("distinct", "two", "table")[min(n_breaks(k), 2)]


def order_pinning_cases():
    """family 2: the two runs-per-group inputs; every row a run of its own over 13 groups, one full tile (1024 records), a tile
    and a row, and past the run threshold; short stretches mixed with single rows; behind the predicate; on the run table"""
    out = [runs_case("with_17_and_40", 2), runs_case("at_most_16", 2)]
    for n in (1024, 1025, 4097):
        out.append(make_case(f"every_row_a_run_{n}_f2", 2, size_layout(n, "round_robin", None), m=2))
    rng = np.random.default_rng(5)
    out.append(make_case("short_stretches_f2", 2, mixed_layout(2500, rng, 3, split=True), m=2))
    out.append(predicate_single_rows_case())
    out.append(run_table_f2_case())
    return out


def exact_cases():
    out = size_cases()
    for filler in ("rr", "fresh"):
        out += [boundary_case(name, filler) for name in BOUNDARIES]
        out.append(carry_then_closes_case(filler))
        out.append(nulls_case(filler))
        out += [predicate_case(20, filler), predicate_case(16, filler)]
    out += [runs_case("with_17_and_40", 1), runs_case("at_most_16", 1)]
    out.append(predicate_drops_everything_case())
    out += [run_path_case(n, form) for n in RUN_SIZES for form in RUN_FORMS]
    out.append(float32_case())
    return out


_ALL = None


def all_cases():
    """every case but the accumulator ladder (acc_case), built once"""
    global _ALL
    if _ALL is None:
        _ALL = exact_cases() + order_pinning_cases() + [ill_conditioned_case()]
        names = [c.name for c in _ALL]
        assert len(set(names)) == len(names)
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


def primer(case, m=None):
    """13 groups (keys -1 .. -13) in 39 rows with the case's columns: partition 0 of every plan.  Executed first, it leaves the
    operator on the hash table for the case's partition, whatever that holds"""
    rng = np.random.default_rng(1)
    n = 3 * N_FILLERS
    m = case.m if m is None else m
    k = -1 - np.arange(n, dtype=np.int64) % N_FILLERS
    keep = None if case.keep is None else np.ones(n, np.int32)
    return Case("primer", 1, k, [f1_values(rng, n) for _ in range(m)], [None] * m, keep, case.x_dtype, cuts=[])
