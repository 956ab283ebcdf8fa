"""TEST INFRASTRUCTURE — chunked, extended-precision CPU reference of TPC-H Q1 / Q6 / Q3 / Q5 at ANY table size, SF100 included.

The synthetic tables are a pure function of the row index (oracle/tpch_gen.c, bit-identical to the device generator by
tests/test_generator.py), so the reference never holds a table: it generates a chunk of rows, folds it into the state of all four
queries and forgets it.  Written in numpy from the SQL text of the queries as ballista_amd/tpch.py states them.  It uses neither
oracle/plan_eval.py, oracle/engine.py's operators nor the C ports of oracle_ops.c, so that all of those can be checked against it
(tests/test_fullsize_reference.py); of ballista_amd it needs only the constant lists below, which callers pass in or which are
restated in oracle/gen.py.  The small tables (`dims`: customer and supplier in the layout of ballista_amd.tpch.dimension_arrays)
are an INPUT.

Arithmetic
  * per-row expressions in Float64, one rounding per node, as written: ext * (1 - disc), (...) * (1 + tax), ext * disc.  numpy
    never contracts a multiply and an add, and the device evaluates rows bit-identically;
  * counts are Python ints;
  * sums: EXTENDED says which of two paths ran.
      EXTENDED (np.longdouble has a 64-bit significand, x87): every chunk-and-group sum is np.sum(x[mask], dtype=np.longdouble),
      numpy's pairwise summation: at most 128 / 8 + 3 sequential additions per leaf block and log2(n / 128) levels above it, < 40
      roundings for any chunk below 2^28 rows; chunk partials are added sequentially in longdouble.  All addends are positive, so
      the result is within (40 + n_chunks) * 2^-64 relative of the exact sum: 1e-17 for SF100 in the default 4 Mi-row chunks
      (144 chunks), 3.3e-16 for SF1 in 1000-row chunks.  SUM_REL_ERROR(n_chunks) returns the bound.  It is used against
      tolerances of 1e-13 (goldens) and 1e-9 (device), four and eight orders above it.
      not EXTENDED (longdouble == double): Float64 pairwise np.sum per chunk, < 40 * 2^-53 = 4.4e-15 relative, and math.fsum
      (exact) over the chunk partials.
  * Q3 sums at most a handful of rows per group and is used with a bound of n_max * 2^-53, so it gets no rounding at all: the
    matched rows are kept (0.55 % of the table), sorted by group, and each group is summed sequentially in longdouble.  The
    result carries `revenue_exact`: True when every such sum provably fits the 64-bit significand (all addends are multiples of
    2^(e_min - 52) and every group total is below 2^(e_min + 12)), which holds for this generator (810 <= addend < 2^17, groups of
    at most 14 rows).  Without EXTENDED each group goes through math.fsum, which is exact up to the final rounding to Float64.

Chunks are generated on the calling thread (the C generator is itself OpenMP-parallel) and folded on a
ThreadPoolExecutor(min(16, CPUs this process may use)); numpy releases the GIL in the folds.  At most threads + 1 chunks are
alive at a time (0.23 GB per 4 Mi-row lineitem chunk), plus the Q3 / Q5 order tables (about 15 M + 4.5 M keys at SF100).
"""
from __future__ import annotations

import datetime
import math
import os
import threading
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import gen

EXTENDED = np.finfo(np.longdouble).nmant >= 63
_ACC = np.longdouble if EXTENDED else np.float64
CHUNK_ROWS = 1 << 22

SEGMENTS = gen.JoinQueryPort.SEGMENTS          # the order ballista_amd.tpch.SEGMENTS indexes c_mktsegment by
NATIONS = gen.NATIONS
REGIONS = gen.REGIONS


def SUM_REL_ERROR(n_chunks):
    """relative error bound of a Q1 / Q6 / Q5 sum of this module over n_chunks chunks (see the module docstring)"""
    return (40 + n_chunks) * 2.0 ** -64 if EXTENDED else 40 * 2.0 ** -53


def _date(s):
    return (datetime.date.fromisoformat(s) - datetime.date(1970, 1, 1)).days


Q1_SHIPDATE_MAX = _date("1998-09-02")           # l_shipdate <= date '1998-09-02'
Q6_DATE_LO, Q6_DATE_HI = _date("1994-01-01"), _date("1995-01-01")
Q6_DISC_LO, Q6_DISC_HI = 0.06 - 0.01, 0.06 + 0.01     # BETWEEN 0.06 - 0.01 AND 0.06 + 0.01, evaluated in Float64
Q6_QTY_MAX = 24.0
Q3_DATE = _date("1995-03-15")
Q5_DATE_LO, Q5_DATE_HI = _date("1994-01-01"), _date("1995-01-01")


def n_threads():
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
    return max(1, min(16, cpus))


def _sum(x):
    return np.sum(x, dtype=_ACC)


def _total(partials):
    """chunk partials -> one number: sequential longdouble additions, or math.fsum of Float64 partials"""
    if not EXTENDED:
        return math.fsum(float(p) for p in partials)
    t = np.longdouble(0)
    for p in partials:
        t = t + p
    return t


class _Lookup:
    """key -> row of a small table; direct indexing when the keys are 1..n in order (every table of this generator), binary search
    otherwise.  find(k) returns (row, found)."""

    def __init__(self, keys):
        keys = np.asarray(keys)
        self.n = len(keys)
        self.dense = self.n > 0 and bool(np.array_equal(keys, np.arange(1, self.n + 1, dtype=keys.dtype)))
        if not self.dense:
            self.order = np.argsort(keys, kind="stable")
            self.sorted = keys[self.order]

    def find(self, k):
        if self.n == 0:
            return np.zeros(len(k), np.int64), np.zeros(len(k), bool)
        if self.dense:
            row = k.astype(np.int64) - 1
            found = (row >= 0) & (row < self.n)
            return np.where(found, row, 0), found
        pos = np.minimum(np.searchsorted(self.sorted, k), self.n - 1)
        return self.order[pos], self.sorted[pos] == k


def _sorted_find(sorted_keys, k):
    """positions of k in the ascending, duplicate-free sorted_keys -> (pos, found)"""
    if len(sorted_keys) == 0:
        return np.zeros(len(k), np.int64), np.zeros(len(k), bool)
    pos = np.minimum(np.searchsorted(sorted_keys, k), len(sorted_keys) - 1)
    return pos, sorted_keys[pos] == k


def _chunks(n, chunk_rows):
    chunk_rows = max(1, int(chunk_rows)) if chunk_rows else max(1, n)
    return [(lo, min(chunk_rows, n - lo)) for lo in range(0, n, chunk_rows)]


def _map_chunks(chunks, generate, fold, threads):
    """fold(generate(lo, n)) for every chunk, results in chunk order.  Generation stays on this thread; at most threads + 1
    generated chunks exist at a time."""
    if threads <= 1 or len(chunks) <= 1:
        return [fold(generate(lo, n)) for lo, n in chunks]
    slots = threading.Semaphore(threads + 1)

    def job(arrays):
        try:
            return fold(arrays)
        finally:
            del arrays
            slots.release()

    futures = []
    with ThreadPoolExecutor(threads) as pool:
        for lo, n in chunks:
            slots.acquire()
            futures.append(pool.submit(job, generate(lo, n)))
        return [f.result() for f in futures]


# ---- orders pass: the build sides of Q3 and Q5 ---------------------------------------------------------------------------

def _fold_orders(o, cust, is_building, c_nation, asia):
    key, date = o["o_orderkey"], o["o_orderdate"]
    out = {}
    # Q3: c_mktsegment = 'BUILDING' and c_custkey = o_custkey and o_orderdate < date '1995-03-15'
    m = date < Q3_DATE
    row, found = cust.find(o["o_custkey"][m])
    keep = found & is_building[row]
    out["q3"] = (key[m][keep], date[m][keep], o["o_shippriority"][m][keep])
    # Q5: o_orderdate >= '1994-01-01' and < '1995-01-01', customer's nation in region ASIA
    m = (date >= Q5_DATE_LO) & (date < Q5_DATE_HI)
    row, found = cust.find(o["o_custkey"][m])
    nat = c_nation[row]
    keep = found & asia[nat]
    out["q5"] = (key[m][keep], nat[keep])
    return out


def _orders_pass(sf, n_orders, key64, dims, chunk_rows, threads):
    c = dims["customer"]
    cust = _Lookup(c["c_custkey"])
    is_building = np.asarray(c["c_mktsegment"]) == SEGMENTS.index("BUILDING") if "c_mktsegment" in c else np.zeros(len(c["c_custkey"]), bool)
    c_nation = np.asarray(c["c_nationkey"])
    asia = np.array([REGIONS[r] == "ASIA" for _, r in NATIONS])
    parts = _map_chunks(_chunks(n_orders, chunk_rows), lambda lo, n: gen.orders_arrays(sf, lo, n, key64=key64),
                        lambda o: _fold_orders(o, cust, is_building, c_nation, asia), threads)
    kdt = np.int64 if key64 else np.int32

    def cat(q, i, dtype):
        return np.concatenate([p[q][i] for p in parts]) if parts else np.zeros(0, dtype)

    k3, d3, p3 = cat("q3", 0, kdt), cat("q3", 1, np.int32), cat("q3", 2, np.int32)
    o3 = np.argsort(k3, kind="stable")
    k5, n5 = cat("q5", 0, kdt), cat("q5", 1, np.int32)
    o5 = np.argsort(k5, kind="stable")
    q3 = dict(keys=k3[o3], date=d3[o3], prio=p3[o3])
    q5 = dict(keys=k5[o5], nation=n5[o5])
    for t in (q3, q5):
        assert np.all(t["keys"][1:] > t["keys"][:-1]), "order keys are unique"
    return q3, q5


# ---- lineitem pass -------------------------------------------------------------------------------------------------------

def _fold_lineitem(a, q3o, q5o, supp, s_nation):
    qty, ext, disc, tax, ship = a["l_quantity"], a["l_extendedprice"], a["l_discount"], a["l_tax"], a["l_shipdate"]
    disc_price = ext * (1.0 - disc)
    charge = disc_price * (1.0 + tax)
    out = {}

    # Q1: where l_shipdate <= date '1998-09-02' group by l_returnflag, l_linestatus (one byte each in this generator)
    keep = ship <= Q1_SHIPDATE_MAX
    code = a["l_returnflag.data"].astype(np.uint16) | (a["l_linestatus.data"].astype(np.uint16) << 8)
    q1 = {}
    for g in np.flatnonzero(np.bincount(code[keep], minlength=1)):
        m = keep & (code == g)
        q1[(chr(int(g) & 0xFF), chr(int(g) >> 8))] = (int(np.count_nonzero(m)),
                                                      [_sum(x[m]) for x in (qty, ext, disc_price, charge, disc)])
    out["q1"] = q1

    # Q6
    m = ((ship >= Q6_DATE_LO) & (ship < Q6_DATE_HI) & (disc >= Q6_DISC_LO) & (disc <= Q6_DISC_HI) & (qty < Q6_QTY_MAX))
    out["q6"] = (int(np.count_nonzero(m)), _sum((ext * disc)[m]))

    # Q3: l_orderkey = o_orderkey and l_shipdate > date '1995-03-15'; the matched rows are kept, summed at the end
    sel = np.flatnonzero(ship > Q3_DATE)
    pos, found = _sorted_find(q3o["keys"], a["l_orderkey"][sel])
    out["q3"] = (pos[found], disc_price[sel[found]])

    # Q5: l_orderkey = o_orderkey and l_suppkey = s_suppkey and c_nationkey = s_nationkey
    pos, found = _sorted_find(q5o["keys"], a["l_orderkey"])
    rows = np.flatnonzero(found)
    nat = q5o["nation"][pos[rows]]
    srow, sfound = supp.find(a["l_suppkey"][rows])
    ok = sfound & (s_nation[srow] == nat)
    rows, nat = rows[ok], nat[ok]
    rev = disc_price[rows]
    cnt = np.bincount(nat, minlength=len(NATIONS))
    out["q5"] = (cnt, [_sum(rev[nat == i]) if cnt[i] else _ACC(0) for i in range(len(NATIONS))])
    return out


def _finish_q1(parts):
    groups = sorted({k for p in parts for k in p["q1"]})
    out = OrderedDict()
    for k in groups:
        cnt = sum(p["q1"][k][0] for p in parts if k in p["q1"])
        s = [_total([p["q1"][k][1][i] for p in parts if k in p["q1"]]) for i in range(5)]
        out[k] = dict(count_order=cnt, sum_qty=s[0], sum_base_price=s[1], sum_disc_price=s[2], sum_charge=s[3],
                      avg_qty=s[0] / cnt, avg_price=s[1] / cnt, avg_disc=s[4] / cnt)
    return out


def _finish_q3(parts, q3o):
    pos = np.concatenate([p["q3"][0] for p in parts]) if parts else np.zeros(0, np.int64)
    rev = np.concatenate([p["q3"][1] for p in parts]) if parts else np.zeros(0, np.float64)
    order = np.argsort(pos, kind="stable")
    pos, rev = pos[order], rev[order]
    n_joined = len(pos)
    if n_joined == 0:
        z = np.zeros(0, np.int64)
        return dict(keys=q3o["keys"][z], date=q3o["date"][z], prio=q3o["prio"][z], revenue=np.zeros(0, _ACC), rows_in_group=z,
                    n_joined=0, n_max=0, revenue_exact=True, order=z)
    starts = np.flatnonzero(np.r_[True, pos[1:] != pos[:-1]])
    counts = np.diff(np.r_[starts, n_joined])
    if EXTENDED:
        total = np.add.reduceat(rev.astype(np.longdouble), starts)          # sequential longdouble additions within a group
        # exactness: addends are multiples of 2^(e_min - 52); a total below 2^(e_min + 12) needs at most 64 significand bits
        e_min = math.frexp(float(rev.min()))[1] - 1
        exact = bool(rev.min() > 0 and float(total.max()) < 2.0 ** (e_min + 12))
    else:
        ends = np.r_[starts[1:], n_joined]
        total = np.array([math.fsum(rev[s:e]) for s, e in zip(starts, ends)], np.float64)
        exact = False
    g = pos[starts]
    date = q3o["date"][g]
    # ORDER BY revenue DESC, o_orderdate (on the Float64 the query reports); the order key breaks exact ties for a total order
    order = np.lexsort((q3o["keys"][g], date, -total.astype(np.float64)))
    return dict(keys=q3o["keys"][g], date=date, prio=q3o["prio"][g], revenue=total, rows_in_group=counts,
                n_joined=int(n_joined), n_max=int(counts.max()), revenue_exact=exact, order=order)


def _finish_q5(parts):
    cnt = np.zeros(len(NATIONS), np.int64)
    for p in parts:
        cnt += p["q5"][0]
    rev = [_total([p["q5"][1][i] for p in parts]) for i in range(len(NATIONS))]
    present = [i for i in range(len(NATIONS)) if cnt[i]]
    present.sort(key=lambda i: (-rev[i], NATIONS[i][0]))                     # ORDER BY revenue DESC
    return dict(rows=[(NATIONS[i][0], rev[i], int(cnt[i])) for i in present], revenue_by_nationkey=rev,
                count_by_nationkey=[int(c) for c in cnt])


def reference(sf, rows=None, orders=None, key64=False, dims=None, chunk_rows=CHUNK_ROWS, threads=None, queries=("q1", "q6", "q3", "q5")):
    """Q1 / Q6 / Q3 / Q5 over lineitem rows [0, rows) and orders rows [0, orders) of the seeded tables at scale factor sf
    (defaults: the scale factor's cardinalities), small tables `dims` (needed for q3 / q5; without "q3" / "q5" in `queries` the
    orders pass is skipped and only q1 / q6 are returned).  chunk_rows None or 0: one chunk.
    `rows` may be a list of row counts: the table is read ONCE, chunk boundaries are placed at every one of them, and the result is
    {rows: result} for each prefix [0, rows) (the chunk partials up to that boundary).

    -> dict(q1={(flag, status): dict(count_order, sum_qty, sum_base_price, sum_disc_price, sum_charge, avg_qty, avg_price, avg_disc)}
            in ORDER BY flag, status order,
            q6=dict(revenue, selected),
            q3=dict(keys, date, prio, revenue, rows_in_group: arrays over the groups in ascending key order; order: the permutation
                    that puts them in ORDER BY revenue DESC, o_orderdate order; n_joined, n_max, revenue_exact),
            q5=dict(rows=[(n_name, revenue, joined rows)] in ORDER BY revenue DESC order, revenue_by_nationkey[25], count_by_nationkey[25]),
            n_chunks, sum_rel_error, rows, orders)
    Sums are np.longdouble when EXTENDED, else Float64."""
    card = gen.cardinalities(sf)
    many = isinstance(rows, (list, tuple))
    prefixes = sorted({int(r) for r in rows}) if many else [card["lineitem"] if rows is None else int(rows)]
    n_orders = card["orders"] if orders is None else int(orders)
    threads = n_threads() if threads is None else threads
    joins = "q3" in queries or "q5" in queries
    empty = dict(keys=np.zeros(0, np.int64 if key64 else np.int32), date=np.zeros(0, np.int32), prio=np.zeros(0, np.int32),
                 nation=np.zeros(0, np.int32))
    q3o, q5o, supp, s_nation = empty, empty, _Lookup(np.zeros(0, np.int32)), np.zeros(0, np.int32)
    if joins:
        if dims is None:
            raise ValueError("q3 / q5 need the small tables: dims=ballista_amd.tpch.dimension_arrays(sf)")
        q3o, q5o = _orders_pass(sf, n_orders, key64, dims, chunk_rows, threads)
        supp, s_nation = _Lookup(dims["supplier"]["s_suppkey"]), np.asarray(dims["supplier"]["s_nationkey"])
    chunks, lo = [], 0
    for r in prefixes:                                   # every prefix ends on a chunk boundary
        chunks += [(lo + a, n) for a, n in _chunks(r - lo, chunk_rows)]
        lo = r
    parts = _map_chunks(chunks, lambda lo, n: gen.lineitem_arrays(sf, lo, n, key64=key64),
                        lambda a: _fold_lineitem(a, q3o, q5o, supp, s_nation), threads)
    results = {}
    for r in prefixes:
        mine = [p for (lo, n), p in zip(chunks, parts) if lo + n <= r]
        out = dict(n_chunks=len(mine), sum_rel_error=SUM_REL_ERROR(len(mine)), rows=r, orders=n_orders)
        out["q1"] = _finish_q1(mine)
        out["q6"] = dict(revenue=_total([p["q6"][1] for p in mine]), selected=sum(p["q6"][0] for p in mine))
        if joins:
            out["q3"] = _finish_q3(mine, q3o)
            out["q3"]["n_orders_surviving"] = len(q3o["keys"])
            out["q5"] = _finish_q5(mine)
        results[r] = out
    return results if many else results[prefixes[0]]
