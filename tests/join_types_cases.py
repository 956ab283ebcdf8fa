"""TEST INFRASTRUCTURE shared by test_join_types_plan.py (CPU) and test_join_types_gpu.py: the inputs of the join-type tests and the
EXPECTED rows of Full / Semi / Anti / RightSemi / RightAnti.

The CPU oracle (oracle/engine.py hash_join) knows Inner, Left and Right.  The five other types are derived from those three results
over the same sides, by the row ids every row carries (li on the build side, ri on the probe side):

  Semi       the build rows whose li occurs in Inner           Anti        the other build rows
  RightSemi  the probe rows whose ri occurs in Inner           RightAnti   the other probe rows
  Full       Left's rows, plus Right's rows whose li is NULL

test_join_types_plan.py checks this derivation against pyarrow's joins on every input below, so it has a witness that is neither
the oracle's join nor the product's."""
import functools
from collections import OrderedDict

import numpy as np

from oracle import engine as og
from oracle.engine import OCol

FULL, SEMI, ANTI, RIGHT_SEMI, RIGHT_ANTI = "Full", "Semi", "Anti", "RightSemi", "RightAnti"
TYPES = [FULL, SEMI, ANTI, RIGHT_SEMI, RIGHT_ANTI]
WIRE = {FULL: 3, SEMI: 4, ANTI: 5}                     # RightSemi / RightAnti have no wire value
PYARROW = {FULL: "full outer", SEMI: "left semi", ANTI: "left anti", RIGHT_SEMI: "right semi", RIGHT_ANTI: "right anti"}
NL, NR = 900, 5000
CUTS = [0, 1025, 3000, NR]                             # probe batches of 1025 (one past the 1024-row selection tile), 1975 and 2000 rows
FORMS = ["int64_unique", "int64_dup", "hot_key", "int32_date32", "utf8_short", "utf8_long"]


def with_ids(prefix, n, cols):
    return OrderedDict(list(cols) + [(prefix + "i", OCol("Int64", np.arange(n, dtype=np.int64)))])


@functools.lru_cache(maxsize=None)
def sides(form, nulls, seed=3, nl=NL, nr=NR):
    """-> (left, right, on): nl build rows (lk.., lx, li) and nr probe rows (rk.., ry, ri); nulls: about 10 % NULL keys on both sides.
    One object per argument list: the tests share the sides and never modify them"""
    rng = np.random.default_rng(seed + 17 * FORMS.index(form))
    lv = (rng.random(nl) > 0.1) if nulls else None
    rv = (rng.random(nr) > 0.1) if nulls else None
    on = [("lk", "rk")]
    if form == "int64_unique":                          # 900 distinct keys; about two thirds of the probe rows find one
        lk = [("lk", OCol("Int64", rng.permutation(3 * nl)[:nl].astype(np.int64) * 10 ** 10 - 5, lv))]
        rk = [("rk", OCol("Int64", rng.integers(0, 3 * nl, nr).astype(np.int64) * 10 ** 10 - 5, rv))]
    elif form == "int64_dup":                           # 300 distinct values over the build rows; the probe rows know two thirds of them
        d = max(1, nl // 3)
        lk = [("lk", OCol("Int64", rng.integers(0, d, nl).astype(np.int64) * 10 ** 10 - 7, lv))]
        rk = [("rk", OCol("Int64", rng.integers(d // 3, d + d // 3 + 1, nr).astype(np.int64) * 10 ** 10 - 7, rv))]
    elif form == "hot_key":                             # one value on half of the build rows and on about half of the probe rows
        lkv = np.where(np.arange(nl) % 2 == 0, 42, 1000 + np.arange(nl) // 4)
        rkv = np.where(rng.random(nr) < 0.5, 42, 1000 + rng.integers(nl // 8, nl // 2, nr))
        lk = [("lk", OCol("Int64", lkv.astype(np.int64), lv))]
        rk = [("rk", OCol("Int64", rkv.astype(np.int64), rv))]
    elif form == "int32_date32":                        # a pair; NULLs in the second part only
        on = [("lk", "rk"), ("ld", "rd")]
        lk = [("lk", OCol("Int32", rng.integers(-20, 20, nl).astype(np.int32))), ("ld", OCol("Date32", rng.integers(9000, 9020, nl).astype(np.int32), lv))]
        rk = [("rk", OCol("Int32", rng.integers(-25, 25, nr).astype(np.int32))), ("rd", OCol("Date32", rng.integers(8995, 9025, nr).astype(np.int32), rv))]
    else:
        if form == "utf8_short":                        # 0 .. 15 bytes: the packed key holds them
            pool = ["", "a", "ABCDEFGHIJKLMNO", "ABCDEFGHIJKLMN"] + ["s%d" % i + "-" * (i % 9) for i in range(400)]
        else:                                           # 16 .. 300 bytes: the wide table
            pool = ["Q" * 16, "Q" * 15 + "R", "Q" * 17, "z" * 300, "z" * 299 + "A"] + ["a-long-join-key-%04d" % i + "f" * (i % 40) for i in range(400)]
        assert len(set(pool)) == len(pool)
        lkl = [pool[int(i)] for i in rng.integers(0, 300, nl)]
        rkl = [pool[int(i)] for i in rng.integers(100, len(pool), nr)]
        rkl[2:7] = pool[:5]                              # the special values find their partners
        if nulls and form == "utf8_short" and nl > 1 and nr > 1026:            # "" next to NULL, on both sides
            lkl[0], lkl[1], lv[0], lv[1] = "", "", True, False
            rkl[0], rkl[1], rkl[1026], rv[0], rv[1], rv[1026] = "", "", "", True, False, True
        lk, rk = [("lk", OCol("Utf8", lkl, lv))], [("rk", OCol("Utf8", rkl, rv))]
    left = with_ids("l", nl, lk + [("lx", OCol("Float64", rng.integers(0, 1000, nl) / 8.0))])
    right = with_ids("r", nr, rk + [("ry", OCol("Int64", rng.integers(0, 10 ** 6, nr)))])
    return left, right, on


def rows_where(batch, keep):
    return OrderedDict((k, c.take(np.nonzero(keep)[0])) for k, c in batch.items())


_ORACLE = {}


def oracle_join(left, right, on, jt):
    """the oracle's Inner / Left / Right join of these sides, computed once per pair of sides (they are never modified)"""
    key = (id(left), id(right), tuple(on), jt)
    if key not in _ORACLE:
        _ORACLE[key] = (left, right, og.hash_join(left, right, on, jt))          # (the sides are kept so that their ids stay theirs)
    return _ORACLE[key][2]


def expected(jt, left, right, on):
    """the rows of HashJoinExec(left, right, on, jt) for the five types the oracle does not join itself"""
    if jt == FULL:
        lj, rj = oracle_join(left, right, on, "Left"), oracle_join(left, right, on, "Right")
        return og.concat_batches([lj, rows_where(rj, ~rj["li"].is_valid())])
    side, ids = (left, "li") if jt in (SEMI, ANTI) else (right, "ri")
    has_partner = np.isin(side[ids].values, oracle_join(left, right, on, "Inner")[ids].values)
    return rows_where(side, has_partner if jt in (SEMI, RIGHT_SEMI) else ~has_partner)


def assert_same_rows(got, want, ids=("li", "ri")):
    """two batches hold the same rows, as multisets keyed by the row ids (an output row of any join type is identified by its
    (li, ri), NULL where a side has no row in it); every column compares exactly.  In numpy: a hot key makes a million rows"""
    if not got or not want:                              # a stream may end without yielding a batch: zero rows
        assert og.batch_len(got) == 0 and og.batch_len(want) == 0, (og.batch_len(got), og.batch_len(want))
        return
    assert list(got.keys()) == list(want.keys()), (list(got.keys()), list(want.keys()))
    n = og.batch_len(want)
    assert og.batch_len(got) == n, "row count %d != %d" % (og.batch_len(got), n)
    ids = [k for k in ids if k in want]

    def order(b):
        return np.lexsort([np.where(b[k].is_valid(), b[k].values, -1) for k in reversed(ids)])
    og_, ow = order(got), order(want)
    for k in want:
        g, w = got[k].take(og_), want[k].take(ow)
        assert g.dtype == w.dtype, (k, g.dtype, w.dtype)
        assert np.array_equal(g.is_valid(), w.is_valid()), "column %s: NULLs differ" % k
        ok = w.is_valid()
        same = g.values[ok] == w.values[ok]
        assert bool(np.all(same)), "column %s: %d values differ, first at sorted row %d" % (k, int((~same).sum()), int(np.nonzero(ok)[0][np.argmin(same)]))
    if ids and n:                                        # the key is a key: no two rows share their ids
        keys = np.stack([np.where(want[k].is_valid(), want[k].values, -1) for k in ids])
        assert len(np.unique(keys, axis=1).T) == n
