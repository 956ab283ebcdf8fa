"""distinct_agg_cases.py is what it says (no GPU): every case holds the values and the row counts it claims, and every mistake the
cases are built against — a NULL counted as a value, -0.0 merged with +0.0, NaN payloads merged, "" merged with NULL, a prefix
taken for an equal string, x compared without the group key — changes a number that test_distinct_agg_gpu.py compares."""
import struct

import numpy as np
import pytest

from oracle import engine as og

import distinct_agg_cases as D
import join_route_cases as RC
import wide_agg_cases as W


def counts(case, mistake=None):
    e = D.expected(case, mistake)
    return e["cd"].to_pylist()


def test_ballot_cases_straddle_every_word_and_block_edge():
    for n in D.BALLOT_SIZES:
        for variant in D.BALLOT_VARIANTS:
            c = D.ballot_case(n, variant)
            t = c.table
            assert og.batch_len(t) == n == c.facts["rows"]
            k, x, ok = t["k"].values, t["x"].values, t["x"].is_valid()
            for a, b in c.facts["straddling"]:
                if b == n - 1:
                    continue                                # (the last row is the variant's)
                assert a % 64 == 63 and b % 64 == 0 and (k[a], x[a], ok[a]) == (k[b], x[b], ok[b])
            _, _, first = D.first_rows(t, ["k"], "x")
            assert bool(first[n - 1]) == c.facts["last_is_first"]
    assert {e for n in D.BALLOT_SIZES for e in (n - 1, n, n + 1)} >= {63, 64, 65, 127, 128, 129, 255, 256, 257}
    # a pair of NULLs across an edge as well: two zero bits that a NULL counted as a value would set
    t = D.ballot_case(257, "last_is_first").table
    assert any(not t["x"].is_valid()[e - 1] and not t["x"].is_valid()[e] for e in range(64, 257, 64)) or \
        any(not t["x"].is_valid()[r] for r in range(257))


def test_table_cases_sit_on_both_sides_of_the_capacity_step():
    assert RC.TABLE_CAPACITY_SOURCE in W.source_text("host/core.hpp")
    assert [RC.table_capacity(n) for n in D.TABLE_SIZES] == [1024, 2048]
    for n in D.TABLE_SIZES:
        for shape in D.TABLE_SHAPES:
            c = D.table_case(n, shape)
            assert og.batch_len(c.table) == n
            assert counts(c) == [c.facts["distinct"]]
            assert len(set(c.table["x"].values.tolist())) == c.facts["distinct"]


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_equality_values_are_one_step_apart():
    assert D.F64["one_ulp"] - D.F64["one"] == 1 and D.F32["one_ulp"] - D.F32["one"] == 1
    assert D.F64["neg_zero"] ^ D.F64["zero"] == 1 << 63 and D.F32["neg_zero"] ^ D.F32["zero"] == 1 << 31
    assert f64(D.F64["zero"]) == f64(D.F64["neg_zero"]) and f64(D.F64["one"]) == -f64(D.F64["neg_one"])
    for bits in (D.F64["nan_a"], D.F64["nan_b"]):
        assert f64(bits) != f64(bits) and bits >> 51 & 1                         # quiet NaNs
    for bits in (D.F32["nan_a"], D.F32["nan_b"]):
        v = np.array([bits], np.uint32).view(np.float32)[0]
        assert v != v and bits >> 22 & 1
        assert np.array([np.float64(v)]).view(np.uint64)[0] & ((1 << 51) - 1) == (bits & ((1 << 22) - 1)) << 29   # the payload survives widening
    u = D.EQUALITY_VALUES["Utf8"]
    assert "" in u and "ab".startswith("a") and len(D.LONG.encode()) == 40
    assert D.LONG[:-1] + "!" in u and D.LONG[:-1] != D.LONG and D.LONG.startswith(D.LONG[:-1])
    for dtype in ("Int32", "Int64", "Date32"):
        v = D.EQUALITY_VALUES[dtype]
        assert {0, 1, -1} <= set(v) and len(set(v)) == len(v)


@pytest.mark.parametrize("dtype", list(D.EQUALITY_VALUES))
def test_equality_cases_count_every_value_once(dtype):
    c = D.equality_case(dtype)
    assert og.batch_len(c.table) == c.facts["rows"]
    assert counts(c) == [c.facts["counts"][0], c.facts["counts"][1]]
    x = c.table["x"]
    assert (~x.is_valid()).sum() == 2
    # every value of the list is in group 0 twice
    ident = [i for i, k in zip(D.identities(x), c.table["k"].values) if k == 0 and i is not None]
    assert len(ident) == 2 * len(set(ident)) == 2 * len(D.EQUALITY_VALUES[dtype])


MISTAKE_CASES = {
    "null_is_a_value": [lambda: D.equality_case("Int64"), lambda: D.null_case("some"), lambda: D.null_case("all"), lambda: D.ballot_case(257, "last_is_first")],
    "zeros_merged": [lambda: D.equality_case("Float64"), lambda: D.equality_case("Float32")],
    "nans_merged": [lambda: D.equality_case("Float64"), lambda: D.equality_case("Float32")],
    "empty_is_null": [lambda: D.equality_case("Utf8")],
    "prefix_is_equal": [lambda: D.equality_case("Utf8")],
    "group_key_ignored": [lambda: D.group_key_case("packed"), lambda: D.group_key_case("wide"), lambda: D.mixed_case()],
}


@pytest.mark.parametrize("mistake", D.MISTAKES)
def test_every_mistake_changes_an_expected_number(mistake):
    assert set(MISTAKE_CASES) == set(D.MISTAKES)
    for make in MISTAKE_CASES[mistake]:
        c = make()
        names = [a.name for a in c.aggs if a.fun in D.DISTINCT_FUNS]
        assert D.numbers(D.expected(c), names) != D.numbers(D.expected(c, mistake), names), c.name


def test_group_key_cases():
    for route in ("packed", "wide"):
        c = D.group_key_case(route)
        e = D.expected(c)
        keyed = dict(zip([None if v is None else int(str(v)[-1]) for v in e["k"].to_pylist()], e["cd"].to_pylist()))
        assert keyed == c.facts["counts"]
        assert og.batch_len(c.table) == c.facts["rows"]
    wide = D.group_key_case("wide").table["k"]
    assert all(len(s.encode()) > 16 for s, ok in zip(wide.values, wide.is_valid()) if ok)      # no 16-byte packed key holds one
    # 7 stands in every group
    t = D.group_key_case("packed").table
    assert {g for g, x in zip(t["k"].to_pylist(), t["x"].to_pylist()) if x == 7} == {0, 1, 2, None}


def test_null_cases():
    e = D.expected(D.null_case("some"))
    assert e["cd"].to_pylist() == [0, 1, 1] and e["sd"].to_pylist() == [None, 5, 6] and e["ad"].to_pylist() == [None, 5.0, 6.0]
    e = D.expected(D.null_case("all"))
    assert e["cd"].to_pylist() == [0, 0, 0] and e["sd"].to_pylist() == [None] * 3
    assert og.batch_len(D.null_case("all").table) == 150 > 128


def test_mixed_and_no_group_cases():
    c = D.mixed_case()
    assert len({a.expr.name for a in c.aggs if a.fun in D.DISTINCT_FUNS}) == c.facts["distinct_args"] == 2
    e = D.expected(c)
    assert len(set(e["sd_a"].to_pylist())) > 1
    e = D.expected(D.no_group_case(0))
    assert (e["cd"].to_pylist(), e["sd"].to_pylist(), e["ad"].to_pylist()) == ([0], [None], [None])
    e = D.expected(D.no_group_case(100))
    assert e["cd"].to_pylist() == [17] and e["sd"].to_pylist() == [sum(range(17))] and e["ad"].to_pylist() == [8.0]


def test_grid_case_takes_a_second_trip():
    assert D.GRID_ROWS > D.GRID_LIMIT == 1_048_576
    src = W.source_text("kernels_hash.hip")
    assert "const size_t cap = (size_t)cfg.device_cus * 16;" in src              # grid_rows: at most 16 blocks per CU
    e = D.grid_expected()
    assert og.batch_len(e) == 1000 and int(e["cd"].values.min()) > 500 and int(e["cd"].values.max()) < 5000


def test_float_sum_case_depends_on_the_order():
    c = D.float_sum_case()
    assert og.batch_len(c.table) == D.FLOAT_ROWS and c.facts["min_reps"] >= 2 and c.facts["max_reps"] <= 5
    x, k = c.table["x"].values, c.table["k"].values
    vals, reps = np.unique(x, return_counts=True)
    assert reps.min() >= 2 and reps.max() <= 5
    # the set sum of a group in two orders: not the same double, in some group
    differs = []
    for grp in range(8):
        g = np.unique(x[k == grp])
        fwd = bwd = 0.0
        for v in g:
            fwd += v
        for v in g[::-1]:
            bwd += v
        assert abs(fwd - bwd) <= 1e-9 * fwd
        differs.append(fwd != bwd)
    assert any(differs)
    # equal values are scattered: some value's occurrences lie in different 64-row words
    rows = np.nonzero(x == vals[5])[0]
    assert len({int(r) // 64 for r in rows}) > 1


def test_property_table_has_nulls_everywhere():
    t = D.property_table()
    assert og.batch_len(t) == D.PROPERTY_ROWS
    for name, c in t.items():
        assert 0 < (~c.is_valid()).sum() < D.PROPERTY_ROWS // 2, name
