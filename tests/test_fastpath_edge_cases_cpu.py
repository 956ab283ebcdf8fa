"""The tables of fastpath_edge_cases.py, checked without a device: test_fastpath_edges_gpu.py compares every device route with the
oracle over these inputs, so here the oracle's answers over them are pinned against a third statement of the same semantics —
one comparison per row over Python floats and ints — and the tables are shown to hold the rows they claim: the literal, both of
its neighbours, every NaN pattern, NULLs over values that would pass, and for the chain cases the condition under which a SUM is
exact in any order of addition."""
import math

import numpy as np
import pytest

from oracle import engine as og

import fastpath_edge_cases as FC
from fastpath_edge_cases import DBL_MAX, DBL_MIN, INF, INT32_MAX, INT32_MIN

N_F64 = 5 * 1024 + 300
N_I32 = 64 * 8 + 65
N_CONJ = 3 * 1024 + 17
CHAIN_SIZES = [1, 513, 2 * 1024 + 513]


def oracle_ids(batch, predicate):
    return og.filter_batch(batch, predicate)["id"].values.tolist()


def has_bits(c, v):
    return bool((np.ascontiguousarray(c.values).view(np.uint64) == np.uint64(FC.bits_of(v))).any())


# ---- one comparison -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", FC.F64_LITERALS, ids=repr)
def test_float_predicates_row_by_row(L):
    schema = FC.PRED_SCHEMA["Float64"]
    b = FC.float_pred_batch(L, N_F64, shift=FC.F64_LITERALS.index(L))
    kept = set()
    for term in FC.single_terms(L):
        want = FC.kept_rows(b, [term])
        p = FC.term_expr(term, schema)
        assert oracle_ids(b, p) == want, term
        assert oracle_ids(b, FC.twice(p)) == want, term
        kept.add(len(want))
        # where the fold takes the term, its closed range keeps the same rows: the statement host/sop.cpp relies on
        r = FC.fold([term], schema)
        if r is not None:
            lo, hi = r["x"]
            assert [i for i, v in enumerate(b["x"].values.tolist()) if lo <= v <= hi] == want, term
        else:
            assert want == [], term
    assert len(kept) > 2                                    # the operators differ on these rows
    if L in (INF, -INF):
        assert FC.fold([("x", "Gt" if L > 0 else "Lt", L, False)], schema) is None
        assert FC.fold([("x", "Lt" if L > 0 else "Gt", L, True)], schema) is None
        assert FC.fold([("x", "GtEq" if L > 0 else "LtEq", L, False)], schema) is not None


@pytest.mark.parametrize("L", FC.F64_LITERALS, ids=repr)
@pytest.mark.parametrize("n", [N_F64, 1024, 1])
def test_float_tables_hold_what_they_claim(L, n):
    b = FC.float_pred_batch(L, n)
    x = b["x"]
    assert len(x) == n and x.values.view(np.uint64)[0] == FC.bits_of(L)             # shift 0: the literal itself at row 0
    if n == 1:
        return
    for v in (L, FC.next_up(L), FC.next_down(L), -L, 0.0, -0.0, 5e-324, -5e-324, INF, -INF):
        assert has_bits(x, v), v
    for bits in FC.NAN_BITS:
        assert (x.values.view(np.uint64) == np.uint64(bits)).any(), hex(bits)
    special = set(FC.float_specials(L).tolist())
    assert all(int(x.values.view(np.uint64)[r]) in special for r in FC.boundary_rows(n))
    assert sum(int(v) not in special for v in x.values.view(np.uint64)) > n // 4     # and ordinary values


def test_a_nan_literal_keeps_nothing_and_is_not_folded():
    schema = FC.PRED_SCHEMA["Float64"]
    b = FC.float_pred_batch(1.0, N_F64)
    for term in FC.single_terms(math.nan):
        assert FC.fold([term], schema) is None
        assert oracle_ids(b, FC.term_expr(term, schema)) == [] == FC.kept_rows(b, [term])


@pytest.mark.parametrize("dtype", ["Int32", "Date32"])
@pytest.mark.parametrize("L", FC.I32_LITERALS)
def test_int_predicates_row_by_row(dtype, L):
    schema = FC.PRED_SCHEMA[dtype]
    for nulls in (False, True):
        b = FC.int_pred_batch(dtype, L, N_I32, shift=FC.I32_LITERALS.index(L), nulls=nulls)
        vals = b["x"].to_pylist()
        assert L in vals and (L == INT32_MIN or L - 1 in vals) and (L == INT32_MAX or L + 1 in vals)
        assert INT32_MIN in vals and INT32_MAX in vals and (not nulls or None in vals)
        for term in FC.single_terms(L):
            want = FC.kept_rows(b, [term])
            p = FC.term_expr(term, schema)
            assert oracle_ids(b, p) == want, term
            assert oracle_ids(b, FC.twice(p)) == want, term
            lo, hi = FC.fold([term], schema)["x"]           # never declined: INT32_MAX + 1 is a double like any other
            assert [i for i, v in enumerate(vals) if v is not None and lo <= v <= hi] == want, term


# ---- conjunctions ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nulls", ["none", "one", "all"])
@pytest.mark.parametrize("case", list(FC.CONJ_CASES))
def test_conjunctions_row_by_row(case, nulls):
    terms = FC.CONJ_CASES[case]
    b = FC.conj_batch(N_CONJ, nulls)
    want = FC.kept_rows(b, terms)
    p = FC.conj_expr(terms, FC.CONJ_SCHEMA)
    assert oracle_ids(b, p) == want
    assert oracle_ids(b, FC.twice(p)) == want
    ranges = FC.fold(terms, FC.CONJ_SCHEMA)
    if case in FC.CONJ_EMPTY:
        assert want == [] and ranges is None
        return
    assert 20 < len(want) < N_CONJ - 20
    assert (ranges is None) == (case == "five_columns")
    if ranges is not None:
        cols = {k: b[k].to_pylist() for k in ranges}
        assert [i for i in range(N_CONJ) if all(cols[k][i] is not None and lo <= cols[k][i] <= hi for k, (lo, hi) in ranges.items())] == want
    touched = {t[0] for t in terms}
    if nulls == "all" or (nulls == "one" and "a" in touched):
        assert len(FC.null_rows_that_would_pass(b, terms)) > 5          # NULLs over values that would pass


# ---- chains ---------------------------------------------------------------------------------------------------------------------

def test_the_designated_operands_are_the_edges_they_are_named_for():
    prod = {a: [f(dict(zip("xyzqi", h))) for h in FC.HOT] for a, (_, f) in FC.CHAINS.items()}
    assert 1.0 - FC.HOT[0][1] == 2.0 ** -53 and prod["x_1my"][0] == 3.0 * 2.0 ** -53
    assert prod["x_1my"][1] == INF and prod["x_1my"][5] == -INF and prod["q"][1] == DBL_MAX
    assert prod["xy"][2] == 0.0 and 5e-324 * 0.5 == 0.0
    # DBL_MIN * (1 - 2^-53) lies halfway between the largest subnormal and DBL_MIN and rounds back to even; DBL_MIN * -0.5 is a
    # subnormal; DBL_MIN * 2^-53 is half the smallest subnormal and rounds to zero
    assert prod["xy"][3] == DBL_MIN and prod["xz"][3] == -DBL_MIN / 2 and 0.0 < -prod["xz"][3] < DBL_MIN
    assert prod["x_1my"][3] == 0.0 and DBL_MIN * 2.0 ** -53 == 0.0
    assert math.isnan(prod["xy"][4]) and prod["x_1my"][4] == INF
    assert all(math.isnan(prod[a][6]) for a in prod if a not in ("y", "z", "q"))
    assert math.isnan(prod["1pz_1my_x"][7]) and prod["casti_x"][7] == INF
    assert prod["zero_minus_x"][8] == -1234.5 and prod["x_3"][8] == 3703.5


def oracle_aggregate(batches, term, case, key_cols):
    group = [(FC.col(k), k) for k in key_cols]
    aggs = FC.chain_aggs(case)
    p = FC.term_expr(term, FC.CHAIN_SCHEMA)
    partials = [og.hash_aggregate(og.filter_batch(b, p), "Partial", group, aggs) for b in batches]
    return og.hash_aggregate(og.concat_batches(partials), "Final", group, aggs)


CHAIN_TERMS = [("p", "LtEq", 0.1, False), ("p", "Gt", -0.0, False), ("p", "Lt", 5e-324, True), ("p", "GtEq", -INF, False),
               ("p", "Eq", DBL_MAX, False), ("p", "Gt", INF, False), ("d", "LtEq", 10471, False), ("d", "Gt", INT32_MAX - 1, False)]


@pytest.mark.parametrize("n", CHAIN_SIZES)
@pytest.mark.parametrize("case", list(FC.CHAIN_CASES))
def test_chain_cases_are_exact_in_any_order_of_addition(case, n):
    aliases = FC.CHAIN_CASES[case][0]
    for k, term in enumerate(CHAIN_TERMS):
        for grouped, keys in [((True, ["ki"]), (True, ["ks", "kt"]), (False, []))[(k + n) % 3]]:
            batches = FC.chain_batches(n, term, case, grouped, operand_set=k)
            assert sum(len(b["x"]) for b in batches) == n and (len(batches) == 2) == (n == 2 * 1024 + 513)
            expected, open_sign = FC.chain_expected(batches, term, case, keys)      # asserts the exactness condition
            got = oracle_aggregate(batches, term, case, keys)
            rows = {tuple(r[:len(keys)]): r[len(keys):] for r in zip(*[c.to_pylist() for c in got.values()])}
            if not keys and not expected:
                assert rows == {(): tuple([None] * len(aliases) + [0])}              # SUM = NULL, COUNT = 0
                continue
            assert set(rows) == set(expected), (term, keys)
            for key, (count, sums) in expected.items():
                assert rows[key][-1] == count
                for a, s, g in zip(aliases, sums, rows[key]):
                    same = (s != s and g != g) or (s == g and (s != 0.0 or "s_" + a in open_sign or math.copysign(1, s) == math.copysign(1, g)))
                    assert same, (term, key, a, s, g)
            if term[1:3] == ("Gt", INF):
                assert not expected
            elif grouped and n >= 511:
                assert len(expected) == 3
                # the key of the dead-only group is in the input and in no result
                assert any(set(zip(*[b[k].to_pylist() for k in keys])) - set(expected) for b in batches)
