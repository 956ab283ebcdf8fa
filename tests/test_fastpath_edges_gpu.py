"""GPU parity of the five routes that consume host/sop.cpp's plan table, at the values where its re-derivation of the expression
semantics can break: predicates with rows AT the bound (the literal, its neighbouring doubles, +-0.0, subnormals, +-inf, NaN of
three bit patterns; Int32 / Date32 at the literal +- 1 and the type's extremes), conjunctions that intersect, repeat, come out
empty or span up to five columns, with NULLs over values that would pass, and SUM chains whose operands cancel, overflow,
underflow through the subnormals, or are inf * 0 and NaN.

    filter      range_bitmap32_kernel (one Int32 / Date32 range), range_bitmap_kernel<1> (one other range: packs of four tiles,
                leftover tiles, ragged tail), range_bitmap_kernel<4> (2-4 ranges)                       -> "range_bitmap"
    aggregate   lean_kernel.h (generic), lean_spec_kernel.h (lean_spec_q1, lean_spec_key1)            -> "scan_agg_lean_kernel"
                sop_kernel.h                                                                            -> "scan_agg_sop_kernel"
    and, for the same rows, the expression VM ("scan_pred_bitmap", "scan_agg_lowcard_*") and the hash table ("scan_agg_hash")

Inputs and the reasons they give exact answers: fastpath_edge_cases.py (checked on the CPU by test_fastpath_edge_cases_cpu.py).
Every case is compared with the CPU oracle with NO float tolerance — kept rows and their order exactly; group keys, counts and
every SUM bit for bit, the sign of an exactly-zero SUM excepted — and asserts from Context.kernel_stats() at BHIP_KERNEL_TIMING=2
that the route it was written for ran.  Every predicate also runs as `p OR p`: the same truth table, which build_sop does not
fold, so the VM is held to the same rows.  Under an A/B switch of tools/README.md only the answers are checked."""
import os

import pytest

import ballista_amd as ba
from ballista_amd.expr import col
from oracle import plan_eval

import fastpath_edge_cases as FC
import helpers
from fastpath_edge_cases import DBL_MAX, INF, INT32_MAX, INT32_MIN

pytestmark = pytest.mark.gpu

SWITCHES = ("BHIP_NO_SOP", "BHIP_NO_LEAN", "BHIP_NO_RANGE_FILTER", "BHIP_LEAN_GENERIC", "BHIP_NO_FIXED_UTF8")
SWITCHED = any(os.environ.get(v, "0") not in ("", "0") for v in SWITCHES)
N_F64 = 5 * 1024 + 300            # one pack of four tiles, one leftover full tile, a ragged tail
N_I32 = 64 * 8 + 65               # one full pass of a wave, a second one that ends inside its second word
N_CONJ = 3 * 1024 + 17
AGG_SIZES = [1, 511, 513, 1023, 1025, 2 * 1024 + 513]


@pytest.fixture(scope="module")
def tctx():
    """a context that names every launch, however small (BHIP_KERNEL_TIMING is read when a context is created)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("BHIP_KERNEL_TIMING", "2")
    try:
        return ba.Context(0)
    finally:
        mp.undo()


def source(ctx, dev, host):
    """a fresh scan of batches that are on the device already (one partition)"""
    m = ba.MemoryExec([list(dev)], ctx)
    m._oracle_partitions = [list(host)]
    return m


# ---- filters ----------------------------------------------------------------------------------------------------------------------

def check_filter(ctx, dev, host, predicate, folded):
    """the rows FilterExec keeps, in order, against the oracle; then the launch that found them"""
    plan = ba.FilterExec(predicate, source(ctx, [dev], [host]))
    ctx.kernel_stats(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    ks = ctx.kernel_stats(reset=True)
    helpers.assert_rows_equal(got, plan_eval.collect(plan), ordered=True)
    if not SWITCHED:
        ran, other = ("range_bitmap", "scan_pred_bitmap") if folded else ("scan_pred_bitmap", "range_bitmap")
        assert ran in ks and other not in ks, (folded, sorted(ks))
    return got


def check_terms(ctx, dev, host, terms, schema, vm_too=True):
    p = FC.conj_expr(terms, schema)
    got = check_filter(ctx, dev, host, p, FC.fold(terms, schema) is not None)
    if vm_too:
        check_filter(ctx, dev, host, FC.twice(p), False)
    return got


@pytest.mark.parametrize("L", FC.F64_LITERALS, ids=repr)
def test_one_float64_range(tctx, L):
    """every operator, literal on either side, over a column holding L, its neighbours and the specials: range_bitmap_kernel<1>"""
    host = FC.float_pred_batch(L, N_F64, shift=FC.F64_LITERALS.index(L))
    dev = helpers.to_device(tctx, host)
    sizes = {len(helpers.rows_of(check_terms(tctx, dev, host, [t], FC.PRED_SCHEMA["Float64"]))) for t in FC.single_terms(L)}
    assert len(sizes) > 2


@pytest.mark.parametrize("L", [INF, -INF], ids=repr)
def test_a_strict_bound_at_infinity_keeps_nothing(tctx, L):
    """x > +inf and x < -inf hold for no row — not for the rows that ARE that infinity, which the neighbouring-double rule would
    keep (nextafter(inf, inf) is inf).  build_sop makes the range empty and the VM runs the predicate"""
    schema = FC.PRED_SCHEMA["Float64"]
    for n in (N_F64, 1024, 1):
        host = FC.float_pred_batch(L, n)
        assert host["x"].values[0] == L
        dev = helpers.to_device(tctx, host)
        for term in (("x", "Gt" if L > 0 else "Lt", L, False), ("x", "Lt" if L > 0 else "Gt", L, True)):
            assert FC.fold([term], schema) is None
            for p in (FC.term_expr(term, schema), FC.twice(FC.term_expr(term, schema))):
                got = check_filter(tctx, dev, host, p, False)
                assert len(helpers.rows_of(got)) == 0


def test_a_nan_literal_keeps_nothing(tctx):
    host = FC.float_pred_batch(1.0, N_F64)
    dev = helpers.to_device(tctx, host)
    for term in FC.single_terms(float("nan")):
        got = check_terms(tctx, dev, host, [term], FC.PRED_SCHEMA["Float64"])
        assert len(helpers.rows_of(got)) == 0


@pytest.mark.parametrize("dtype", ["Int32", "Date32"])
@pytest.mark.parametrize("L", FC.I32_LITERALS)
def test_one_int32_range(tctx, dtype, L):
    """range_bitmap32_kernel: integer bounds (INT32_MIN - 1 and INT32_MAX + 1 included: they match nothing), with and without NULLs"""
    for nulls in (False, True):
        host = FC.int_pred_batch(dtype, L, N_I32, shift=FC.I32_LITERALS.index(L), nulls=nulls)
        dev = helpers.to_device(tctx, host)
        for t in FC.single_terms(L):
            check_terms(tctx, dev, host, [t], FC.PRED_SCHEMA[dtype])


@pytest.mark.parametrize("n", [1, 1024])
def test_one_row_and_exactly_one_tile(tctx, n):
    for L in FC.F64_LITERALS:
        host = FC.float_pred_batch(L, n, shift=0 if n == 1 else FC.F64_LITERALS.index(L))
        dev = helpers.to_device(tctx, host)
        for t in FC.single_terms(L):
            check_terms(tctx, dev, host, [t], FC.PRED_SCHEMA["Float64"], vm_too=False)
    for dtype, L in (("Int32", INT32_MAX), ("Date32", INT32_MIN), ("Int32", 0)):
        host = FC.int_pred_batch(dtype, L, n)
        dev = helpers.to_device(tctx, host)
        for t in FC.single_terms(L):
            check_terms(tctx, dev, host, [t], FC.PRED_SCHEMA[dtype], vm_too=False)
    host = FC.conj_batch(n)
    dev = helpers.to_device(tctx, host)
    for case in ("intersection", "three_columns", "four_columns"):
        check_terms(tctx, dev, host, FC.CONJ_CASES[case], FC.CONJ_SCHEMA)


@pytest.mark.parametrize("nulls", ["none", "one", "all"])
def test_conjunctions(tctx, nulls):
    """one column twice (range_bitmap_kernel<1>, or the 32-bit kernel), two to four columns (range_bitmap_kernel<4>), empty
    intersections and five columns (the VM); NULLs in one range column, then in all of them"""
    host = FC.conj_batch(N_CONJ, nulls)
    dev = helpers.to_device(tctx, host)
    for case, terms in FC.CONJ_CASES.items():
        got = check_terms(tctx, dev, host, terms, FC.CONJ_SCHEMA)
        kept = len(helpers.rows_of(got))
        assert kept == 0 if case in FC.CONJ_EMPTY else 20 < kept < N_CONJ - 20, case
        if nulls == "all" and case not in FC.CONJ_EMPTY:
            assert len(FC.null_rows_that_would_pass(host, terms)) > 5


# ---- aggregates -------------------------------------------------------------------------------------------------------------------

# one term per special literal (+-0.0, +-inf, +-5e-324, +-DBL_MAX), operators and orientations mixed; rows of the predicate column
# sit at the literal and at both of its neighbours (fastpath_edge_cases.pred_values)
FLOAT_TERMS = [("p", "LtEq", 0.0, False), ("p", "Gt", -0.0, False), ("p", "Lt", 5e-324, True), ("p", "GtEq", -5e-324, False),
               ("p", "Lt", DBL_MAX, False), ("p", "Eq", -DBL_MAX, False), ("p", "LtEq", INF, True), ("p", "Gt", -INF, False),
               ("p", "Lt", INF, False), ("p", "GtEq", -INF, True), ("p", "LtEq", 0.1, False)]
NOTHING_TERMS = [("p", "Gt", INF, False), ("p", "Lt", INF, True), ("p", "Lt", -INF, False), ("p", "Gt", -INF, True)]
DATE_TERMS = [("d", "LtEq", 10471, False), ("d", "GtEq", 10471, True), ("d", "LtEq", INT32_MAX - 1, False), ("d", "LtEq", INT32_MIN, False)]
LOWCARD = ("scan_agg_lowcard_g1", "scan_agg_lowcard_g4", "scan_agg_lowcard_g8", "scan_agg_lowcard_g1_batches",
           "scan_agg_lowcard_g4_batches", "scan_agg_lowcard_g8_batches")
KEYS_OF = {"generic": ["ki"], "lean_spec_q1": ["ks", "kt"], "lean_spec_key1": ["k1"], "sop": ["kl"], "hash": ["ki"]}


def assert_route(ctx, ks, route):
    """the launches of the Partial aggregate (the Final one over its few state rows always runs on the VM: COUNT merges as an
    integer sum, which is no chain)"""
    if SWITCHED:
        return
    lean, sop, hashed = "scan_agg_lean_kernel" in ks, "scan_agg_sop_kernel" in ks, "scan_agg_hash" in ks
    if route in ("generic", "lean_spec_q1", "lean_spec_key1"):
        assert lean and not sop and not hashed, (route, sorted(ks))
        assert ctx.kernel_name(variant=True) == "scan_agg_lean_kernel/" + ("lean_generic" if route == "generic" else route)
    elif route == "sop":
        assert sop and not lean and not hashed, (route, sorted(ks))
    elif route == "vm":
        assert not lean and not sop and not hashed and sum(ks[k][1] for k in LOWCARD if k in ks) >= 1, (route, sorted(ks))
    else:
        assert hashed, (route, sorted(ks))


def check_aggregate(ctx, n, term, case, route, keys, predicate=None, operand_set=0, n_groups=3, expect_route=None):
    """FilterExec -> HashAggregateExec Partial -> Merge -> Final over one chain case, against the oracle, exactly"""
    host = FC.chain_batches(n, term, case, grouped=bool(keys), operand_set=operand_set, n_groups=n_groups, seed=len(case))
    expected, open_sign = FC.chain_expected(host, term, case, keys)          # asserts that the sums are exact in any order
    dev = [helpers.to_device(ctx, b) for b in host]
    group = [(col(k), k) for k in keys]
    aggs = FC.chain_aggs(case)
    p = predicate if predicate is not None else FC.term_expr(term, FC.CHAIN_SCHEMA)
    passes = 2 if route.startswith("lean_spec") else 1          # the second scan of the same buffers knows the keys' width
    for k in range(passes):
        part = ba.HashAggregateExec(ba.plan.PARTIAL, group, aggs, ba.FilterExec(p, source(ctx, dev, host)))
        fin = ba.HashAggregateExec(ba.plan.FINAL, group, aggs, ba.MergeExec(part))            # a fresh plan: no hints from another case
        ctx.kernel_stats(reset=True)
        got = helpers.concat(helpers.collect_product(fin))
        ks = ctx.kernel_stats(reset=True)
        helpers.assert_rows_equal(got, plan_eval.collect(fin), ordered=False, float_rtol=0, key_cols=keys, zero_sign_cols=open_sign)
        if keys:
            assert len(helpers.rows_of(got)) == len(expected), (term, case)        # a group without a live row does not appear
        elif not expected:
            assert all(got[c].to_pylist() == [None] for c in got if c.startswith("s_")) and got["n"].to_pylist() == [0]
        assert_route(ctx, ks, expect_route or route)
        if k == 1 and not SWITCHED and expected:
            assert ctx.lean_key_form() == "fixed"
    return expected


def lean_cases():
    return [c for c, (_, steps, columns_only) in FC.CHAIN_CASES.items() if columns_only and steps <= FC.SOP_NSTEP]


@pytest.mark.parametrize("n", AGG_SIZES)
def test_generic_wide_load_kernel(tctx, n):
    """lean_kernel.h: one Int32 key (or none), one Float64 range, chains of columns only"""
    for k, case in enumerate(lean_cases()):
        for j in range(3):
            term = FLOAT_TERMS[(k + n + 4 * j) % len(FLOAT_TERMS)]
            check_aggregate(tctx, n, term, case, "generic", ["ki"] if (k + j) % 3 else [], operand_set=k + j)


@pytest.mark.parametrize("n", AGG_SIZES)
@pytest.mark.parametrize("route", ["lean_spec_q1", "lean_spec_key1"])
def test_specialised_wide_load_kernels(tctx, route, n):
    """lean_spec_kernel.h: the Q1 shape — a Date32 bound with rows at the bound and +- 1, one or two 1-byte Utf8 keys, 5 steps"""
    for k, term in enumerate(DATE_TERMS):
        check_aggregate(tctx, n, term, "q1_five", route, KEYS_OF[route], operand_set=k + n)


@pytest.mark.parametrize("n", AGG_SIZES)
def test_register_kernel(tctx, n):
    """sop_kernel.h: an Int64 key, a literal factor, a CAST of an Int32 column"""
    for k, case in enumerate(["literal_factor", "cast_factor", "q1_prefixes", "eight_steps"]):
        for j in range(3):
            term = FLOAT_TERMS[(3 * k + j + n) % len(FLOAT_TERMS)]
            check_aggregate(tctx, n, term, case, "sop", ["kl"], operand_set=k + j)


@pytest.mark.parametrize("n", AGG_SIZES)
def test_expression_vm_register_kernel(tctx, n):
    """the same plans with the predicate written `p OR p`, and nine chain steps under a plain predicate: scan_agg_lowcard_*"""
    for k, case in enumerate(["literal_factor", "cast_factor", "q1_prefixes", "q1_five", "three_factors", "zero_minus_x"]):
        for j in range(2):
            term = FLOAT_TERMS[(2 * k + j + n) % len(FLOAT_TERMS)]
            keys = [["kl"], ["ki"], []][(k + j) % 3]
            check_aggregate(tctx, n, term, case, "vm", keys, predicate=FC.twice(FC.term_expr(term, FC.CHAIN_SCHEMA)), operand_set=k + j)
    check_aggregate(tctx, n, FLOAT_TERMS[n % len(FLOAT_TERMS)], "nine_steps", "vm", ["ki"], operand_set=n)


@pytest.mark.parametrize("n", [513, 1025, 2 * 1024 + 513])
def test_hash_table(tctx, n):
    """eleven live groups: more than the register paths hold"""
    for k, case in enumerate(["x_1my", "q1_prefixes", "xm25_y", "same_length_last_differs"]):
        for j in range(2):
            term = FLOAT_TERMS[(2 * k + j + n) % len(FLOAT_TERMS)]
            expected = check_aggregate(tctx, n, term, case, "hash", ["ki"], operand_set=k + j, n_groups=11)
            assert len(expected) > 8


@pytest.mark.parametrize("shape", ["generic", "lean_spec_key1", "sop", "hash"])
def test_aggregates_under_a_strict_bound_at_infinity(tctx, shape):
    """p > +inf and p < -inf over a column that holds the infinity: no group (a global aggregate: SUM NULL, COUNT 0) on the plans
    of every route; the range is empty, so it is the VM that runs them"""
    for n in (513, 2 * 1024 + 513):
        for k, term in enumerate(NOTHING_TERMS):
            assert FC.fold([term], FC.CHAIN_SCHEMA) is None
            host = FC.chain_batches(n, term, "x_1my", n_groups=11 if shape == "hash" else 3)
            assert any(float(term[2]) in b["p"].values for b in host)               # rows AT the infinity
            case = {"generic": "x_1my", "lean_spec_key1": "q1_five", "sop": "literal_factor", "hash": "x_1my"}[shape]
            keys = [] if shape == "generic" and k % 2 else KEYS_OF[shape]
            expected = check_aggregate(tctx, n, term, case, shape, keys, n_groups=11 if shape == "hash" else 3, expect_route="vm")
            assert not expected
