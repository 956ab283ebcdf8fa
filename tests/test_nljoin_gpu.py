"""GPU parity of NestedLoopJoinExec on its four routes (kernels_nljoin.hip: nlj_compare_count / nlj_compare_emit, nlj_cross_pairs;
the shared tail of ops_join.cpp), all eight join types, through the C ABI by the Python mirror.

Expected rows: nljoin_cases.expected — the numpy cross product filtered by the oracle's evaluator, checked against a nested loop in
plain Python in test_nljoin_plan.py.  Rows compare as multisets keyed by the row ids li / ri, floats by bit pattern.  Sizes are the
smallest at which each mechanism can break: build rows around the LDS tile NLJ_BUILD_TILE (read from the header), probe batches around
the wave (64), the workgroup (256) and the 1024-row selection tile; 150 x 400 rows for the value and general-route cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd.expr import col
from oracle import engine as og

import helpers
import join_filter_cases as JF
import join_types_cases as JT
import nljoin_cases as NC

pytestmark = pytest.mark.gpu
T = NC.TILE
EXISTENCE = JF.BUILD_SIDE + JF.PROBE_SIDE


# ---- 1. the fused route at the edges of its shapes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("nl", [0, 1, T - 1, T, T + 1, 2 * T + 3])
def test_fused_route_shape_edges(ctx, nl):
    """build rows around the LDS tile, in two partitions; probe batches of 0, 1, 63, 64, 65, 255, 256, 257 and 1025 rows in two partitions"""
    left, right = NC.sides(True, nl, NC.NR_SHAPES)
    flt = NC.predicate("band", left, right)
    for jt in (JF.INNER, JF.RIGHT, JT.RIGHT_ANTI):
        got = NC.check(ctx, left, right, jt, flt, "compare", batch_rows=NC.PROBE_BATCHES)
    if nl > 1:
        li, _ = NC.pairs(left, right, flt)
        assert 0 < len(li) < nl * NC.NR_SHAPES // 20 and li.max() >= nl - 2
    else:
        assert og.batch_len(got) >= NC.NR_SHAPES - 20


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("jt", NC.ALL_TYPES)
def test_every_type_on_the_fused_route(ctx, jt, merge):
    """Left / Full / Semi / Anti through one right partition and through a MergeExec over two; the others over two partitions"""
    left, right = NC.sides(True, T + 1, NC.NR_SHAPES)
    NC.check(ctx, left, right, jt, NC.predicate("two_terms", left, right), "compare", batch_rows=NC.PROBE_BATCHES, merge=merge)


def test_every_pair_kept(ctx):
    left, right = NC.sides(False, T + 1, 257)
    got = NC.check(ctx, left, right, JF.INNER, NC.predicate("all", left, right), "compare", batch_rows=[257])
    assert og.batch_len(got) == (T + 1) * 257
    for jt in (JT.FULL, JT.ANTI, JT.RIGHT_ANTI):
        NC.check(ctx, left, right, jt, NC.predicate("all", left, right), "compare", batch_rows=[257])


# ---- 2. the fused route at the edges of its values ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,nulls,jt", NC.value_cases(), ids=lambda v: str(v))
def test_fused_route_value_edges(ctx, name, nulls, jt):
    """six operators x Int32, Date32, Int64 at its ends, UInt64 across 2^63, Float64 and Float32 with NaN, +-0.0 and +-inf; one, two and
    four terms; right column first; no, sparse and full selectivity; NULLs on both sides incl. rows 63 / 64"""
    got = NC.run_case(ctx, name, nulls, jt, "compare")
    if name == "none" and jt == JF.INNER:
        assert og.batch_len(got) == 0


# ---- 3. the general route -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,nulls,jt", NC.general_cases(), ids=lambda v: str(v))
def test_general_route(ctx, name, nulls, jt):
    """arithmetic, Utf8 <, one-sided terms, constant truth values, and a fusable conjunction with one term that is not"""
    NC.run_case(ctx, name, nulls, jt, "general")


# ---- 4. no filter -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", NC.ALL_TYPES)
def test_cross_and_exists_routes(ctx, jt):
    left, right = NC.sides(True, NC.NL, NC.NR)
    got = NC.check(ctx, left, right, jt, None, "exists" if jt in EXISTENCE else "cross", merge=jt == JT.FULL)
    want = {JT.SEMI: NC.NL, JT.ANTI: 0, JT.RIGHT_SEMI: NC.NR, JT.RIGHT_ANTI: 0}.get(jt, NC.NL * NC.NR)
    assert og.batch_len(got) == want


# ---- 5. empty sides -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", NC.ALL_TYPES)
@pytest.mark.parametrize("case", ["empty_build", "empty_probe"])
@pytest.mark.parametrize("route", ["cross", "compare", "general"])
def test_empty_sides(ctx, route, case, jt):
    left, right = NC.sides(True, 70, 130)
    name = {"cross": None, "compare": "band", "general": "two_sided"}[route]
    flt = NC.predicate(name, left, right) if name else None
    nl, nr = (0, 130) if case == "empty_build" else (70, 0)
    l, r = helpers.slice_batch(left, 0, nl), helpers.slice_batch(right, 0, nr)
    build = helpers.memory_exec(ctx, [[l]])
    probe = helpers.memory_exec(ctx, [[helpers.slice_batch(r, 0, nr // 2), helpers.slice_batch(r, nr // 2, nr)]])
    got = JF.rows(ba.NestedLoopJoinExec(build, probe, jt, filter=flt))
    NC.assert_same_rows(got, JF.from_pairs(jt, l, r, [], [], []))
    want = {JF.INNER: 0, JF.LEFT: nl, JF.RIGHT: nr, JT.FULL: nl + nr, JT.SEMI: 0, JT.ANTI: nl, JT.RIGHT_SEMI: 0, JT.RIGHT_ANTI: nr}[jt]
    assert og.batch_len(got) == want
    if jt == JF.RIGHT and nr:                              # every probe row, with NULL left columns
        assert not got["li"].is_valid().any() and sorted(got["ri"].values) == list(range(nr))


# ---- 6. the switches, each in a process of its own ------------------------------------------------------------------------------------------------

def run_child(mode, **env):
    child = os.path.join(helpers.ROOT, "tests", "nljoin_gpu_child.py")
    p = subprocess.run([sys.executable, child, mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def test_general_route_over_many_ragged_chunks():
    """BHIP_NLJ_CHUNK_PAIRS=1000 against 150 build rows: 60 chunks a probe stream, none aligned to a probe row or a bitmap word"""
    out = run_child("chunked", BHIP_NLJ_CHUNK_PAIRS="1000")
    assert "OK chunked %d" % (len(NC.general_cases()) + len(NC.ALL_TYPES)) in out


def test_fused_route_equals_general_route():
    """BHIP_NO_NLJ_FUSED=1: the value-edge cases report "general" and meet the same expected rows, bit for bit"""
    out = run_child("nofused", BHIP_NO_NLJ_FUSED="1")
    assert "OK nofused %d" % len(NC.value_cases()) in out


# ---- 7. parents ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["band", "two_sided", None])
@pytest.mark.parametrize("jt", [JF.INNER, JF.LEFT, JF.RIGHT, JT.FULL, JT.SEMI, JT.RIGHT_ANTI])
def test_a_projection_that_reads_one_column_of_each_side(ctx, jt, name):
    left, right = NC.sides(True, NC.NL, NC.NR)
    flt = NC.predicate(name, left, right) if name else None
    ids = [c for c in ("li", "ri") if not (c == "ri" and jt in JF.BUILD_SIDE) and not (c == "li" and jt in JF.PROBE_SIDE)]
    exprs = [(col(c), c) for c in ids]
    got = JF.rows(ba.ProjectionExec(exprs, NC.join_plan(ctx, left, right, jt, flt)))
    NC.assert_same_rows(got, og.project(NC.expected(jt, left, right, flt), exprs))


# ---- 8. the order of the output is a function of the input ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["band", "two_sided", None])
def test_two_runs_give_the_same_rows_in_the_same_order(ctx, name):
    left, right = NC.sides(True, T + 1, 700)
    flt = NC.predicate(name, left, right) if name else None
    a, b = (NC.bit_patterns(JF.rows(NC.join_plan(ctx, left, right, JF.INNER, flt))) for _ in range(2))
    assert og.batch_len(a) > 0 and list(a) == list(b)
    for k in a:
        assert np.array_equal(a[k].values, b[k].values) and np.array_equal(a[k].is_valid(), b[k].is_valid()), k
    if name == "band":                                     # ... and known: probe rows in batch order, a row's build rows ascending
        li, ri = NC.pairs(left, right, flt)
        assert np.array_equal(a["li"].values, li) and np.array_equal(a["ri"].values, ri)
