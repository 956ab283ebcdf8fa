"""GPU parity of HashJoinExec's single-key build and probe routes at their edges (host/ops_join.cpp try_narrow; kernels_join.hip
tiny_rank_build, join_key_stats, rank_bits_sorted / rank_bits_any, rank_perm, join_rank_probe, join_filter_probe; kernels_hash.hip
join_build_narrow[64], join_key_present[64]).

Expected rows: join_route_cases.expected — a dict join in plain Python, checked against the CPU oracle in test_join_route_cases_cpu.py,
which also proves that every case lies on the side of its limit that its name says.  Rows compare as multisets keyed by the row ids
li / ri, floats by bit pattern.  Every case asserts the route it took from what the library reports: the kernel names of a context
made under BHIP_KERNEL_TIMING=2, join_key_form() and join_probe_form().  The process-wide switches (the CAS table and the A/B partners
of the probe variants) run in children: join_routes_gpu_child.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ballista_amd as ba
from oracle import engine as og

import helpers
import join_filter_cases as JF
import join_types_cases as JT
import join_route_cases as RC

pytestmark = pytest.mark.gpu
ALL = RC.all_cases()
IDS = [RC.case_id(c) for c in ALL]


@pytest.fixture(scope="module")
def tctx():
    return RC.timing_context()


# ---- 1. every build case, join type and probe form -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_build_route(tctx, case):
    """Inner / Left / Right / Full against a probe stream with and without NULL keys: 6682 rows in batches of 1 .. 2049 around the wave, a
    pass of a wave and the selection tile, with the window-edge keys of the case's own window, a batch without a match and one of matches"""
    for probe_nulls in (False, True):
        for jt in RC.TYPES:
            RC.run_case(tctx, case, jt, probe_nulls, route=case.route)


# ---- 2. probe shapes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", [JF.INNER, JF.LEFT])
@pytest.mark.parametrize("name", list(RC.FILTERS))
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_range_filter_below_the_probe_side(tctx, order, name, jt):
    """one and JOIN_FILTER_MAX Int32 / Date32 range terms fused into the probe kernel: an empty range, ranges nothing fails, bounds at the
    Int32 ends; the terms' count is read back from the probe launches' algorithmic bytes"""
    got = RC.run_filter_shape(tctx, order, name, jt)
    if "empty" in name:
        assert og.batch_len(got) == (0 if jt == JF.INNER else RC.SHAPE_NL)


@pytest.mark.parametrize("jt", [JF.INNER, JF.RIGHT])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("build", ["rank", "table"])
@pytest.mark.parametrize("form", ["first_column", "pairs"])
def test_two_four_byte_keys(tctx, form, build, order, jt):
    """first_column: the second key compared inside the probe (RESID); pairs: both packed into one 8-byte key — on a rank map and on
    the CAS table"""
    RC.run_pair_shape(tctx, form, build, order, jt)


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_parent_reads_no_build_column(tctx, order):
    """nothing staged: a sorted one-column build side is probed by its key-set words alone (rank/bits), a shuffled one by the packed map"""
    RC.run_semi_shape(tctx, order)


# ---- 3. the rows are a function of the input ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in ALL if c.dtype in ("Int32", "Int64") and c.name in
                                  ("tiny/sorted_n1023", "rank/sorted_n1025", "rank/window_limit_n1025", "table/n300", "rank/shuffled_n4097")], ids=RC.case_id)
def test_two_runs_give_the_same_rows(ctx, case):
    left, right = RC.sides(case, True)
    plan = ba.HashJoinExec(RC.build_exec(ctx, left), RC.probe_exec(ctx, right), RC.ON, JT.FULL)
    a, b = JF.rows(plan), JF.rows(plan)
    RC.assert_same_rows(a, b)
    RC.assert_same_rows(a, RC.expected(JT.FULL, left, right))


@pytest.mark.parametrize("case", [c for c in ALL if c.route in ("tiny", "rank_sorted") and RC.is_sorted(c) and len(c.bkeys) > 2], ids=RC.case_id)
def test_a_shuffled_copy_of_a_sorted_build_side_joins_the_same_rows(tctx, case):
    """rank = row against rank -> row through the permutation: the same build rows (row ids and all) in another order"""
    own, _ = RC.sides(case, False)
    perm = np.random.default_rng(len(case.bkeys)).permutation(len(case.bkeys))
    shuffled = type(own)((k, c.take(perm)) for k, c in own.items())
    tctx.kernel_stats(reset=True)
    RC.run_case(tctx, case, JF.INNER, False, left=shuffled)
    names = set(tctx.kernel_stats(reset=True))
    assert tctx.join_probe_form() == RC.rank_probe_form(perm=True, width=RC.WIDTH[case.dtype])
    if case.route == "rank_sorted" and len(case.bkeys) > RC.TINY_BUILD_ROWS:
        assert {"rank_bits_any", "rank_perm"} <= names and "rank_bits_sorted" not in names


# ---- 4. the switches, each in a process of its own ----------------------------------------------------------------------------------------------

def run_child(mode, **env):
    child = os.path.join(helpers.ROOT, "tests", "join_routes_gpu_child.py")
    p = subprocess.run([sys.executable, child, mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def n_cases(*prefixes):
    return sum(len(RC.cases(p)) for p in prefixes)


def test_every_tiny_and_rank_case_through_the_forced_cas_table():
    """BHIP_JOIN_TABLE=1: join_build_narrow[64] for every case the rank map takes by default, and the same expected rows"""
    out = run_child("table", BHIP_JOIN_TABLE="1")
    assert "OK table %d" % n_cases("tiny/", "rank/") in out


def test_key_set_bitmap_in_front_of_the_forced_cas_table():
    """BHIP_JOIN_TABLE=1 and 2^18 / 2^18 + 37 unique keys spanning < 2^30: join_key_present and join_key_present64 run (the child asserts
    their names), the probe's window test is krange64"""
    out = run_child("present", BHIP_JOIN_TABLE="1")
    assert "OK present 4" in out


def test_tiny_cases_through_the_general_rank_map():
    out = run_child("notiny", BHIP_NO_TINY_BUILD="1")
    assert "OK notiny %d" % n_cases("tiny/") in out


@pytest.mark.parametrize("mode,env", [("noscalar", "BHIP_PROBE_NO_SCALAR_MAP"), ("flat", "BHIP_PROBE_MAP_FLAT"), ("nobits", "BHIP_PROBE_NO_BITS")])
def test_probe_variant_switch(mode, env):
    """the A/B partner of a probe variant on the rank cases and the probe shapes: join_probe_form() names the partner, the rows are the
    same.  flat: the window test is in_window, no longer the buffer descriptor's range check"""
    out = run_child(mode, **{env: "1"})
    assert "OK %s %d" % (mode, n_cases("rank/") + len(RC.shape_runs())) in out


def test_eight_rows_per_lane():
    out = run_child("rows8", BHIP_PROBE_ROWS="8")
    assert "OK rows8 %d" % (n_cases("rank/") + len(RC.shape_runs())) in out


def test_rank_window_bound_of_2_to_the_10():
    """BHIP_RANK_WINDOW_LOG2=10: the rank cases with a range above 1024 go to the CAS table by the bound, not by sparsity"""
    out = run_child("window10", BHIP_RANK_WINDOW_LOG2="10")
    assert "OK window10 %d" % n_cases("rank/") in out
