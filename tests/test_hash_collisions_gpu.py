"""The open-addressing tables of HashJoinExec's general table (kernels_hash.hip join_upsert / join_find / join_owner_walk, packed and
wide keys) and of HashAggregateExec's hash path (table_upsert under scan_agg_hash and run_groups, merge_assign) on keys that COLLIDE
BY CONSTRUCTION: a cluster that wraps past slot 0, neighbours that share their 32-bit tag, different keys of one 64-bit hash, keys that
differ in one word of their image only, a capacity step.  The cases are hash_table_cases.py's; test_hash_table_cases_cpu.py proves
that each is what it says and that a table which took a tag or a hash for a key, compared one word, forgot the mask or stopped at a
foreign tag would give other rows.

Joins compare as multisets keyed by the row ids li / ri (the row count included), aggregates by their key columns: every value is an
integer and nothing here has a tolerance."""
import numpy as np
import pytest

import ballista_amd as ba
from oracle import engine as og

import helpers
import hash_table_cases as HT
import join_filter_cases as JF
import join_route_cases as RC

pytestmark = pytest.mark.gpu

JOIN_IDS = [HT.join_case_id(c) for c in HT.JOIN_CASES]
AGG_CASES = HT.agg_cases()


def join_rows(ctx, left, right, form, jt, flt=None):
    plan = ba.HashJoinExec(HT.build_exec(ctx, left), HT.probe_exec(ctx, right, jt), HT.ON[form], jt, filter=flt)
    got = JF.rows(plan)
    assert ctx.join_key_form() == HT.TABLE_FORM[form], (ctx.join_key_form(), form)
    return got


# ---- joins ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jt", HT.ALL_TYPES)
@pytest.mark.parametrize("case", HT.JOIN_CASES, ids=JOIN_IDS)
def test_join_on_constructed_collisions(ctx, case, jt):
    """family x form x {unique, duplicates} x the eight join types"""
    _, form, _ = case
    left, right, _, _ = HT.join_sides(*case)
    assert og.batch_len(left) < 520 and og.batch_len(right) < 2000
    got = join_rows(ctx, left, right, form, jt)
    HT.NC.assert_same_rows(got, HT.expected_rows(jt, left, right, form))
    if jt == JF.INNER:                                      # the count on its own: a doubled pair cannot hide
        assert og.batch_len(got) == len(HT.expected_pairs(left, right, form)[0])


@pytest.mark.parametrize("jt", HT.ALL_TYPES)
@pytest.mark.parametrize("form", list(HT.FORMS))
def test_null_keys_neither_enter_nor_match_the_cluster(ctx, form, jt):
    """NULLs on both sides of a wrapping cluster, every NULL row storing a cluster key's values"""
    left, right, _, _ = HT.join_sides("wrap_cluster", form, "duplicates", nulls=True)
    got = join_rows(ctx, left, right, form, jt)
    HT.NC.assert_same_rows(got, HT.expected_rows(jt, left, right, form))


@pytest.mark.parametrize("variation", HT.VARIATIONS)
@pytest.mark.parametrize("form", list(HT.FORMS))
def test_variations_reach_the_probe_kernels_they_name(form, variation):
    """a unique build side: join_probe_match (join_owner_walk); duplicates — and packed1_dup always, which holds one — the head / next
    chains under join_probe_count / join_probe_emit; Semi: join_probe_exists, and join_exists_flags finds a duplicate's representative
    again with join_find.  Names of a BHIP_KERNEL_TIMING=2 context (kernel_name() in host/ops_join.cpp)"""
    ctx = RC.timing_context()
    left, right, _, _ = HT.join_sides("wrap_cluster", form, variation)
    w = "_wide" if HT.TABLE_FORM[form] == "wide" else ""
    ctx.kernel_stats(reset=True)
    HT.NC.assert_same_rows(join_rows(ctx, left, right, form, JF.INNER), HT.expected_rows(JF.INNER, left, right, form))
    names = set(ctx.kernel_stats(reset=True))
    chains = variation == "duplicates" or form == "packed1_dup"
    assert "join_build" + w in names, sorted(names)
    assert ("join_probe_match" + w in names) == (not chains), sorted(names)
    assert ({"join_probe_count" + w, "join_probe_emit" + w} <= names) == chains, sorted(names)
    HT.NC.assert_same_rows(join_rows(ctx, left, right, form, HT.JT.SEMI), HT.expected_rows(HT.JT.SEMI, left, right, form))
    names = set(ctx.kernel_stats(reset=True))
    # (a unique build side's rows are their own representatives: the wide form of join_exists_flags runs only where it looks them up)
    assert {"join_build" + w, "join_probe_exists" + w, "join_exists_flags" + (w if chains else "")} <= names, sorted(names)


def _filter_case(form):
    return ("equal_hash" if ("equal_hash", form) not in HT.LEFT_OUT else "equal_tag_neighbours", form, "duplicates")


@pytest.mark.parametrize("jt", HT.FILTER_TYPES)
@pytest.mark.parametrize("form", list(HT.FORMS))
def test_residual_filter_over_colliding_chains(ctx, form, jt):
    """ri % 3 != 0 over the candidates of the equal-hash keys with duplicates (packed1_dup, which has no two keys of one hash: the
    equal-tag neighbours): the filter neither reorders nor drops chain rows"""
    left, right, _, _ = HT.join_sides(*_filter_case(form))
    got = join_rows(ctx, left, right, form, jt, HT.residual_filter(left, right, form))
    HT.NC.assert_same_rows(got, HT.filtered_rows(jt, left, right, form))


@pytest.mark.parametrize("form", [f for f in HT.FORMS if ("equal_hash", f) not in HT.LEFT_OUT])
def test_racing_build_gives_the_same_rows_twice(ctx, form):
    """the build is racing CAS claims and atomicExch chain pushes: the order of a chain may differ from run to run, its rows may not"""
    left, right, _, _ = HT.join_sides("equal_hash", form, "duplicates")
    first = join_rows(ctx, left, right, form, JF.INNER)
    second = join_rows(ctx, left, right, form, JF.INNER)
    HT.NC.assert_same_rows(first, second)
    HT.NC.assert_same_rows(second, HT.expected_rows(JF.INNER, left, right, form))


# ---- aggregates -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", AGG_CASES, ids=[c.name for c in AGG_CASES])
def test_aggregate_on_constructed_collisions(case):
    """the row table, the run table and the merge table: the route by kernel names, the number of groups, every value exactly.  A context
    of its own per case: no dispatch state learned on one case picks the route of the next"""
    ctx = RC.timing_context()
    plan = ba.HashAggregateExec(ba.plan.PARTIAL, case.group, case.aggs, helpers.memory_exec(ctx, case.partitions))
    ctx.kernel_stats(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    names = set(ctx.kernel_stats(reset=True))
    HT.assert_agg_route(names, case.facts["route"])
    assert og.batch_len(got) == case.facts["n_groups"]
    helpers.assert_rows_equal(got, HT.expected_groups(case), ordered=False, float_rtol=0.0, key_cols=HT.agg_key_names(case))
    assert int(np.sum(got["n[count]"].values)) == case.facts["n_rows"]
