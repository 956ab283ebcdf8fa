"""GPU: the hash aggregate's Float64 sums (ballista_amd/csrc/kernels_dagg.hip, host/ops_agg_hash.cpp) add every group's runs
in row order — bit for bit.

The inputs and the reference are tests/det_sum_cases.py (checked on the CPU by test_det_sum_cases_cpu.py).  Families 1 (exact
values) and 2 (run sums whose other orders give other bits) compare bit for bit, an exactly zero sum's sign excepted; family 3
(ill-conditioned values inside runs, whose tree is not restated) within the bound for any order of addition, and bit-identical
between repeats and batch cuts.  Keys, row counts, COUNTs and validity always compare exactly.

Every plan has the case's primer as partition 0 (13 groups), executed first: the operator is on the hash table when the case's
partition runs, whatever it holds.  Every run reads the launch list of a BHIP_KERNEL_TIMING=2 context and asserts det_segments,
det_apply and det_spill_lists, det_spill_combine exactly when some group has more than DET_LIST_MAX runs, the fused predicate
(scan_agg_hash without the run kernels) and the run path the case claims.  The segment kernel's passes (one per four sums) are
one named launch: m = 5, 8 (two passes) and m = 9 (three) are pinned through their results against m = 4."""
import os
import subprocess
import sys
from collections import OrderedDict

import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from oracle.engine import OCol

import det_sum_cases as K
import helpers

pytestmark = pytest.mark.gpu

CHILD = os.environ.get("BHIP_NO_RUN_AGG") == "1"
CASES = K.all_cases()
IDS = [c.name for c in CASES]
SPEC = K.agg_spec(2, avg_of=1, count_of=0)         # SUM(x0), SUM(x1), COUNT(*), AVG(x1), COUNT(x0)
REGISTER = ("scan_agg_lowcard_g1", "scan_agg_lowcard_g4", "scan_agg_lowcard_g8", "scan_agg_lowcard_g4_batches",
            "scan_agg_lowcard_g8_batches", "merge_partials")


@pytest.fixture(scope="module")
def ctx():
    old = os.environ.get("BHIP_KERNEL_TIMING")
    os.environ["BHIP_KERNEL_TIMING"] = "2"                 # every launch, however small (read when a context is created)
    try:
        yield ba.Context(0)
    finally:
        if old is None:
            os.environ.pop("BHIP_KERNEL_TIMING", None)
        else:
            os.environ["BHIP_KERNEL_TIMING"] = old


def device_plan(ctx, case, spec, cut, mode="Partial"):
    parts = [K.host_batches(K.primer(case), False, OCol), K.host_batches(case, cut, OCol)]
    return K.plan(ba, E, helpers.memory_exec(ctx, parts), case, spec, mode)


def execute(ctx, plan, p):
    ctx.kernel_stats(reset=True)
    got = helpers.concat([helpers.from_device(b) for b in plan.execute(p)])
    return got, ctx.kernel_stats(reset=True)


def assert_route(case, ks):
    """the launches of the case's partition: the ordered sums, the combine the run counts call for, the path the case claims"""
    for name in ("scan_agg_hash", "det_segments", "det_apply", "det_spill_lists"):
        assert name in ks, (case.name, name, sorted(ks))
    assert not set(REGISTER) & set(ks), (case.name, sorted(ks))
    assert ("det_spill_combine" in ks) == (K.max_runs(case) > K.LIST_MAX), (case.name, K.max_runs(case), sorted(ks))
    route = None if CHILD else case.route
    sampled = not CHILD and case.keep is None and case.n >= K.RUN_ROWS
    assert ("run_heads" in ks) == sampled, (case.name, sorted(ks))
    assert ("run_slots" in ks) == (route is not None), (case.name, route, sorted(ks))
    assert ("run_groups" in ks) == (route == "table"), (case.name, route, sorted(ks))
    assert ("run_tail_resolve" in ks) == (route == "two") and ("run_tail_remap" in ks) == (route == "two"), (case.name, route, sorted(ks))


def run_case(ctx, case, spec, cut):
    """the primer's partition, then the case's -> (its result, its launches)"""
    plan = device_plan(ctx, case, spec, cut)
    got, ks = execute(ctx, plan, 0)
    K.check_result(got, [K.primer(case)], spec, "Partial", helpers)
    got, ks = execute(ctx, plan, 1)
    assert_route(case, ks)
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_partial_sums_in_row_order(ctx, case):
    """as one batch and cut into the case's batches (cuts at rows 1, 63, 64, an empty batch, 1000, 2053): the same expected
    values, since all batches of a partition are one row range"""
    gate = "gamma" if case.family == 3 else "bits"
    results = []
    for cut in (False, True, False) if case.family == 3 else (False, True):
        got = run_case(ctx, case, SPEC, cut)
        K.check_result(got, [case], SPEC, "Partial", helpers, gate=gate)
        results.append(K.sorted_by_key(got) if got else got)
    for other in results[1:]:                              # (families 1 and 2: implied by the expected bits, zero signs aside)
        if case.family == 3:
            helpers.assert_bit_exact(other, results[0])


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("case", [c for c in CASES if c.family == 1], ids=[c.name for c in CASES if c.family == 1])
def test_partial_then_final(ctx, case):
    """Partial over the primer's and the case's partitions -> Merge -> Final: SUM, AVG = SUM / count, COUNT"""
    plan = device_plan(ctx, case, SPEC, True, mode="Final")
    ctx.kernel_stats(reset=True)
    got = helpers.concat(helpers.collect_product(plan))
    ks = ctx.kernel_stats(reset=True)
    assert "det_segments" in ks and "scan_agg_hash" in ks, sorted(ks)
    K.check_result(got, [K.primer(case), case], SPEC, "Final", helpers)


@pytest.mark.skipif(CHILD, reason="in-process paths only in the parent run")
@pytest.mark.parametrize("family", [1, 3])
def test_accumulator_passes(ctx, family):
    """m = 1, 4 (one pass of the segment kernel), 5, 8 (two) and 9 (three) sums of different columns over runs that straddle
    tiles and a 17-run group: only the first pass counts runs and rows, so with m >= 5 the row counts, the non-NULL counts and
    the first four sums are those of m = 4, bit for bit"""
    whole = K.acc_case(family)
    gate = "gamma" if family == 3 else "bits"
    by_m = {}
    for m in K.ACC_M:
        case, spec = whole.with_args(m), K.agg_spec(m)
        assert len(spec) <= K.MAX_ACCS
        for cut in (False, True):
            got = run_case(ctx, case, spec, cut)
            K.check_result(got, [case], spec, "Partial", helpers, gate=gate)
            got = K.sorted_by_key(got)
            if m in by_m:
                helpers.assert_bit_exact(got, by_m[m])
            by_m[m] = got
    shared = list(by_m[4])
    assert shared == ["k", "s0[sum]", "s1[sum]", "s2[sum]", "s3[sum]", "n[count]", "a0[count]", "a0[sum]"]
    for m in (5, 8, 9):
        helpers.assert_bit_exact(OrderedDict((n, by_m[m][n]) for n in shared), by_m[4])


@pytest.mark.skipif(CHILD, reason="this is the child run's parent")
def test_without_the_run_paths_the_sums_are_the_same_bits():
    """every case again in a child process with BHIP_NO_RUN_AGG=1 (read once per process): clustered input goes through the
    table, slot numbers differ, the expected values do not"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BHIP_NO_RUN_AGG="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-k", "test_partial_sums_in_row_order",
                        os.path.abspath(__file__)], cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{len(CASES)} passed" in p.stdout, p.stdout[-2000:]
