"""The cases of tests/det_sum_cases.py are what they claim to be, and their reference agrees with the oracle (no GPU).

- every case meets the premise of its value family (exactness; the three alternative folds of every group with >= 3 runs differ
  in bits from the row-order fold; multi-row stretches of family 2 inside one tile): a case that does not is an error here;
- the layouts reach the edges they are named after (runs per group around DET_LIST_MAX, tile-straddling runs, 1024 records in
  a tile, the run-path forms, the batch cuts);
- the reference against plan_eval over the same HashAggregateExec plan: family 1 bit for bit, families 2 and 3 — where the
  oracle adds in another order — within the bound for any order around the exact (Fraction) sum;
- a handful of values written out by hand, so that the reference is not its own only witness."""
from fractions import Fraction

import numpy as np
import pytest

from ballista_amd import expr as E
from oracle import plan_eval
from oracle.engine import OCol

import det_sum_cases as K
import helpers
import plan_nodes

CASES = K.all_cases()
IDS = [c.name for c in CASES]


def oracle_result(case, spec, cut, mode="Partial", m=None):
    parts = [K.host_batches(K.primer(case, m), False, OCol, m), K.host_batches(case, cut, OCol, m)]
    plan = K.plan(plan_nodes, E, plan_nodes.MemoryExec(parts), case, spec, mode)
    if mode == "Partial":
        return helpers.concat(plan_eval.execute(plan, 1))
    return plan_eval.collect(plan)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_meets_the_premise_of_its_family(case):
    if case.family == 1:
        K.check_family1(case)
    elif case.family == 2:
        assert K.check_family2(case) >= 2
    else:
        assert any(hi - lo > K.CHUNK for _, lo, hi in K.runs(case))
        # Python's own left fold lies inside the bound the GPU tier uses
        ref, ex = K.reference(case), K.exact(case)
        for key in ref.keys:
            for j in range(case.m):
                if ref.sums[key][j] is not None:
                    assert abs(Fraction(ref.sums[key][j]) - ex[key][j][0]) <= K.gamma_bound(ref.rows[key], ex[key][j][1])
    groups = len(K.runs_per_group(case))
    if not case.name.startswith(("size_", "predicate_drops")):
        assert groups >= 12, groups
    assert len(K.runs_per_group(K.primer(case))) == 13


def test_family1_holds_both_zeros_and_negative_values():
    x = np.concatenate([c.xs[0].astype(np.float64) for c in CASES if c.family == 1])
    assert np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x)) and np.any(x < 0) and np.any(x > 0)
    assert np.abs(x).max() > 2.0 ** 19


def test_sizes_and_layouts():
    for n in K.SIZES:
        rr, one, rnd = (K.by_name(f"size_{n}_{kind}") for kind in ("round_robin", "one_key", "random"))
        assert rr.n == one.n == rnd.n == n
        assert len(K.runs(rr)) == n and len(K.runs(one)) == (n + K.TILE - 1) // K.TILE
        assert n < 13 or len(K.runs_per_group(rnd)) == 13
    full = K.by_name("size_1024_round_robin")
    assert sum(1 for _, lo, _ in K.runs(full) if lo < K.TILE) == K.TILE         # a tile's staging area, full


def test_boundary_runs_sit_where_they_are_named():
    for filler in ("rr", "fresh"):
        for name, (lo, hi) in K.BOUNDARIES.items():
            c = K.by_name(f"boundary_{name}_{filler}")
            mine = [(a, b) for key, a, b in K.runs(c) if key == 7]
            cuts = [lo] + [t for t in range(K.TILE, hi, K.TILE) if t > lo] + [hi]
            assert mine == list(zip(cuts[:-1], cuts[1:])), (name, mine)
            assert filler == "rr" or K.max_runs(c) <= K.LIST_MAX
            assert filler == "fresh" or c.n < 300 or K.max_runs(c) > K.LIST_MAX
        assert [b - a for key, a, b in K.runs(K.by_name(f"boundary_four_runs_{filler}")) if key == 7] == [524, 1024, 1024, 28]
        c = K.by_name(f"carry_then_closes_{filler}")
        r = K.runs(c)
        assert (7, 70, 128) in r and (8, 128, 140) in r and r[-1] == (9, c.n - 9, c.n) and c.n % K.CHUNK


def test_runs_per_group_straddle_the_list_limit():
    for family in (1, 2):
        many, few = K.by_name(f"runs_per_group_with_17_and_40_f{family}"), K.by_name(f"runs_per_group_at_most_16_f{family}")
        assert [K.runs_per_group(many)[k] for k in range(1, 7)] == [1, 2, 15, 16, 17, 40]
        assert K.max_runs(few) == K.LIST_MAX and K.max_runs(many) == 40
        for c in (many, few):                        # the runs of the watched groups lie in more than one tile
            assert len({lo // K.TILE for key, lo, _ in K.runs(c) if key == 4}) >= 3


def test_accumulator_ladder():
    c = K.acc_case()
    K.check_family1(c)
    assert K.ACC_M == (1, 4, 5, 8, 9) and c.m == 9 and K.PASS_ACCS == 4 and len(K.agg_spec(9, count_of=1)) <= K.MAX_ACCS
    assert K.runs_per_group(c)[50] == 17 and c.with_args(4).m == 4
    assert K.reference(c.with_args(4)).sums[50] == K.reference(c).sums[50][:4]


def test_null_and_predicate_placements():
    for filler in ("rr", "fresh"):
        c = K.by_name(f"nulls_{filler}")
        v = c.valid(0)
        assert not v[0] and not v[63] and not v[1023] and not v[200:210].any() and v[1:63].all()
        assert (K.max_runs(K.by_name(f"predicate_16_runs_{filler}")) > K.LIST_MAX) == (filler == "rr")
        assert K.max_runs(K.by_name(f"predicate_20_runs_{filler}")) > K.LIST_MAX
        keep = K.by_name(f"predicate_20_runs_{filler}").keep
        assert not keep[25] and not keep[63] and not keep[1023] and not keep[192:256].any() and keep[191] and keep[256]
    assert len(K.runs(K.by_name("predicate_drops_every_row"))) == 0


def test_claimed_run_paths():
    """what a case claims about the run paths is what its keys say; the three forms at 4096 and 4097 rows, none at 4095"""
    for c in CASES + [K.acc_case()]:
        assert K.derived_route(c) == c.route, c.name
    for form, route in zip(K.RUN_FORMS, ("distinct", "two", "table")):
        assert [K.by_name(f"run_path_{form}_{n}").route for n in K.RUN_SIZES] == [None, route, route]
    assert K.by_name("run_table_f2").route == "table"


def test_batch_cuts():
    big = K.by_name("size_4097_random")
    assert big.cuts == [1, 63, 64, 64, 1000, 2053] and (64, 64) in big.batches(True) and big.batches(False) == [(0, 4097)]
    assert all(c.batches(True)[-1][1] == c.n and c.batches(True)[0][0] == 0 for c in CASES)
    assert K.by_name("size_1_one_key").batches(True) == [(0, 1)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_against_the_oracle(case):
    spec = K.agg_spec(case.m, avg_of=1, count_of=0)
    gate = "bits" if case.family == 1 else "gamma"
    K.check_result(oracle_result(case, spec, cut=True), [case], spec, "Partial", helpers, gate=gate)
    if case.family == 1:
        K.check_result(oracle_result(case, spec, cut=False, mode="Final"), [K.primer(case), case], spec, "Final", helpers)


def test_reference_against_the_oracle_with_nine_sums():
    c = K.acc_case()
    for m in K.ACC_M:
        spec = K.agg_spec(m)
        K.check_result(oracle_result(c.with_args(m), spec, cut=True, m=m), [c.with_args(m)], spec, "Partial", helpers)


# ---- values written out by hand ------------------------------------------------------------------------------------------------------

def alternating(values, other=0.125):
    """key 5 holds `values` in single-row runs, rows of key 6 between them"""
    k, x = [], []
    for v in values:
        k += [5, 6]
        x += [v, other]
    return K.Case("by_hand", 2, k, [x])


@pytest.mark.parametrize("r", [3, 16, 17, 40])
def test_fixed_pattern_by_hand(r):
    p = K.fixed_pattern(r)
    assert p[0] == 1.0 and p[1] == 9007199254740992.0 and p[-1] == -4503599627370496.0 and set(p[2:-1]) <= {1.0} and len(p) == r
    c = alternating(p)
    ref = K.reference(c)
    assert ref.run_sums[5][0] == p and ref.rows[5] == r and ref.nonnull[5] == [r]
    # 1 + 2^53 rounds to 2^53 (tie to even), every further 1 is absorbed, - 2^52 is exact
    assert ref.sums[5][0] == 4503599627370496.0
    assert ref.sums[6][0] == 0.125 * r
    # reversed: -2^52 + (r - 3) ones are exact below 2^53, + 2^53 exact, + 1 exact; first run last: 2^52 + 1; last run first:
    # -2^52 + 1 + 2^53 = 2^52 + 1, then r - 3 ones
    assert K.alternative_folds(p) == [4503599627370496.0 + (r - 2), 4503599627370497.0, 4503599627370497.0 + (r - 3)]
    assert K.pins_the_order(p) and not K.pins_the_order([1.0, 2.0, 3.0])


def test_straddling_run_of_eighths_by_hand():
    n = 1040
    k = np.where((np.arange(n) >= 1020) & (np.arange(n) < 1030), 5, 1000 + np.arange(n) % 13)
    x = np.full(n, 0.5)
    x[1020:1030] = np.arange(1, 11) / 8.0
    ok = np.ones(n, np.bool_)
    ok[1021] = False                                            # 2/8 is NULL: + 0.0 inside the first run
    c = K.Case("by_hand", 1, k, [x], [ok])
    assert [r for r in K.runs(c) if r[0] == 5] == [(5, 1020, 1024), (5, 1024, 1030)]
    ref = K.reference(c)
    assert ref.run_sums[5][0] == [1.0, 5.625] and ref.sums[5][0] == 6.625 and ref.rows[5] == 10 and ref.nonnull[5] == [9]
    cols, floats = K.expected([c], K.agg_spec(1), "Final")
    at = list(cols["k"][1]).index(5)
    assert cols["s0"][1][at] == 6.625 and cols["a0"][1][at] == 6.625 / 9 and cols["n"][1][at] == 10 and floats == ["s0", "a0"]


def test_nulls_and_dropped_rows_by_hand():
    k = [5, 5, 6, 6, 5, 7, 7]
    x = [1.5, 2.0, -0.0, 4.0, 8.0, 3.0, 3.0]
    ok = [True, False, False, False, True, True, True]
    keep = [1, 1, 1, 1, 1, 0, 0]
    c = K.Case("by_hand", 1, k, [x], [ok], keep)
    ref = K.reference(c)
    assert ref.keys == [5, 6] and ref.rows == {5: 3, 6: 2} and ref.nonnull == {5: [2], 6: [0]}
    assert ref.run_sums[5][0] == [1.5, 8.0] and ref.sums[5][0] == 9.5 and ref.sums[6][0] is None
    cols, _ = K.expected([c], K.agg_spec(1, count_of=0), "Partial")
    assert list(cols) == ["k", "s0[sum]", "n[count]", "a0[count]", "a0[sum]", "c0[count]"]
    assert list(cols["s0[sum]"][2]) == [True, False] and list(cols["a0[count]"][1]) == [2, 0] and list(cols["n[count]"][1]) == [3, 2]
    # a kept row between two dropped ones is a run of its own; a dropped row cuts a run in two
    c = K.Case("by_hand", 1, [5] * 5, [[1.0, 2.0, 4.0, 8.0, 16.0]], keep=[1, 0, 1, 0, 1])
    assert K.runs(c) == [(5, 0, 1), (5, 2, 3), (5, 4, 5)] and K.reference(c).sums[5][0] == 21.0


def test_gamma_bound_by_hand():
    assert K.gamma_bound(1, Fraction(10)) == 0
    assert K.gamma_bound(3, Fraction(1)) == Fraction(2, 2 ** 53 - 2)
