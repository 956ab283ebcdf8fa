"""CPU tier of HashJoinExec's residual join filter: the derivation of the expected rows that the GPU tests compare against
(join_filter_cases.expected) witnessed by a nested loop in plain Python, guards on the inputs of the main predicate, and the plan
itself (schemas, display, with_new_children, the plan-time errors) over leaves decoded without a device."""
import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd.expr import col, lit

import join_filter_cases as JF
import join_types_cases as JT

LEFT = [("lk", "Int64", True), ("ls", "Utf8", False), ("k", "Int32", False)]
RIGHT = [("rk", "Int64", False), ("ry", "Float64", True), ("k", "Int32", False)]
ON = [("lk", "rk"), ("k", "k")]


# ---- the expectation builder against a nested loop --------------------------------------------------------------------------------

@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("form", JF.FORMS)
def test_expected_rows_agree_with_a_nested_loop(form, nulls):
    left, right, on = JF.sides(form, nulls, 3, 60, 200)
    some_pairs = False
    for name, (_, py_pred) in JF.PREDICATES.items():
        flt = JF.predicate(name, left, right, on)
        li, ri = JF.nested_loop_pairs(left, right, on, py_pred)
        n_cand, kli, kri = JF.kept_pairs(left, right, on, flt)
        assert sorted(zip(li, ri)) == sorted(zip(kli.tolist(), kri.tolist())), name
        assert len(li) == {"never": 0, "always": n_cand}.get(name, len(li))
        some_pairs = some_pairs or 0 < len(li) < n_cand
        for jt in JF.ALL_TYPES:
            JT.assert_same_rows(JF.expected(jt, left, right, on, flt), JF.from_pairs(jt, left, right, on, li, ri))
    assert some_pairs


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("form", ["int64_unique", "int64_dup", "hot_key"])
def test_the_main_predicate_keeps_about_half_and_strands_rows_of_both_sides(form, nulls):
    """guards: a later change of the inputs must not turn the filter tests into unfiltered ones"""
    left, right, on = JF.sides(form, nulls)
    inner = JT.oracle_join(left, right, on, JF.INNER)
    n_cand, kli, kri = JF.kept_pairs(left, right, on, JF.predicate("two_sided", left, right, on))
    share = len(kli) / n_cand
    cand_l, cand_r = np.unique(inner["li"].values), np.unique(inner["ri"].values)
    lost_l, lost_r = len(np.setdiff1d(cand_l, kli)), len(np.setdiff1d(cand_r, kri))
    print(form, nulls, "candidates", n_cand, "kept share %.3f" % share, "build rows losing all", lost_l, "probe rows losing all", lost_r)
    assert 0.3 <= share <= 0.7
    assert lost_l >= 20 and lost_r >= 200


# ---- the plan ------------------------------------------------------------------------------------------------------------------------

def children():
    return JF.decoded_leaf("build", LEFT), JF.decoded_leaf("probe", RIGHT)


INNER_SCHEMA = {"lk": "Int64", "ls": "Utf8", "k": "Int32", "rk": "Int64", "ry": "Float64"}
FILTER = E.coerce((col("ry") > lit(1.5)).and_(col("ls") < lit("x")), INNER_SCHEMA)


@pytest.mark.parametrize("jt", JF.ALL_TYPES)
def test_schema_display_and_with_new_children(jt):
    l, r = children()
    plain = ba.HashJoinExec(l, r, ON, jt)
    none = ba.HashJoinExec(l, r, ON, jt, filter=None)
    filtered = ba.HashJoinExec(l, r, ON, jt, filter=FILTER)
    assert filtered.schema() == plain.schema() == none.schema()
    head = "HashJoinExec: mode=CollectLeft, join_type=%s, on=[(lk, rk), (k, k)]" % jt
    assert plain.display().splitlines()[0] == head                      # byte for byte what it was
    assert none.display() == plain.display()
    first = filtered.display().splitlines()[0]
    assert first.startswith(head + ", filter=") and "ry" in first and "ls" in first
    assert filtered.display().splitlines()[1:] == plain.display().splitlines()[1:]
    again = filtered.with_new_children(filtered.children())
    assert again.display() == filtered.display() and again.schema() == filtered.schema()
    assert plain.with_new_children(plain.children()).display() == plain.display()


def test_plan_time_errors():
    l, r = children()
    with pytest.raises(ba.PlanError, match="No field named 'nope'"):
        ba.HashJoinExec(l, r, ON, JF.INNER, filter=col("nope") > lit(1))
    # the right key `k` is dropped from the filter's schema (its name means the left column); the right-only `rk` is there
    ba.HashJoinExec(l, r, ON, JT.SEMI, filter=E.coerce(col("k") < col("rk"), INNER_SCHEMA))
    with pytest.raises(ba.PlanError, match="must return boolean values, not Float64"):      # PlanError: BHIP_EINVAL
        ba.HashJoinExec(l, r, ON, JF.LEFT, filter=col("ry") + lit(1.0))
    with pytest.raises(ba.NotImplementedOnGpu):
        ba.HashJoinExec(l, r, ON, JT.ANTI, filter=E.BinaryExpr(col("ls"), "Like", lit("a_c" + "x" * 300)))
    # a filter that reads no column has no batch to run over: refused, for every type
    for jt in JF.ALL_TYPES:
        with pytest.raises(ba.NotImplementedOnGpu, match="reads no column"):
            ba.HashJoinExec(l, r, ON, jt, filter=lit(1) < lit(2))


@pytest.mark.parametrize("jt", [JT.SEMI, JT.ANTI, JT.RIGHT_SEMI, JT.RIGHT_ANTI])
def test_a_clashing_name_counts_for_the_filter_schema_of_an_existence_join(jt):
    same = [("a", "Int64", False), ("b", "Utf8", True)]
    l, r = JF.decoded_leaf("build", same), JF.decoded_leaf("probe", same)
    assert ba.HashJoinExec(l, r, [("a", "a")], jt).schema() == same                  # without a filter: as before
    with pytest.raises(ba.PlanError, match="join output would have two columns named 'b'"):
        ba.HashJoinExec(l, r, [("a", "a")], jt, filter=col("a") > lit(1))
