"""CPU tier of NestedLoopJoinExec: the derivation of the expected pairs that the GPU tests compare against (nljoin_cases.pairs: numpy
cross product + the oracle's evaluator) witnessed by a nested loop in plain Python for every predicate of the case table, and the plan
itself (schemas, display, children, partitioning, every plan-time refusal) over leaves decoded from wire plans, without a device."""
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L
from ballista_amd import expr as E
from ballista_amd.expr import col, lit

import helpers
import join_filter_cases as JF
import join_types_cases as JT
import nljoin_cases as NC
import proto_encode as pe

LEFT = [("lk", "Int64", True), ("ls", "Utf8", False), ("la", "Int32", False)]
RIGHT = [("rk", "Int64", False), ("ry", "Float64", True), ("ra", "Int32", False)]
SCHEMA = {n: t for n, t, _ in LEFT + RIGHT}
BAND = E.coerce((col("lk") >= col("rk")).and_(col("la") < col("ra")), SCHEMA)


def children():
    return JF.decoded_leaf("build", LEFT), JF.decoded_leaf("probe", RIGHT)


def two_partitions(cols):
    return ba.ExecutionPlan.from_proto(None, pe.shuffle_reader([("job", 1, 0, "ex", "host", 1), ("job", 1, 1, "ex", "host", 1)], list(cols)))


# ---- the expectation builder against a nested loop --------------------------------------------------------------------------------

@pytest.mark.parametrize("nulls", [False, True])
def test_expected_pairs_agree_with_a_nested_loop(nulls):
    left, right = NC.sides(nulls, 60, 130)
    n_all = 60 * 130
    counts = {}
    for name, (_, py_pred, _) in NC.CASES.items():
        li, ri = JF.nested_loop_pairs(left, right, [], py_pred)
        kli, kri = NC.pairs(left, right, NC.predicate(name, left, right))
        assert list(zip(li, ri)) == list(zip(kli.tolist(), kri.tolist())), name          # the same pairs in the same (probe-major) order
        counts[name] = len(li)
    assert counts["none"] == counts["never"] == 0 and counts["all"] == counts["always"] == n_all
    assert 0 < counts["band"] < n_all // 20                                              # sparse
    for x in NC.POOLS:                                                                   # every operator of every type decides something
        for op in NC.PYOP:
            assert 0 < counts["%s_%s" % (x, op)] < n_all, (x, op)
    if nulls:                                                                            # ... and a NULL is never a partner
        la, ra = left["la"].is_valid(), right["ra"].is_valid()
        kli, kri = NC.pairs(left, right, NC.predicate("a_NotEq", left, right))
        assert la[kli].all() and ra[kri].all() and not la.all() and not ra[63] and not ra[64]


def test_no_filter_is_the_cross_product():
    left, right = NC.sides(True, 7, 5)
    li, ri = NC.pairs(left, right, None)
    assert list(zip(li.tolist(), ri.tolist())) == [(i, j) for j in range(5) for i in range(7)]
    NC.assert_same_rows(NC.expected(JT.ANTI, left, right, None), JT.rows_where(left, [False] * 7))
    NC.assert_same_rows(NC.expected(JT.RIGHT_SEMI, left, right, None), right)


def test_tile_and_chunk_constants_match_the_header():
    assert NC.TILE == ba.plan.NLJ_BUILD_TILE == 1024
    assert NC.TILE % 256 == 0 and NC.TILE % 64 == 0
    assert NC.header_constant("NLJ_MAX_TERMS") == 4 and NC.header_constant("NLJ_BLOCK") == 256
    assert NC.header_constant("NLJ_CHUNK_PAIRS") == 1 << 24


# ---- the plan ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flt", [None, BAND], ids=["cross", "filter"])
@pytest.mark.parametrize("jt", NC.ALL_TYPES)
def test_schema_display_children_and_partitioning(jt, flt):
    l, r = children()
    plan = ba.NestedLoopJoinExec(l, r, jt, filter=flt)
    left_null = jt in (JF.RIGHT, JT.FULL)
    right_null = jt in (JF.LEFT, JT.FULL)
    lf = [(n, t, u or left_null) for n, t, u in LEFT]
    rf = [(n, t, u or right_null) for n, t, u in RIGHT]
    assert plan.schema() == (lf if jt in JF.BUILD_SIDE else rf if jt in JF.PROBE_SIDE else lf + rf)
    text = plan.display().splitlines()
    want = "NestedLoopJoinExec: join_type=%s, filter=%s" % (jt, "None" if flt is None else "((lk GtEq rk) And (la Lt ra))")
    assert text[0] == want
    assert len(text) == 3 and all(t.startswith("  CsvExec: path=mem://") for t in text[1:])
    assert plan.output_partitioning().count == 1 and len(plan.children()) == 2
    again = plan.with_new_children(plan.children())
    assert again.display() == plan.display() and again.schema() == plan.schema()
    for bad in ([l], [l, r, r]):
        with pytest.raises(ba.PlanError, match="NestedLoopJoinExec wrong number of children"):
            plan.with_new_children(bad)


def test_default_arguments_are_the_inner_cross_join():
    l, r = children()
    assert ba.NestedLoopJoinExec(l, r).display() == ba.NestedLoopJoinExec(l, r, JF.INNER, filter=None).display()
    assert ba.NestedLoopJoinExec(l, r).display().startswith("NestedLoopJoinExec: join_type=Inner, filter=None\n")


@pytest.mark.parametrize("jt", NC.ALL_TYPES)
def test_a_right_child_of_two_partitions(jt):
    l = JF.decoded_leaf("build", LEFT)
    two = two_partitions(RIGHT)
    assert two.output_partitioning().count == 2
    for flt in (None, BAND):
        if jt in NC.ONE_PARTITION:
            with pytest.raises(ba.NotImplementedOnGpu, match="%s join over a right child of 2 partitions: put a MergeExec under the right child" % jt):
                ba.NestedLoopJoinExec(l, two, jt, filter=flt)
            assert ba.NestedLoopJoinExec(l, ba.MergeExec(two), jt, filter=flt).output_partitioning().count == 1
        else:
            assert ba.NestedLoopJoinExec(l, two, jt, filter=flt).output_partitioning().count == 2
    # the build side may have any number
    assert ba.NestedLoopJoinExec(two_partitions(LEFT), JF.decoded_leaf("probe", RIGHT), jt).output_partitioning().count == 1


def test_plan_time_errors():
    l, r = children()
    with pytest.raises(ba.PlanError, match="No field named 'nope'"):
        ba.NestedLoopJoinExec(l, r, JF.INNER, filter=col("nope") > lit(1))
    with pytest.raises(ba.PlanError, match="must return boolean values, not Float64"):
        ba.NestedLoopJoinExec(l, r, JF.LEFT, filter=col("ry") + lit(1.0))
    with pytest.raises(ba.NotImplementedOnGpu):                                           # Utf8Lowering's checks apply
        ba.NestedLoopJoinExec(l, r, JT.ANTI, filter=E.BinaryExpr(col("ls"), "Like", lit("a_c" + "x" * 300)))
    for jt in NC.ALL_TYPES:
        with pytest.raises(ba.NotImplementedOnGpu, match="reads no column"):
            ba.NestedLoopJoinExec(l, r, jt, filter=lit(1) < lit(2))
    with pytest.raises(ba.PlanError, match="Unsupported join type"):
        ba.NestedLoopJoinExec(l, r, "Cross")
    h = L.C.c_void_p()
    for bad in (-1, 8):
        assert L.lib().bhip_plan_nested_loop_join(l._h, r._h, bad, None, L.C.byref(h)) == L.ENOTIMPL
        assert b"Unsupported join type" in L.lib().bhip_last_error()


def test_duplicate_names():
    same = [("a", "Int64", False), ("b", "Utf8", True)]
    l, r = JF.decoded_leaf("build", same), JF.decoded_leaf("probe", same)
    for jt in (JF.INNER, JF.LEFT, JF.RIGHT, JT.FULL):
        with pytest.raises(ba.PlanError, match="join output would have two columns named 'a'"):
            ba.NestedLoopJoinExec(l, r, jt)
    for jt in JF.BUILD_SIDE + JF.PROBE_SIDE:
        assert ba.NestedLoopJoinExec(l, r, jt).schema() == same                            # one side only: no clash in the output
        with pytest.raises(ba.PlanError, match="join output would have two columns named 'a'"):
            ba.NestedLoopJoinExec(l, r, jt, filter=col("a") > lit(1))                      # ... but in the filter's schema


def test_header_values_of_the_join_types_the_mirror_uses():
    header = open(helpers.ROOT + "/include/ballista_hip.h").read()
    for name, py in [("INNER", JF.INNER), ("LEFT", JF.LEFT), ("RIGHT", JF.RIGHT), ("FULL", JT.FULL), ("SEMI", JT.SEMI), ("ANTI", JT.ANTI),
                     ("RIGHT_SEMI", JT.RIGHT_SEMI), ("RIGHT_ANTI", JT.RIGHT_ANTI)]:
        assert "BHIP_JOIN_%s = %d" % (name, ba.HashJoinExec._JT[py]) in header
    assert "bhip_plan_nested_loop_join" in L.SYMBOLS and "bhip_ctx_nested_loop_form" in L.SYMBOLS
    assert L.lib().bhip_ctx_nested_loop_form(None) == b""                                   # no context: the empty form, not a crash
    assert callable(ba.Context.nested_loop_form)


def test_hash_join_without_keys_answers_as_before():
    l, r = children()
    h = L.C.c_void_p()
    assert L.lib().bhip_plan_hash_join(l._h, r._h, 0, None, None, 0, L.C.byref(h)) == L.EINVAL
    assert L.lib().bhip_last_error() == b"HashJoinExec needs at least one key pair"
    with pytest.raises(ba.PlanError, match="HashJoinExec needs at least one key pair"):
        ba.HashJoinExec(l, r, [], JF.INNER, filter=BAND)
