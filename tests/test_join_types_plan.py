"""CPU tier of HashJoinExec's Full / Semi / Anti / RightSemi / RightAnti join types: the plans (wire values 3, 4, 5 decode; the two
probe-side forms have no wire value), their output schemas, the partition rule of the build-side answers, and the derivation of
the expected rows that the GPU tests compare against (join_types_cases.expected), witnessed by pyarrow's joins.

Plans are built without a device, as wire plans decoded by bhip_plan_from_proto; the HashJoinExecNode is encoded by hand because
the test encoder knows the three join types of the reference's revision only."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from oracle.engine import OCol

import helpers
import join_types_cases as JT
import plan_nodes as N
import proto_encode as pe

NP = {"Int64": np.int64, "Int32": np.int32, "Date32": np.int32, "Float64": np.float64}


def leaf(name, cols):
    m = N.MemoryExec([[OrderedDict((n, OCol(t, [] if t == "Utf8" else np.zeros(0, NP[t]), np.zeros(0, np.bool_) if u else None)) for n, t, u in cols)]],
                     schema=cols)
    m.name = "mem://" + name
    return m


def join_bytes(left, right, on, wire_jt):
    """PhysicalPlanNode{hash_join = 9}: left = 1, right = 2, on = 3 {left = 1, right = 2}, join_type = 4; left / right: encoded plans"""
    body = pe.f_bytes(1, left) + pe.f_bytes(2, right) + b"".join(pe.f_bytes(3, pe.f_str(1, a) + pe.f_str(2, b)) for a, b in on)
    return pe.f_bytes(9, body + pe.f_varint(4, wire_jt))


def decoded(data):
    return ba.ExecutionPlan.from_proto(None, data)


LEFT = [("lk", "Int64", True), ("ls", "Utf8", False), ("k", "Int32", False)]
RIGHT = [("rk", "Int64", False), ("ry", "Float64", True), ("k", "Int32", False)]
ON = [("lk", "rk"), ("k", "k")]


@pytest.mark.parametrize("jt", [JT.FULL, JT.SEMI, JT.ANTI])
def test_wire_values_3_4_5_decode(jt):
    plan = decoded(join_bytes(pe.plan(leaf("build", LEFT)), pe.plan(leaf("probe", RIGHT)), ON, JT.WIRE[jt]))
    text = plan.display().splitlines()
    assert text[0] == "HashJoinExec: mode=CollectLeft, join_type=%s, on=[(lk, rk), (k, k)]" % jt
    assert len(text) == 3 and all(t.startswith("  CsvExec: path=mem://") for t in text[1:])
    if jt == JT.FULL:       # left fields then right fields, the same-named right key dropped, every field nullable
        want = [(n, t, True) for n, t, _ in LEFT] + [(n, t, True) for n, t, _ in RIGHT if n != "k"]
    else:                   # the left fields, unchanged
        want = LEFT
    assert plan.schema() == want
    assert plan.output_partitioning().count == 1


def test_wire_value_6_is_unknown():
    with pytest.raises(ba.PlanError, match="unknown JoinType 6"):
        decoded(join_bytes(pe.plan(leaf("build", LEFT)), pe.plan(leaf("probe", RIGHT)), ON, 6))


def test_python_names_and_abi_values():
    P = ba.plan
    assert (P.FULL, P.SEMI, P.ANTI, P.RIGHT_SEMI, P.RIGHT_ANTI) == tuple(JT.TYPES)
    assert [P.HashJoinExec._JT[t] for t in (P.INNER, P.LEFT, P.RIGHT, P.FULL, P.SEMI, P.ANTI, P.RIGHT_SEMI, P.RIGHT_ANTI)] == list(range(8))
    header = open(helpers.ROOT + "/include/ballista_hip.h").read()
    for i, name in enumerate(["INNER", "LEFT", "RIGHT", "FULL", "SEMI", "ANTI", "RIGHT_SEMI", "RIGHT_ANTI"]):
        assert "BHIP_JOIN_%s = %d" % (name, i) in header


def test_name_clashes_count_only_in_the_output():
    same = [("a", "Int64", False), ("b", "Utf8", True)]
    sides = pe.plan(leaf("build", same)), pe.plan(leaf("probe", same))
    for jt in (JT.SEMI, JT.ANTI):
        assert decoded(join_bytes(*sides, [("a", "a")], JT.WIRE[jt])).schema() == same
    with pytest.raises(ba.PlanError, match="join output would have two columns named 'b'"):
        decoded(join_bytes(*sides, [("a", "a")], JT.WIRE[JT.FULL]))


@pytest.mark.parametrize("jt", [JT.FULL, JT.SEMI, JT.ANTI])
def test_a_build_side_answer_needs_one_right_partition(jt):
    """a build row's fate depends on every probe row and a stream sees one right partition: two partitions are refused, with the
    way out in the message; a MergeExec in between is the way out; with_new_children keeps the join type"""
    build = pe.plan(leaf("build", LEFT))
    fields = [(n, t, u) for n, t, u in RIGHT]
    two = pe.shuffle_reader([("job", 1, 0, "ex", "host", 1), ("job", 1, 1, "ex", "host", 1)], fields)
    assert decoded(two).output_partitioning().count == 2
    with pytest.raises(ba.NotImplementedOnGpu, match="MergeExec"):
        decoded(join_bytes(build, two, ON, JT.WIRE[jt]))
    merged = pe.f_bytes(14, pe.f_bytes(1, two))
    plan = decoded(join_bytes(build, merged, ON, JT.WIRE[jt]))
    assert plan.children()[1].as_any() == "MergeExec"
    again = plan.with_new_children(plan.children())
    assert again.display() == plan.display() and "join_type=%s" % jt in again.display()
    assert again.schema() == plan.schema()
    # the same node over a right child of two partitions: the rule holds there too
    with pytest.raises(ba.NotImplementedOnGpu, match="MergeExec"):
        plan.with_new_children([plan.children()[0], decoded(two)])


# ---- the expectation builder against pyarrow -------------------------------------------------------------------------------------

def to_arrow(batch):
    import pyarrow as pa
    arrays = []
    for c in batch.values():
        t = {"Utf8": pa.string(), "Int64": pa.int64(), "Int32": pa.int32(), "Date32": pa.int32(), "Float64": pa.float64()}[c.dtype]
        arrays.append(pa.array(c.to_pylist(), type=t))
    return pa.table(arrays, names=list(batch.keys()))


def from_arrow(table, like):
    """a pyarrow table as an oracle batch with the columns (and Arrow type names) of `like`"""
    out = OrderedDict()
    for k, c in like.items():
        col = table.column(k).combine_chunks()
        vals = col.fill_null("" if c.dtype == "Utf8" else 0).to_numpy(zero_copy_only=False)
        out[k] = OCol(c.dtype, list(vals) if c.dtype == "Utf8" else vals, col.is_valid().to_numpy(zero_copy_only=False))
    return out


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("form", JT.FORMS)
def test_expected_rows_agree_with_pyarrow(form, nulls):
    left, right, on = JT.sides(form, nulls)
    lt, rt = to_arrow(left), to_arrow(right)
    for jt in JT.TYPES:
        want = lt.join(rt, keys=[a for a, _ in on], right_keys=[b for _, b in on], join_type=JT.PYARROW[jt], coalesce_keys=False)
        got = JT.expected(jt, left, right, on)
        assert sorted(want.column_names) == sorted(got.keys())
        JT.assert_same_rows(got, from_arrow(want, got))
    # the inputs exercise what they are meant to: both answers occur on both sides
    for jt in JT.TYPES[1:]:
        assert 0 < len(JT.expected(jt, left, right, on)["li" if jt in (JT.SEMI, JT.ANTI) else "ri"].values) < (JT.NL if jt in (JT.SEMI, JT.ANTI) else JT.NR)
