"""CPU tier of the wide-key join: a HashJoinExec whose key layout does not fit the 16-byte packed key is a plan like any other
(it used to be refused at plan time), the plan errors that have nothing to do with key width stay, and the introspection hook is
part of the C ABI and of its Python mirror.  Plans are built without a device, as wire plans decoded by bhip_plan_from_proto —
the decoder, `with_new_children` and the Python constructor all go through the one C++ constructor."""
from collections import OrderedDict

import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L
from oracle.engine import OCol

import plan_nodes as N
import proto_encode as pe


def leaf(name, cols):
    m = N.MemoryExec([[OrderedDict((n, OCol(t, [] if t == "Utf8" else np.zeros(0, {"Int64": np.int64, "Int32": np.int32, "Date32": np.int32,
                                                                                   "Float64": np.float64}[t]))) for n, t in cols)]])
    m.name = "mem://" + name
    return m


def decoded(join):
    return ba.ExecutionPlan.from_proto(None, pe.plan(join))


LAYOUTS = {
    "three_int64": [("a", "Int64"), ("b", "Int64"), ("c", "Int64")],
    "two_utf8_beside_int64s": [("a", "Int64"), ("s", "Utf8"), ("b", "Int32"), ("t", "Utf8"), ("d", "Date32")],      # 16 fixed bytes: nothing left for the strings
    "int32_date32_int64_utf8": [("a", "Int32"), ("d", "Date32"), ("b", "Int64"), ("s", "Utf8")],
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("jt", [N.INNER, N.LEFT, N.RIGHT])
def test_a_join_on_keys_wider_than_the_packed_key_is_a_plan(layout, jt):
    keys = LAYOUTS[layout]
    left = leaf("build", [("l_" + n, t) for n, t in keys] + [("lx", "Float64")])
    right = leaf("probe", [("r_" + n, t) for n, t in keys] + [("ry", "Int64")])
    on = [("l_" + n, "r_" + n) for n, _ in keys]
    plan = decoded(N.HashJoinExec(left, right, on, jt))
    text = plan.display().splitlines()
    assert text[0] == "HashJoinExec: mode=CollectLeft, join_type=%s, on=[%s]" % (jt, ", ".join("(%s, %s)" % p for p in on))
    assert len(text) == 3 and all(t.startswith("  CsvExec: path=mem://") for t in text[1:])
    # left fields then right fields, the side an outer join may leave without a partner nullable
    want = [("l_" + n, t, jt == N.RIGHT) for n, t in keys] + [("lx", "Float64", jt == N.RIGHT)]
    want += [("r_" + n, t, jt == N.LEFT) for n, t in keys] + [("ry", "Int64", jt == N.LEFT)]
    assert plan.schema() == want


def test_two_utf8_keys_alone_still_fit_and_construct():
    left, right = leaf("build", [("ls", "Utf8"), ("lt", "Utf8")]), leaf("probe", [("rs", "Utf8"), ("rt", "Utf8")])
    plan = decoded(N.HashJoinExec(left, right, [("ls", "rs"), ("lt", "rt")], N.INNER))
    assert [n for n, _, _ in plan.schema()] == ["ls", "lt", "rs", "rt"]


def test_plan_errors_that_are_not_about_key_width_stay():
    left = leaf("build", [("a", "Int64"), ("b", "Int64"), ("c", "Int64")])
    right = leaf("probe", [("x", "Int64"), ("y", "Int64"), ("z", "Int32")])
    with pytest.raises(ba.PlanError, match="different types"):
        decoded(N.HashJoinExec(left, right, [("a", "x"), ("b", "y"), ("c", "z")], N.INNER))
    with pytest.raises(ba.PlanError, match="does not have column"):
        decoded(N.HashJoinExec(left, right, [("a", "x"), ("b", "y"), ("c", "nope")], N.INNER))
    # more key columns than a key program holds: refused at plan time, as the wide-key aggregate refuses them
    many = [("k%d" % i, "Int64") for i in range(9)]
    with pytest.raises(ba.NotImplementedOnGpu, match="more than 8 key columns"):
        decoded(N.HashJoinExec(leaf("build", many), leaf("probe", [("r" + n, t) for n, t in many]), [(n, "r" + n) for n, _ in many], N.INNER))


def test_join_key_form_hook_is_declared_exported_and_mirrored():
    assert "bhip_ctx_join_key_form" in L.SYMBOLS
    assert L.lib().bhip_ctx_join_key_form(None) == b""               # no context: the empty form, not a crash
    assert callable(ba.Context.join_key_form)
