"""CPU tier of the top-k change: tpch.q3_final / q3_plan take `limit`; with limit=10 the plan ends in q3.sql's `limit 10` as a
GlobalLimitExec over the unchanged sort, and without it the plan is, byte for byte, what it was before the argument existed.
The measurement hook is part of the C ABI and of its Python mirror."""
import ballista_amd as ba
from ballista_amd import _lib as L, tpch
from oracle import gen

import plan_nodes as N
import proto_encode as pe

Q3_DISPLAY = (
    "SortExec: [revenue DESC NULLS FIRST, o_orderdate ASC NULLS FIRST]\n"
    "  ProjectionExec: expr=[l_orderkey as l_orderkey, revenue as revenue, o_orderdate as o_orderdate, o_shippriority as o_shippriority]\n"
    "    HashAggregateExec: mode=Final, gby=[l_orderkey, o_orderdate, o_shippriority], aggr=[SUM(l_orderkey)]\n"
    "      MergeExec\n"
    "        HashAggregateExec: mode=Partial, gby=[l_orderkey, o_orderdate, o_shippriority], aggr=[SUM((l_extendedprice Multiply (1 Minus l_discount)))]\n"
    "          HashJoinExec: mode=CollectLeft, join_type=Inner, on=[(o_orderkey, l_orderkey)]\n"
    "            ProjectionExec: expr=[o_orderkey as o_orderkey, o_orderdate as o_orderdate, o_shippriority as o_shippriority]\n"
    "              HashJoinExec: mode=CollectLeft, join_type=Inner, on=[(c_custkey, o_custkey)]\n"
    "                ProjectionExec: expr=[c_custkey as c_custkey]\n"
    "                  FilterExec: (c_mktsegment Eq 'BUILDING')\n"
    "                    CsvExec: path=mem://customer, delimiter='|', has_header=false, projection=[c_custkey, c_nationkey, c_mktsegment]\n"
    "                FilterExec: (o_orderdate Lt Date32(9204))\n"
    "                  CsvExec: path=mem://orders, delimiter='|', has_header=false, projection=[o_orderkey, o_custkey, o_orderdate, o_shippriority]\n"
    "            ProjectionExec: expr=[l_orderkey as l_orderkey, l_extendedprice as l_extendedprice, l_discount as l_discount]\n"
    "              FilterExec: (l_shipdate Gt Date32(9204))\n"
    "                CsvExec: path=mem://lineitem, delimiter='|', has_header=false, projection=[l_orderkey, l_suppkey, l_quantity, l_extendedprice, l_discount, l_tax, l_returnflag, l_linestatus, l_shipdate]\n"
)


def q3_display(monkeypatch, **kw):
    def leaf(name, batch):
        m = N.MemoryExec([[batch]])
        m.name = "mem://" + name
        return m
    sf = 0.001
    monkeypatch.setattr(tpch, "P", N)       # the plan builders over the GPU-free plan descriptions
    described = tpch.q3_plan(leaf("customer", gen.customer(sf)), leaf("orders", gen.orders(sf)), leaf("lineitem", gen.lineitem(sf)), **kw)
    monkeypatch.undo()
    return ba.ExecutionPlan.from_proto(None, pe.plan(described)).display()


def test_q3_without_a_limit_is_the_plan_it_was(monkeypatch):
    assert q3_display(monkeypatch) == Q3_DISPLAY
    assert q3_display(monkeypatch, limit=None) == Q3_DISPLAY


def test_q3_with_limit_10_puts_a_global_limit_over_the_unchanged_sort(monkeypatch):
    text = q3_display(monkeypatch, limit=10)
    lines = text.splitlines()
    assert lines[0] == "GlobalLimitExec: limit=10"
    assert lines[1] == "  " + Q3_DISPLAY.splitlines()[0]
    assert [l[2:] for l in lines[1:]] == Q3_DISPLAY.splitlines()


def test_sort_limit_form_hook_is_declared_exported_and_mirrored():
    assert "bhip_ctx_sort_limit_form" in L.SYMBOLS
    assert L.lib().bhip_ctx_sort_limit_form(None) == b""             # no context: the empty form, not a crash
    assert callable(ba.Context.sort_limit_form)
