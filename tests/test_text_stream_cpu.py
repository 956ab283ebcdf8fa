"""The text scan leaf (ballista_amd.CsvExec, bhip_plan_text_scan) where no device is needed: the argument checks the Python
class makes before it reaches the library, and the wire plan's CSV leaf decoded without a context."""
import os

import pytest

import ballista_amd as ba
from ballista_amd import expr as E
from ballista_amd._lib import PlanError

import helpers
import proto_encode as pe

SCHEMA = [("a", E.INT32, True), ("s", E.UTF8, False)]


@pytest.mark.parametrize("delimiter", [",,", "", b"ab"])
def test_csv_exec_refuses_a_delimiter_that_is_not_one_byte(delimiter):
    with pytest.raises(PlanError, match="one byte"):
        ba.CsvExec(None, ["x.csv"], SCHEMA, delimiter=delimiter)


@pytest.mark.parametrize("slab_bytes", [1000, 3 << 30, (16 << 10) + 512, 8 << 10, -(16 << 10), (2 << 30) + (16 << 10)])
def test_csv_exec_refuses_a_slab_size_outside_its_range(slab_bytes):
    with pytest.raises(PlanError, match="multiple of 16 KiB between 16 KiB and 2 GiB"):
        ba.CsvExec(None, ["x.csv"], SCHEMA, slab_bytes=slab_bytes)


def test_csv_exec_refuses_an_empty_file_list():
    with pytest.raises(PlanError, match="without a file"):
        ba.CsvExec(None, [], SCHEMA)


def test_text_scan_symbol_is_bound():
    from ballista_amd import _lib
    assert "bhip_plan_text_scan" in _lib.SYMBOLS
    assert [f[0] for f in _lib.TextScanOpts._fields_] == ["format", "csv", "slab_bytes"]


@pytest.mark.parametrize("delimiter,has_header", [("|", False), (",", True), (";", False)])
def test_csv_leaf_of_the_wire_plan_without_a_context_describes_the_device_scan(delimiter, has_header):
    tbl = os.path.join(helpers.GOLDEN, "tbl")
    fields = [("n_nationkey", "Int32", False), ("n_name", "Utf8", False), ("n_regionkey", "Int32", False), ("n_comment", "Utf8", False)]
    body = (pe.f_str(1, tbl) + pe.f_packed(2, [1, 0]) + pe.f_bytes(3, pe.schema(fields)) + pe.f_str(4, ".tbl") +
            pe.f_varint(5, 1 if has_header else 0) + pe.f_varint(6, 32768) + pe.f_str(7, delimiter) +
            pe.f_str(8, os.path.join(tbl, "nation_nation.tbl")))
    plan = ba.ExecutionPlan.from_proto(None, pe.f_bytes(2, body))
    assert plan.as_any() == "CsvExec" and plan.output_partitioning().partition_count() == 1
    assert [n for n, _, _ in plan.schema()] == ["n_name", "n_nationkey"]
    text = plan.display()
    assert text.startswith("CsvExec: path=" + tbl) and f"delimiter='{delimiter}'" in text and "device scan" in text
    assert "projection=[n_name, n_nationkey]" in text and "files=1" in text
    assert "batch_size is not used" in text                 # batches are cut by bytes of text, one per slab
    if not (delimiter == "|" and not has_header):
        assert ("has_header=true" if has_header else "has_header=false") in text
    with pytest.raises(ba.ExecutionError, match="no device context"):
        plan.execute(0)
