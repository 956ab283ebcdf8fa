"""ParquetExec on the files of tests/parquet_files.py: the page, run and NULL edges pyarrow's default writer never produces (pages that
end inside a validity word, concatenated Boolean pages, dictionary fallback with NULLs, REQUIRED fields, empty and all-NULL pages,
index widths up to 32 bits, hand-written run tables, the legacy dictionary encoding id, uncompressed V2 pages in a Snappy chunk,
float specials, strings around the take kernels' staging area).  The expected value is pyarrow's read of the same file; every
comparison is exact — floats by bit pattern.  tests/test_parquet_decode_cpu.py pins the host half of the same cases without a GPU;
what is left for this tier is the device half: pq_expand_runs, pq_scatter_valid, narrow_i32, the take kernels, copy_bits and
rebase_offsets of concat_batches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

import parquet_files as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_back(ctx, paths, **kw):
    import ballista_amd as ba
    plan = ba.ParquetExec(paths, ctx, **kw)
    return [b.to_pyarrow() for p in range(plan.output_partitioning().partition_count()) for b in plan.execute(p)]


def expected(paths, projection=None):
    """pyarrow's read of the files, in file order, and the row count of every non-empty row group"""
    tables, rows = [], []
    for p in paths:
        f = pq.ParquetFile(p)
        t = pq.read_table(p)
        tables.append(t.select([t.schema.names[i] for i in projection]) if projection else t)
        rows += [f.metadata.row_group(g).num_rows for g in range(f.metadata.num_row_groups) if f.metadata.row_group(g).num_rows]
    return pa.concat_tables(tables), rows


def same(batches, want, rows):
    assert [b.num_rows for b in batches] == rows                 # one batch per row group, in file order
    got = pa.Table.from_batches(batches)
    assert got.schema.names == want.schema.names
    for name in want.schema.names:
        g, w = got[name].combine_chunks(), want[name].combine_chunks()
        valid = w.is_valid().to_numpy(zero_copy_only=False)
        assert np.array_equal(g.is_valid().to_numpy(zero_copy_only=False), valid), name
        if pa.types.is_floating(w.type):
            assert g.type == w.type, name
            u = np.uint64 if w.type == pa.float64() else np.uint32
            gb, wb = (a.to_numpy(zero_copy_only=False).view(u)[valid] for a in (g, w))
            assert np.array_equal(gb, wb), (name, [(hex(a), hex(b)) for a, b in zip(gb, wb) if a != b][:5])
        elif pa.types.is_string(w.type):
            assert g.cast(pa.binary()).equals(w.cast(pa.binary())), name
        else:
            assert g.cast(w.type).equals(w), name


@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_scan_equals_pyarrow(ctx, tmp_path, case):
    _, write, kw = case
    paths = write(str(tmp_path))                                  # asserts the case's structural precondition
    want, rows = expected(paths, kw.get("projection"))
    same(read_back(ctx, paths, **kw), want, rows)


@pytest.mark.parametrize("case", P.VALIDITY_CASES, ids=[c[0] for c in P.VALIDITY_CASES])
def test_valid_counts_below_the_arrow_export(ctx, tmp_path, case):
    """COUNT(col) and a `col IS NOT NULL` filter read the device validity words themselves: a stray bit behind a piece's length or a bit a
    partial-word copy_bits lost shows here even where the Arrow export would hide it"""
    import ballista_amd as ba
    from ballista_amd import expr as E
    from ballista_amd.expr import col
    _, write, kw = case
    paths = write(str(tmp_path))
    want, _ = expected(paths)
    names = want.schema.names
    valid = {n: len(want) - want[n].null_count for n in names}
    agg = ba.HashAggregateExec(ba.plan.PARTIAL, [], [E.Count(col(n), n) for n in names], ba.ParquetExec(paths, ctx))
    parts = [b.to_pydict() for b in agg.collect()]
    assert {n: sum(p[n + "[count]"][0] for p in parts) for n in names} == valid
    for i, n in enumerate(names):
        flt = ba.FilterExec(E.IsNotNullExpr(col(n)), ba.ParquetExec(paths, ctx, projection=[i]))
        assert sum(b.num_rows for b in flt.collect()) == valid[n], n


def test_page_at_a_time_routes_in_a_child_process(tmp_path):
    """BHIP_PARQUET_PER_PAGE is read once per process: one fresh child reads the NULL-free files the staged routes otherwise take
    (unaligned_pages without NULLs, required_fields, hand_staging) page by page; its batches, written as Arrow IPC files, must equal pyarrow"""
    manifest = []
    for name, write, kw in P.PER_PAGE_CASES:
        d = tmp_path / name
        d.mkdir()
        manifest.append(dict(name=name, paths=write(str(d)), out=str(d / "got.arrow")))
    (tmp_path / "manifest.json").write_text(json.dumps(manifest))
    env = dict(os.environ, BHIP_PARQUET_PER_PAGE="1", PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path / "manifest.json")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, f"child ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    for m in manifest:
        want, rows = expected(m["paths"])
        with pa.OSFile(m["out"], "rb") as f:
            same(pa.ipc.open_file(f).read_all().to_batches(), want, rows)


if __name__ == "__main__":                                            # the child of test_page_at_a_time_routes_in_a_child_process
    import ballista_amd as ba
    assert os.environ.get("BHIP_PARQUET_PER_PAGE") == "1"
    context = ba.Context(0)
    for m in json.load(open(sys.argv[1])):
        got = read_back(context, m["paths"])
        with pa.OSFile(m["out"], "wb") as sink, pa.ipc.new_file(sink, got[0].schema) as w:
            for b in got:
                w.write_batch(b)
        print("read", m["name"], flush=True)
