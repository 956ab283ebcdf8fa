#!/usr/bin/env python3
"""CSV scan against the `.tbl` scan and a CPU reader (run on the GPU box): the reference's lineitem fixture lines repeated to
~MB MiB of text (default 1024), all 16 fields, as
  a  `.tbl` text through RecordBatch.from_tbl
  b  the same rows as quote-free comma CSV with a header through RecordBatch.from_csv
  c  the same with every string field quoted

  exp_csv.py                      the whole experiment: every GPU step is a child process under its own time limit, and the first
                                  step that fails ends the run.  Per-kernel times come from `rocprofv3 --kernel-trace --stats` runs
                                  (no counters), three per format, alternating; end-to-end times (text in host memory, copy included)
                                  from unprofiled runs, against pyarrow.csv.read_csv with 16 threads on the text of b.
  exp_csv.py --other-tree DIR     also alternates every format on another built checkout of this repository (e.g. the parent commit)
                                  with this one, and judges this one by the other's own run-to-run spread
  exp_csv.py --out DIR            where the profiler's traces go (default: a fresh temporary directory)
  exp_csv.py scan FORMAT          one child: 4 scans of FORMAT, prints the median end-to-end time as one JSON line
  exp_csv.py cpu                  one child: pyarrow.csv.read_csv on the text of b
"""
import csv, glob, io, json, os, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("BHIP_EXP_TREE", ROOT))       # a child of --other-tree imports that checkout's package and library
MB = int(os.environ.get("MB", 1024))
STRINGS = (8, 9, 13, 14, 15)


def lineitem_schema():
    from ballista_amd import expr as E
    return [("l_orderkey", E.INT32), ("l_partkey", E.INT32), ("l_suppkey", E.INT32), ("l_linenumber", E.INT32),
            ("l_quantity", E.FLOAT64), ("l_extendedprice", E.FLOAT64), ("l_discount", E.FLOAT64), ("l_tax", E.FLOAT64),
            ("l_returnflag", E.UTF8), ("l_linestatus", E.UTF8), ("l_shipdate", E.DATE32), ("l_commitdate", E.DATE32),
            ("l_receiptdate", E.DATE32), ("l_shipinstruct", E.UTF8), ("l_shipmode", E.UTF8), ("l_comment", E.UTF8)]


def make_text(fmt):
    """-> (text, header) with the same rows in every format"""
    unit = open(os.path.join(ROOT, "tests", "golden", "tbl", "lineitem_partition0.tbl"), "rb").read()
    reps = max(1, MB * (1 << 20) // len(unit))
    if fmt == "a":
        return unit * reps, b""
    rows = [ln.split("|")[:-1] for ln in unit.decode().split("\n") if ln]
    assert not any("," in c or '"' in c for r in rows for c in r[:15])
    # the comments of the fixture hold commas: format b has to stay free of quotes, so they become semicolons in b and c alike
    rows = [r[:15] + [r[15].replace(",", ";")] for r in rows]
    if fmt == "c":
        rows = [[('"' + c + '"') if k in STRINGS else c for k, c in enumerate(r)] for r in rows]
    body = "".join(",".join(r) + "\n" for r in rows).encode()
    header = (",".join(n for n, _ in lineitem_schema()) + "\n").encode()
    return header + body * reps, header


def child_scan(fmt):
    import ballista_amd as ba
    schema = lineitem_schema()
    text, _ = make_text(fmt)
    ctx = ba.Context(0)
    ms = []
    for it in range(4):
        ctx.synchronize()
        t0 = time.perf_counter()
        rb = ba.RecordBatch.from_tbl(ctx, text, schema) if fmt == "a" else ba.RecordBatch.from_csv(ctx, text, schema)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms[1:])
    print(json.dumps(dict(format=fmt, text_mib=len(text) / 2 ** 20, rows=rb.num_rows, ms_first=ms[0], ms_median_of_3=med,
                          text_gbs=len(text) / med / 1e6)), flush=True)


def child_cpu():
    import pyarrow as pa, pyarrow.csv as pacsv
    pa.set_cpu_count(16)
    text, _ = make_text("b")
    t = {"Int32": pa.int32(), "Float64": pa.float64(), "Utf8": pa.string(), "Date32": pa.date32()}
    types = {n: t[d] for n, d in lineitem_schema()}
    ms = []
    for it in range(3):
        t0 = time.perf_counter()
        table = pacsv.read_csv(io.BytesIO(text), read_options=pacsv.ReadOptions(use_threads=True),
                               convert_options=pacsv.ConvertOptions(column_types=types))
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(reader="pyarrow.csv.read_csv, 16 threads", text_mib=len(text) / 2 ** 20, rows=table.num_rows,
                          ms_min_of_3=min(ms), text_gbs=len(text) / min(ms) / 1e6)), flush=True)


def step(label, cmd, limit, env=None):
    """one child under its own time limit; a failure ends the experiment (nothing else is started on the GPU)"""
    full = ["timeout", "-k", "10", str(limit)] + cmd
    r = subprocess.run(full, cwd=ROOT, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(f"{label}: exit {r.returncode}\n{r.stdout[-3000:]}", flush=True)
        sys.exit(r.returncode)
    return r.stdout


def kernel_times(out, label, fmt, env=None):
    """-> {kernel: average ms per call} of one profiled child, whose trace goes under out/label"""
    d = os.path.join(out, label)
    step(label, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                 "scan", fmt], 240, env)
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[-1:]:
        for r in csv.DictReader(open(f)):
            name = r["Name"].split("(")[0].replace("bhip::", "").replace("void ", "")
            name = name.replace("tbl_copy_strings", "text_copy_strings").replace("csv_copy_strings", "text_copy_strings")  # a checkout with two copy kernels
            if name.startswith(("tbl_", "csv_", "text_")):
                out[name] = float(r["AverageNs"]) / 1e6
    return out


def main():
    other = os.path.abspath(sys.argv[sys.argv.index("--other-tree") + 1]) if "--other-tree" in sys.argv else None
    out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else tempfile.mkdtemp(prefix="exp_csv_")
    os.makedirs(out, exist_ok=True)
    runs = {}
    order = []
    for k in range(3):                                   # alternating: a, (a on the other build), b, (b ...), c, (c ...) — three times
        for fmt in "abc":
            order += [(f"{fmt}{k}", fmt, None)] + ([(f"{fmt}_other{k}", fmt, {"BHIP_EXP_TREE": other})] if other else [])
    for label, fmt, env in order:
        runs[label] = kernel_times(out, label, fmt, env)
        print(f"{label:9s} " + "  ".join(f"{n} {ms:.3f}" for n, ms in sorted(runs[label].items())) + f"  | sum {sum(runs[label].values()):.3f} ms", flush=True)
    names = lambda p: sorted({n for l, r in runs.items() if l.startswith(p) and l[len(p):].isdigit() for n in r})
    med = lambda p, n: statistics.median(runs[f"{p}{k}"].get(n, 0.0) for k in range(3))
    a_sums = [sum(runs[f"a{k}"].values()) for k in range(3)]
    spread = max(a_sums) - min(a_sums)
    print(f"\nformat a, kernel time per scan (one launch of each; copy_strings per Utf8 column): runs {', '.join('%.3f' % s for s in a_sums)} ms, "
          f"spread {spread:.3f} ms ({100 * spread / statistics.median(a_sums):.1f} %)")
    for p in ("a", "b", "c"):
        print(f"format {p} median of 3: " + "  ".join(f"{n} {med(p, n):.3f}" for n in names(p)) + f"  | sum {sum(med(p, n) for n in names(p)):.3f} ms")
    sa, sb, sc = (sum(med(p, n) for n in names(p)) for p in ("a", "b", "c"))
    print(f"b / a = {sb / sa:.3f} ({sb - sa:+.3f} ms against a spread of {spread:.3f} ms);  c / a = {sc / sa:.3f}")
    for ta, tb in (("tbl_count_kernel", "csv_count_kernel"), ("tbl_starts_kernel", "tbl_starts_kernel"), ("tbl_parse_kernel", "csv_parse_kernel<false>"),
                   ("text_copy_strings_kernel", "text_copy_strings_kernel")):
        print(f"  pass {ta:24s} a {med('a', ta):.3f} ms   b {tb:24s} {med('b', tb):.3f} ms")
    for fmt in "abc" if other else "":                   # the yardstick is the other checkout's own spread, measured in this run
        sums = [sum(runs[f"{fmt}{k}"].values()) for k in range(3)]
        o_sums = [sum(runs[f"{fmt}_other{k}"].values()) for k in range(3)]
        o_spread = max(o_sums) - min(o_sums)
        diff = statistics.median(sums) - statistics.median(o_sums)
        print(f"format {fmt}: this checkout runs {', '.join('%.3f' % s for s in sums)} ms, median {statistics.median(sums):.3f};  the other "
              f"{', '.join('%.3f' % s for s in o_sums)} ms, median {statistics.median(o_sums):.3f}, spread {o_spread:.3f};  this - the other = "
              f"{diff:+.3f} ms: {'within' if diff <= o_spread else 'BEYOND'} the other's spread")
        for n in names(fmt):
            print(f"    {n:28s} this {med(fmt, n):.3f} ms   the other {med(fmt + '_other', n):.3f} ms")
    print("\nend to end, text in host memory (copy included), profiler off:")
    for fmt in ("a", "b", "c"):
        print(step(f"scan {fmt}", [sys.executable, os.path.abspath(__file__), "scan", fmt], 240).strip().splitlines()[-1], flush=True)
    print(step("cpu", [sys.executable, os.path.abspath(__file__), "cpu"], 600).strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "scan":
        child_scan(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "cpu":
        child_cpu()
    else:
        main()
