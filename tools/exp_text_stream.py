#!/usr/bin/env python3
"""The streamed text scan leaf against the whole-file leaf of another build (run on the GPU box): the reference's lineitem
fixture lines repeated to a `.tbl` file of MB MiB (default 2048), read once so that it sits in the page cache, all 16 fields,
scanned through the wire plan's CsvScanExecNode with no resolver and drained.

  exp_text_stream.py                    the whole experiment: every GPU step is a child process under its own time limit, and the
                                        first step that fails ends the run.  Three alternating rounds of: the other checkout (if
                                        given), then this one with BHIP_TEXT_SLAB_MB = 64, 256 and 1024; medians of the end-to-end
                                        time and the text rate per configuration; then one `rocprofv3 --kernel-trace
                                        --memory-copy-trace --stats` run (no counters) of the 256 MiB case: per-kernel times,
                                        whether the copy of slab k + 1 overlaps the kernels of slab k, the largest idle gap
                                        between the kernels of two slabs.
  exp_text_stream.py --other-tree DIR   a built checkout of the parent commit (whole file as one batch) to alternate with
  exp_text_stream.py --out DIR          where the file and the profiler's traces go (default: a fresh temporary directory)
  exp_text_stream.py scan FILE          one child: 3 scans of FILE, one JSON line (first scan, median of the other two)
"""
import csv, glob, json, os, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))                 # proto_encode: the wire plan's encoder
sys.path.insert(0, os.environ.get("BHIP_EXP_TREE", ROOT))       # a child of --other-tree imports that checkout's package and library
MB = int(os.environ.get("MB", 2048))
FIELDS = [("l_orderkey", "Int32"), ("l_partkey", "Int32"), ("l_suppkey", "Int32"), ("l_linenumber", "Int32"), ("l_quantity", "Float64"),
          ("l_extendedprice", "Float64"), ("l_discount", "Float64"), ("l_tax", "Float64"), ("l_returnflag", "Utf8"), ("l_linestatus", "Utf8"),
          ("l_shipdate", "Date32"), ("l_commitdate", "Date32"), ("l_receiptdate", "Date32"), ("l_shipinstruct", "Utf8"),
          ("l_shipmode", "Utf8"), ("l_comment", "Utf8")]


def write_file(path):
    unit = open(os.path.join(ROOT, "tests", "golden", "tbl", "lineitem_partition0.tbl"), "rb").read()
    block = unit * 4096
    with open(path, "wb") as f:
        for _ in range(max(1, MB * (1 << 20) // len(block))):
            f.write(block)
    with open(path, "rb") as f:                                  # once through: the page cache holds it
        while f.read(1 << 26):
            pass
    return os.path.getsize(path)


def child_scan(path):
    import ballista_amd as ba
    import proto_encode as pe
    body = (pe.f_str(1, path) + pe.f_bytes(3, pe.schema([(n, t, False) for n, t in FIELDS])) + pe.f_str(4, ".tbl") + pe.f_varint(6, 32768) +
            pe.f_str(7, "|") + pe.f_str(8, path))
    ctx = ba.Context(0)
    plan = ba.ExecutionPlan.from_proto(ctx, pe.f_bytes(2, body))
    n_bytes = os.path.getsize(path)
    ms = []
    for it in range(3):
        ctx.synchronize()
        t0 = time.perf_counter()
        stats = plan.execute(0).drain()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms[1:])
    print(json.dumps(dict(tree=os.environ.get("BHIP_EXP_TREE", ROOT), slab_mb=os.environ.get("BHIP_TEXT_SLAB_MB"), text_mib=n_bytes / 2 ** 20,
                          rows=stats["num_rows"], batches=stats["num_batches"], ms_first=ms[0], ms=med, text_gbs=n_bytes / med / 1e6,
                          peak_mib=ctx.memory()[1] / 2 ** 20)), flush=True)


def step(label, cmd, limit, env=None):
    """one child under its own time limit; a failure ends the experiment (nothing else is started on the GPU)"""
    full = ["timeout", "-k", "10", str(limit)] + cmd
    e = {k: v for k, v in os.environ.items() if k != "BHIP_TEXT_SLAB_MB"}
    r = subprocess.run(full, cwd=ROOT, env=dict(e, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(f"{label}: exit {r.returncode}\n{r.stdout[-3000:]}", flush=True)
        sys.exit(r.returncode)
    return r.stdout


def trace_report(d, n_bytes):
    """what the profiled run of the 256 MiB case shows: per-kernel averages, copy / kernel overlap, idle gaps between slabs"""
    def rows(pattern):
        files = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
        return list(csv.DictReader(open(files[-1]))) if files else []
    for r in rows("*kernel_stats.csv"):
        name = r["Name"].split("(")[0].replace("bhip::", "").replace("void ", "")
        if name.startswith(("tbl_", "csv_")):
            print(f"  {name:28s} calls {r['Calls']:>4s}  average {float(r['AverageNs']) / 1e6:8.3f} ms  total {float(r['TotalDurationNs']) / 1e6:9.3f} ms")
    kernels = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows("*kernel_trace.csv")))
    copies = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Direction", "")) for r in rows("*memory_copy_trace.csv")))
    big = [c for c in copies if "HOST_TO_DEVICE" in c[2].upper() and c[1] - c[0] > 1_000_000]          # the slabs: > 1 ms each
    text = [k for k in kernels if "tbl_" in k[2]]
    firsts = [i for i, k in enumerate(text) if "tbl_count_kernel" in k[2]]
    n_slabs = -(-n_bytes // (256 << 20))
    firsts = firsts[-n_slabs:]                                    # the last scan of the child
    big = big[-n_slabs:]
    if not firsts or not big:
        print("  (no kernel / copy trace found)")
        return
    overlapped = sum(1 for c in big if any(k[0] < c[1] and c[0] < k[1] for k in text))
    print(f"  slab copies (host to device, last scan): {len(big)}, average {statistics.mean(c[1] - c[0] for c in big) / 1e6:.2f} ms; "
          f"{overlapped} of them overlap a tbl_* kernel")
    gaps = [(text[i][0] - text[i - 1][1]) / 1e6 for i in firsts[1:]]
    busy = [(text[(firsts[j + 1] if j + 1 < len(firsts) else len(text)) - 1][1] - text[i][0]) / 1e6 for j, i in enumerate(firsts)]
    print(f"  kernels of one slab, first start to last end: median {statistics.median(busy):.2f} ms")
    print(f"  idle on the task's stream between the last kernel of slab k and the first of slab k + 1: "
          f"median {statistics.median(gaps):.2f} ms, largest {max(gaps):.2f} ms")


def main():
    other = os.path.abspath(sys.argv[sys.argv.index("--other-tree") + 1]) if "--other-tree" in sys.argv else None
    out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else tempfile.mkdtemp(prefix="exp_text_stream_")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "lineitem.tbl")
    n_bytes = write_file(path)
    print(f"{path}: {n_bytes / 2 ** 20:.0f} MiB", flush=True)
    configs = ([("other", {"BHIP_EXP_TREE": other})] if other else []) + [(f"slab{mb}", {"BHIP_TEXT_SLAB_MB": str(mb)}) for mb in (64, 256, 1024)]
    runs = {label: [] for label, _ in configs}
    me = [sys.executable, os.path.abspath(__file__), "scan", path]
    for k in range(3):                                            # alternating rounds
        for label, env in configs:
            line = step(f"{label} round {k}", me, 600, env).strip().splitlines()[-1]
            runs[label].append(json.loads(line))
            print(f"round {k} {label:8s} {line}", flush=True)
    print()
    for label, _ in configs:
        ms = [r["ms"] for r in runs[label]]
        print(f"{label:8s} end to end median {statistics.median(ms):9.1f} ms (runs {', '.join('%.1f' % m for m in ms)}; spread {max(ms) - min(ms):.1f} ms)  "
              f"{n_bytes / statistics.median(ms) / 1e6:6.2f} GB/s of text  first scan of a process {statistics.median(r['ms_first'] for r in runs[label]):.1f} ms  "
              f"batches {runs[label][0]['batches']}  peak {runs[label][0]['peak_mib']:.0f} MiB")
    d = os.path.join(out, "trace256")
    step("trace", ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me, 900,
         {"BHIP_TEXT_SLAB_MB": "256"})
    print("\nrocprofv3 --kernel-trace --memory-copy-trace --stats, BHIP_TEXT_SLAB_MB=256:")
    trace_report(d, n_bytes)
    os.remove(path)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "scan":
        child_scan(sys.argv[2])
    else:
        main()
