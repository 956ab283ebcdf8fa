#!/usr/bin/env python3
"""HashJoinExec with a residual join filter at size, and the unfiltered joins beside the parent commit (run on the GPU box; seeded
inputs made here; PARENT_TREE=path names a checkout of the parent commit with its library built — the binding resolves every symbol
of its own header, so the parent's library runs under the parent's package; what needs it is skipped without it).

  1. unfiltered     bench.py --query q3 / q5 (SF100, 20 steps, 3 warm-up, no CPU baseline) on this build and on the parent's,
                    alternating, BENCH_ROUNDS runs each: ms per step of every run, the median and the spread (max - min) per build.
                    The bar: the medians differ by no more than the spread of the parent's own runs.
  2. Inner          HashJoinExec(Inner, filter) on this build against FilterExec over HashJoinExec(Inner) on the parent's (and on
                    this build): 1 M build rows, two per key, 16 M probe rows in four batches with keys drawn from 1.25 x the build's
                    key range; filter lx * 8000.0 > ry, about half of the candidates pass.  Every output column is gathered.
  3. Semi, Left     the same inputs and filter; no parent equivalent exists: a baseline for later work.  rows/s are probe rows.

Every variant of parts 2 / 3 runs in a child process of its own under `timeout` (a failed child ends the script): inputs resident on
the device, one warm-up run, then RUNS timed runs of a fresh plan (construction + collect, the build side built in every run).  The
variants alternate within a round, ROUNDS rounds; printed per variant: the median of all its timed runs with min .. max and the rows
that came out.  A last pass with BHIP_KERNEL_TIMING=1 lists the kernels of one run of each variant of this build.
  tools/exp_join_filter.py > profiles/join_filter.txt      PARTS=1,2,3 BUILD_ROWS PROBE_ROWS RUNS=10 ROUNDS=1 BENCH_ROUNDS=3 override"""
import json, os, statistics, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("BHIP_TREE") or HERE              # the tree whose package and library a child runs (this one, or the parent's)
sys.path.insert(0, ROOT)

# (name, build): the plans of parts 2 and 3
VARIANTS = {
    2: [("inner_then_FilterExec", "parent"), ("inner_then_FilterExec", "this"), ("Inner_filter", "this"), ("Inner_unfiltered", "this")],
    3: [("Semi_filter", "this"), ("Left_filter", "this")],
}


def child(name):
    import numpy as np
    import ballista_amd as ba
    from ballista_amd import expr as E
    from ballista_amd.expr import col, lit
    nb, npr = int(os.environ.get("BUILD_ROWS", 1_000_000)), int(os.environ.get("PROBE_ROWS", 16_000_000))
    runs = int(os.environ.get("RUNS", 10))
    rng = np.random.default_rng(31)
    n_keys = nb // 2
    lk = (rng.permutation(nb) // 2).astype(np.int64)
    rk = rng.integers(0, n_keys + n_keys // 4, npr).astype(np.int64)
    ctx = ba.Context(0)
    left = ba.RecordBatch.from_columns(ctx, [("lk", "Int64", lk, None), ("lx", "Float64", rng.integers(0, 1000, nb) / 8.0, None),
                                             ("li", "Int64", np.arange(nb, dtype=np.int64), None)])
    ry = rng.integers(0, 10 ** 6, npr).astype(np.int64)
    cut = (npr + 3) // 4
    right = [ba.RecordBatch.from_columns(ctx, [("rk", "Int64", rk[lo:lo + cut], None), ("ry", "Int64", ry[lo:lo + cut], None),
                                               ("ri", "Int64", np.arange(lo, min(lo + cut, npr), dtype=np.int64), None)])
             for lo in range(0, npr, cut)]
    schema = {"lk": "Int64", "lx": "Float64", "li": "Int64", "rk": "Int64", "ry": "Int64", "ri": "Int64"}
    pred = E.coerce(col("lx") * lit(8000.0) > col("ry"), schema)
    sides = lambda: (ba.MemoryExec([[left]], ctx), ba.MemoryExec([right], ctx))
    on = [("lk", "rk")]
    if name == "inner_then_FilterExec":
        make = lambda: ba.FilterExec(pred, ba.HashJoinExec(*sides(), on, "Inner"))
    elif name == "Inner_unfiltered":
        make = lambda: ba.HashJoinExec(*sides(), on, "Inner")
    else:
        make = lambda: ba.HashJoinExec(*sides(), on, name.split("_")[0], filter=pred)
    ctx.synchronize()
    ms, rows = [], 0
    for it in range(runs + 1):                          # the first run warms the allocator and the code objects
        plan = make()
        ctx.synchronize()
        if it == 1 and os.environ.get("BHIP_KERNEL_TIMING"):
            ctx.kernel_stats(reset=True)
        t0 = time.perf_counter()
        out = plan.collect()
        ctx.synchronize()
        if it:
            ms.append((time.perf_counter() - t0) * 1e3)
        rows = sum(b.num_rows for b in out)
        del out, plan
    res = dict(name=name, form=ctx.join_key_form(), ms=[round(x, 3) for x in ms], rows_out=rows, probe_rows=npr)
    if os.environ.get("BHIP_KERNEL_TIMING"):
        ks = sorted(ctx.kernel_stats().items(), key=lambda kv: -kv[1][0])[:12]
        res["kernel_ms_launches"] = {k: (round(v[0] / runs, 3), v[1] // runs) for k, v in ks}
    print(json.dumps(res), flush=True)


def run(cmd, lib, env_extra, what):
    tree = os.path.abspath(os.environ["PARENT_TREE"]) if lib == "parent" else HERE
    env = dict(os.environ, BHIP_TREE=tree, **env_extra)
    p = subprocess.run(["timeout", "-k", "10", os.environ.get("STEP_TIMEOUT", "240")] + cmd, env=env, stdout=subprocess.PIPE, text=True, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"{what} ({lib} build) ended with status {p.returncode}: stopping")
    return json.loads(p.stdout.strip().splitlines()[-1])


def spread(xs):
    return max(xs) - min(xs)


def bench_part(have_parent):
    rounds = int(os.environ.get("BENCH_ROUNDS", 3))
    builds = (["parent"] if have_parent else []) + ["this"]
    print("part 1 (unfiltered joins: bench.py --gpus 1 --query Q --steps 20 --warmup 3 --no-cpu-baseline, ms per step; %d alternating runs per build)" % rounds)
    for q in ("q3", "q5"):
        ms = {b: [] for b in builds}
        for _ in range(rounds):
            for b in builds:
                r = run([sys.executable, "bench.py", "--gpus", "1", "--query", q, "--steps", "20", "--warmup", "3", "--no-cpu-baseline"], b, {}, "bench " + q)
                ms[b].append(r["ms_per_step"])
        for b in builds:
            print("  %s %-6s build  median %7.3f ms  spread %6.3f ms  runs %s" % (q, b, statistics.median(ms[b]), spread(ms[b]), " ".join("%.3f" % x for x in ms[b])), flush=True)
        if have_parent:
            d = statistics.median(ms["this"]) - statistics.median(ms["parent"])
            print("  %s this - parent = %+.3f ms against the parent's own spread of %.3f ms: %s" % (q, d, spread(ms["parent"]), "within" if abs(d) <= spread(ms["parent"]) else "OUTSIDE"), flush=True)


def join_part(part, have_parent):
    rounds = int(os.environ.get("ROUNDS", 1))
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    variants = [v for v in VARIANTS[part] if v[1] == "this" or have_parent]
    ms, info = {v: [] for v in variants}, {}
    for _ in range(rounds):                             # the variants alternate: a drift of the machine hits all of them alike
        for v in variants:
            r = run(me + [v[0]], v[1], {}, v[0])
            ms[v] += r["ms"]
            info[v] = r
    print("part %d (%s)" % (part, {2: "Inner with the filter against FilterExec over the join", 3: "Semi and Left with the filter"}[part]))
    for v in variants:
        s = sorted(ms[v])
        med = statistics.median(s)
        print("  %-22s %-6s build  table %-6s  median %9.3f ms  spread %8.3f (min %9.3f .. max %9.3f, %d runs)  rows out %10d  %7.3f G probe rows/s"
              % (v[0], v[1], info[v]["form"], med, s[-1] - s[0], s[0], s[-1], len(s), info[v]["rows_out"], info[v]["probe_rows"] / med / 1e6), flush=True)
    if part == 2:
        print("  candidates = rows out of Inner_unfiltered, kept pairs = rows out of Inner_filter")
    for v in variants:
        if v[1] == "this":
            r = run(me + [v[0]], v[1], {"BHIP_KERNEL_TIMING": "1", "RUNS": "1"}, v[0])
            print("  kernels of one %s run (ms, launches): %s" % (v[0], json.dumps(r["kernel_ms_launches"])), flush=True)


def main():
    parts = [int(p) for p in os.environ.get("PARTS", "1,2,3").split(",")]
    have_parent = bool(os.environ.get("PARENT_TREE"))
    print("# build rows %s (two per key), probe rows %s in four batches, %s timed runs per child; ms = plan construction + collect, build side included"
          % (os.environ.get("BUILD_ROWS", 1_000_000), os.environ.get("PROBE_ROWS", 16_000_000), os.environ.get("RUNS", 10)))
    for part in parts:
        if part == 1:
            bench_part(have_parent)
        else:
            join_part(part, have_parent)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
