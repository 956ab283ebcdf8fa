#!/usr/bin/env python3
"""NestedLoopJoinExec at size against the only form the parent commit has for a join without a key: HashJoinExec on a constant key
column present on both sides, with the same predicate as its residual filter (run on the GPU box; seeded inputs made here;
PARENT_TREE=path names a checkout of the parent commit with its library built — the baseline runs under the parent's package and
library; without it the same emulation runs on this build and says so).

  shape      build 2^12 rows (x Int64, id), probe 2^20 rows in batches of 2^16 (lo, hi Int64, id): 2^28 candidate pairs a batch, under
             the hash join's 2^32 limit; every row of either side carries the constant key 0.
  predicate  the band  lo <= x AND x < hi, x and lo uniform over [0, 10^6), hi = lo + width: width 10^4 keeps about 1 % of the pairs,
             width 10^2 about 0.01 %.  Inner join, every output column gathered.
  variants   baseline (HashJoinExec on the constant key + filter), general (NestedLoopJoinExec, BHIP_NO_NLJ_FUSED=1), compare
             (NestedLoopJoinExec, the fused kernel)

Every variant runs in a child process of its own under `timeout` (a failed child ends the script): inputs resident on the device, one
warm-up run, then RUNS timed runs of a fresh plan (construction + collect + synchronise, the build side collected in every run).  The
variants alternate within a round, ROUNDS rounds.  Printed per variant and selectivity: the median of all timed runs, min .. max (the
spread), rows out, candidate pairs/s; then the ratios and the verdicts of the two acceptance questions (compare faster than the
baseline by more than the two spreads; general not slower than the baseline beyond them).  A last pass with BHIP_KERNEL_TIMING=2 (every
launch timed) lists the kernels of one run of each variant; KERNELS_ONLY=1 runs that pass alone.
  tools/exp_nljoin.py > profiles/nljoin.txt      BUILD_ROWS PROBE_ROWS BATCH_ROWS RUNS=5 ROUNDS=2 WIDTHS=10000,100 override"""
import json, os, statistics, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("BHIP_TREE") or HERE              # the tree whose package and library a child runs (this one, or the parent's)
sys.path.insert(0, ROOT)

VARIANTS = [("baseline", "parent", {}), ("general", "this", {"BHIP_NO_NLJ_FUSED": "1"}), ("compare", "this", {})]


def child(name, width):
    import numpy as np
    import ballista_amd as ba
    from ballista_amd import expr as E
    from ballista_amd.expr import col
    nb, npr = int(os.environ.get("BUILD_ROWS", 1 << 12)), int(os.environ.get("PROBE_ROWS", 1 << 20))
    cut, runs = int(os.environ.get("BATCH_ROWS", 1 << 16)), int(os.environ.get("RUNS", 5))
    rng = np.random.default_rng(47)
    x = rng.integers(0, 10 ** 6, nb).astype(np.int64)
    lo = rng.integers(0, 10 ** 6, npr).astype(np.int64)
    ctx = ba.Context(0)
    left = ba.RecordBatch.from_columns(ctx, [("kl", "Int64", np.zeros(nb, np.int64), None), ("x", "Int64", x, None),
                                             ("li", "Int64", np.arange(nb, dtype=np.int64), None)])
    right = [ba.RecordBatch.from_columns(ctx, [("kr", "Int64", np.zeros(min(cut, npr - s), np.int64), None), ("lo", "Int64", lo[s:s + cut], None),
                                               ("hi", "Int64", lo[s:s + cut] + width, None),
                                               ("ri", "Int64", np.arange(s, min(s + cut, npr), dtype=np.int64), None)])
             for s in range(0, npr, cut)]
    schema = {"kl": "Int64", "x": "Int64", "li": "Int64", "kr": "Int64", "lo": "Int64", "hi": "Int64", "ri": "Int64"}
    pred = E.coerce((col("lo") <= col("x")).and_(col("x") < col("hi")), schema)
    sides = lambda: (ba.MemoryExec([[left]], ctx), ba.MemoryExec([right], ctx))
    if name == "baseline":
        make = lambda: ba.HashJoinExec(*sides(), [("kl", "kr")], "Inner", filter=pred)
    else:
        make = lambda: ba.NestedLoopJoinExec(*sides(), "Inner", filter=pred)
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
    form = ctx.join_key_form() if name == "baseline" else ctx.nested_loop_form()
    res = dict(name=name, form=form, ms=[round(v, 3) for v in ms], rows_out=rows, pairs=nb * npr)
    if os.environ.get("BHIP_KERNEL_TIMING"):
        ks = sorted(ctx.kernel_stats().items(), key=lambda kv: -kv[1][0])[:10]
        res["kernel_ms_launches"] = {k: (round(v[0] / runs, 3), v[1] // runs) for k, v in ks}
    print(json.dumps(res), flush=True)


def run(cmd, lib, env_extra, what):
    tree = os.path.abspath(os.environ["PARENT_TREE"]) if lib == "parent" and os.environ.get("PARENT_TREE") else HERE
    env = dict(os.environ, BHIP_TREE=tree, **env_extra)
    p = subprocess.run(["timeout", "-k", "10", os.environ.get("STEP_TIMEOUT", "240")] + cmd, env=env, stdout=subprocess.PIPE, text=True, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"{what} ({lib} build) ended with status {p.returncode}: stopping")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    rounds = int(os.environ.get("ROUNDS", 2))
    widths = [int(w) for w in os.environ.get("WIDTHS", "10000,100").split(",")]
    me = [sys.executable, os.path.abspath(__file__), "--child"]
    have_parent = bool(os.environ.get("PARENT_TREE"))
    print("# build rows %s, probe rows %s in batches of %s, %s timed runs per child, %d alternating rounds; ms = plan construction + collect"
          % (os.environ.get("BUILD_ROWS", 1 << 12), os.environ.get("PROBE_ROWS", 1 << 20), os.environ.get("BATCH_ROWS", 1 << 16), os.environ.get("RUNS", 5), rounds))
    print("# baseline = HashJoinExec on a constant key + the predicate as residual filter, on the %s"
          % ("PARENT commit's library" if have_parent else "library of THIS build (no PARENT_TREE given: not the parent commit)"))
    def kernel_pass(width):
        # level 2: every launch is timed (level 1 leaves out launches over fewer than 2^18 rows, and a probe batch has 2^16)
        for name, lib, env in VARIANTS:
            r = run(me + [name, str(width)], lib, dict(env, BHIP_KERNEL_TIMING="2", RUNS="1"), name)
            print("  kernels of one %s run (ms, launches): %s" % (name, json.dumps(r["kernel_ms_launches"])), flush=True)

    for width in widths:
        if os.environ.get("KERNELS_ONLY"):              # the per-kernel split alone
            print("band width %d" % width)
            kernel_pass(width)
            continue
        ms, info = {v[0]: [] for v in VARIANTS}, {}
        for _ in range(rounds):                         # the variants alternate: a drift of the machine hits all of them alike
            for name, lib, env in VARIANTS:
                r = run(me + [name, str(width)], lib, env, name)
                ms[name] += r["ms"]
                info[name] = r
        pairs = info["compare"]["pairs"]
        print("band width %d: %d of %d pairs kept (%.4f %%)" % (width, info["compare"]["rows_out"], pairs, 100.0 * info["compare"]["rows_out"] / pairs))
        med, spr = {}, {}
        for name, lib, _ in VARIANTS:
            s = sorted(ms[name])
            med[name], spr[name] = statistics.median(s), s[-1] - s[0]
            print("  %-9s %-6s build  route %-8s median %10.3f ms  spread %9.3f (min %10.3f .. max %10.3f, %d runs)  rows out %10d  %8.3f G pairs/s"
                  % (name, lib if have_parent else "this", info[name]["form"], med[name], spr[name], s[0], s[-1], len(s), info[name]["rows_out"],
                     pairs / med[name] / 1e6), flush=True)
        assert info["baseline"]["rows_out"] == info["general"]["rows_out"] == info["compare"]["rows_out"]
        noise = spr["baseline"] + spr["compare"]
        print("  baseline / compare = %.2fx; compare is %s than the baseline by more than the two spreads (%.3f ms)"
              % (med["baseline"] / med["compare"], "FASTER" if med["baseline"] - med["compare"] > noise else "NOT faster", noise))
        noise = spr["baseline"] + spr["general"]
        print("  baseline / general = %.2fx; general is %s than the baseline beyond the two spreads (%.3f ms)"
              % (med["baseline"] / med["general"], "SLOWER" if med["general"] - med["baseline"] > noise else "not slower", noise), flush=True)
        kernel_pass(width)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
