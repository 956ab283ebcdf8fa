#!/usr/bin/env python3
"""Step times of the existence joins against the joins that could stand in for them (run on the GPU box; seeded inputs made here).

  1. unique build   Semi and Anti against Left, one left column read: build 15 M unique Int32 keys (shuffled), probe 60 M rows in
                    four batches, keys drawn from 1.25 x the build's key range (about 3 partners per build key, 80 % of the probe
                    rows find one).  Left also on a library built from the parent commit (PARENT_LIB=path), where that is given,
                    and with BHIP_NO_NARROW_JOIN=1: on the general table, which is what the existence types always build.
  2. duplicates     the same with 8 build rows per key: Left enumerates every pair, the mark form must not.
  3. probe side     RightSemi (general table) against today's Inner "semi-join" (unique build, no build column read: the rank
                    map's key-set words; and the same join on the general table), one right column read.  No bar: the ratio is the
                    case for or against a narrow variant.

Every variant runs in a child process of its own under `timeout` (a failed child ends the script): one warm-up run, then RUNS timed
runs of plan construction + collect (the build side is built in every run).  The variants alternate within a round, ROUNDS rounds.
Printed per variant: the median of all its timed runs with their min .. max, and the rows that came out.  A last pass with
BHIP_KERNEL_TIMING=1 lists the kernels of one run of each variant of this build.
  tools/exp_join_types.py > profiles/join_types.txt      BUILD_ROWS=15000000 PROBE_ROWS=60000000 RUNS=5 ROUNDS=2 override"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (join type, build, general: BHIP_NO_NARROW_JOIN=1 — the join the existence types are compared with, on the table form they use)
VARIANTS = {
    1: [("Left", "parent", False), ("Left", "this", False), ("Left", "this", True), ("Semi", "this", False), ("Anti", "this", False)],
    2: [("Left", "parent", False), ("Left", "this", False), ("Semi", "this", False), ("Anti", "this", False)],
    3: [("Inner", "this", False), ("Inner", "this", True), ("RightSemi", "this", False)],
}


def child(part, jt):
    import numpy as np
    import ballista_amd as ba
    from ballista_amd.expr import col
    nb, npr = int(os.environ.get("BUILD_ROWS", 15_000_000)), int(os.environ.get("PROBE_ROWS", 60_000_000))
    runs = int(os.environ.get("RUNS", 5))
    per_key = 8 if part == 2 else 1
    rng = np.random.default_rng(20 + part)
    n_keys = nb // per_key
    lk = rng.permutation(nb).astype(np.int32) // per_key
    rk = rng.integers(0, n_keys + n_keys // 4, npr).astype(np.int32)
    ctx = ba.Context(0)
    left = ba.RecordBatch.from_columns(ctx, [("lk", "Int32", lk, None), ("lv", "Int64", np.arange(nb, dtype=np.int64), None)])
    cut = (npr + 3) // 4
    right = [ba.RecordBatch.from_columns(ctx, [("rk", "Int32", rk[lo:lo + cut], None), ("rv", "Int64", np.arange(lo, min(lo + cut, npr), dtype=np.int64), None)])
             for lo in range(0, npr, cut)]
    out_col = "rv" if part == 3 else "lv"
    make = lambda: ba.ProjectionExec([(col(out_col), out_col)],
                                     ba.HashJoinExec(ba.MemoryExec([[left]], ctx), ba.MemoryExec([right], ctx), [("lk", "rk")], jt))
    ctx.synchronize()
    ms, rows = [], 0
    for it in range(runs + 1):
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
    res = dict(part=part, jt=jt, form=ctx.join_key_form(), ms=[round(x, 3) for x in ms], rows_out=rows)
    if os.environ.get("BHIP_KERNEL_TIMING"):
        ks = sorted(ctx.kernel_stats().items(), key=lambda kv: -kv[1][0])[:8]
        res["kernel_ms_launches"] = {k: (round(v[0] / runs, 3), v[1] // runs) for k, v in ks}
    print(json.dumps(res), flush=True)


def run_child(part, jt, lib, env_extra):
    env = dict(os.environ, **env_extra)
    if lib == "parent":
        env["BHIP_LIB_PATH"] = os.path.abspath(os.environ["PARENT_LIB"])
    cmd = ["timeout", "-k", "10", os.environ.get("STEP_TIMEOUT", "180"), sys.executable, os.path.abspath(__file__), "--child", str(part), jt]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise SystemExit(f"part {part} {jt} ({lib} build) ended with status {p.returncode}: stopping")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    rounds = int(os.environ.get("ROUNDS", 2))
    parts = [int(p) for p in os.environ.get("PARTS", "1,2,3").split(",")]
    have_parent = bool(os.environ.get("PARENT_LIB"))
    print("# build rows %s, probe rows %s, %s timed runs per child, %d rounds; ms = plan construction + collect, build side included"
          % (os.environ.get("BUILD_ROWS", 15_000_000), os.environ.get("PROBE_ROWS", 60_000_000), os.environ.get("RUNS", 5), rounds))
    for part in parts:
        variants = [v for v in VARIANTS[part] if v[1] == "this" or have_parent]
        ms, info = {v: [] for v in variants}, {}
        for _ in range(rounds):                         # the variants alternate: a drift of the machine hits all of them alike
            for v in variants:
                r = run_child(part, v[0], v[1], {"BHIP_NO_NARROW_JOIN": "1"} if v[2] else {})
                ms[v] += r["ms"]
                info[v] = r
        print("part %d (%s)" % (part, {1: "unique build", 2: "8 build rows per key", 3: "probe-side existence, unique build"}[part]))
        for v in variants:
            s = sorted(ms[v])
            print("  %-9s %-6s build  table %-6s  median %9.3f ms  (min %9.3f .. max %9.3f, %d runs)  rows out %d"
                  % (v[0], v[1], info[v]["form"], s[len(s) // 2], s[0], s[-1], len(s), info[v]["rows_out"]), flush=True)
        for v in variants:
            if v[1] == "this":
                r = run_child(part, v[0], v[1], dict({"BHIP_KERNEL_TIMING": "1", "RUNS": "1"}, **({"BHIP_NO_NARROW_JOIN": "1"} if v[2] else {})))
                print("  kernels of one %s run, table %s (ms, launches): %s" % (v[0], r["form"], json.dumps(r["kernel_ms_launches"])), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), sys.argv[3])
    else:
        main()
