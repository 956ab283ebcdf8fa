#!/usr/bin/env python3
"""COUNT(DISTINCT x) in HashAggregateExec's Single mode against the only form the operators before it have: the two-level rewrite
GROUP BY k, x -> COUNT(x) GROUP BY k, each level a Final over the Merge of a Partial (run on the GPU box; seeded inputs made here).

  shape     a Q16-shaped aggregate: ROWS rows (default 8 M: partsupp at SF10), three group columns as a dictionary-coded
            (p_brand, p_type, p_size) would be — Int16 x 25, Int16 x 150, Int32 x 5 values = 18 750 groups — and x Int64
            (ps_suppkey).  The four columns are 16 bytes without NULLs, so the rewrite's first level stays on the packed-key route.
  variants  dup4: every distinct (k, x) pair about 4 times, at scattered rows; dup1: every row a pair of its own.
  plans     single: HashAggregateExec(Single, k, COUNT_DISTINCT(x)); rewrite: the two levels.

Every (plan, variant) runs in a child process of its own under `timeout` (a failed child ends the script): inputs resident on the
device, one warm-up run, then RUNS timed runs of a FRESH plan (construction + collect + synchronise).  The plans alternate within a
round, ROUNDS rounds.  Printed per plan and variant: the median of all timed runs with min .. max, the groups and the sum of the
counts (equal between the plans, or the script fails); then the ratio single / rewrite; then one pass with BHIP_KERNEL_TIMING=2 (every
launch timed) listing the kernels of one run of each, `distinct_claim` / `distinct_mark` among them.
  tools/exp_count_distinct.py > profiles/count_distinct.txt      ROWS RUNS=7 ROUNDS=2 STEP_TIMEOUT=240 override"""
import json, os, statistics, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

PLANS = ("single", "rewrite")
VARIANTS = ("dup4", "dup1")
KEYS = ("brand", "type", "size")


def child(plan_name, variant):
    import numpy as np
    import ballista_amd as ba
    from ballista_amd import expr as E
    from ballista_amd.expr import col
    n, runs = int(os.environ.get("ROWS", 8_000_000)), int(os.environ.get("RUNS", 7))
    rng = np.random.default_rng(16)
    pairs = n // 4 if variant == "dup4" else n
    g = rng.integers(0, 18750, pairs)
    pair = rng.permutation(np.repeat(np.arange(pairs), n // pairs))          # which pair a row holds: equal pairs at scattered rows
    x = rng.permutation(pairs).astype(np.int64)[pair]                         # one x per pair, all different
    g = g[pair]
    ctx = ba.Context(0)
    batch = ba.RecordBatch.from_columns(ctx, [("brand", "Int16", (g % 25).astype(np.int16), None), ("type", "Int16", (g // 25 % 150).astype(np.int16), None),
                                              ("size", "Int32", (g // 3750).astype(np.int32), None), ("x", "Int64", x, None)])
    group = [(col(k), k) for k in KEYS]
    P = ba.plan

    def final_over_partial(grp, count_of, below):
        aggs = [E.Count(col(count_of), "n")]
        part = ba.HashAggregateExec(P.PARTIAL, grp, aggs, below)
        return ba.HashAggregateExec(P.FINAL, [(col(nm), nm) for _, nm in grp], [E.AggregateExpr("COUNT", col("n[count]"), "n")], ba.MergeExec(part))

    def make():
        m = ba.MemoryExec([[batch]], ctx)
        if plan_name == "single":
            return ba.HashAggregateExec(P.SINGLE, group, [E.CountDistinct(col("x"), "n")], m)
        return final_over_partial(group, "x", final_over_partial(group + [(col("x"), "x")], "x", m))

    ctx.synchronize()
    ms, groups, total = [], 0, 0
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
        groups = sum(b.num_rows for b in out)
        total = int(sum(int(b.column(b.num_columns - 1)[1].sum()) for b in out))
        del out, plan
    res = dict(plan=plan_name, variant=variant, rows=n, pairs=pairs, ms=[round(v, 3) for v in ms], groups=groups, sum_of_counts=total)
    if os.environ.get("BHIP_KERNEL_TIMING"):
        ks = sorted(ctx.kernel_stats().items(), key=lambda kv: -kv[1][0])[:12]
        res["kernel_ms_launches"] = {k: (round(v[0] / runs, 3), v[1] // runs) for k, v in ks}
    print(json.dumps(res), flush=True)


def run(plan_name, variant, env_extra):
    env = dict(os.environ, **env_extra)
    p = subprocess.run(["timeout", "-k", "10", os.environ.get("STEP_TIMEOUT", "240"), sys.executable, os.path.abspath(__file__), "child", plan_name, variant],
                       env=env, stdout=subprocess.PIPE, text=True, cwd=HERE)
    if p.returncode != 0:
        raise SystemExit(f"{plan_name} / {variant} ended with status {p.returncode}: stopping")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    rounds = int(os.environ.get("ROUNDS", 2))
    times, facts = {}, {}
    for variant in VARIANTS:
        for _ in range(rounds):
            for plan_name in PLANS:
                r = run(plan_name, variant, {"BHIP_KERNEL_TIMING": ""})
                times.setdefault((plan_name, variant), []).extend(r["ms"])
                facts[(plan_name, variant)] = (r["rows"], r["pairs"], r["groups"], r["sum_of_counts"])
        a, b = facts[("single", variant)], facts[("rewrite", variant)]
        if a != b or a[3] != a[1]:
            raise SystemExit(f"{variant}: single {a} and rewrite {b} disagree, or the counts do not add up to the pairs")
    print("COUNT(DISTINCT x) GROUP BY 3 columns: Single mode against the two-level rewrite; ms per fresh plan, median (min .. max) of", rounds, "x RUNS runs")
    for variant in VARIANTS:
        rows, pairs, groups, total = facts[("single", variant)]
        print(f"{variant}: {rows} rows, {pairs} distinct (k, x) pairs ({rows / pairs:.1f} rows per pair), {groups} groups, sum of counts {total}")
        med = {}
        for plan_name in PLANS:
            v = times[(plan_name, variant)]
            med[plan_name] = statistics.median(v)
            print(f"  {plan_name:8s} {med[plan_name]:8.3f} ms  ({min(v):.3f} .. {max(v):.3f}; {len(v)} runs)  {rows / med[plan_name] / 1e6:.2f} G rows/s")
        print(f"  single / rewrite = {med['single'] / med['rewrite']:.2f}")
    print("kernels of one run, ms per run (launches), BHIP_KERNEL_TIMING=2:")
    for variant in VARIANTS:
        for plan_name in PLANS:
            r = run(plan_name, variant, {"BHIP_KERNEL_TIMING": "2", "RUNS": "3"})
            print(f"  {variant} {plan_name}: " + ", ".join(f"{k} {ms} ({n})" for k, (ms, n) in r["kernel_ms_launches"].items()))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
