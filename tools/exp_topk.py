#!/usr/bin/env python3
"""ORDER BY ... LIMIT k as a top-k selection against the full sort + head slice (run on the GPU box).

Steps, each in a fresh child process under `timeout`, chained so that a failed step ends the script, each once as built and once
with BHIP_NO_TOPK=1 (the limit over the sort runs the full sort and the head slice: the route before the selection existed):
  ORDER BY l_extendedprice DESC LIMIT 10 / 1000 over 64 Mi and 600 M generated lineitem rows (l_extendedprice, l_orderkey, l_shipdate);
  Q3 with limit=10 at the SF100 sizes bench.py uses.
Prints ms per step (median of the timed runs), the top-k kernels' lines of kernel_stats and the context's peak bytes.
  tools/exp_topk.py > profiles/topk.txt            ROWS_BIG=600037902 BATCH_ROWS=33554432 RUNS=5 override the sizes"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(step):
    os.environ.setdefault("BHIP_KERNEL_TIMING", "1")
    import ballista_amd as ba
    from ballista_amd import tpch, distributed as D, expr as E
    from ballista_amd.expr import col
    ctx = ba.Context(0)
    runs = int(os.environ.get("RUNS", 5))
    if step["kind"] == "lineitem":
        rows, per = step["rows"], int(os.environ.get("BATCH_ROWS", 32 << 20))
        cols = ["l_orderkey", "l_extendedprice", "l_shipdate"]
        parts = [ba.plan.tpch_lineitem(ctx, 100.0, tpch.SEED, lo, min(per, rows - lo), columns=cols) for lo in range(0, rows, per)]
        make = lambda: ba.GlobalLimitExec(ba.SortExec([E.PhysicalSortExpr(col("l_extendedprice"), descending=True)],
                                                      ba.MemoryExec([parts], ctx)), step["k"])
    else:
        w = D.Workload("q3", ctx, D.ProcessGroup.single(), 100.0, tpch.table_rows(100.0))
        w.load("strong")
        t = w.t
        make = lambda: tpch.q3_plan(t["customer"], t["orders"], t["lineitem"], limit=step["k"])
    ctx.synchronize()
    in_use, _ = ctx.memory()
    ms, out = [], None
    try:
        for it in range(runs + 1):
            plan = make()
            ctx.synchronize()
            if it == 1:
                ctx.kernel_stats(reset=True)
            t0 = time.perf_counter()
            out = plan.collect()
            ctx.synchronize()
            if it:
                ms.append((time.perf_counter() - t0) * 1e3)
            del plan
    except ba.BallistaError as e:
        print(json.dumps(dict(step=step, no_topk=os.environ.get("BHIP_NO_TOPK", "0"), error=str(e)[:200], in_use=in_use)), flush=True)
        return
    ks = {k: v for k, v in ctx.kernel_stats().items() if k.startswith("topk_") or k in ("select_indices", "bucket_sort", "sort_key_fixed")}
    _, peak = ctx.memory()
    print(json.dumps(dict(step=step, no_topk=os.environ.get("BHIP_NO_TOPK", "0"), form=ctx.sort_limit_form(), ms_median=sorted(ms)[len(ms) // 2],
                          ms=[round(x, 3) for x in ms], rows_out=sum(b.num_rows for b in out), in_use_before=in_use, peak=peak,
                          kernel_ms_launches={k: (round(v[0], 3), v[1]) for k, v in ks.items()})), flush=True)


def main():
    big = int(os.environ.get("ROWS_BIG", 600_037_902))
    steps = [dict(kind="lineitem", rows=64 << 20, k=10), dict(kind="lineitem", rows=64 << 20, k=1000),
             dict(kind="q3", k=10),
             dict(kind="lineitem", rows=big, k=10), dict(kind="lineitem", rows=big, k=1000)]
    only = os.environ.get("STEPS")
    if only:
        steps = [steps[int(i)] for i in only.split(",")]
    for step in steps:
        for no_topk in ("0", "1"):
            env = dict(os.environ, BHIP_NO_TOPK=no_topk)
            rc = subprocess.call(["timeout", "-k", "10", os.environ.get("STEP_TIMEOUT", "240"), sys.executable, os.path.abspath(__file__), "--child", json.dumps(step)], env=env)
            if rc != 0:
                raise SystemExit(f"step {step} (BHIP_NO_TOPK={no_topk}) ended with status {rc}: stopping")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(json.loads(sys.argv[2]))
    else:
        main()
