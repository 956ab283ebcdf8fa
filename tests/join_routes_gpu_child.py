"""The cases of test_join_routes_gpu.py that need a process of their own, because the library reads its switches once: started by that
test with the switch in the environment, never by pytest (no test_ prefix).

  table     BHIP_JOIN_TABLE=1: every tiny and rank case through the CAS table (join_build_narrow[64]), the same expected rows
  present   BHIP_JOIN_TABLE=1: 2^18 and 2^18 + 37 unique keys spanning < 2^30, Int32 and Int64: join_key_present / join_key_present64
  notiny    BHIP_NO_TINY_BUILD=1: the tiny cases through the general rank map
  noscalar  BHIP_PROBE_NO_SCALAR_MAP=1 |
  flat      BHIP_PROBE_MAP_FLAT=1      | the rank cases and the probe shapes: join_probe_form() names the variant's A/B partner
  nobits    BHIP_PROBE_NO_BITS=1       |
  rows8     BHIP_PROBE_ROWS=8          |
  window10  BHIP_RANK_WINDOW_LOG2=10: the rank cases with a range above 1024 on the CAS table, by the bound"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import ballista_amd as ba  # noqa: E402

import join_filter_cases as JF  # noqa: E402
import join_types_cases as JT  # noqa: E402
import join_route_cases as RC  # noqa: E402

SWITCH = {"table": ("BHIP_JOIN_TABLE", "1"), "present": ("BHIP_JOIN_TABLE", "1"), "notiny": ("BHIP_NO_TINY_BUILD", "1"),
          "noscalar": ("BHIP_PROBE_NO_SCALAR_MAP", "1"), "flat": ("BHIP_PROBE_MAP_FLAT", "1"), "nobits": ("BHIP_PROBE_NO_BITS", "1"),
          "rows8": ("BHIP_PROBE_ROWS", "8"), "window10": ("BHIP_RANK_WINDOW_LOG2", "10")}


def route_in(mode, case):
    """the route a case takes under the mode's switch"""
    n, kmin, kmax = RC.key_stats(case)
    route = case.route
    if mode == "table":
        return "packed/table" if route.startswith("packed/") else "table"
    if mode == "notiny" and route == "tiny":
        return "rank_sorted" if RC.is_sorted(case) else "rank_any"
    if mode == "notiny" and route == "packed/tiny":
        return "packed/rank"
    if mode == "window10" and route in ("rank_sorted", "rank_any", "packed/rank") and kmax - kmin > 1 << 10:
        return "packed/table" if route.startswith("packed/") else "table"
    return route


def main(mode):
    name, value = SWITCH[mode]
    assert os.environ[name] == value
    ctx = RC.timing_context()
    n = 0
    if mode == "present":
        for dtype in ("Int32", "Int64"):
            for rows in (RC.PRESENT_MIN_ROWS, RC.PRESENT_MIN_ROWS + 37):
                left, right, _ = RC.present_sides(dtype, rows)
                for jt in (JF.INNER, JT.FULL):
                    plan = ba.HashJoinExec(RC.build_exec(ctx, left), RC.probe_exec(ctx, right, [1025, 3975]), RC.ON, jt)
                    ctx.kernel_stats(reset=True)
                    RC.assert_same_rows(JF.rows(plan), RC.expected(jt, left, right))
                    names = set(ctx.kernel_stats(reset=True))
                    present = "join_key_present" if RC.WIDTH[dtype] == 4 else "join_key_present64"
                    assert {present, "join_build_narrow", "join_filter_probe"} <= names, sorted(names)
                    assert not names & ({"join_key_present", "join_key_present64", "rank_bits_any", "rank_bits_sorted", "join_rank_probe"} - {present}), sorted(names)
                    assert ctx.join_key_form() == "narrow" and ctx.join_probe_form() == "filter/table+present", ctx.join_probe_form()
                n += 1
        print("OK", mode, n)
        return
    prefixes = {"table": ("tiny/", "rank/"), "notiny": ("tiny/",)}.get(mode, ("rank/",))
    for prefix in prefixes:
        for case in RC.cases(prefix):
            route = route_in(mode, case)
            # Inner without NULL probe keys: the one-read kernel's variants; Full with them: the general kernel and both outer flags
            forbid = ("tiny_rank_build",) if mode == "notiny" else ()
            RC.run_case(ctx, case, JF.INNER, False, route=route, mode=mode, forbid=forbid)
            RC.run_case(ctx, case, JT.FULL, True, route=route, mode=mode, forbid=forbid)
            n += 1
    if mode in ("noscalar", "flat", "nobits", "rows8"):
        for run, args in RC.shape_runs():
            run(ctx, *args, mode=mode)
            n += 1
    print("OK", mode, n)


if __name__ == "__main__":
    main(sys.argv[1])
