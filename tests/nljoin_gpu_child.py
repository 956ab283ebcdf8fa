"""The cases of test_nljoin_gpu.py that need a process of their own, because the library reads its switches once: started by that test
with the switch in the environment, never by pytest (no test_ prefix).

  chunked   BHIP_NLJ_CHUNK_PAIRS=<n>, n neither a multiple of the build rows nor of 64: the general-route cases and the cross joins over
            many ragged chunks — matched and hit bits add up over the chunks, unmatched and existence rows are decided after the last one
  nofused   BHIP_NO_NLJ_FUSED=1: the fused-route cases report "general" and give the same rows"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import ballista_amd as ba  # noqa: E402

import join_filter_cases as JF  # noqa: E402
import nljoin_cases as NC  # noqa: E402


def main(mode):
    ctx = ba.Context(0)
    n = 0
    if mode == "chunked":
        chunk = int(os.environ["BHIP_NLJ_CHUNK_PAIRS"])
        assert chunk % NC.NL and chunk % 64 and NC.NL * NC.NR > 20 * chunk
        for name, nulls, jt in NC.general_cases():
            NC.run_case(ctx, name, nulls, jt, "general")
            n += 1
        left, right = NC.sides(True, NC.NL, NC.NR)
        for jt in NC.ALL_TYPES:
            NC.check(ctx, left, right, jt, None, "exists" if jt in JF.BUILD_SIDE + JF.PROBE_SIDE else "cross")
            n += 1
        NC.run_case(ctx, "band", True, JF.INNER, "compare")                  # the fused route takes no chunks
    elif mode == "nofused":
        assert os.environ["BHIP_NO_NLJ_FUSED"] == "1"
        for name, nulls, jt in NC.value_cases():
            NC.run_case(ctx, name, nulls, jt, "general")
            n += 1
    else:
        raise SystemExit("unknown mode " + mode)
    print("OK", mode, n)


if __name__ == "__main__":
    main(sys.argv[1])
