"""GPU tier of the scan launch-form tests (kernels_util.hip exclusive_scan_t and launch_rank_pack over scan_device.h): the three users
of scan_cases.py at sizes on each side of n == 0, SCAN_ONE_LAUNCH_MAX and SCAN_TWO_LAUNCH_CHUNKS chunks.  The expectations are
scan_cases' (checked against second statements in test_scan_cases_cpu.py); offsets and bytes compare exactly, pairs as multisets of
row ids.  The three sizes of about 8.39 M rows are the smallest at which the three-launch form exists."""
import numpy as np
import pytest

import ballista_amd as ba
from ballista_amd import _lib as L, expr as E
from ballista_amd.expr import col

import helpers
import join_filter_cases as JF
import join_route_cases as RC
import scan_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tctx():
    return RC.timing_context()


def utf8_buffers(rb, i):
    """-> (offsets, value bytes) of Utf8 column i as they lie in the batch, no string made of them"""
    _, dtype, _, nbytes, has_valid = rb.column_info(i)
    assert dtype == "Utf8" and not has_valid
    n = rb.num_rows
    off, data = np.zeros(n + 1, np.int32), np.zeros(max(1, nbytes), np.uint8)
    L.check(L.lib().bhip_batch_column_to_host(rb._h, i, data.ctypes.data, off.ctypes.data, None))
    return off, data[:nbytes]


@pytest.mark.parametrize("name, n, form", SC.SIZES, ids=SC.SIZE_IDS)
def test_cast_int32_to_utf8_offsets_and_bytes(ctx, name, n, form):
    """u32 -> i32 with the total behind the last offset (utf8_from_lengths): all n + 1 offsets, and the value bytes of every row up to
    SCAN_ONE_LAUNCH_MAX + 1 rows; beyond, of scan_cases.windows: the first 2 * C rows, the 2 * C rows around the last chunk boundary and
    the last 2 * C rows"""
    v = SC.cast_values(n)
    src = helpers.memory_exec(ctx, [[{"v": SC.OCol("Int32", v)}]])
    out = ba.ProjectionExec([(E.CastExpr(col("v"), E.UTF8), "s")], src).collect()
    if n == 0 and not out:
        return                                                              # (an operator may yield nothing for no rows)
    assert len(out) == 1 and out[0].num_rows == n
    off, data = utf8_buffers(out[0], 0)
    want = SC.cast_offsets(n)
    bad = np.nonzero(off != want)[0]
    assert len(bad) == 0, (name, form, [(int(i), int(off[i]), int(want[i])) for i in bad[:5]])
    assert len(data) == want[n]
    for a, b in SC.windows(n):
        assert data[want[a]:want[b]].tobytes() == SC.cast_text(v[a:b]), (name, a, b)


def joined_pairs(plan):
    """(li, ri) of a join's output, straight from its Int32 id columns"""
    li, ri = [], []
    for rb in plan.collect():
        names = [rb.column_info(i)[0] for i in range(rb.num_columns)]
        li.append(rb.column(names.index("li"))[1])
        ri.append(rb.column(names.index("ri"))[1])
    return (np.concatenate(li), np.concatenate(ri)) if li else (np.zeros(0, np.int32), np.zeros(0, np.int32))


@pytest.mark.parametrize("name, n, form", SC.SIZES, ids=SC.SIZE_IDS)
def test_general_table_probe_pairs(ctx, name, n, form):
    """u32 -> u64 without the total (enumerate_pairs: count -> scan -> emit): n probe rows with 0 to 3 partners each on a build side with
    duplicate keys; every pair, as a multiset"""
    left, right = SC.id_side("l", SC.BUILD_KEYS), SC.id_side("r", SC.probe_keys(n))
    plan = ba.HashJoinExec(helpers.memory_exec(ctx, [[left]]), helpers.memory_exec(ctx, [[right]]), RC.ON, JF.INNER)
    li, ri = joined_pairs(plan)
    assert ctx.join_key_form() == "packed"
    wl, wr = SC.probe_pairs(n)
    assert len(li) == len(wl), (name, form, len(li), len(wl))
    nb = len(SC.BUILD_KEYS)
    assert li.min(initial=0) >= 0 and li.max(initial=0) < nb
    got, want = SC.pair_codes(li, ri, nb), SC.pair_codes(wl, wr, nb)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (name, form, [(int(got[i]), int(want[i])) for i in bad[:5]])


@pytest.mark.parametrize("case", SC.rank_cases(), ids=SC.RANK_IDS)
def test_rank_map_by_granule_count(tctx, case):
    """launch_rank_pack through the narrow join on unique Int32 keys: the granule counts of scan_cases.RANK_SIZES (the three-launch one
    is a map of about 0.4 GB); every probe key's partner, the keys of the first and the last granule of each chunk among them"""
    left, right = SC.id_side("l", case.bkeys), SC.id_side("r", case.pkeys)
    tctx.kernel_stats(reset=True)
    plan = ba.HashJoinExec(RC.build_exec(tctx, left), helpers.memory_exec(tctx, [[right]]), RC.ON, JF.INNER)
    li, ri = joined_pairs(plan)
    names = set(tctx.kernel_stats(reset=True))
    assert tctx.join_key_form() == "narrow"
    assert {"rank_pack", "rank_bits_sorted" if case.order == "sorted" else "rank_bits_any"} <= names and "join_build_narrow" not in names, sorted(names)
    assert ("rank_perm" in names) == (case.order == "shuffled")
    wl, wr = SC.dict_join(case.bkeys, case.pkeys)
    assert len(li) == len(wl), (len(li), len(wl))
    nb = len(case.bkeys)
    got, want = SC.pair_codes(li, ri, nb), SC.pair_codes(wl, wr, nb)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(got[i]) // nb, int(got[i]) % nb, int(want[i]) % nb) for i in bad[:5]]
