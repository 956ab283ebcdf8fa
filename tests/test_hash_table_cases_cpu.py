"""CPU tier of the constructed-collision tests: `unmix64` inverts `mix64`; the restated key image, hashes and tables of
hash_table_cases.py stand in the sources as restated; every case IS what it claims under that restatement (homes, tags, full hashes,
pairwise different keys, absent keys absent, the cluster's slots across slot 0, the rows on the stated side of a capacity step); the
restated tables give the dict join and the dict group count on every case, and each `mistake` changes the result of the cases named
for it; the dict join and the dict aggregate agree with the CPU oracle's HashJoinExec and HashAggregateExec."""
import re

import numpy as np
import pytest

from oracle import engine as og
from oracle.engine import OCol

import helpers
import hash_table_cases as HT
import join_filter_cases as JF
import join_types_cases as JT
import join_route_cases as RC
import repartition_cases as RP

JOIN_IDS = [HT.join_case_id(c) for c in HT.JOIN_CASES]
AGG_CASES = HT.agg_cases()
AGG_IDS = [c.name for c in AGG_CASES]
NULLABLE = [("wrap_cluster", form, "duplicates") for form in HT.FORMS]


# ---- mix64 and its inverse ---------------------------------------------------------------------------------------------------------------

def test_unmix64_inverts_mix64():
    rng = np.random.default_rng(64)
    words = [0, 1, 1 << 63, (1 << 64) - 1] + [int(x) for x in rng.integers(0, 1 << 64, 4000, dtype=np.uint64)]
    for x in words:
        assert HT.mix64(HT.unmix64(x)) == x and HT.unmix64(HT.mix64(x)) == x, hex(x)
    # a key solved for a wanted hash has that hash, in every form, forwards and backwards
    for h in words[:200]:
        assert HT.key_hash("packed1_dup", HT.key_with_hash("packed1_dup", h)) == h
        assert HT.key_hash("packed2", HT.key_with_hash("packed2", h, (h % 1000 - 7,))) == h
        assert HT.key_hash("wide3", HT.key_with_hash("wide3", h, (-5, h % 77))) == h
        assert HT.key_hash("packed2", HT.key_with_hash_and_tail("packed2", h, (h % 1000 - 7,))) == h
        assert HT.key_hash("wide3", HT.key_with_hash_and_tail("wide3", h, (-5, h % 77))) == h


# ---- the restatement against the sources ---------------------------------------------------------------------------------------------------

def _squeeze(text):
    return re.sub(r"\s+", " ", text)


@pytest.mark.parametrize("name", list(HT.PINNED))
def test_restatement_is_pinned_to_the_source_text(name):
    rel, text = HT.PINNED[name]
    assert _squeeze(text) in _squeeze(RC.source_text(rel)), \
        "%s has changed where hash_table_cases.py restates it: revisit `%s` there (and this text in PINNED)" % (rel, name)


def test_constants_are_the_sources():
    assert HT.MERGE_SLOTS == 2048 and HT.SEL_TILE == 1024 and HT.PROBE_ROWS == {"Packed": 4, "Wide": 1}
    assert HT.MERGE_GROUP_LIMIT == 1024 and HT.REGISTER_GROUPS == 8 and HT.RUN_MIN_ROWS == 4096
    for rows in HT.PROBE_ROWS.values():                    # both sides of one wave pass of join_owner_walk, and of the selection tile
        assert {64 * rows - 1, 64 * rows, 64 * rows + 1} <= set(HT.PROBE_BATCHES)
    assert HT.SEL_TILE + 1 in HT.PROBE_BATCHES and 1 in HT.PROBE_BATCHES and HT.N_PROBE == sum(HT.PROBE_BATCHES) == 1986 < 2000
    for rel, text in HT.AGG_ROUTE_SOURCE:
        assert text in RC.source_text(rel), "the launch %s of %s has changed its name: revisit AGG_ROUTE_KERNELS" % (text, rel)
    # MemoryExec marks a column nullable exactly when it carries a validity bitmap
    assert "d.nullable = 1 if validity is not None else 0" in open(helpers.ROOT + "/ballista_amd/plan.py").read()
    # three Int64 columns do not fit the 16-byte key, two do
    assert HT.W.packed_layout([("Int64", False)] * 3) == (False, None) and HT.W.packed_layout([("Int64", False)] * 2)[0]
    assert [HT.table_capacity(n) for n in (511, 512, 513, 4096, 4097)] == [1024, 1024, 2048, 8192, 16384]


def test_packed_key_by_hand():
    m = HT.M64
    assert HT.packed_key([("Int64", 5, False), ("Int64", -1, False)]) == (5, m)
    assert HT.packed_key([("Int64", -2, False)]) == (m - 1, 0)                                  # widen_key: (value, 0)
    v = 0x1122334455667788
    assert HT.packed_key([("Int64", v, True)]) == (0x2233445566778801, 0x11)                    # 1 | v << 8, v >> 56
    assert HT.packed_key([("Int64", -1, True)]) == (0xFFFFFFFFFFFFFF01, 0xFF)
    assert HT.packed_key([("Int64", None, True)]) == (0, 0) and HT.packed_key([("Int64", 0, True)]) == (1, 0)
    assert HT.packed_key([("Int32", -1, False), ("Int32", 7, True), ("Int32", 3, False)]) == (0x000007_01_FFFFFFFF, 0x03 << 8)
    with pytest.raises(AssertionError):
        HT.packed_key([("Int64", 1, False)] * 3)
    assert HT.hash_key(5, 0) == HT.mix64(HT.mix64(5)) and HT.hash_key(0, 0) == HT.mix64(HT.mix64(0))
    # the wide row hash is repartition_cases.restated_hash, which the repartitioning tests have checked against the device
    rng = np.random.default_rng(3)
    tri = rng.integers(-2 ** 63, 2 ** 63 - 1, (50, 3), endpoint=True)
    want = RP.restated_hash([OCol("Int64", tri[:, j]) for j in range(3)]).tolist()
    assert [HT.wide_hash(tuple(int(x) for x in r)) for r in tri] == want


# ---- the join cases are what they claim --------------------------------------------------------------------------------------------------------

def _facts(case):
    family_id, form, variation = case
    left, right, fam, keys = HT.join_sides(*case)
    return family_id, form, variation, left, right, fam, keys


@pytest.mark.parametrize("case", HT.JOIN_CASES, ids=JOIN_IDS)
def test_join_case_is_what_it_claims(case):
    family_id, form, variation, left, right, fam, keys = _facts(case)
    nl = og.batch_len(left)
    cap = HT.table_capacity(nl)
    assert cap == fam.cap and nl < 520 and og.batch_len(right) == HT.N_PROBE
    want_rows = HT.FAMILY_IDS[family_id][1]
    if want_rows is not None:                              # on the stated side of 512
        assert nl == want_rows and cap == (1024 if want_rows <= 512 else 2048)
    build = HT.row_keys(left, "l", form)
    probe = HT.row_keys(right, "r", form)
    assert None not in build and None not in probe
    present = set(build)
    assert present == set(keys) and len(set(keys)) == len(keys)                                  # pairwise different
    assert set(fam.cluster) <= present and not set(fam.absent) & present and len(set(fam.absent)) == len(fam.absent) >= 3
    assert set(fam.cluster) | set(fam.absent) <= set(probe)
    counts = {k: build.count(k) for k in keys}
    if variation == "duplicates":
        assert set(counts.values()) == {1, 2, 3, 4} and {counts[k] for k in fam.cluster} >= {1, 2, 3, 4}
        assert build != sorted(build)
    elif form == "packed1_dup":                             # one duplicate, of a filler key: the join leaves the narrow routes
        assert sorted(counts.values()) == [1] * (len(keys) - 1) + [2] and all(counts[k] == 1 for k in fam.cluster)
    else:
        assert set(counts.values()) == {1}
    home = lambda k: HT.home_of(form, k, cap)
    tag = lambda k: HT.tag_of(form, k)
    fillers = keys[len(fam.cluster):]
    assert [home(k) for k in fillers] == [HT.FILLER_HOME0 + i for i in range(len(fillers))]      # one slot each, far from every cluster
    members = fam.cluster + fam.absent
    if fam.name == "wrap_cluster":
        assert len(fam.cluster) >= 12 and {home(k) for k in members} == {cap - 1, cap - 2} and fam.facts["homes"] == (cap - 2, cap - 1)
    elif fam.name == "equal_tag_neighbours":
        s = fam.facts["first_home"]
        assert len(fam.cluster) >= 6 and [home(k) for k in fam.cluster] == [s + i // 2 for i in range(len(fam.cluster))]
        assert {tag(k) for k in members} == {fam.facts["tag"]} and [home(k) for k in fam.absent] == [s, s + 1, s + 2]
        hashes = [HT.key_hash(form, k) for k in members]
        assert len(set(hashes)) == len(hashes) and len({h >> 32 for h in hashes}) == 1            # they differ below bit 32 only
    elif fam.name == "equal_hash":
        assert len(fam.cluster) >= 5 and {HT.key_hash(form, k) for k in members} == {fam.facts["hash"]}
        assert len({k[0] for k in members}) > 1 and len({k[-1] for k in members}) == len(members)
    else:
        for x, y, differs in fam.facts["pairs"]:
            assert x != y and home(x) == home(y) and tag(x) == tag(y) and x in present and y in present
            assert (x[:-1] == y[:-1] and x[-1] != y[-1]) if differs == "last" else (x[1:] == y[1:] and x[0] != y[0])
        assert {d for _, _, d in fam.facts["pairs"]} == {"last", "first"}
        assert all(any(home(a) == home(x) and tag(a) == tag(x) for x, _, _ in fam.facts["pairs"]) for a in fam.absent)
    # the restated build: the cluster's slots are consecutive from its first home, across slot 0 where the case says so
    pairs, t = HT.restated_pairs(form, build, probe)
    slots = sorted(t.find(k) for k in fam.cluster)
    assert fam.facts["crosses_zero"] == (0 in slots and cap - 1 in slots)
    if fam.name == "k1_only":                               # (a cluster of two per pair)
        for x, y, _ in fam.facts["pairs"]:
            assert sorted([t.find(x), t.find(y)]) == [home(x), home(x) + 1] and t.owner[home(x) + 2] is None
    else:
        first = min(home(k) for k in fam.cluster)
        run = [(first + i) % cap for i in range(len(fam.cluster))]
        assert sorted(run) == slots and t.owner[(first + len(fam.cluster)) % cap] is None
    if fam.facts["crosses_zero"]:
        assert slots[:len(fam.cluster) - 2] == list(range(len(fam.cluster) - 2)) and HT.FILLER_HOME0 > len(members)
    for k in fam.absent:                                    # an absent key walks its whole cluster to the empty slot behind it
        assert t.find(k) is None
    # ... and with mistake=None the restated table IS the dict join
    li, ri = HT.expected_pairs(left, right, form)
    assert pairs == sorted(zip(li.tolist(), ri.tolist())) and 0 < len(pairs)
    matched = set(ri.tolist())
    assert 0 < len(matched) < HT.N_PROBE


@pytest.mark.parametrize("case", NULLABLE, ids=[c[1] for c in NULLABLE])
def test_nullable_join_case(case):
    """NULLs on both sides of a wrap_cluster: the NULL rows store a cluster key's values and still neither build nor match"""
    _, form, _ = case
    left, right, fam, keys = HT.join_sides(*case, nulls=True)
    plain = HT.join_sides(*case)
    build, probe = HT.row_keys(left, "l", form), HT.row_keys(right, "r", form)
    assert build.count(None) == 8 and probe.count(None) == 38
    stored = lambda b, p: list(zip(*[b["%sk%d" % (p, j)].values.tolist() for j in range(HT.FORMS[form])]))
    for b, p, ks in ((left, "l", build), (right, "r", probe)):
        under = [s for s, k in zip(stored(b, p), ks) if k is None]
        assert set(under) <= set(fam.cluster)                                                   # a cluster key under every NULL
        for j in range(HT.FORMS[form]):
            assert not b["%sk%d" % (p, j)].is_valid().all()
    pairs, _ = HT.restated_pairs(form, build, probe)
    li, ri = HT.expected_pairs(left, right, form)
    assert pairs == sorted(zip(li.tolist(), ri.tolist()))
    null_l = {i for i, k in enumerate(build) if k is None}
    null_r = {j for j, k in enumerate(probe) if k is None}
    assert not null_l & set(li.tolist()) and not null_r & set(ri.tolist())
    # were validity ignored, the NULL rows would find partners
    ignoring, _ = HT.restated_pairs(form, stored(left, "l"), stored(right, "r"))
    assert len(ignoring) > len(pairs)
    assert og.batch_len(left) == og.batch_len(plain[0]) + 8
    for jt in (JF.INNER, JF.LEFT, JF.RIGHT, JT.FULL):
        want = JT.expected(jt, left, right, HT.ON[form]) if jt == JT.FULL else JT.oracle_join(left, right, HT.ON[form], jt)
        JT.assert_same_rows(HT.expected_rows(jt, left, right, form), want)


@pytest.mark.parametrize("case", HT.JOIN_CASES, ids=JOIN_IDS)
def test_dict_join_equals_the_oracle(case):
    """og.hash_join is what oracle/plan_eval.py evaluates a HashJoinExec with (Inner / Left / Right); Full by join_types_cases' derivation"""
    _, form, _, left, right, _, _ = _facts(case)
    on = HT.ON[form]
    for jt in (JF.INNER, JF.LEFT, JF.RIGHT, JT.FULL):
        want = JT.expected(jt, left, right, on) if jt == JT.FULL else JT.oracle_join(left, right, on, jt)
        JT.assert_same_rows(HT.expected_rows(jt, left, right, form), want)
    for jt in JT.TYPES[1:]:                                 # Semi, Anti, RightSemi, RightAnti: derived from the oracle's Inner join
        JT.assert_same_rows(HT.expected_rows(jt, left, right, form), JT.expected(jt, left, right, on))


@pytest.mark.parametrize("form", list(HT.FORMS))
def test_residual_filter_is_ri_mod_3(form):
    fam = "equal_hash" if ("equal_hash", form) not in HT.LEFT_OUT else "equal_tag_neighbours"
    left, right, _, _ = HT.join_sides(fam, form, "duplicates")
    flt = HT.residual_filter(left, right, form)
    inner = JT.oracle_join(left, right, HT.ON[form], JF.INNER)
    p = og.evaluate(flt, inner)
    assert p.is_valid().all() and np.array_equal(p.values.astype(np.bool_), inner["ri"].values % 3 != 0)
    kept = int((inner["ri"].values % 3 != 0).sum())
    assert 0 < kept < og.batch_len(inner)
    for jt in HT.FILTER_TYPES:
        JT.assert_same_rows(HT.filtered_rows(jt, left, right, form), JF.expected(jt, left, right, HT.ON[form], flt))


# ---- the aggregate cases -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", AGG_CASES, ids=AGG_IDS)
def test_agg_case_is_what_it_claims(case):
    f = case.facts
    t = HT.agg_table(case)
    n = og.batch_len(t)
    images = HT.agg_images(case)
    cap = f["capacity"]
    assert n == f["n_rows"] and len(set(images)) == f["n_groups"] and len(case.partitions) == 1
    assert np.array_equal(t["rn"].values, np.arange(n))
    home = lambda k: HT.hash_key(*k) & (cap - 1)
    route = f["route"]
    runs = [i for i in range(n) if i == 0 or images[i] != images[i - 1]]
    if route == "rows":
        assert cap == HT.table_capacity(n) and n < HT.RUN_MIN_ROWS and f["n_groups"] > HT.REGISTER_GROUPS and len(case.partitions[0]) == 1
        assert 2 * len(runs) > n                           # shuffled: no clustering to find, were there rows enough to look
        m = re.search(r"capacity_turnover_(\d+)", case.name)
        if m:
            assert n == int(m.group(1)) and cap == (1024 if n <= 512 else 2048)
    elif route == "runs":
        assert cap == HT.table_capacity(n) and n >= HT.RUN_MIN_ROWS and len(runs) == f["n_runs"] and 2 * len(runs) <= n
        lengths = np.diff(runs + [n])
        assert lengths.min() >= 3 and lengths.max() <= 5
        heads = [images[i] for i in runs]
        assert min(heads.count(k) for k in set(heads)) >= 2                                     # every key comes back in a later run
        firsts = [k[0] ^ (1 << 63) for k in heads]                                              # (run_heads compares the first part unsigned)
        assert sum(1 for x, y in zip(firsts, firsts[1:]) if y <= x) > 1                          # more than ONE break: neither distinct runs nor two stretches
        m = re.search(r"capacity_turnover_(\d+)", case.name)
        if m:
            assert n == int(m.group(1)) and cap == (8192 if n <= 4096 else 16384)
    else:
        assert cap == HT.MERGE_SLOTS and f["n_groups"] <= HT.MERGE_GROUP_LIMIT and len(case.partitions[0]) >= 3
        at = 0
        for b, g in zip(case.partitions[0], f["groups_per_batch"]):
            nb = og.batch_len(b)
            assert 0 < nb < 256 and len(set(images[at:at + nb])) == g <= HT.REGISTER_GROUPS       # one workgroup per batch holds them
            at += nb
    fam = f.get("family")
    if fam is not None:
        cluster = [HT.image(HT.AGG_FORM, k) for k in fam.cluster]
        assert set(cluster) <= set(images) and fam.cap == cap
        if fam.name == "wrap_cluster":
            assert len(cluster) == 12 and {home(k) for k in cluster} == {cap - 1, cap - 2}
        elif fam.name == "equal_hash":
            assert len(cluster) >= 5 and len({HT.hash_key(*k) for k in cluster}) == 1
        else:
            for x, y, differs in fam.facts["pairs"]:
                ix, iy = HT.image(HT.AGG_FORM, x), HT.image(HT.AGG_FORM, y)
                assert home(ix) == home(iy) and ((ix[0] == iy[0] and ix[1] != iy[1]) if differs == "last" else (ix[1] == iy[1] and ix[0] != iy[0]))
    else:                                                   # the nullable key: one k0, the spill byte alone differs, three at one home
        shared = [HT.packed_key([("Int64", v, True)]) for v in f["shared_home"]]
        assert len(shared) == 3 and len({k[0] for k in shared}) == 1 and len({k[1] for k in shared}) == 3 and len({home(k) for k in shared}) == 1
        assert set(shared) <= set(images) and (0, 0) in images and (1, 0) in images
        valid = [k for k in images if k not in ((0, 0), (1, 0))]
        assert len({k[0] for k in valid}) == 1 and len(set(valid)) == HT.SPILL_GROUPS and t["k"].valid is not None
    # the restated table finds the groups of the dict
    count, table = HT.restated_group_count(case)
    assert count == f["n_groups"] == og.batch_len(HT.expected_groups(case))
    if fam is not None and fam.facts["crosses_zero"]:
        slots = set(table.occupied())
        assert {cap - 2, cap - 1, 0, 1, 2, 9} <= slots


@pytest.mark.parametrize("case", AGG_CASES, ids=AGG_IDS)
def test_dict_aggregate_equals_the_oracle(case):
    """og.hash_aggregate is what oracle/plan_eval.py evaluates a HashAggregateExec with"""
    want = og.hash_aggregate(HT.agg_table(case), "Partial", case.group, case.aggs)
    helpers.assert_rows_equal(HT.expected_groups(case), want, ordered=False, key_cols=HT.agg_key_names(case))


def test_every_family_runs_on_every_table_it_exists_for():
    names = set(AGG_IDS)
    for route in ("rows", "runs", "merge"):
        for fam in HT.AGG_FAMILIES:
            assert "%s/%s" % (route, fam) in names
    assert {"rows/capacity_turnover_512", "rows/capacity_turnover_513", "runs/capacity_turnover_4096", "runs/capacity_turnover_4097"} <= names
    assert ("merge", "capacity_turnover") in HT.AGG_LEFT_OUT and not any(n.startswith("merge/capacity") for n in names)
    built = {(HT.FAMILY_IDS[f][0], form) for f, form, _ in HT.JOIN_CASES}
    assert built | set(HT.LEFT_OUT) == {(f, form) for f in HT.FAMILIES for form in HT.FORMS} and not built & set(HT.LEFT_OUT)


# ---- discrimination ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mistake", [m for m in HT.MISTAKES if m is not None])
def test_every_mistake_changes_the_cases_named_for_it(mistake):
    named = HT.discrimination()[mistake]
    assert named
    for entry in named:
        if entry[0] == "join":
            _, family_id, form, variation = entry
            left, right, _, _ = HT.join_sides(family_id, form, variation)
            build, probe = HT.row_keys(left, "l", form), HT.row_keys(right, "r", form)
            right_pairs = set(HT.restated_pairs(form, build, probe)[0])
            wrong = set(HT.restated_pairs(form, build, probe, mistake)[0])
            assert wrong != right_pairs, entry
            if mistake in ("no_wrap", "stop_at_foreign_tag"):
                assert wrong < right_pairs, entry           # pairs go missing
            elif mistake in ("tag_is_key", "hash_is_key"):
                assert wrong - right_pairs, entry           # pairs of different keys appear
        else:
            case = HT.find_agg(entry[1])
            assert HT.restated_group_count(case, mistake)[0] != case.facts["n_groups"], entry


def test_discrimination_table_covers_every_mistake():
    d = HT.discrimination()
    assert list(d) == [m for m in HT.MISTAKES if m is not None]
    for forms in ({e[2] for e in d[m] if e[0] == "join"} for m in ("tag_is_key", "no_wrap", "stop_at_foreign_tag")):
        assert forms == set(HT.FORMS)                       # every key form of the general table
    assert {e[2] for e in d["hash_is_key"] if e[0] == "join"} == {"packed2", "wide3"}
    for m in ("k0_only", "no_wrap", "hash_is_key"):        # the three untagged tables as well
        assert {e[1].split("/")[0] for e in d[m] if e[0] == "agg"} == {"rows", "runs", "merge"}
