"""CPU tier of the wide-key aggregate tests: every case of wide_agg_cases.py IS what it says — its colliding keys are pairwise different
and start at the stated slot, its chain wraps past slot 0, its boundary values straddle the packed key's share by one byte, and each
wrong equality (and a probe loop without the wrap) changes the number of groups of the case built against it, while the right one
gives the oracle's — computed with the restated hash and slot arithmetic and with constants looked up in the sources."""
import glob
import os
import re

import numpy as np
import pytest

from oracle import engine as og

import join_route_cases as RC
import repartition_cases as RP
import wide_agg_cases as W

DISCRIMINATION = W.discrimination()


# ---- the constants the GPU tier leans on ----------------------------------------------------------------------------------------------------

def test_constants_are_the_sources():
    wide, agg = W.source_text("host/ops_agg_wide.cpp"), W.source_text("host/ops_agg.cpp")
    assert W.HINT_SOURCE in wide and W.HINT_ROWS == 4096
    assert "constexpr int VM_MAX_COLS = %d;" % W.MAX_GROUP_EXPRS in W.source_text("vm_isa.h")
    assert 'if (group_.size() > (size_t)VM_MAX_COLS) fail(BHIP_ENOTIMPL, "%s");' % W.MESSAGES["too_many"] in wide
    assert "struct WideKeyCols { ColumnRef col[VM_MAX_COLS]; int32_t n; int32_t pad; };" in W.source_text("host/hash_kernels.h")
    assert 'const char* const kRepName = "__group_rep";' in wide
    assert """fail(BHIP_EINVAL, std::string("column name '") + kRepName + "' is reserved");""" in wide
    for line in W.HEAD_SOURCE:
        assert line in agg, line
    assert (W.HEAD_ROWS, W.HEAD_SAMPLE) == ((1 << 17) + 1, 32768)
    # the three messages are raised as a KeyWidthError, the type the wide-key routes catch: by nobody else, and nobody reads an error's text
    assert 'fail_key_width("%s");' % W.MESSAGES["layout"] in W.source_text("host/expr.cpp")
    assert 'fail_key_width("%s");' % W.MESSAGES["value"] in W.source_text("host/ops_basic.cpp")
    assert 'fail_key_width("%s");' % W.MESSAGES["key_parts"] in W.source_text("host/expr.cpp")
    host = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(RC.CSRC, "host", "*"))}
    assert sum(text.count("fail_key_width(") for name, text in host.items() if name.endswith(".cpp")) == 3
    assert "[[noreturn]] inline void fail_key_width(const std::string& m) { throw KeyWidthError(m); }" in host["core.hpp"]
    assert "explicit KeyWidthError(const std::string& m) : Error(BHIP_ENOTIMPL, m) {}" in host["core.hpp"]
    for name, text in host.items():
        assert "key_width_error" not in text and "what()).find" not in text and "m.find(" not in text, name
    assert wide.count("catch (const KeyWidthError&)") == 2 and host["ops_join.cpp"].count("catch (const KeyWidthError&)") == 3
    for line in W.ELISION_SOURCE:
        assert line in wide, line
    assert RC.TABLE_CAPACITY_SOURCE in W.source_text("host/core.hpp")
    assert "const uint64_t cap = table_capacity((uint64_t)n);" in wide
    assert [RC.table_capacity(n) for n in (1, 511, 512, 513, 4097, W.BIG)] == [1024, 1024, 1024, 2048, 16384, 262144]
    assert W.BIG == 2 * 35_000 and RC.table_capacity(W.BIG) == 2 * 2 * 65536       # (the table of 70 000 distinct keys is 53 % of a half)


def test_slot_arithmetic_is_the_kernels():
    """the slot is mix64(row hash) & mask, the row hash the one the repartitioning tests restate (hash_row: -0.0 folded onto +0.0, a NULL
    as the Int64 "nullnull")"""
    kernel = W.source_text("kernels_hash.hip")
    assert "uint64_t slot = mix64(hashes2 ? mix64(hashes[row] ^ hashes2[row]) : hashes[row]) & mask;" in kernel
    assert "slot = (slot + 1) & mask;" in kernel[kernel.index("wide_key_assign_kernel("):kernel.index("struct alignas(16) NarrowSlot64")]
    scan = W.source_text("kernels_scan.hip")
    assert "uint64_t bits = 0x%Xull;" % W.NULL_BITS in scan and "h = mix64(h ^ bits);" in scan
    assert W.NULL_BITS == int.from_bytes(b"nullnull", "big") == RP.NULL_BITS
    assert int(RP.mix64(np.uint64(12345))) == RC.mix64(12345)                       # the two restatements of mix64 are one function
    h = RP.restated_hash([og.OCol("Int64", [7])])
    assert int(W.slots_of(h, 1024)[0]) == RC.mix64(RC.mix64(7)) & 1023


def test_equality_function_has_the_branches_the_cases_aim_at():
    kernel = W.source_text("kernels_hash.hip")
    body = kernel[kernel.index("__device__ inline bool wide_keys_equal("):kernel.index("wide_key_assign_kernel(")]
    for line in ("if (va != vb) return false;", "if (!va) continue;", "case DT_UTF8: {", "if (a1 - a0 != b1 - b0) return false;", "case DT_BOOLEAN: {",
                 "if (dt_load(r.dtype, r.data, a) != dt_load(r.dtype, r.data, b)) return false;"):
        assert line in body, line


# ---- A. equality ---------------------------------------------------------------------------------------------------------------------------------

def test_equality_cases_cover_the_types_and_values_of_the_issue():
    assert list(W.VALUES) == ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64", "Date32", "Date64", "Timestamp(Microsecond)",
                              "Float32", "Float64", "Boolean", "Utf8"]
    for t, vals in W.VALUES.items():
        assert None in vals and len(set(vals)) == len(vals), t
    for t in ("Int8", "Int16", "Int32", "Int64"):
        bits = 8 * np.dtype(og.NP_TYPES[t]).itemsize
        assert {0, 1, -1, -(1 << (bits - 1)), (1 << (bits - 1)) - 1} <= set(W.VALUES[t])
    f64 = np.array([v for v in W.F64_VALUES if v is not None], np.uint64).view(np.float64)
    f32 = np.array([v for v in W.F32_VALUES if v is not None], np.uint32).view(np.float32)
    for f in (f64, f32):
        assert np.isnan(f).sum() == 3 and np.isinf(f).sum() == 2 and (f == 0).sum() == 2 and np.signbit(f[f == 0]).sum() == 1
        assert ((f != 0) & (np.abs(f) < np.finfo(f.dtype).tiny)).sum() == 1         # a subnormal
    # quiet NaNs only: widening a Float32 keeps their payloads apart
    assert all(v & 0x00400000 for v in W.F32_VALUES if v is not None and (v & 0x7FFFFFFF) > 0x7F800000)
    u = W.UTF8_VALUES
    assert {"", None, "a", "a\x00", "ab"} <= set(u)
    long_ = [x for x in u if x is not None and len(x.encode()) == 40]
    assert len(long_) == 3 and long_[0][:-1] == long_[1][:-1] and long_[0][-1] != long_[1][-1] and long_[0][1:] == long_[2][1:] and long_[0][0] != long_[2][0]
    assert "é".encode() == b"\xc3\xa9" and "ê".encode() == b"\xc3\xaa" and "ĩ".encode() == b"\xc4\xa9" and {"é", "ê", "ĩ"} <= set(u)
    assert W.UTF8_PAIRS == [(("ab", "c"), ("a", "bc")), (("", "x"), ("x", ""))]


@pytest.mark.parametrize("case", W.EQUALITY_CASES, ids=lambda c: c.name)
def test_equality_pairs_share_their_slot(case):
    """the two keys of every pair differ in exactly one of k1 / k2 (or swap a NULL between them, or agree once concatenated), all keys are
    pairwise different, and both keys of a pair start at the same slot of the table the route will make — only then does wide_keys_equal
    ever see them side by side"""
    t = W.table_of(case)
    n = og.batch_len(t)
    names = W.keys_of(case)
    assert case.facts["capacity"] == RC.table_capacity(n) and names[-1] == "salt"
    K = W.cells_of(t, names)
    slot = W.slots_of(np.array(K.hashes, np.uint64), case.facts["capacity"])
    by_salt = {}
    for r in range(n):
        by_salt.setdefault(K.cols[-1][r][1], {})[tuple(c[r] for c in K.cols[:-1])] = int(slot[r])
    assert len(by_salt) == case.facts["pairs"] and sum(len(v) for v in by_salt.values()) == case.facts["n_groups"] == 2 * case.facts["pairs"]
    one_column = 0
    for salt, keys in by_salt.items():
        (ka, sa), (kb, sb) = keys.items()
        assert sa == sb, (salt, ka, kb)
        assert ka != kb
        one_column += sum(x != y for x, y in zip(ka, kb)) == 1
    assert one_column >= case.facts["pairs"] - 3                                     # all but (NULL, base) / (base, NULL) and the two Utf8 pairs
    # wide: by layout, or by the 40-byte partner beside a layout that fits
    ok, longest = W.packed_layout(W.key_parts(case))
    assert not ok or longest < len(W.LONG.encode())
    assert W.restated_group_count(case) == W.oracle_group_count(case) == case.facts["n_groups"]


def test_arrow_slice_case():
    rb, case = W.arrow_slice_case()
    t = W.table_of(case)
    assert rb.offset if hasattr(rb, "offset") else True
    assert all(col.offset == W.ARROW_START for col in rb.columns) and W.ARROW_START % 8 != 0 and rb.num_rows == W.ARROW_ROWS > 64
    for name in t:
        assert rb.column(name).to_pylist() == t[name].to_pylist(), name
    # two NULL keys never store the same bytes, and some group holds several NULL rows
    for name in ("a", "s"):
        under = [v for v, ok in zip(t[name].values.tolist(), t[name].is_valid().tolist()) if not ok]
        assert len(under) > 10 and len(set(under)) == len(under)
    assert W.restated_group_count(case) == W.oracle_group_count(case) == case.facts["n_groups"]
    assert W.restated_group_count(case, W.WRONG["null_payload_compared"]) > case.facts["n_groups"]


# ---- B. collisions ---------------------------------------------------------------------------------------------------------------------------------

def test_slot_collision_case():
    tri, slot = W.collision_draw()
    cap = W.COLLISION_CAPACITY
    assert len(tri) == 1 << 17 and int(((slot == cap - 2) | (slot == cap - 1)).sum()) >= 2 * 64
    case = W.slot_collision_case()
    t = W.table_of(case)
    n = og.batch_len(t)
    assert n < 512 and RC.table_capacity(n) == cap == case.facts["capacity"] == 1024
    keys = W.key_list(case)
    assert len(keys) == len(set(keys)) == W.COLLISION_KEYS >= 64 and [k.dtype for k in t.values()][:3] == ["Int64"] * 3
    K = W.cells_of(t, W.keys_of(case))
    home = W.slots_of(np.array(K.hashes, np.uint64), cap)
    assert set(home.tolist()) == {cap - 2, cap - 1} == set(case.facts["slots"])
    counts = np.unique(np.array([hash(tuple(c[r] for c in K.cols)) for r in range(n)]), return_counts=True)[1]
    assert counts.min() >= 4                                                          # several rows each
    assert not np.all(np.diff(t["a"].values) >= 0)                                    # shuffled
    rep, table = W.group_by_representatives(K, cap)
    occupied = [s for s, o in enumerate(table) if o is not None]
    assert occupied == list(range(0, W.COLLISION_KEYS - 2)) + [cap - 2, cap - 1] or occupied == list(range(0, W.COLLISION_KEYS - 1)) + [cap - 1]
    assert len(set(rep)) == W.oracle_group_count(case) == W.COLLISION_KEYS


@pytest.mark.parametrize("case", W.equal_hash_cases(), ids=lambda c: c.name)
def test_equal_hash_cases(case):
    t = W.table_of(case)
    K = W.cells_of(t, W.keys_of(case))
    keys = W.key_list(case)
    assert len(keys) == len(set(keys)) == case.facts["n_groups"] == 5
    by_hash = {}
    for r in range(og.batch_len(t)):
        by_hash.setdefault(K.hashes[r], set()).add(tuple(c[r] for c in K.cols))
    assert sorted(len(v) for v in by_hash.values()) == [1, 2, 2]
    want = {(True, 0), (True, 1 << 63)} if case.name == "equal_hash_zeros" else {(False, W.NULL_BITS), (True, W.NULL_BITS)}
    for same in by_hash.values():
        if len(same) == 2:                                                            # equal hashes, equal b and c, and the stated first cells
            ka, kb = same
            assert ka[1:] == kb[1:] and {ka[0], kb[0]} == want
    assert W.restated_group_count(case) == W.oracle_group_count(case) == 5


# ---- discrimination ---------------------------------------------------------------------------------------------------------------------------------

def test_every_wrong_equality_of_the_issue_has_a_case():
    assert list(DISCRIMINATION) == ["validity_ignored", "null_payload_compared", "utf8_length_ignored", "utf8_first_15_bytes", "utf8_concatenated",
                                    "zeros_equal", "nans_equal", "boolean_ignored", "equal_hash_is_equal_key", "no_wrap"]
    assert set(DISCRIMINATION) == set(W.WRONG) | {"no_wrap"} and all(DISCRIMINATION.values())


@pytest.mark.parametrize("wrong", list(DISCRIMINATION))
def test_wrong_equality_changes_the_group_count(wrong):
    for case in DISCRIMINATION[wrong]:
        right = W.restated_group_count(case)
        assert right == W.oracle_group_count(case) == case.facts["n_groups"], case.name
        got = W.restated_group_count(case, wrap=False) if wrong == "no_wrap" else W.restated_group_count(case, W.WRONG[wrong])
        assert got != right, (wrong, case.name, got)


# ---- C. sizes ----------------------------------------------------------------------------------------------------------------------------------------

def test_size_cases():
    assert W.SIZES == [1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097] and W.SHAPES == ["one_group", "all_distinct", "two_alternating", "sqrt_groups"]
    assert RC.table_capacity(512) < RC.table_capacity(513) and W.HINT_ROWS in W.SIZES and W.HINT_ROWS - 1 in W.SIZES
    for n in (1, 2, 65, 513, 4097):
        for shape in W.SHAPES:
            case = W.size_case(shape, n)
            rows = [og.batch_len(b) for b in case.partitions[0]]
            assert len(case.partitions) == 1 and rows == [n // 2, 0, n - n // 2]
            want = {"one_group": 1, "all_distinct": n, "two_alternating": min(n, 2)}.get(shape, case.facts["n_groups"])
            assert case.facts["n_groups"] == want == W.oracle_group_count(case), case.name
            assert case.facts["hash_inner"] == (n >= 4096)
            ok, _ = W.packed_layout(W.key_parts(case))
            assert not ok                                                             # three Int64: wide by layout
        assert 1 <= W.size_case("sqrt_groups", n).facts["n_groups"] <= max(1, int(n ** 0.5))
    v = W.size_case("all_distinct", 4097).partitions[0][2]["v"]
    assert np.all(v.values * 8 == np.round(v.values * 8)) and np.abs(v.values).max() <= 4 and not v.is_valid().all()
    # the table of all-distinct keys is exactly half full where 2 n is a power of two
    assert RC.table_capacity(512) == 2 * 512 and RC.table_capacity(4096) == 2 * 4096


# ---- D. the fall-over ----------------------------------------------------------------------------------------------------------------------------------

def test_layout_rule_is_the_builders():
    expr = W.source_text("host/expr.cpp")
    for line in W.LAYOUT_SOURCE:
        assert line in expr, line
    assert W.TOO_LONG_SOURCE in W.source_text("vm_device.h")
    assert "else { k.kind = dt_is_float(t) ? KP_VSLOT_F64 : KP_VSLOT; k.width = t == DT_FLOAT32 ? 8 : dtype_width(t); }" in expr
    assert "k.width += nullable ? 1 : 0;" in expr
    # the outcomes other tests pin: 15 bytes are the most a lone Utf8 key holds; a 10-byte string beside an Int32 fits
    p15 = re.search(r'^P15 = "([A-Z]+)"\s+# 15 bytes: the most a single Utf8 join key holds in the packed key$', W.tests_file_text("test_join_wide_keys_gpu.py"), re.M)
    assert p15 and len(p15.group(1)) == 15 == W.fits("utf8")
    ten = re.search(r'\("([A-Z]+)", "x"\),\s+# 10 bytes \(\+ the Int32 part = the 16-byte packed key\)', W.tests_file_text("test_lean_gpu.py"))
    assert ten and len(ten.group(1)) == 10 <= W.fits("utf8_int32")
    assert [W.fits(k) for k in W.LAYOUTS] == [15, 11, 7]
    assert W.packed_layout([("Int64", False), ("Int64", False)]) == (True, None) and W.packed_layout([("Int64", False)] * 3) == (False, None)
    assert W.packed_layout([("Int64", True), ("Int64", False)]) == (False, None)      # the NULL byte is the seventeenth
    assert W.packed_layout([("Utf8", False)] * 8) == (True, 1) and W.packed_layout([("Utf8", False)] * 9) == (False, None)


@pytest.mark.parametrize("layout", list(W.LAYOUTS))
def test_fallover_values_straddle_the_share(layout):
    fit = W.fits(layout)
    for where in W.FALLOVER_WHERE:
        case = W.fallover_case(layout, where)
        assert W.key_parts(case) == W.LAYOUT_PARTS[layout]                            # NULL-free key columns: no NULL byte in the layout
        assert W.packed_layout(W.key_parts(case)) == (True, fit)
        lens = [[len(s.encode()) for s in b["s"].values] for part in case.partitions for b in part]
        flat = [x for b in lens for x in b]
        longest_other = max(len(s.encode()) for part in case.partitions for b in part for s in b["t"].values)
        assert longest_other <= W.fits("two_utf8")
        if where == "fits":
            assert max(flat) == fit and case.facts["wide"] is False
            continue
        assert sorted(flat)[-2:] == [fit, fit + 1] and flat.count(fit + 1) == 1       # the value that fits is there too, one byte shorter
        at = {"row_0": (0, 0), "last_row": (2, -1), "filtered": (1, W.FALLOVER_ROWS // 2 - W.FALLOVER_ROWS // 3), "partition_1": (1, W.FALLOVER_ROWS // 2),
              "after_hint": (1, -1)}[where]
        assert lens[at[0]][at[1]] == fit + 1, where
        t = W.table_of(case)
        long_row = flat.index(fit + 1)
        assert (t["f"].values <= 0.5).tolist() == [r == long_row for r in range(len(flat))]
        if where == "filtered":
            kept = og.filter_batch(t, W.KEEP)
            assert max(len(s.encode()) for s in kept["s"].values) == fit and case.facts["wide"] is None
        if where in ("partition_1", "after_hint"):
            assert len(case.partitions) == 2 and max(lens[0]) <= fit
        if where == "after_hint":                                                     # partition 0: many rows, three groups, short keys
            p0 = case.partitions[0][0]
            assert og.batch_len(p0) == 3000 and og.batch_len(og.hash_aggregate(p0, "Partial", case.group, case.aggs)) == 3


def test_head_sample_case():
    case = W.head_sample_case()
    (t,), = case.partitions
    assert og.batch_len(t) == W.HEAD_ROWS == (1 << 17) + 1 and len(case.aggs) == case.facts["accumulators"] > 4
    lens = np.array([len(s) for s in t["s"].values])
    assert lens[-1] == 16 > W.fits("utf8") and lens[:-1].max() == 1 and np.nonzero(lens > 1)[0].tolist() == [W.HEAD_ROWS - 1]
    assert W.HEAD_ROWS - 1 >= W.HEAD_SAMPLE and len(set(t["s"].values[:W.HEAD_SAMPLE])) == 3 <= 4
    # (no fast path measures the keys first: that needs more than 2 bytes per value on average)
    assert "b0.cols[ci].data_bytes <= 2 * b0.n_rows" in W.source_text("host/ops_agg.cpp") and lens.sum() <= 2 * W.HEAD_ROWS


# ---- E, F, G ---------------------------------------------------------------------------------------------------------------------------------------------

def test_mode_table():
    t = W.mode_table()
    n = og.batch_len(t)
    g = np.array([int(s[-2:]) for s in t["s"].values])
    assert set(g.tolist()) == set(range(W.MODE_GROUPS)) and min(len(s) for s in t["s"].values) > W.fits("utf8")
    dead = g == W.NULL_GROUP
    assert dead.sum() > 10
    for name, dtype in (("x", "Int32"), ("y", "Float32"), ("z", "Float64")):
        assert t[name].dtype == dtype and not t[name].is_valid()[dead].any() and 0 < t[name].is_valid()[~dead].mean() < 1
    assert np.all(t["y"].values.astype(np.float64) * 8 == np.round(t["y"].values.astype(np.float64) * 8))
    parts = W.mode_partitions(2)
    a, b = (set(p[0]["s"].values) for p in parts)
    assert len(parts) == 2 and a == b and len(a) == W.MODE_GROUPS                    # every wide key in both partitions' states
    assert [f.fun for f in W.MODE_AGGS[:3]] == ["AVG"] * 3 and W.MODE_STRING_AGGS[-1].fun == "MIN"
    want = og.hash_aggregate(t, "Partial", W.MODE_KEYS, W.MODE_AGGS)
    dead_out = np.array([s.endswith("%02d" % W.NULL_GROUP) for s in want["s"].values])
    assert dead_out.any() and not want["az[sum]"].is_valid()[dead_out].any() and not want["sz[sum]"].is_valid()[dead_out].any()
    assert (want["cz[count]"].values[dead_out] == 0).all() and (want["az[count]"].values[dead_out] == 0).all()


def test_string_tables():
    t = W.string_minmax_table()
    by_group = {}
    for s, m in zip(t["s"].values, t["m"].to_pylist()):
        by_group.setdefault(s, []).append(m)
    assert min(len(s) for s in by_group) > W.fits("utf8_int32")
    sets = [set(v) for v in by_group.values()]
    assert {None} in sets and {""} in sets and any("" in s and len(s) > 2 for s in sets)
    assert any(v.count("same") > 1 for v in by_group.values()) and any(max(x.encode()) >= 0x80 for s in sets for x in s if x)
    e = W.string_expr_table()
    assert all(s.isascii() for s in e["a"].values)                                   # lower() of other text is declined
    assert e["cc"].to_pylist() == [None if x is None or y is None else x + y for x, y in zip(e["a"].to_pylist(), e["b"].to_pylist())]
    assert not e["a"].is_valid().all() and not e["b"].is_valid().all()
    for name, (device_keys, oracle_keys) in W.STRING_EXPR_KEYS.items():
        want = og.hash_aggregate(e, "Partial", oracle_keys, W.VALUE_AGGS)
        assert [n for _, n in device_keys] == [n for _, n in oracle_keys]
        assert max(len(s.encode()) for s in want["k"].values) > W.fits("utf8"), name   # the values outgrow the packed key


def test_many_keys_cases():
    for n_keys in (16, 17):
        case = W.many_keys_case(n_keys)
        assert len(case.group) == n_keys and (n_keys <= W.MAX_GROUP_EXPRS) == (n_keys == 16)
        assert case.facts["n_groups"] == W.oracle_group_count(case) >= 40
        assert W.packed_layout(W.key_parts(case)) == (False, None)
    # groups that differ only in a column past the eighth (the second hash pass)
    t = W.many_keys_table(16)
    rows = set(zip(*[t["k%d" % j].to_pylist() for j in range(16)]))
    assert len(set(r[:8] for r in rows)) < len(rows)


def test_no_aggregate_shares_a_name_with_a_key():
    """(a Final's result would hold two columns of one name, and the comparison would see only the later one)"""
    cases = W.EQUALITY_CASES + [W.arrow_slice_case()[1], W.slot_collision_case(), W.head_sample_case(), W.many_keys_case(16)] + W.equal_hash_cases()
    cases += [W.size_case(s, 65) for s in W.SHAPES] + [W.fallover_case(k, w) for k in W.LAYOUTS for w in W.FALLOVER_WHERE]
    pairs = [(c.group, c.aggs) for c in cases] + [(W.MODE_KEYS, W.MODE_STRING_AGGS), (W.MODE_KEYS, W.STRING_AGGS)]
    pairs += [(keys, W.VALUE_AGGS) for keys, _ in W.STRING_EXPR_KEYS.values()]
    for group, aggs in pairs:
        names = [n for _, n in group] + [a.name for a in aggs]
        assert len(set(names)) == len(names), names
