// ops_join.cpp — HashJoinExec (Inner / Left / Right / Full, and the existence joins Semi / Anti / RightSemi / RightAnti), left = build side.
//
// Reference: HashJoinExec::try_new(left, right, on: &[(String, String)], join_type) built at
// rust/core/src/serde/physical_plan/from_proto.rs:253-276 (join types :268-272, key pairs by
// column NAME :256-260); the 4-argument constructor of that DataFusion revision is the
// collect-left mode: every task drains the whole left child and probes it with one right
// partition.  Output schema = left fields then right fields, a right key column
// dropped when it has the same name as its left partner (Appendix A).  Row order unspecified.
// The existence joins put ONE side in the output, unchanged: Semi / Anti the build rows with / without a partner, RightSemi /
// RightAnti the probe rows.  NULL keys never match, so Anti and RightAnti emit the rows that have one (NOT EXISTS semantics).
// And NestedLoopJoinExec, the join without a key (the last section): its own front end over the same probe tail (JoinExec::Probe).
#include <mutex>

#include "../nljoin_kernels.h"
#include "../util_kernels.h"
#include "hash_kernels.h"
#include "plan.hpp"
#include "sop.hpp"

namespace bhip {

// the keys of one side's rows in the form of a general table (side_keys): packed 16-byte keys, or (wide) 64-bit row hashes and the
// key columns themselves; and the selection of the rows without a NULL key part
struct SideKeys {
    BufferPtr keys, sel;            // 2 x u64 per row (packed) / one row hash per row (wide); sel: only with has_sel
    bool has_sel = false;
    WideKeyCols cols = {};          // wide: the key columns (n = 0: the packed form)
    JoinSideKeys view() const {
        return JoinSideKeys{keys ? keys->as<uint64_t>() : nullptr, has_sel ? sel->as<uint64_t>() : nullptr, cols.n ? &cols : nullptr};
    }
};

// the general table's kernels under the names profiles, DESIGN.md and the tests know them by: the packed form's, "_wide" for the other
enum JoinKernel { K_BUILD, K_PROBE_COUNT, K_PROBE_EMIT, K_PROBE_MATCH, K_PROBE_EXISTS, K_EXISTS_FLAGS };
static const char* kernel_name(JoinKernel k, bool wide) {
    static const char* const names[][2] = {{"join_build", "join_build_wide"},
                                           {"join_probe_count", "join_probe_count_wide"},
                                           {"join_probe_emit", "join_probe_emit_wide"},
                                           {"join_probe_match", "join_probe_match_wide"},
                                           {"join_probe_exists", "join_probe_exists_wide"},
                                           {"join_exists_flags", "join_exists_flags_wide"}};
    return names[k][wide ? 1 : 0];
}

struct JoinBuildSide {
    BatchPtr batch;                 // all left rows
    SideKeys keys;                  // general table: the build rows' keys in its form (table.keys128 / table.cols point into it; a wide
                                    // table's row hashes are dropped after the build)
    BufferPtr owner, head, next, dup;
    JoinTable table;
    bool unique = false;            // no two build rows share a key: probe rows have at most one partner
    bool wide = false;              // keys of any width: `table` over row hashes, equality on the key columns keys.cols of `batch`
    bool narrow = false;            // ONE integer key, unique: NarrowJoinTable instead of JoinTable
    int narrow_width = 0;           // its key bytes (4: Int32 / Date32, 8: Int64 / UInt64)
    BufferPtr slots, present, rpack, rbits, rperm;
    NarrowJoinTable ntable;
    Column key_holder;              // two-column join: the key column built for it (packed pair, or the first key with both validities)
    bool resid = false;             // two-column join by the first key; the second is compared on every match (ntable.resid_build)
};

static const char* join_name(int t) {
    static const char* const names[] = {"Inner", "Left", "Right", "Full", "Semi", "Anti", "RightSemi", "RightAnti"};
    return names[t];
}
// the answer is per BUILD row (the output holds left columns only) / per PROBE row (right columns only)
static bool build_existence(int t) { return t == BHIP_JOIN_SEMI || t == BHIP_JOIN_ANTI; }
static bool probe_existence(int t) { return t == BHIP_JOIN_RIGHT_SEMI || t == BHIP_JOIN_RIGHT_ANTI; }
// a right key column named like its left partner: the Inner join's output schema keeps the left one only
static bool named_like_left_key(const std::vector<std::pair<std::string, std::string>>& on, const std::string& right_name) {
    for (auto& p : on)
        if (p.second == right_name && p.first == p.second) return true;
    return false;
}

HashJoinExec::HashJoinExec(PlanPtr left, PlanPtr right, std::vector<std::pair<std::string, std::string>> on, int join_type, ExprPtr filter)
    : JoinExec(std::move(left), std::move(right), join_type, std::move(filter)), on_(std::move(on)) {
    ctx_ = left_->context();
    if (join_type < BHIP_JOIN_INNER || join_type > BHIP_JOIN_RIGHT_ANTI) fail(BHIP_ENOTIMPL, "Unsupported join type");
    // a build row's fate depends on every probe row, and a stream sees one right partition (Left emits its unmatched rows once
    // per task and stays that way; the types added after it do not inherit that)
    if ((join_type == BHIP_JOIN_FULL || build_existence(join_type)) && right_->output_partitioning().count > 1)
        fail(BHIP_ENOTIMPL, std::string(join_name(join_type)) + " join over a right child of " + std::to_string(right_->output_partitioning().count) +
                                " partitions: put a MergeExec under the right child");
    const Schema& ls = *left_->schema();
    const Schema& rs = *right_->schema();
    for (auto& p : on_) {
        const int li = ls.index_of(p.first), ri = rs.index_of(p.second);
        if (li < 0) fail(BHIP_EINVAL, "The left side of the join does not have column '" + p.first + "'");
        if (ri < 0) fail(BHIP_EINVAL, "The right side of the join does not have column '" + p.second + "'");
        if (ls.fields[li].dtype != rs.fields[ri].dtype)
            fail(BHIP_EINVAL, "join keys " + p.first + " / " + p.second + " have different types (" +
                                  dtype_name(ls.fields[li].dtype) + " vs " + dtype_name(rs.fields[ri].dtype) + ")");
        left_keys_.push_back(p.first);
    }
    auto s = std::make_shared<Schema>();
    const bool left_nullable = join_type == BHIP_JOIN_RIGHT || join_type == BHIP_JOIN_FULL;
    const bool right_nullable = join_type == BHIP_JOIN_LEFT || join_type == BHIP_JOIN_FULL;
    for (auto f : ls.fields) {
        if (probe_existence(join_type)) break;
        if (left_nullable) f.nullable = true;
        s->fields.push_back(f);
    }
    for (size_t i = 0; i < rs.fields.size(); ++i) {
        if (build_existence(join_type)) break;
        if (!probe_existence(join_type) && named_like_left_key(on_, rs.fields[i].name)) continue;
        Field f = rs.fields[i];
        if (right_nullable) f.nullable = true;
        if (s->index_of(f.name) >= 0) fail(BHIP_EINVAL, "join output would have two columns named '" + f.name + "'");
        s->fields.push_back(f);
        right_cols_.push_back((int)i);
    }
    schema_ = s;
    if (filter_) check_filter(on_);
    // key layout must be valid (surfaces BHIP_ENOTIMPL at plan time); one the packed key cannot hold goes to the wide-key table,
    // whose row-hash program has to be valid instead
    ScanParams P;
    try {
        ProgramBuilder pb(ls);
        for (auto& k : left_keys_) pb.add_key(make_column(k), true);
        pb.finish(P);
    } catch (const KeyWidthError&) {
        static_wide_ = true;
        ProgramBuilder hb(ls);
        hb.set_hash_only();
        for (auto& k : left_keys_) hb.add_key(make_column(k), true);
        hb.finish(P);
    }
    cache_ = std::make_shared<BuildCache>();
}

// The residual filter is typed against the Inner join's output schema whatever the join type: the left fields, then the right fields
// minus a right key column named like its left partner (the name then means the left column).  The checks are FilterExec's.
void JoinExec::check_filter(const std::vector<std::pair<std::string, std::string>>& on) {
    const Schema &ls = *left_->schema(), &rs = *right_->schema();
    Schema fs;
    std::vector<FilterCol> origin;
    for (size_t i = 0; i < ls.fields.size(); ++i) {
        fs.fields.push_back(ls.fields[i]);
        origin.push_back(FilterCol{true, (int)i, ls.fields[i]});
    }
    for (size_t i = 0; i < rs.fields.size(); ++i) {
        if (named_like_left_key(on, rs.fields[i].name)) continue;
        // (the existence types' outputs would not clash, but the filter's schema does: a ProjectionExec renames)
        if (fs.index_of(rs.fields[i].name) >= 0) fail(BHIP_EINVAL, "join output would have two columns named '" + rs.fields[i].name + "'");
        fs.fields.push_back(rs.fields[i]);
        origin.push_back(FilterCol{false, (int)i, rs.fields[i]});
    }
    std::vector<std::string> used;
    collect_columns(filter_, used);
    for (auto& u : used) {
        const int i = fs.index_of(u);
        if (i < 0) fail(BHIP_EINVAL, "No field named '" + u + "'");
        bool seen = false;
        for (auto& fc : filter_cols_) seen = seen || fc.field.name == u;
        if (!seen) filter_cols_.push_back(origin[i]);
    }
    // (a constant filter would run over a batch without columns; TRUE is the unfiltered join, FALSE / NULL a plan without partners)
    if (filter_cols_.empty()) fail(BHIP_ENOTIMPL, "Join filter that reads no column of either side: " + filter_->to_string());
    if (expr_type(filter_, fs) != DT_BOOLEAN)
        fail(BHIP_EINVAL, "Join filter must return boolean values, not " + std::string(dtype_name(expr_type(filter_, fs))));
    Utf8Lowering low(fs);
    const ExprPtr lowered = low.rewrite(filter_);
    low.validate();
    const SchemaPtr aug = low.schema();
    ProgramBuilder pb(*aug);
    pb.set_predicate(lowered);      // surfaces BHIP_ENOTIMPL at plan time
}

PlanPtr HashJoinExec::with_new_children(const std::vector<PlanPtr>& c) const {
    if (c.size() != 2) fail(BHIP_EINVAL, "HashJoinExec wrong number of children");
    return std::make_shared<HashJoinExec>(c[0], c[1], on_, join_type_, filter_);
}

std::string HashJoinExec::describe() const {
    std::string s = std::string("HashJoinExec: mode=CollectLeft, join_type=") + join_name(join_type_) + ", on=[";
    for (size_t i = 0; i < on_.size(); ++i) s += (i ? ", " : "") + std::string("(") + on_[i].first + ", " + on_[i].second + ")";
    s += "]";
    if (filter_) s += ", filter=" + filter_->to_string();
    return s;
}

// the integer key columns that need no packed 16-byte image: 4 (Int32 / Date32), 8 (Int64 / UInt64) bytes wide, else 0
static int int_key_width(int t) { return (t == DT_INT32 || t == DT_DATE32) ? 4 : (t == DT_INT64 || t == DT_UINT64) ? 8 : 0; }

// the keys of the rows of `b` (key columns `cols`) in a general table's form: packed keys, or (wide) row hashes and the key columns;
// and the "no NULL key part" selection
static SideKeys side_keys(const Exec& ex, const Batch& b, const std::vector<std::string>& cols, bool wide) {
    SideKeys k;
    // one NULL-free integer key column (every TPC-H join): the image is a widening copy, no expression program
    if (!wide && cols.size() == 1) {
        const int ci = b.schema->index_of(cols[0]);
        const Column& c = b.cols[ci];
        const int w = int_key_width(c.dtype);
        if (w && !c.validity) {
            k.keys = make_buffer(ex, (size_t)b.n_rows * 16 + 16);
            TIMED_LAUNCH_N(ex, "widen_key", b.n_rows, launch_widen_key(ex.cfg(), c.data->ptr(), w, b.n_rows, k.keys->as<uint64_t>()));
            return k;
        }
    }
    ProgramBuilder pb(*b.schema);
    if (wide) pb.set_hash_only();
    ExprPtr pred;
    for (auto& c : cols) {
        const int ci = b.schema->index_of(c);
        if (b.schema->fields[ci].nullable || b.cols[ci].validity) {
            auto e = std::make_shared<Expr>();
            e->kind = BHIP_EXPR_IS_NOT_NULL;
            e->args = {make_column(c)};
            pred = pred ? make_binary(pred, "And", e) : ExprPtr(e);
        }
        if (wide) k.cols.col[k.cols.n++] = b.cols[ci].ref();
    }
    if (pred) pb.set_predicate(pred);
    for (auto& c : cols) pb.add_key(make_column(c), true);
    ScanParams P;
    pb.finish(P);
    ProgramBuilder::bind(P, pb.columns(), b, pb.creates_nulls());
    k.keys = make_buffer(ex, (size_t)b.n_rows * (wide ? 8 : 16) + 16);
    k.has_sel = (bool)pred;
    if (k.has_sel) k.sel = validity_buffer(ex, b.n_rows);
    if (b.n_rows == 0) return k;
    Temp tmp(ex);
    ScanStatus* st = tmp.get<ScanStatus>(1);
    HIP_CHECK(hipMemsetAsync(st, 0, sizeof(ScanStatus), ex.stream));
    uint64_t* out = k.keys->as<uint64_t>();
    TIMED_LAUNCH_N(ex, "scan_keys", b.n_rows,
                   launch_scan_keys(ex.cfg(), P, wide ? nullptr : out, wide ? out : nullptr, k.has_sel ? k.sel->as<uint64_t>() : nullptr, st));
    check_scan_status(ex, st);
    return k;
}

// TWO key pairs of 4-byte integer columns, the same type on both sides (UInt32 counts here, and not for a single key below)
bool HashJoinExec::pair_keys() const {
    if (on_.size() != 2) return false;
    const Schema &ls = *left_->schema(), &rs = *right_->schema();
    for (auto& p : on_) {
        const int lt = ls.fields[ls.index_of(p.first)].dtype, rt = rs.fields[rs.index_of(p.second)].dtype;
        if ((int_key_width(lt) != 4 && lt != DT_UINT32) || lt != rt) return false;
    }
    return true;
}

// the key column the single-key path works on: the column itself, or the two 4-byte key columns packed into one Int64 column
static Column pack_key_pair(const Exec& ex, const Column& a, const Column& b, int64_t n) {
    Column k = alloc_column(ex, DT_INT64, n, a.validity || b.validity);
    TIMED_LAUNCH_N(ex, "pack_key_pair", n, launch_pack_key_pair(ex.cfg(), a.data->ptr(), b.data->ptr(), a.validity_words(), b.validity_words(), n,
                                                                 k.data->as<uint64_t>(), k.validity_words()));
    return k;
}

// ONE key pair of integer columns of the same width on both sides: 4 (Int32 / Date32), 8 (Int64 / UInt64), else 0; two 4-byte
// pairs count as one 8-byte key
int HashJoinExec::narrow_key_width() const {
    if (pair_keys()) return 8;
    if (on_.size() != 1) return 0;
    const Schema &ls = *left_->schema(), &rs = *right_->schema();
    const int lt = ls.fields[ls.index_of(on_[0].first)].dtype, rt = rs.fields[rs.index_of(on_[0].second)].dtype;
    if (int_key_width(lt) == 4 && int_key_width(rt) == 4) return 4;
    if (lt == rt && int_key_width(lt) == 8) return 8;
    return 0;
}

// A child of a join, executed so that the columns this join only passes on (everything but its keys) may arrive as views: the
// child is a HashJoinExec, or a projection of plain columns over one (the shape of TPC-H's join chains).  Anything else: execute().
static bool join_views_disabled() {
    static const bool no_views = env_flag("BHIP_NO_JOIN_VIEWS");
    return no_views;
}
// the join below a join: its columns `needed` and `keys` come out, and all but `keys` (which the join above reads) may be views
static StreamPtr open_join_below(const HashJoinExec& hj, int partition, const Exec& ex, std::vector<bool> needed, const std::vector<int>& keys) {
    std::vector<bool> defer(needed.size(), true);
    for (int k : keys) { needed[k] = true; defer[k] = false; }
    return hj.execute_needed(partition, ex, needed, defer);
}
static StreamPtr open_join_child(const PlanPtr& child, int partition, const Exec& ex, const std::vector<std::string>& key_names) {
    auto is_key = [&](const std::string& n) { return std::find(key_names.begin(), key_names.end(), n) != key_names.end(); };
    if (join_views_disabled()) return child->execute(partition, ex);
    std::vector<int> keys;
    if (auto hj = dynamic_cast<const HashJoinExec*>(child.get())) {
        const Schema& js = *hj->schema();
        for (size_t i = 0; i < js.fields.size(); ++i)
            if (is_key(js.fields[i].name)) keys.push_back((int)i);
        return open_join_below(*hj, partition, ex, std::vector<bool>(js.fields.size(), true), keys);
    }
    auto pr = dynamic_cast<const ProjectionExec*>(child.get());
    const HashJoinExec* hj = pr ? dynamic_cast<const HashJoinExec*>(pr->input().get()) : nullptr;
    if (!hj) return child->execute(partition, ex);
    const Schema& js = *hj->schema();
    std::vector<int> src;
    std::vector<bool> needed(js.fields.size(), false);
    for (auto& en : pr->exprs()) {
        if (en.first->kind != BHIP_EXPR_COLUMN) return child->execute(partition, ex);
        const int i = js.index_of(en.first->name);
        if (i < 0) return child->execute(partition, ex);
        src.push_back(i);
        needed[i] = true;
        if (is_key(en.second)) keys.push_back(i);                          // a key of the parent join (possibly under another output name too)
    }
    std::shared_ptr<RecordBatchStream> inner(open_join_below(*hj, partition, ex, needed, keys).release());
    const SchemaPtr sch = pr->schema();
    return StreamPtr(new LazyStream(sch, [inner, sch, src]() {
        std::vector<BatchPtr> out;
        while (BatchPtr b = inner->next()) {
            auto nb = new_batch(b->ctx, sch, b->n_rows);
            for (int i : src) nb->cols.push_back(b->cols[i]);
            out.push_back(nb);
        }
        return out;
    }));
}

// ---- build side ------------------------------------------------------------------------------------------------------------

// a finished rank map (bs.rpack, and bs.rbits / bs.rperm where they exist) goes into the table the probe kernels read
static void publish_rank_map(JoinBuildSide& bs, uint64_t kmin, uint64_t range, uint32_t rzero) {
    static const bool no_scalar_map = env_flag("BHIP_PROBE_NO_SCALAR_MAP");
    NarrowJoinTable& T = bs.ntable;
    T.kmin64 = kmin;
    T.kmin = (uint32_t)kmin;
    T.rpack = bs.rpack->as<uint64_t>();
    T.rbits = bs.rbits ? bs.rbits->as<uint32_t>() : nullptr;
    T.scalar_map = no_scalar_map ? 0u : 1u;
    T.rzero = rzero;
    T.rperm = bs.rperm ? bs.rperm->as<uint32_t>() : nullptr;
    T.krange64 = range;
    bs.narrow = bs.unique = true;
}

// the single-key structures over key column `kc` of width `nkw` (the `n` build rows; `cap` table slots): rank map, else CAS table;
// false: the keys are not unique
static bool try_narrow(const Exec& ex, JoinBuildSide* bs, int64_t n, uint64_t cap, const Column& kc, int nkw) {
    // BHIP_JOIN_TABLE=1: always the CAS table (+ key-set bitmap), the round-1 design — the A/B partner of the rank map
    static const bool force_table = env_flag("BHIP_JOIN_TABLE");
    // optimistic: the build side of a key join is almost always unique
    const uint64_t* ksel = kc.validity_words();
    const uint64_t bias = nkw == 4 ? 0x80000000ull : (1ull << 63);
    memset(&bs->ntable, 0, sizeof(bs->ntable));
    bs->narrow_width = nkw;
    bs->dup = make_buffer(ex, 8);
    Temp tmp(ex);
    struct Stats3 { uint64_t v[3]; };
    // a dimension table's keys (<= 1024 rows spanning <= 2^16 values: Q5's nation and region): statistics, key set, packed map and
    // permutation in ONE launch and ONE host read (kernels_join.hip: tiny_rank_build_kernel) instead of four launches and two or
    // three reads; anything else — a wider span, duplicate keys — carries on below as if nothing had happened
    static const bool no_tiny = env_flag("BHIP_NO_TINY_BUILD");
    if (!no_tiny && !force_table && n >= 1 && n <= tiny_rank_build_max_rows()) {
        BufferPtr rp = make_buffer(ex, tiny_rank_build_map_words() * 8 + 16), pm = index_buffer(ex, n);
        uint64_t* out = tmp.get<uint64_t>(3);
        TIMED_LAUNCH(ex, "tiny_rank_build", launch_tiny_rank_build(ex.cfg(), kc.data->ptr(), nkw, ksel, (uint32_t)n, rp->as<uint64_t>(), pm->as<uint32_t>(), out));
        const Stats3 got = read_device(ex, reinterpret_cast<const Stats3*>(out));
        const bool unsorted = got.v[2] & 1, dup = got.v[2] & 2, built = got.v[2] & 4;
        if (built && !dup) {
            const uint64_t range = got.v[1] - got.v[0];
            bs->rpack = rp;
            if (unsorted) bs->rperm = pm;
            // (no stream_wait: the read above has waited for the kernel, so the map is complete before it is published)
            publish_rank_map(*bs, got.v[0] ^ bias, range, 2u * ((uint32_t)(range >> 6) + 1u));
            return true;
        }
    }
    // one pass: min / max / "strictly increasing"
    uint64_t* stats = tmp.get<uint64_t>(3);
    {
        FillMany fm;                                         // the duplicate flag and the seed {~0, 0, 0} of the statistics: one launch
        fm.add(bs->dup->ptr(), 8);
        fm.add(stats, 8, 0xFFFFFFFFu);
        fm.add(stats + 1, 16);
        TIMED_LAUNCH(ex, "fill_many", launch_fill_many(ex.cfg(), fm));
    }
    TIMED_LAUNCH_N(ex, "join_key_stats", n, launch_join_key_stats(ex.cfg(), kc.data->ptr(), nkw, ksel, (uint32_t)n, stats));
    const Stats3 back = read_device(ex, reinterpret_cast<const Stats3*>(stats));        // one pinned-slot read, no staged copy
    const uint64_t* host_stats = back.v;
    const bool any_key = host_stats[0] <= host_stats[1];
    const uint64_t range = any_key ? host_stats[1] - host_stats[0] : 0;
    const uint64_t kmin = (host_stats[0] ^ bias);                        // raw key bits of the smallest key
    const bool sorted = host_stats[2] == 0;
    // a window of at most 2^36 values (granule indices and `rzero` are 32-bit; SF1000 order keys span 1.5 - 6 x 10^9 and hash
    // partitioning does not narrow a rank's window) that is not absurdly sparse (<= 1 KiB of map per build row).
    // BHIP_RANK_WINDOW_LOG2 lowers the bound (30 = the round-2 limit: the A/B partner, profiles/r03_rank_window_ab.txt)
    static const int window_log2 = [] { const int b = env_int("BHIP_RANK_WINDOW_LOG2", 36); return b < 10 ? 10 : (b > 36 ? 36 : b); }();
    const bool window_ok = any_key && range <= (1ull << window_log2) && range / 4096 <= (uint64_t)n + 256;
    if (window_ok && !force_table) {
        // ---- rank map ----------------------------------------------------------------------------------------------
        const int64_t n_words = (int64_t)(range >> 6) + 1, n_gran = 2 * n_words;
        // the key-set words outlive the build when they are small (<= 256 MiB: windows up to 2^31 values): semi-joins probe them
        const bool keep_bits = (size_t)n_words * 8 <= ((size_t)256 << 20);
        if (keep_bits) bs->rbits = make_buffer(ex, ((size_t)n_words + 2) * 8);
        uint64_t* bits = keep_bits ? bs->rbits->as<uint64_t>() : tmp.get<uint64_t>((size_t)n_words + 2);
        bs->rpack = make_buffer(ex, (size_t)n_gran * 8 + 16);
        {
            FillMany fm;
            fm.add(bs->rpack->as<uint64_t>() + n_gran, 8);         // NarrowJoinTable::rzero
            fm.add(bits, ((size_t)n_words + 2) * 8);               // the key set, and the granules at and behind `rzero`
            TIMED_LAUNCH(ex, "fill_many", launch_fill_many(ex.cfg(), fm));
        }
        TIMED_LAUNCH_N(ex, sorted ? "rank_bits_sorted" : "rank_bits_any", n,
                       launch_rank_bits(ex.cfg(), kc.data->ptr(), nkw, ksel, (uint32_t)n, kmin, sorted, bits, bs->dup->as<uint32_t>()));
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_gran));
        uint64_t* total = tmp.get<uint64_t>(1);
        TIMED_LAUNCH_N(ex, "rank_pack", n_gran, launch_rank_pack(ex.stream, reinterpret_cast<const uint32_t*>(bits), n_gran, bs->rpack->as<uint64_t>(), total, scan_tmp));
        bool dup = false;
        if (!sorted) {
            dup = read_device(ex, bs->dup->as<uint32_t>()) != 0;           // duplicates would collide in perm[]
            if (!dup) {
                bs->rperm = index_buffer(ex, n);
                TIMED_LAUNCH_N(ex, "rank_perm", n, launch_rank_perm(ex.cfg(), kc.data->ptr(), nkw, ksel, (uint32_t)n, kmin, bs->rpack->as<uint64_t>(),
                                                                   bs->rperm->as<uint32_t>()));
            }
        }
        if (!dup) {
            stream_wait(ex);                 // other tasks (other streams) read the map: complete before it is published
            publish_rank_map(*bs, kmin, range, (uint32_t)n_gran);
            return true;
        }
        bs->rpack.reset();
        bs->rbits.reset();
    } else {
        // ---- CAS table (sparse keys), with the key set as a bitmap in front of it when the window allows -------------
        const size_t slot_bytes = nkw == 4 ? 8 : 16;
        bs->slots = make_buffer(ex, cap * slot_bytes);
        HIP_CHECK(hipMemsetAsync(bs->slots->ptr(), 0, cap * slot_bytes, ex.stream));
        bs->ntable.kmin64 = kmin;
        bs->ntable.kmin = (uint32_t)kmin;
        bs->ntable.slots = bs->slots->as<uint64_t>();
        bs->ntable.mask = cap - 1;
        bs->ntable.dup_flag = bs->dup->as<uint32_t>();
        TIMED_LAUNCH_N(ex, "join_build_narrow", n, launch_join_build_narrow(ex.cfg(), bs->ntable, kc.data->ptr(), nkw, ksel, (uint32_t)n));
        if (any_key && range <= (1ull << 30) && n >= (1 << 18)) {
            const size_t words = (size_t)range / 32 + 2;
            bs->present = make_buffer(ex, words * 4);
            HIP_CHECK(hipMemsetAsync(bs->present->ptr(), 0, words * 4, ex.stream));
            if (nkw == 4)
                TIMED_LAUNCH_N(ex, "join_key_present", n, launch_join_key_present(ex.cfg(), kc.data->as<uint32_t>(), ksel, (uint32_t)n, (uint32_t)kmin,
                                                                                 bs->present->as<uint32_t>()));
            else
                TIMED_LAUNCH_N(ex, "join_key_present64", n, launch_join_key_present64(ex.cfg(), kc.data->as<uint64_t>(), ksel, (uint32_t)n, kmin,
                                                                                     bs->present->as<uint32_t>()));
        }
        if (read_device(ex, bs->dup->as<uint32_t>()) == 0) {
            bs->ntable.dup_flag = nullptr;
            if (bs->present) {
                bs->ntable.present = bs->present->as<uint32_t>();
                bs->ntable.krange64 = range;
            }
            bs->narrow = bs->unique = true;
            return true;
        }
        bs->slots.reset();
        bs->present.reset();
    }
    memset(&bs->ntable, 0, sizeof(bs->ntable));
    return false;
}

// the general table, duplicates chained through next[]: over packed 16-byte keys (any key types that fit them), or (wide) over
// row hashes with the key columns of the build batch as the keys — any width
static void build_general_table(const Exec& ex, JoinBuildSide* bs, const std::vector<std::string>& key_names, uint64_t cap, bool wide) {
    const int64_t n = bs->batch->n_rows;
    bs->keys = side_keys(ex, *bs->batch, key_names, wide);
    bs->wide = wide;
    bs->owner = make_buffer(ex, cap * 8);
    bs->head = make_buffer(ex, cap * 4);
    bs->next = make_buffer(ex, (size_t)(n + 1) * 4);            // (the table's chain links: scratch, no column's offsets)
    HIP_CHECK(hipMemsetAsync(bs->owner->ptr(), 0, cap * 8, ex.stream));
    HIP_CHECK(hipMemsetAsync(bs->head->ptr(), 0, cap * 4, ex.stream));
    bs->table.owner = bs->owner->as<uint64_t>();
    bs->table.head = bs->head->as<uint32_t>();
    bs->table.next = bs->next->as<uint32_t>();
    bs->table.mask = cap - 1;
    bs->table.keys128 = wide ? nullptr : bs->keys.keys->as<uint64_t>();
    bs->table.cols = wide ? &bs->keys.cols : nullptr;
    bs->dup = make_buffer(ex, 8);
    HIP_CHECK(hipMemsetAsync(bs->dup->ptr(), 0, 8, ex.stream));
    bs->table.dup_flag = bs->dup->as<uint32_t>();
    TIMED_LAUNCH_N(ex, kernel_name(K_BUILD, wide), n, launch_join_build(ex.cfg(), bs->table, bs->keys.view(), (uint32_t)n));
    // other tasks (other HIP streams) will read the table: it must be complete before it is published
    bs->unique = read_device(ex, bs->dup->as<uint32_t>()) == 0;
    bs->table.dup_flag = nullptr;
    if (wide) bs->keys.keys.reset();        // the row hashes: only the build read them (emit_build_rows computes them again for its one pass)
}

// the wide-key table over the build batch of `packed`, beside it in the cache: for the probe batches whose keys outgrow the packed key
std::shared_ptr<const JoinBuildSide> HashJoinExec::wide_sibling(const Exec& ex, const JoinBuildSide& packed) const {
    std::lock_guard<std::mutex> g(cache_->mu);
    if (!cache_->wide) {
        auto w = std::make_shared<JoinBuildSide>();
        w->batch = packed.batch;
        build_general_table(ex, w.get(), left_keys_, table_capacity((uint64_t)w->batch->n_rows), true);
        cache_->wide = w;
    }
    ex.ctx->set_join_key_form("wide");
    return cache_->wide;
}

// collect the left child -> the single-key structures where the key types allow -> else the general table (packed keys where they
// hold the key values, else wide) -> cache
std::shared_ptr<const JoinBuildSide> HashJoinExec::build_side(const Exec& ex) const {
    std::lock_guard<std::mutex> g(cache_->mu);
    auto report = [&](const JoinBuildSide& b) { ex.ctx->set_join_key_form(b.narrow ? "narrow" : (b.wide || cache_->wide) ? "wide" : "packed"); };
    if (cache_->built) { report(*cache_->built); return cache_->built; }
    auto bs = std::make_shared<JoinBuildSide>();
    std::vector<BatchPtr> parts;
    const int np = left_->output_partitioning().count;
    for (int p = 0; p < np; ++p)
        for (auto& b : nonempty_batches(*open_join_child(left_, p, ex, left_keys_))) parts.push_back(b);
    // concat works on ordinary columns; and a small build side (Q5: the five nations of a region) is gathered here, once, so that
    // all its columns travel on as views over ONE index vector (a view in, a view out: one more index vector to compose per join above)
    if (parts.size() > 1 || (parts.size() == 1 && parts[0]->n_rows <= 65536))
        for (auto& b : parts) b = materialize_batch(ex, b);
    bs->batch = single_batch(ex, left_->schema(), parts);
    const int64_t n = bs->batch->n_rows;
    // build rows are addressed by 32-bit slots / ranks in every table form
    if (n > 0x7FFFFFF0ll) fail(BHIP_ENOTIMPL, "hash join build side of more than 2^31 rows per partition");
    const uint64_t cap = table_capacity((uint64_t)n);
    static const bool narrow_disabled = env_flag("BHIP_NO_NARROW_JOIN");
    // the existence probes read the general table's owner words, a residual filter enumerates candidates through its chains: no
    // narrow structures for them
    const bool existence = build_existence(join_type_) || probe_existence(join_type_);
    const int nkw = narrow_disabled || existence || filter_ ? 0 : narrow_key_width();
    bool narrow = false;
    if (nkw && n > 0) {
        const Schema& lsch = *bs->batch->schema;
        const Column& c0 = bs->batch->cols[lsch.index_of(left_keys_[0])];
        if (pair_keys()) {
            const Column& c1 = bs->batch->cols[lsch.index_of(left_keys_[1])];
            // ON (a, b) = (c, d), 4-byte integers.  First choice: the build side unique on `a` alone (a key and an attribute it determines:
            // TPC-H Q5's s_suppkey, s_nationkey) — the join goes by `a` (rank map where the keys are dense) and a match stands only if
            // the second columns agree (join_filter_probe_kernel<RESID>).  Second: both columns packed into one 8-byte key.
            Column first = c0;
            if (c1.validity) {                         // a build row with a NULL in either part matches nothing
                first.validity = validity_buffer(ex, n);
                HIP_CHECK(launch_and_bitmaps(ex.cfg(), c0.validity_words(), c1.validity->as<uint64_t>(), n, first.validity->as<uint64_t>()));
            }
            if (try_narrow(ex, bs.get(), n, cap, first, 4)) {
                bs->key_holder = first;
                bs->ntable.resid_build = c1.data->as<uint32_t>();
                bs->resid = narrow = true;
            } else {
                const Column packed = pack_key_pair(ex, c0, c1, n);
                narrow = try_narrow(ex, bs.get(), n, cap, packed, 8);
                if (narrow) bs->key_holder = packed;
            }
        } else {
            narrow = try_narrow(ex, bs.get(), n, cap, c0, nkw);
        }
    }
    if (!narrow) {
        // BHIP_JOIN_WIDE=1 (read at every build: one process can run both forms): the wide table wherever the packed one would be built
        bool wide = static_wide_ || wide_keys_.load() || env_flag("BHIP_JOIN_WIDE");
        if (!wide) {
            try {
                build_general_table(ex, bs.get(), left_keys_, cap, false);
            } catch (const KeyWidthError&) {                    // a build value longer than its share of the packed key
                wide_keys_.store(true);
                wide = true;
            }
        }
        if (wide) build_general_table(ex, bs.get(), left_keys_, cap, true);
    }
    cache_->built = bs;
    report(*bs);
    return bs;
}

// the integer image of a double range [lo, hi] over Int32 values (empty: lo > hi) — the SOP plan table keeps ranges as doubles
static void int_bounds(double lo, double hi, int32_t* lo_i, int32_t* hi_i) {
    *lo_i = 1; *hi_i = 0;
    if (lo != lo || hi != hi || lo > 2147483647.0 || hi < -2147483648.0) return;
    const double l = __builtin_ceil(lo), h = __builtin_floor(hi);
    *lo_i = l <= -2147483648.0 ? (int32_t)(-2147483647 - 1) : (int32_t)l;
    *hi_i = h >= 2147483647.0 ? (int32_t)2147483647 : (int32_t)h;
}

namespace {

// where the probe rows come from: right_ = [ProjectionExec(plain columns)] over [CoalesceBatchesExec]* over [FilterExec] over src.
// The probe then runs on src's UNFILTERED batches and only the rows that join are ever gathered (late materialisation).
struct ProbeChain {
    bool ok = false;
    PlanPtr src;
    ExprPtr pred;                  // may be null
    std::vector<int> src_of;       // column i of right_'s schema -> column of src's schema
};

ProbeChain probe_chain(const PlanPtr& right) {
    ProbeChain c;
    const ExecutionPlan* p = right.get();
    PlanPtr cur = right;
    const ProjectionExec* proj = dynamic_cast<const ProjectionExec*>(p);
    if (proj) {
        for (auto& en : proj->exprs())
            if (en.first->kind != BHIP_EXPR_COLUMN) return c;          // computed columns: the operator runs as it stands
        cur = proj->input();
    }
    while (auto co = dynamic_cast<const CoalesceBatchesExec*>(cur.get())) cur = co->input();
    if (auto flt = dynamic_cast<const FilterExec*>(cur.get())) {
        c.pred = flt->predicate();
        cur = flt->input();
    }
    c.src = cur;
    const Schema& ss = *c.src->schema();
    if (proj) {
        for (auto& en : proj->exprs()) {
            const int j = ss.index_of(en.first->name);
            if (j < 0) return c;
            c.src_of.push_back(j);
        }
    } else {
        for (size_t i = 0; i < right->schema()->fields.size(); ++i) c.src_of.push_back((int)i);
    }
    c.ok = true;
    return c;
}

// `pred` as an AND of integer ranges over NULL-free Int32 / Date32 columns of `b` (the fused probe's filter form)
bool int_ranges_of(const ExprPtr& pred, const Batch& b, ProbeFilter& F) {
    memset(&F, 0, sizeof(F));
    if (!pred) return true;
    SopPlan rp;
    if (!build_sop(*b.schema, pred, {}, {}, rp) || rp.prog.n_ranges < 1 || rp.prog.n_ranges > JOIN_FILTER_MAX) return false;
    for (int i = 0; i < rp.prog.n_ranges; ++i) {
        const SopRange& r = rp.prog.ranges[i];
        if (!r.is32) return false;
        const Column& c = b.cols[rp.col_map[r.col]];
        if (c.validity || (c.dtype != DT_INT32 && c.dtype != DT_DATE32)) return false;
        F.col[i] = c.data->as<int32_t>();
        int_bounds(r.lo, r.hi, &F.lo[i], &F.hi[i]);
    }
    F.n = rp.prog.n_ranges;
    return true;
}

// where the output columns of probed rows are gathered from: the batch `src`, whose column for right output column k is rmap[k]
// (nullptr: right_cols_[k]) and whose row of probe row i is remap[i] (nullptr: row i)
// (fmap: the same for the right columns the residual filter reads, J.filter_cols_ in their order; nullptr: the column's own index)
struct ProbeOut {
    const Batch* src;
    const std::vector<int>* rmap;
    const uint32_t* remap;
    const std::vector<int>* fmap = nullptr;
};

// what a tiled probe kernel leaves behind, in scratch: the selection bitmap of the emitting rows and their count per SEL_TILE rows,
// and their partners.  The general table's kernel writes a partner per probe row.  The fused kernel owns whole tiles (it writes
// every bitmap word of one) and, where a build column is read, stages each tile's emitting rows and their partners, so that one
// compaction yields both index vectors with no pass over the bitmap (a semi-join stages nothing: it has only the bitmap to compact).
// The existence probe of the general table (RightSemi / RightAnti) writes the bitmap and the counts and no partners.
struct TileSelection {
    const bool fused;
    const int64_t n, n_tiles;
    uint64_t* bitmap;
    uint32_t* tile_counts;
    uint64_t* tile_off;
    uint64_t* total;
    void* scan_tmp;
    uint32_t *partner = nullptr, *staging = nullptr, *staging_rows = nullptr;
    TileSelection(Temp& tmp, int64_t rows, bool fused_probe, bool stage, bool partners = true)
        : fused(fused_probe), n(rows), n_tiles((rows + SEL_TILE - 1) / SEL_TILE) {
        bitmap = tmp.get<uint64_t>(fused ? (size_t)n_tiles * (SEL_TILE / 64) + 1 : (size_t)(n + 63) / 64 + 1);
        tile_counts = tmp.get<uint32_t>((size_t)n_tiles + 1);
        tile_off = tmp.get<uint64_t>((size_t)n_tiles + 1);
        total = tmp.get<uint64_t>(1);
        scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_tiles));
        if (!fused && partners) partner = tmp.get<uint32_t>((size_t)n + 1);
        else if (stage) { staging = tmp.get<uint32_t>((size_t)n_tiles * SEL_TILE); staging_rows = tmp.get<uint32_t>((size_t)n_tiles * SEL_TILE); }
    }
};

// the index pairs of one probe's output rows; lbuf / rbuf: the buffers that own them (the fused path: the output's view columns
// then hold them), unset: they are scratch of the probe
struct JoinIndices {
    uint32_t *lidx = nullptr, *ridx = nullptr;
    BufferPtr lbuf, rbuf;
};

}  // namespace

// ---- probe side: the state of one execute_needed() stream ---------------------------------------------------------------------
// The front end — where the pairs or candidates of a probe batch come from — is the join's own: the hash join's is the methods from
// compact() to probe_right_side() below (H: that join; null under a NestedLoopJoinExec, whose front end is NestedLoopJoinExec::Run).
// The tail is shared: emit / finish, filter_candidates, resolve_kept, select_by_hits, emit_build_rows.
struct JoinExec::Probe {
    const JoinExec& J;
    const HashJoinExec* const H;
    const int partition;
    const Exec& ex;
    const std::vector<bool>&needed, &deferrable;
    const LaunchCfg cfg;
    const std::shared_ptr<const JoinBuildSide> bs;
    const Batch& L;
    const size_t n_lcols;
    const bool right_outer, left_outer, pair;
    // Semi / Anti: the probe only marks (no output before the end of the stream); RightSemi / RightAnti: it only selects probe rows
    const bool mark_only, select_only, anti;
    const size_t n_lout;                 // left columns in the output (right output column k is column n_lout + k of the schema)
    bool need_left = false;
    BufferPtr matched;                   // Left / Full: one bit per build row some probe row matched; Semi / Anti: per key, on its representative row
                                         // (under a residual filter: per build row for all four — two rows of one key can differ under it)
    std::shared_ptr<const JoinBuildSide> sibling;   // the wide table beside a packed `bs`, once a batch of this stream went through it
    std::vector<std::string> rcols;
    SchemaPtr key_schema;                // the probe-side key columns alone, under their names
    std::vector<BatchPtr> out;

    Probe(const JoinExec& j, const HashJoinExec* h, std::shared_ptr<const JoinBuildSide> built, int part, const Exec& e, const std::vector<bool>& need,
          const std::vector<bool>& defer)
        : J(j), H(h), partition(part), ex(e), needed(need), deferrable(defer), cfg(e.cfg()), bs(std::move(built)), L(*bs->batch), n_lcols(L.cols.size()),
          right_outer(j.join_type_ == BHIP_JOIN_RIGHT || j.join_type_ == BHIP_JOIN_FULL),
          left_outer(j.join_type_ == BHIP_JOIN_LEFT || j.join_type_ == BHIP_JOIN_FULL), pair(h && h->pair_keys()),
          mark_only(build_existence(j.join_type_)), select_only(probe_existence(j.join_type_)),
          anti(j.join_type_ == BHIP_JOIN_ANTI || j.join_type_ == BHIP_JOIN_RIGHT_ANTI), n_lout(select_only ? 0 : n_lcols) {
        for (size_t i = 0; i < n_lout; ++i) need_left = need_left || needed[i];
        if (left_outer || mark_only) {
            matched = make_buffer(ex, matched_bytes());
            HIP_CHECK(hipMemsetAsync(matched->ptr(), 0, matched_bytes(), ex.stream));
        }
        if (!H) return;
        auto ks = std::make_shared<Schema>();
        const Schema& rs = *J.right_->schema();
        for (auto& p : H->on_) {
            rcols.push_back(p.second);
            ks->fields.push_back(rs.fields[rs.index_of(p.second)]);
        }
        key_schema = ks;
    }
    size_t matched_bytes() const { return (size_t)(L.n_rows / 32 + 2) * 4; }
    uint32_t* matched_bits() const { return matched ? matched->as<uint32_t>() : nullptr; }

    // output batch from index pairs; o.src: the batch the right columns are gathered from (nullptr: they are NULL).  Columns no
    // parent reads stay placeholders.  The schema holds the left columns (n_lout of them: none for RightSemi / RightAnti, whose
    // lidx is null) and then the right columns J.right_cols_ (none for Semi / Anti).
    // (lbuf / rbuf: the buffers that own lidx / ridx, when the caller has them — view columns keep them instead of a copy)
    void emit(const ProbeOut& o, const uint32_t* lidx, const uint32_t* ridx, int64_t n_out, const BufferPtr& lbuf = nullptr, const BufferPtr& rbuf = nullptr) {
        const Schema& os = *J.schema_;
        auto b = new_batch(ex.ctx, J.schema_, n_out);
        b->cols.resize(os.fields.size());
        for (size_t i = 0; i < b->cols.size(); ++i) { b->cols[i].dtype = os.fields[i].dtype; b->cols[i].length = n_out; }
        // [0]: gathered now; [1]: handed on as views (the parent asked for them that way; a column that arrives as a view is
        // composed with this join's indices either way)
        std::vector<const Column*> lc[2], rc[2];
        std::vector<size_t> lpos[2], rpos[2];
        for (size_t i = 0; i < n_lout; ++i)
            if (needed[i]) { lc[deferrable[i] ? 1 : 0].push_back(&L.cols[i]); lpos[deferrable[i] ? 1 : 0].push_back(i); }
        for (int v = 0; v < 2; ++v) {
            if (lc[v].empty()) continue;
            if (lidx) {
                auto got = take_columns(ex, lc[v], lidx, n_out, right_outer, false, v == 1, lbuf);
                for (size_t k = 0; k < got.size(); ++k) b->cols[lpos[v][k]] = std::move(got[k]);
            } else {
                for (size_t k = 0; k < lc[v].size(); ++k) b->cols[lpos[v][k]] = null_column(ex, lc[v][k]->dtype, n_out);
            }
        }
        for (size_t k = 0; k < J.right_cols_.size(); ++k) {
            const size_t oi = n_lout + k;
            if (!needed[oi]) continue;
            if (!o.src) { b->cols[oi] = null_column(ex, os.fields[oi].dtype, n_out); continue; }
            rc[deferrable[oi] ? 1 : 0].push_back(&o.src->cols[o.rmap ? (*o.rmap)[k] : J.right_cols_[k]]);
            rpos[deferrable[oi] ? 1 : 0].push_back(oi);
        }
        for (int v = 0; v < 2; ++v) {
            if (rc[v].empty()) continue;
            auto got = take_columns(ex, rc[v], ridx, n_out, left_outer, false, v == 1, rbuf);
            for (size_t k = 0; k < got.size(); ++k) b->cols[rpos[v][k]] = std::move(got[k]);
        }
        out.push_back(b);
    }

    // an index vector of n entries: scratch of this probe, or (keep) a buffer of its own
    uint32_t* index_vector(Temp& tmp, bool keep, uint64_t n, BufferPtr& own) {
        if (!keep) return tmp.get<uint32_t>((size_t)n);
        own = index_buffer(ex, (int64_t)n);
        return own->as<uint32_t>();
    }

    // the end of every probe: the probe rows' rows of o.src through o.remap, then the output batch
    void finish(Temp& tmp, const ProbeOut& o, JoinIndices ix, uint64_t n_out) {
        if (o.remap) {
            BufferPtr obuf;
            uint32_t* orig = index_vector(tmp, (bool)ix.rbuf, n_out, obuf);
            TIMED_LAUNCH_N(ex, "take_fixed", n_out, launch_take_fixed(cfg, o.remap, 4, ix.ridx, (int64_t)n_out, orig));
            ix.ridx = orig;
            ix.rbuf = obuf;
        }
        emit(o, ix.lidx, ix.ridx, (int64_t)n_out, ix.lbuf, ix.rbuf);
        // (no wait: the index scratch is released in stream order — host/core.cpp Context::alloc)
    }

    // a tiled probe's result -> index vectors -> output
    void compact(Temp& tmp, const TileSelection& s, const ProbeOut& o) {
        HIP_CHECK(exclusive_scan_u32_u64(ex.stream, s.tile_counts, s.n_tiles, s.tile_off, false, s.total, s.scan_tmp));
        const uint64_t n_out = read_device(ex, s.total);
        if (n_out == 0) return;
        JoinIndices ix;
        if (s.partner || s.staging) ix.lidx = index_vector(tmp, s.fused, n_out, ix.lbuf);
        ix.ridx = index_vector(tmp, s.fused, n_out, ix.rbuf);
        if (s.staging) {
            TIMED_LAUNCH_N(ex, "join_compact_staged", s.n, launch_join_compact_staged(cfg, s.staging, s.tile_off, n_out, s.n_tiles, ix.lidx, s.staging_rows, ix.ridx));
        } else {
            TIMED_LAUNCH_N(ex, "select_indices", s.n, launch_select_indices(cfg, s.bitmap, s.tile_off, s.n, ix.ridx));
            if (s.partner && need_left) TIMED_LAUNCH_N(ex, "take_fixed", n_out, launch_take_fixed(cfg, s.partner, 4, ix.ridx, (int64_t)n_out, ix.lidx));
        }
        finish(tmp, o, ix, n_out);
    }

    // the key-equal pairs of one probe batch through the chains of `t`: count -> scan -> read -> emit.  -> their number; ix.lidx /
    // ix.ridx: scratch of `tmp` (a probe row's pairs consecutive).  outer: a probe row without a pair yields (none, row); mark: the
    // build rows' bits (null: none)
    uint64_t enumerate_pairs(Temp& tmp, const JoinBuildSide& t, const JoinSideKeys& keys, int64_t n_right, bool outer, uint32_t* mark,
                             const char* too_many, JoinIndices& ix) {
        uint64_t* total = tmp.get<uint64_t>(1);
        uint32_t* counts = tmp.get<uint32_t>((size_t)n_right + 1);
        uint64_t* offsets = tmp.get<uint64_t>((size_t)n_right + 1);
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_right));
        TIMED_LAUNCH_N(ex, kernel_name(K_PROBE_COUNT, t.wide), n_right, launch_join_probe_count(cfg, t.table, keys, (uint32_t)n_right, outer, counts));
        HIP_CHECK(exclusive_scan_u32_u64(ex.stream, counts, n_right, offsets, false, total, scan_tmp));
        const uint64_t n = read_device(ex, total);
        if (n > 0xFFFFFFF0ull) fail(BHIP_EEXEC, too_many);
        if (n == 0) return 0;
        ix.lidx = tmp.get<uint32_t>((size_t)n);
        ix.ridx = tmp.get<uint32_t>((size_t)n);
        TIMED_LAUNCH_N(ex, kernel_name(K_PROBE_EMIT, t.wide), n_right,
                       launch_join_probe_emit(cfg, t.table, keys, (uint32_t)n_right, outer, offsets, ix.lidx, ix.ridx, mark));
        return n;
    }

    // ---- general table: `probe` holds the key columns of the probe rows under their names -----------------------------------------
    // (a packed build side whose keys this batch's values outgrow: the batch goes through the wide table over the same build rows,
    // HashJoinExec::wide_sibling.  Below this point the form only names the kernels: the launchers pick it from the keys.)
    void probe_general(const Batch& probe, const ProbeOut& o) {
        const int64_t n_right = probe.n_rows;
        if (n_right == 0) return;
        std::shared_ptr<const JoinBuildSide> t = bs;
        SideKeys pk;
        if (!t->wide) {
            try {
                pk = side_keys(ex, probe, rcols, false);
            } catch (const KeyWidthError&) {
                t = sibling = H->wide_sibling(ex, *bs);
            }
        }
        if (t->wide) pk = side_keys(ex, probe, rcols, true);
        const JoinSideKeys keys = pk.view();
        if (J.filter_) { probe_filtered(*t, o, keys, n_right); return; }
        Temp tmp(ex);
        if (mark_only || select_only) {
            // existence: one probe per row whatever the duplication (the slot's owner stands for its key).  Semi / Anti leave bits
            // for emit_build_rows; RightSemi / RightAnti a selection of the probe rows, compacted as the unique build side's is
            auto exists = [&](uint64_t* bitmap, uint32_t* tile_counts, uint32_t* mark) {
                TIMED_LAUNCH_N(ex, kernel_name(K_PROBE_EXISTS, t->wide), n_right,
                               launch_join_probe_exists(cfg, t->table, keys, (uint32_t)n_right, anti, bitmap, tile_counts, mark));
            };
            if (mark_only) { exists(nullptr, nullptr, matched_bits()); return; }
            TileSelection s(tmp, n_right, false, false, false);
            exists(s.bitmap, s.tile_counts, nullptr);
            compact(tmp, s, o);
            return;
        }
        if (t->unique) {
            // one probe per row -> selection bitmap -> indices (the index pass of FilterExec)
            TileSelection s(tmp, n_right, false, false);
            TIMED_LAUNCH_N(ex, kernel_name(K_PROBE_MATCH, t->wide), n_right,
                           launch_join_probe_match(cfg, t->table, keys, (uint32_t)n_right, right_outer, s.partner, s.bitmap, s.tile_counts, matched_bits()));
            compact(tmp, s, o);
            return;
        }
        JoinIndices ix;
        const uint64_t n_out = enumerate_pairs(tmp, *t, keys, n_right, right_outer, matched_bits(), "join output of one probe batch exceeds 2^32 rows", ix);
        if (n_out) finish(tmp, o, ix, n_out);
    }

    // ---- residual filter: candidates (the key-equal pairs, enumerated as an Inner join whatever the join type and the build side's
    // duplication) -> the filter over the gathered columns it reads -> join_pairs_resolve: the kept pairs, the build rows' `matched`
    // bits and the probe rows' `hit` bits -> the output of the join type.  A row all of whose candidates fail has no partner.
    // the filter over the candidates: the ascending positions it keeps
    int64_t filter_candidates(Temp& tmp, const ProbeOut& o, const uint32_t* lidx, const uint32_t* ridx, uint64_t n_cand, BufferPtr& sel) {
        if (o.remap) {
            uint32_t* orig = tmp.get<uint32_t>((size_t)n_cand);
            TIMED_LAUNCH_N(ex, "take_fixed", n_cand, launch_take_fixed(cfg, o.remap, 4, ridx, (int64_t)n_cand, orig));
            ridx = orig;
        }
        std::vector<const Column*> lc, rc;
        std::vector<size_t> lpos, rpos;
        for (size_t k = 0; k < J.filter_cols_.size(); ++k) {
            const auto& fc = J.filter_cols_[k];
            if (fc.left) { lc.push_back(&L.cols[fc.index]); lpos.push_back(k); }
            else { rc.push_back(&o.src->cols[o.fmap ? (*o.fmap)[k] : fc.index]); rpos.push_back(k); }
        }
        auto fs = std::make_shared<Schema>();
        auto fb = new_batch(ex.ctx, fs, (int64_t)n_cand);
        fb->cols.resize(J.filter_cols_.size());
        if (!lc.empty()) {
            auto got = take_columns(ex, lc, lidx, (int64_t)n_cand, false);
            for (size_t k = 0; k < got.size(); ++k) fb->cols[lpos[k]] = std::move(got[k]);
        }
        if (!rc.empty()) {
            auto got = take_columns(ex, rc, ridx, (int64_t)n_cand, false);
            for (size_t k = 0; k < got.size(); ++k) fb->cols[rpos[k]] = std::move(got[k]);
        }
        for (size_t k = 0; k < J.filter_cols_.size(); ++k) {
            Field f = J.filter_cols_[k].field;
            f.nullable = f.nullable || (bool)fb->cols[k].validity;
            fs->fields.push_back(f);
        }
        return filter_indices(ex, *fb, J.filter_, sel);
    }

    // Right / Full / RightSemi / RightAnti answer per probe row of a batch: the `hit` words of its n_right rows (none otherwise)
    bool need_hit() const { return right_outer || select_only; }
    TileSelection hit_words(Temp& tmp, int64_t n_right, bool zero) {
        TileSelection s(tmp, need_hit() ? n_right : 0, false, false, false);
        if (need_hit() && zero) HIP_CHECK(hipMemsetAsync(s.bitmap, 0, ((size_t)(n_right + 63) / 64) * 8, ex.stream));
        return s;
    }

    // candidates (a probe row's consecutive) -> the filter -> join_pairs_resolve: the kept pairs as an output batch, their build rows'
    // `matched` bits and their probe rows' bits in `hit` (s.bitmap)
    void resolve_kept(Temp& tmp, const ProbeOut& o, const JoinIndices& cand, uint64_t n_cand, const TileSelection& s) {
        if (!n_cand) return;
        const uint32_t *lidx = cand.lidx, *ridx = cand.ridx;
        BufferPtr sel;
        const uint64_t n_keep = (uint64_t)filter_candidates(tmp, o, lidx, ridx, n_cand, sel);
        if (!n_keep) return;
        // all kept: the candidates are the pairs, and only the bits are left to set
        const bool all = n_keep == n_cand, pairs = !mark_only && !select_only;
        JoinIndices ix = cand;
        if (pairs && !all) {
            ix.lidx = tmp.get<uint32_t>((size_t)n_keep);
            ix.ridx = tmp.get<uint32_t>((size_t)n_keep);
        }
        if ((pairs && !all) || matched || need_hit())
            TIMED_LAUNCH_N(ex, "join_pairs_resolve", n_keep,
                           launch_join_pairs_resolve(cfg, all ? nullptr : sel->as<uint32_t>(), lidx, ridx, n_keep, pairs && !all ? ix.lidx : nullptr,
                                                     pairs && !all ? ix.ridx : nullptr, matched_bits(), need_hit() ? s.bitmap : nullptr));
        if (pairs) finish(tmp, o, ix, n_keep);
    }

    // the probe rows with (RightSemi) / without (Right / Full: with NULL left columns; RightAnti) a partner, from the batch's `hit` words
    void select_by_hits(Temp& tmp, const ProbeOut& o, const TileSelection& s, int64_t n_right) {
        if (!need_hit()) return;
        TIMED_LAUNCH_N(ex, "join_hit_select", n_right, launch_join_hit_select(cfg, s.bitmap, (uint32_t)n_right, right_outer || anti, s.tile_counts));
        HIP_CHECK(exclusive_scan_u32_u64(ex.stream, s.tile_counts, s.n_tiles, s.tile_off, false, s.total, s.scan_tmp));
        const uint64_t n_sel = read_device(ex, s.total);
        if (n_sel == 0) return;
        JoinIndices ix;
        ix.ridx = tmp.get<uint32_t>((size_t)n_sel);
        TIMED_LAUNCH_N(ex, "select_indices", n_right, launch_select_indices(cfg, s.bitmap, s.tile_off, n_right, ix.ridx));
        finish(tmp, o, ix, n_sel);
    }

    void probe_filtered(const JoinBuildSide& t, const ProbeOut& o, const JoinSideKeys& keys, int64_t n_right) {
        Temp tmp(ex);
        JoinIndices cand;
        const uint64_t n_cand = enumerate_pairs(tmp, t, keys, n_right, false, nullptr, "join filter: the key-equal candidate pairs of one probe batch exceed 2^32", cand);
        const TileSelection s = hit_words(tmp, n_right, true);
        resolve_kept(tmp, o, cand, n_cand, s);
        select_by_hits(tmp, o, s, n_right);
    }

    // ---- narrow build side: one pass over the probe rows: ranges -> key-set bit -> rank map / table (kernels_join.hip) -----
    // n probe rows whose keys are `kc` (and, for a two-column join by its first key, whose second keys are `resid`)
    void probe_narrow(int64_t n, const ProbeFilter& F, const Column& kc, const Column* resid, const ProbeOut& o) {
        if (n == 0) return;
        Temp tmp(ex);
        TileSelection s(tmp, n, true, need_left);
        // algorithmic bytes: the predicate columns and the key column once, one selection bit per row
        // (named after the kernel the launcher picks — kernels_join.hip launch_join_filter_probe: rank map, no NULL probe keys,
        // an inner join -> join_rank_probe_kernel — so that bench.py's roofline line and the rocprofv3 summaries agree)
        const bool direct = bs->ntable.rpack != nullptr && !kc.validity && !left_outer && !right_outer;
        char form[JOIN_PROBE_FORM_LEN];
        TIMED_LAUNCH_B(ex, direct ? "join_rank_probe" : "join_filter_probe", n, (uint64_t)n * (uint64_t)(bs->narrow_width + 4 * F.n) + (uint64_t)n / 8,
                       launch_join_filter_probe(cfg, bs->ntable, F, kc.data->ptr(), bs->narrow_width,
                                                kc.validity_words(), (uint32_t)n, right_outer, s.bitmap,
                                                s.tile_counts, s.staging, matched_bits(),
                                                resid ? resid->data->as<uint32_t>() : nullptr, s.staging_rows, form));
        ex.ctx->set_join_probe_form(form);
        compact(tmp, s, o);
    }

    // probe n rows whose key columns (in on_'s order) are `keys`, dropping the rows outside F's ranges (F.n = 0: none; a narrow
    // build side only): one key, or two keys as first key + residual or packed into one (whichever the build side chose), through
    // the narrow structures; anything else through the general table, which reads the keys by their probe-side names
    void probe_rows(int64_t n, const std::vector<Column>& keys, const ProbeFilter& F, const ProbeOut& o) {
        if (!bs->narrow) {
            Batch kb;
            kb.schema = key_schema;
            kb.ctx = o.src->ctx;
            kb.n_rows = n;
            kb.cols = keys;
            probe_general(kb, o);
        } else if (!pair) {
            probe_narrow(n, F, keys[0], nullptr, o);
        } else if (!bs->resid) {
            probe_narrow(n, F, pack_key_pair(ex, keys[0], keys[1], n), nullptr, o);
        } else {
            Column first = keys[0];
            if (keys[1].validity) {                    // a NULL in either part never matches
                first.validity = validity_buffer(ex, n);
                HIP_CHECK(launch_and_bitmaps(cfg, keys[0].validity_words(), keys[1].validity->as<uint64_t>(), n, first.validity->as<uint64_t>()));
            }
            probe_narrow(n, F, first, &keys[1], o);
        }
    }

    void probe_right_side() {
        ProbeFilter no_filter;
        memset(&no_filter, 0, sizeof(no_filter));
        const ProbeChain chain = probe_chain(J.right_);
        std::vector<Column> keys(rcols.size());
        if (!chain.ok) {
            auto rs = open_join_child(J.right_, partition, ex, rcols);          // payload columns of a join below may arrive as views
            while (BatchPtr rb = rs->next()) {
                for (size_t k = 0; k < rcols.size(); ++k) keys[k] = rb->cols[rb->schema->index_of(rcols[k])];
                probe_rows(rb->n_rows, keys, no_filter, ProbeOut{rb.get(), nullptr, nullptr});
            }
            return;
        }
        static const bool fused_disabled = env_flag("BHIP_NO_FUSED_PROBE");
        const Schema& rsch = *J.right_->schema();
        std::vector<int> rmap, key_src;                    // right OUTPUT column k / key k -> source column
        for (int ci : J.right_cols_) rmap.push_back(chain.src_of[ci]);
        for (auto& rc : rcols) key_src.push_back(chain.src_of[rsch.index_of(rc)]);
        std::vector<int> fmap;                             // column k of the residual filter (a right one) -> source column
        for (auto& fc : J.filter_cols_) fmap.push_back(fc.left ? -1 : chain.src_of[fc.index]);
        // a join below (no filter in between): only the columns read here, and everything but the keys may arrive as views
        StreamPtr ss;
        auto src_hj = dynamic_cast<const HashJoinExec*>(chain.src.get());
        if (src_hj && !chain.pred && !join_views_disabled()) {
            std::vector<bool> need(chain.src->schema()->fields.size(), false);
            for (size_t k = 0; k < J.right_cols_.size(); ++k)
                if (needed[n_lout + k]) need[rmap[k]] = true;
            for (int c : fmap)
                if (c >= 0) need[c] = true;
            ss = open_join_below(*src_hj, partition, ex, need, key_src);
        } else {
            ss = chain.src->execute(partition, ex);
        }
        while (BatchPtr b = ss->next()) {
            if (b->n_rows == 0) continue;
            for (size_t k = 0; k < key_src.size(); ++k) keys[k] = b->cols[key_src[k]];
            int64_t n = b->n_rows;
            BufferPtr sel;
            ProbeFilter F;
            // the filter runs inside the probe kernel where it can; else it runs first and the key columns of the surviving rows are probed
            if (!(bs->narrow && !fused_disabled && int_ranges_of(chain.pred, *b, F))) {
                F = no_filter;
                if (chain.pred) {
                    n = filter_indices(ex, *b, chain.pred, sel);
                    if (n == 0) continue;
                    for (auto& kc : keys) kc = take_batch_column(ex, kc, sel->as<uint32_t>(), n);
                }
            }
            probe_rows(n, keys, F, ProbeOut{b.get(), &rmap, sel ? sel->as<uint32_t>() : nullptr, &fmap});
        }
    }

    // the end of the stream, from the `matched` bits: the build rows without a partner (anti: Left / Full, with NULL right columns,
    // and Anti) or with one (Semi), as one batch.  Left / Full marked every matched row; Semi / Anti marked the representative of
    // every matched key, in `bs`'s table and — where a batch went through it — in the sibling's, whose representatives differ
    void emit_build_rows() {
        const int64_t n_left = L.n_rows;
        if (!(left_outer || mark_only) || n_left == 0) return;
        Temp tmp(ex);
        uint32_t* flags = tmp.get<uint32_t>((size_t)n_left + 1);
        uint64_t* offsets = tmp.get<uint64_t>((size_t)n_left + 1);
        uint64_t* total = tmp.get<uint64_t>(1);
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_left));
        // (a residual filter marks the very rows that passed it; so does every route of a join without keys)
        const bool direct = left_outer || bs->unique || J.filter_ || !H;
        const bool want_unmatched = left_outer || anti;
        auto flags_of = [&](const JoinBuildSide& t, bool anti_now, bool merge) {
            // a wide table's rows find their slots by their hashes, which are not kept after the build: once more, for this one pass
            const bool rehash = t.wide && !direct;
            JoinSideKeys keys = t.keys.view();
            SideKeys again;
            if (rehash) {
                again = side_keys(ex, L, H->left_keys_, true);
                keys.keys = again.keys->as<uint64_t>();
            }
            TIMED_LAUNCH_N(ex, kernel_name(K_EXISTS_FLAGS, rehash), n_left,
                           launch_join_exists_flags(cfg, t.table, keys, matched->as<uint32_t>(), (uint32_t)n_left, direct, anti_now, merge, flags));
        };
        if (sibling && !direct) flags_of(*sibling, false, false);
        flags_of(*bs, want_unmatched, sibling && !direct);
        HIP_CHECK(exclusive_scan_u32_u64(ex.stream, flags, n_left, offsets, false, total, scan_tmp));
        const uint64_t n_rows = read_device(ex, total);
        if (n_rows) {
            uint32_t* lidx = tmp.get<uint32_t>((size_t)n_rows);
            TIMED_LAUNCH(ex, "compact_flags", launch_compact_flags(cfg, flags, offsets, (uint32_t)n_left, lidx));
            emit(ProbeOut{nullptr, nullptr, nullptr}, lidx, nullptr, (int64_t)n_rows);
        }
    }
};

StreamPtr HashJoinExec::execute(int partition, const Exec& ex) const {
    return execute_needed(partition, ex, std::vector<bool>(schema_->fields.size(), true));
}

StreamPtr HashJoinExec::execute_needed(int partition, const Exec& ex, const std::vector<bool>& needed_in, const std::vector<bool>& deferrable_in) const {
    check_partition(*this, partition);
    auto self = std::static_pointer_cast<const HashJoinExec>(shared_from_this());
    std::vector<bool> needed = needed_in, deferrable = deferrable_in;
    needed.resize(schema_->fields.size(), true);
    deferrable.resize(schema_->fields.size(), false);
    return StreamPtr(new LazyStream(schema_, [self, partition, ex, needed, deferrable]() {
        Probe p(*self, self.get(), self->build_side(ex), partition, ex, needed, deferrable);
        p.probe_right_side();
        p.emit_build_rows();
        return std::move(p.out);
    }));
}

// ---- nested loop join ---------------------------------------------------------------------------------------------------------------
// NestedLoopJoinExec: no key, so no table — the build side is the collected left rows and nothing else, and the candidates of a probe
// batch are ALL its pairs with them, numbered p = ri * nL + li.  Three routes per probe batch (Context::nested_loop_form):
//   cross    no filter: the pairs of a chunk [p0, p1) are written out (nlj_cross_pairs) and emitted, a batch per chunk
//   general  any filter: the same chunks as candidates through the shared tail (filter_candidates -> join_pairs_resolve -> finish);
//            the matched / hit bits add up over the chunks, the probe rows are selected once after the last one
//   compare  a filter that is an AND of up to four `left column OP right column` terms: nlj_compare_count -> scan -> nlj_compare_emit
//            (kernels_nljoin.hip) — a pair costs register compares, and only the partners ever reach memory
// and `exists` for an existence type without a filter: every row of a side has a partner iff the other side has a row.

static uint64_t nlj_chunk_pairs() {
    // BHIP_NLJ_CHUNK_PAIRS=<n>: pairs per chunk (a test forces many ragged chunks on a small input); candidates are addressed by
    // 32-bit positions inside a chunk
    static const uint64_t chunk = [] {
        const char* v = getenv("BHIP_NLJ_CHUNK_PAIRS");
        const long long n = v ? atoll(v) : 0;
        return n < 1 ? NLJ_CHUNK_PAIRS : (uint64_t)(n > (1ll << 30) ? (1ll << 30) : n);
    }();
    return chunk;
}

NestedLoopJoinExec::NestedLoopJoinExec(PlanPtr left, PlanPtr right, int join_type, ExprPtr filter)
    : JoinExec(std::move(left), std::move(right), join_type, std::move(filter)) {
    ctx_ = left_->context();
    if (join_type < BHIP_JOIN_INNER || join_type > BHIP_JOIN_RIGHT_ANTI) fail(BHIP_ENOTIMPL, "Unsupported join type");
    // a build row's fate depends on every probe row, and a stream sees one right partition
    if ((join_type == BHIP_JOIN_LEFT || join_type == BHIP_JOIN_FULL || build_existence(join_type)) && right_->output_partitioning().count > 1)
        fail(BHIP_ENOTIMPL, std::string(join_name(join_type)) + " join over a right child of " + std::to_string(right_->output_partitioning().count) +
                                " partitions: put a MergeExec under the right child");
    const Schema &ls = *left_->schema(), &rs = *right_->schema();
    auto s = std::make_shared<Schema>();
    const bool left_nullable = join_type == BHIP_JOIN_RIGHT || join_type == BHIP_JOIN_FULL;
    const bool right_nullable = join_type == BHIP_JOIN_LEFT || join_type == BHIP_JOIN_FULL;
    for (auto f : ls.fields) {
        if (probe_existence(join_type)) break;
        if (left_nullable) f.nullable = true;
        s->fields.push_back(f);
    }
    for (size_t i = 0; i < rs.fields.size(); ++i) {
        if (build_existence(join_type)) break;
        Field f = rs.fields[i];
        if (right_nullable) f.nullable = true;
        if (s->index_of(f.name) >= 0) fail(BHIP_EINVAL, "join output would have two columns named '" + f.name + "'");
        s->fields.push_back(f);
        right_cols_.push_back((int)i);
    }
    schema_ = s;
    cache_ = std::make_shared<BuildCache>();
    if (!filter_) return;
    check_filter({});
    // the fused form: AND of terms `column OP column`, one column of each side, both of one fixed-width type (so the coercion put
    // no cast over either).  Anything else — a literal, arithmetic, a cast, Utf8, Boolean, a fifth term — takes the general route.
    std::vector<ExprPtr> conj{filter_};
    for (size_t i = 0; i < conj.size();) {
        const ExprPtr e = conj[i];
        if (e->kind == BHIP_EXPR_BINARY && e->name == "And" && e->args.size() == 2) {
            conj[i] = e->args[0];
            conj.insert(conj.begin() + i + 1, e->args[1]);
        } else {
            ++i;
        }
    }
    static const char* const ops[] = {"Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq"};                     // CmpKind order
    static const int flipped[] = {CMP_EQ, CMP_NE, CMP_GT, CMP_GE, CMP_LT, CMP_LE};
    for (auto& e : conj) {
        int cmp = -1;
        for (int k = 0; k < 6; ++k)
            if (e->kind == BHIP_EXPR_BINARY && e->name == ops[k]) cmp = k;
        if (cmp < 0 || e->args.size() != 2 || e->args[0]->kind != BHIP_EXPR_COLUMN || e->args[1]->kind != BHIP_EXPR_COLUMN) { terms_.clear(); return; }
        int l = ls.index_of(e->args[0]->name), r = rs.index_of(e->args[1]->name);
        if (l < 0 || r < 0) {                                  // right column first: the same term with the operator flipped
            l = ls.index_of(e->args[1]->name);
            r = rs.index_of(e->args[0]->name);
            cmp = flipped[cmp];
        }
        const int t = l >= 0 && r >= 0 ? ls.fields[l].dtype : 0;
        if (!t || t != rs.fields[r].dtype || dt_width(t) == 0 || conj.size() > (size_t)NLJ_MAX_TERMS) { terms_.clear(); return; }
        terms_.push_back(Term{l, r, cmp, dt_is_float(t) ? NLJ_F64 : (t == DT_UINT64 ? NLJ_U64 : NLJ_I64)});
    }
}

PlanPtr NestedLoopJoinExec::with_new_children(const std::vector<PlanPtr>& c) const {
    if (c.size() != 2) fail(BHIP_EINVAL, "NestedLoopJoinExec wrong number of children");
    return std::make_shared<NestedLoopJoinExec>(c[0], c[1], join_type_, filter_);
}

std::string NestedLoopJoinExec::describe() const {
    return std::string("NestedLoopJoinExec: join_type=") + join_name(join_type_) + ", filter=" + (filter_ ? filter_->to_string() : std::string("None"));
}

// the left child, all its partitions, as one batch; built once and shared by every right partition's task
std::shared_ptr<const JoinBuildSide> NestedLoopJoinExec::build_side(const Exec& ex) const {
    std::lock_guard<std::mutex> g(cache_->mu);
    if (cache_->built) return cache_->built;
    auto bs = std::make_shared<JoinBuildSide>();
    std::vector<BatchPtr> parts;
    const int np = left_->output_partitioning().count;
    for (int p = 0; p < np; ++p)
        for (auto& b : nonempty_batches(*left_->execute(p, ex))) parts.push_back(materialize_batch(ex, b));
    bs->batch = single_batch(ex, left_->schema(), parts);
    // build rows are 32-bit indices, and 0xFFFFFFFF is the NULL row of the outer joins
    if (bs->batch->n_rows > 0x7FFFFFF0ll) fail(BHIP_ENOTIMPL, "nested loop join build side of more than 2^31 rows");
    stream_wait(ex);                     // other tasks (other streams) read the batch: complete before it is published
    cache_->built = bs;
    return bs;
}

struct NestedLoopJoinExec::Run : JoinExec::Probe {
    const NestedLoopJoinExec& N;
    const uint64_t nL;
    uint64_t probe_rows = 0;             // of the whole stream
    Run(const NestedLoopJoinExec& n, int part, const Exec& e, const std::vector<bool>& need, const std::vector<bool>& defer)
        : Probe(n, nullptr, n.build_side(e), part, e, need, defer), N(n), nL((uint64_t)L.n_rows) {}

    void set_all(void* bits, size_t bytes) { HIP_CHECK(hipMemsetAsync(bits, 0xFF, bytes, ex.stream)); }

    // the candidates [p0, p1) as index vectors in `tmp`
    JoinIndices pairs_of(Temp& tmp, uint64_t p0, uint64_t p1) {
        JoinIndices ix;
        ix.lidx = tmp.get<uint32_t>((size_t)(p1 - p0));
        ix.ridx = tmp.get<uint32_t>((size_t)(p1 - p0));
        TIMED_LAUNCH_N(ex, "nlj_cross_pairs", p1 - p0, launch_nlj_cross_pairs(cfg, (uint32_t)nL, p0, p1, ix.lidx, ix.ridx));
        return ix;
    }

    // no filter.  Existence types enumerate nothing; the others emit every pair, a batch per chunk.  Either way a side's rows all
    // have a partner, or none has: the bits are set wholesale.
    void cross(const ProbeOut& o, int64_t n_right) {
        if (matched) set_all(matched->ptr(), matched_bytes());
        Temp tmp(ex);
        // probe rows come out of here when all have a partner (RightSemi) or none has (RightAnti; Right / Full: with NULL left columns)
        const bool all_hit = nL > 0;
        if (need_hit() && (select_only ? all_hit != anti : !all_hit)) {
            const TileSelection s = hit_words(tmp, n_right, !all_hit);
            if (all_hit) set_all(s.bitmap, ((size_t)(n_right + 63) / 64) * 8);
            select_by_hits(tmp, o, s, n_right);
        }
        if (mark_only || select_only) return;
        const uint64_t total = nL * (uint64_t)n_right, chunk = nlj_chunk_pairs();
        for (uint64_t p0 = 0; p0 < total; p0 += chunk) {
            Temp ctmp(ex);
            const uint64_t p1 = std::min(total, p0 + chunk);
            finish(ctmp, o, pairs_of(ctmp, p0, p1), p1 - p0);
        }
    }

    void general(const ProbeOut& o, int64_t n_right) {
        Temp tmp(ex);
        const TileSelection s = hit_words(tmp, n_right, true);
        const uint64_t total = nL * (uint64_t)n_right, chunk = nlj_chunk_pairs();
        for (uint64_t p0 = 0; p0 < total; p0 += chunk) {
            Temp ctmp(ex);
            const uint64_t p1 = std::min(total, p0 + chunk);
            resolve_kept(ctmp, o, pairs_of(ctmp, p0, p1), p1 - p0, s);
        }
        select_by_hits(tmp, o, s, n_right);
    }

    void compare(const ProbeOut& o, int64_t n_right) {
        NljTerms T;
        memset(&T, 0, sizeof(T));
        T.n = (int32_t)N.terms_.size();
        for (int i = 0; i < T.n; ++i) {
            const Term& t = N.terms_[i];
            T.t[i].build = L.cols[t.left].ref();
            T.t[i].probe = o.src->cols[t.right].ref();
            T.t[i].cmp = t.cmp;
            T.t[i].vclass = t.vclass;
        }
        Temp tmp(ex);
        uint64_t* total = tmp.get<uint64_t>(1);
        uint32_t* counts = tmp.get<uint32_t>((size_t)n_right + 1);
        uint64_t* offsets = tmp.get<uint64_t>((size_t)n_right + 1);
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_right));
        const TileSelection s = hit_words(tmp, n_right, false);                   // (the count kernel writes every word)
        TIMED_LAUNCH_N(ex, "nlj_compare_count", n_right,
                       launch_nlj_compare_count(cfg, T, (uint32_t)nL, (uint32_t)n_right, counts, matched_bits(), need_hit() ? s.bitmap : nullptr));
        if (!mark_only && !select_only) {
            HIP_CHECK(exclusive_scan_u32_u64(ex.stream, counts, n_right, offsets, false, total, scan_tmp));
            const uint64_t n = read_device(ex, total);
            if (n > 0xFFFFFFF0ull) fail(BHIP_EEXEC, "join output of one probe batch exceeds 2^32 rows");
            if (n) {
                JoinIndices ix;
                ix.lidx = tmp.get<uint32_t>((size_t)n);
                ix.ridx = tmp.get<uint32_t>((size_t)n);
                TIMED_LAUNCH_N(ex, "nlj_compare_emit", n_right, launch_nlj_compare_emit(cfg, T, (uint32_t)nL, (uint32_t)n_right, offsets, ix.lidx, ix.ridx));
                finish(tmp, o, ix, n);
            }
        }
        select_by_hits(tmp, o, s, n_right);
    }

    void run() {
        // BHIP_NO_NLJ_FUSED=1: the general route where the fused one would run (the A/B partner)
        static const bool no_fused = env_flag("BHIP_NO_NLJ_FUSED");
        auto rs = N.right_->execute(partition, ex);
        while (BatchPtr rb = rs->next()) {
            const int64_t n_right = rb->n_rows;
            if (n_right > 0x7FFFFFF0ll) fail(BHIP_ENOTIMPL, "nested loop join probe batch of more than 2^31 rows");
            probe_rows += (uint64_t)n_right;
            const ProbeOut o{rb.get(), nullptr, nullptr};
            const char* form = !N.filter_ ? (mark_only || select_only ? "exists" : "cross") : (!N.terms_.empty() && !no_fused ? "compare" : "general");
            ex.ctx->set_nested_loop_form(form);
            if (n_right == 0) continue;
            if (!N.filter_) cross(o, n_right);
            else if (form[0] == 'c') compare(o, n_right);
            else general(o, n_right);
        }
        emit_build_rows();
    }
};

StreamPtr NestedLoopJoinExec::execute(int partition, const Exec& ex) const {
    return execute_needed(partition, ex, std::vector<bool>(schema_->fields.size(), true));
}

StreamPtr NestedLoopJoinExec::execute_needed(int partition, const Exec& ex, const std::vector<bool>& needed_in) const {
    check_partition(*this, partition);
    auto self = std::static_pointer_cast<const NestedLoopJoinExec>(shared_from_this());
    std::vector<bool> needed = needed_in;
    needed.resize(schema_->fields.size(), true);
    const std::vector<bool> deferrable(schema_->fields.size(), false);
    return StreamPtr(new LazyStream(schema_, [self, partition, ex, needed, deferrable]() {
        Run r(*self, partition, ex, needed, deferrable);
        r.run();
        return std::move(r.out);
    }));
}

}  // namespace bhip
