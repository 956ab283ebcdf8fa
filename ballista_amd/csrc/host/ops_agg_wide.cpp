// ops_agg_wide.cpp — HashAggregateExec over group keys that do not fit the 16-byte packed key (several Utf8 columns,
// long strings: TPC-H Q10 groups by c_name, c_address, c_phone, c_comment ...).  Reference operator:
// rust/core/src/serde/physical_plan/from_proto.rs:173-252 (HashAggregateExec, any group expressions).
//
// Two steps on top of the packed-key machinery:
//   1. wide_key_assign_kernel (kernels_hash.hip) gives every input row a representative row with an equal key
//      (hash table of row ids over 64-bit row hashes; equality on the key columns themselves, NULL == NULL);
//   2. the ordinary aggregate runs with that ONE Int32 column as its key, and the key columns of the result are
//      gathered from the input at the representative rows.
// Also here: the Single mode (run_single) — Final over Partial as one operator, and COUNT / SUM / AVG (DISTINCT x) on top of it
// through distinct_claim_kernel / distinct_mark_kernel, which mark the first row of every distinct (group key, x).  No wire form.
#include "../str_kernels.h"
#include "hash_kernels.h"
#include "plan.hpp"

namespace bhip {

namespace {
const char* const kRepName = "__group_rep";

// The 64-bit row hash of `exprs` over every row of `in`, in the caller's scratch.  One hash program holds VM_MAX_KEYPARTS key parts: up to
// 8 expressions are one pass, 9 .. 16 a second pass over the rest into `second` (else null).  The kernels fold the two hashes of a row;
// equality is on the key columns either way.
struct RowHashes { uint64_t* first; uint64_t* second; };
RowHashes hash_rows(const Exec& ex, Temp& tmp, const Schema& schema, const Batch& in, const std::vector<ExprPtr>& exprs) {
    const size_t n = (size_t)in.n_rows;
    RowHashes h{tmp.get<uint64_t>(n), exprs.size() > (size_t)VM_MAX_KEYPARTS ? tmp.get<uint64_t>(n) : nullptr};
    ScanStatus* st = tmp.get<ScanStatus>(1);
    for (size_t first = 0; first < exprs.size(); first += VM_MAX_KEYPARTS) {
        ProgramBuilder pb(schema);
        pb.set_hash_only();
        for (size_t i = first; i < std::min(exprs.size(), first + VM_MAX_KEYPARTS); ++i) pb.add_key(exprs[i]);
        ScanParams P;
        pb.finish(P);
        ProgramBuilder::bind(P, pb.columns(), in, pb.creates_nulls());
        HIP_CHECK(hipMemsetAsync(st, 0, sizeof(ScanStatus), ex.stream));
        TIMED_LAUNCH(ex, "scan_keys", launch_scan_keys(ex.cfg(), P, nullptr, first ? h.second : h.first, nullptr, st));
        check_scan_status(ex, st);
    }
    return h;
}
}  // namespace

bool HashAggregateExec::run_single_partial(const Exec& ex, std::vector<BatchPtr>& out) const {
    static const bool disabled = env_flag("BHIP_NO_FINAL_ELISION");
    if (disabled || mode_ != BHIP_AGG_FINAL) return false;
    const ExecutionPlan* p = input_.get();
    PlanPtr below;
    while (true) {
        if (auto m = dynamic_cast<const MergeExec*>(p)) { below = m->input(); p = below.get(); continue; }
        if (auto c = dynamic_cast<const CoalesceBatchesExec*>(p)) { below = c->input(); p = below.get(); continue; }
        break;
    }
    auto pa = dynamic_cast<const HashAggregateExec*>(p);
    if (!pa || !below || pa->mode_ != BHIP_AGG_PARTIAL || pa->output_partitioning().count != 1 || pa->strings_) return false;
    if (pa->group_.size() != group_.size() || pa->aggr_.size() != aggr_.size()) return false;
    const Schema& ps = *pa->schema();
    // this operator's keys must be the partial's key columns, in order, and the functions must be the same
    for (size_t i = 0; i < group_.size(); ++i)
        if (group_[i].first->kind != BHIP_EXPR_COLUMN || group_[i].first->name != ps.fields[i].name) return false;
    for (size_t i = 0; i < aggr_.size(); ++i)
        if (aggr_[i].fn != pa->aggr_[i].fn) return false;
    // the Partial emits its group table as this operator's columns (AVG = sum / count in the emit kernel): no state batch at all
    if (group_.empty() || !pa->wide_keys_.load()) {
        try {
            out = pa->run_packed(0, ex, this);
            return true;
        } catch (const KeyWidthError&) {
            if (group_.empty()) throw;                       // no GROUP BY, no wide form
            pa->wide_keys_.store(true);
        }
    }
    // wide keys: the Partial's state batch, then AVG = [sum] / [count] as a projection
    std::vector<std::pair<ExprPtr, std::string>> exprs;
    for (size_t i = 0; i < group_.size(); ++i) exprs.push_back({make_column(ps.fields[i].name), group_[i].second});
    size_t pos = group_.size();
    for (auto& a : aggr_) {
        if (a.fn == BHIP_AGG_AVG) {
            auto cast = std::make_shared<Expr>();
            cast->kind = BHIP_EXPR_CAST;
            cast->dtype = DT_FLOAT64;
            cast->args = {make_column(ps.fields[pos].name)};                          // [count]
            exprs.push_back({make_binary(make_column(ps.fields[pos + 1].name), "Divide", ExprPtr(cast)), a.name});
            pos += 2;
        } else {
            exprs.push_back({make_column(ps.fields[pos].name), a.name});
            pos += 1;
        }
    }
    auto s = below->execute(0, ex);
    while (BatchPtr b = s->next()) out.push_back(project_batch(ex, *b, exprs, schema_));
    return true;
}

std::vector<BatchPtr> HashAggregateExec::run(int partition, const Exec& ex) const {
    if (mode_ == BHIP_AGG_SINGLE) return run_single(partition, ex);
    if (strings_) return run_strings(partition, ex);
    {
        std::vector<BatchPtr> out;
        if (run_single_partial(ex, out)) return out;
    }
    if (!group_.empty() && wide_keys_.load()) return run_wide(partition, ex);
    try {
        return run_packed(partition, ex);
    } catch (const KeyWidthError&) {
        if (group_.empty()) throw;
    }
    wide_keys_.store(true);
    return run_wide(partition, ex);
}

std::vector<BatchPtr> HashAggregateExec::run_wide(int partition, const Exec& ex) const {
    const SchemaPtr in_schema = input_->schema();
    if (in_schema->index_of(kRepName) >= 0) fail(BHIP_EINVAL, std::string("column name '") + kRepName + "' is reserved");
    if (group_.size() > (size_t)VM_MAX_COLS) fail(BHIP_ENOTIMPL, "more than 16 group expressions");
    std::vector<BatchPtr> parts = nonempty_batches(*input_->execute(partition, ex));
    if (parts.empty()) return {};
    const BatchPtr in = concat_batches(ex, in_schema, parts);
    parts.clear();
    const int64_t n = in->n_rows;
    if (n > 0x7FFFFFF0ll) fail(BHIP_ENOTIMPL, "wide-key aggregate over more than 2^31 input rows per partition");
    const LaunchCfg cfg = ex.cfg();

    // ---- key columns, their row hashes, the representative of every row -------------------------------------
    std::vector<ExprPtr> exprs;
    std::vector<Column> keys;
    for (auto& g : group_) {
        exprs.push_back(g.first);
        keys.push_back(evaluate_column(ex, *in, g.first));
    }
    Column rep = alloc_column(ex, DT_INT32, n, false);
    {
        Temp tmp(ex);
        const RowHashes h = hash_rows(ex, tmp, *in_schema, *in, exprs);
        const uint64_t cap = table_capacity((uint64_t)n);
        uint32_t* table = tmp.get<uint32_t>(cap);
        HIP_CHECK(hipMemsetAsync(table, 0, cap * 4, ex.stream));
        WideKeyCols K;
        memset(&K, 0, sizeof(K));
        K.n = (int32_t)keys.size();
        for (size_t i = 0; i < keys.size(); ++i) K.col[i] = keys[i].ref();
        TIMED_LAUNCH(ex, "wide_key_assign", launch_wide_key_assign(cfg, K, h.first, h.second, table, cap - 1, (uint32_t)n, rep.data->as<uint32_t>()));
    }

    // ---- the ordinary aggregate, keyed by the representative row ---------------------------------------------
    auto s2 = std::make_shared<Schema>();
    auto aug = new_batch(ex.ctx, s2, n);
    s2->fields.push_back(Field{kRepName, DT_INT32, false});
    aug->cols.push_back(rep);
    // Partial: the arguments are expressions over the input's names; Final: the state columns follow the key by position
    const size_t first = mode_ == BHIP_AGG_PARTIAL ? 0 : group_.size();
    for (size_t i = first; i < in_schema->fields.size(); ++i) {
        s2->fields.push_back(in_schema->fields[i]);
        aug->cols.push_back(in->cols[i]);
    }
    auto src = std::make_shared<MemoryExec>(ex.ctx, s2, std::vector<std::vector<BatchPtr>>{{BatchPtr(aug)}});
    auto inner = std::make_shared<HashAggregateExec>(
        mode_, std::vector<std::pair<ExprPtr, std::string>>{{make_column(kRepName), kRepName}}, aggr_, src);
    if (n >= 4096) inner->path_hint_.store(-1);                     // many rows: straight to the device-wide table
    std::vector<BatchPtr> res = inner->run_packed(0, ex);

    // ---- key columns of the groups: the input's, at the representative rows ----------------------------------
    std::vector<BatchPtr> outv;
    for (auto& r : res) {
        auto out = new_batch(ex.ctx, schema_, r->n_rows);
        std::vector<const Column*> kp;
        for (auto& k : keys) kp.push_back(&k);
        std::vector<Column> got = take_columns(ex, kp, r->cols[0].data->as<uint32_t>(), r->n_rows, false);
        for (auto& c : got) out->cols.push_back(std::move(c));
        for (size_t i = 1; i < r->cols.size(); ++i) out->cols.push_back(r->cols[i]);
        outv.push_back(out);
    }
    return outv;
}

// ---- Single mode: raw rows in, final values out; COUNT / SUM / AVG (DISTINCT x) ----------------------------------------
// Final(Merge(Partial(source))) with the operator's expressions: the Merge is there because run_single_partial's elision only
// fires through one — with it the pair is ONE aggregation whose group table is emitted as the Final's columns.
namespace {
PlanPtr final_over_partial(const std::vector<std::pair<ExprPtr, std::string>>& group, const std::vector<AggregateDesc>& aggr, const PlanPtr& source) {
    auto partial = std::make_shared<HashAggregateExec>(BHIP_AGG_PARTIAL, group, aggr, source);
    const Schema& ps = *partial->schema();
    std::vector<std::pair<ExprPtr, std::string>> fgroup;
    for (auto& g : group) fgroup.push_back({make_column(g.second), g.second});
    std::vector<AggregateDesc> faggr;
    size_t pos = group.size();
    for (auto& a : aggr) {                                   // a Final reads its states by position: the argument only names the first
        faggr.push_back(AggregateDesc{a.fn, make_column(ps.fields[pos].name), a.name});
        pos += a.fn == BHIP_AGG_AVG ? 2 : 1;
    }
    return std::make_shared<HashAggregateExec>(BHIP_AGG_FINAL, fgroup, faggr, std::make_shared<MergeExec>(partial));
}
std::string distinct_name(size_t i) { return "__distinct_" + std::to_string(i); }
}  // namespace

void HashAggregateExec::check_single() {
    const Schema& in = *input_->schema();
    // every group must lie in ONE input partition: execute(p) sees partition p alone
    const Partitioning part = input_->output_partitioning();
    if (part.count > 1) {
        bool ok = part.scheme == BHIP_PART_HASH && !group_.empty() && !part.exprs.empty();
        for (auto& pe : part.exprs) {
            bool found = false;
            for (auto& g : group_) found = found || g.first->to_string() == pe->to_string();
            ok = ok && found;
        }
        if (!ok)
            fail(BHIP_EINVAL, "Single aggregate over an input of " + std::to_string(part.count) +
                                  " partitions that is not hash-partitioned on group expressions: put a MergeExec or a RepartitionExec(Hash on the "
                                  "group expressions) under it");
    }
    std::vector<AggregateDesc> plain = aggr_;
    bool group_strings = false;
    for (auto& g : group_) group_strings = group_strings || has_lowered_node(g.first, in);
    for (auto& a : plain) {
        if (a.fn < BHIP_AGG_SUM || a.fn > BHIP_AGG_AVG_DISTINCT) fail(BHIP_ENOTIMPL, "Unsupported aggregate function");
        if (!is_distinct_fn(a.fn)) continue;
        a.fn = distinct_plain_fn(a.fn);
        const std::string printed = a.arg->to_string();
        bool seen = false;
        for (auto& d : distinct_args_) seen = seen || d->to_string() == printed;
        if (seen) continue;
        if (has_lowered_node(a.arg, in) || (a.arg->kind == BHIP_EXPR_LITERAL && a.arg->dtype == DT_UTF8))
            fail(BHIP_ENOTIMPL, "DISTINCT over a string function: " + printed + " (project it to a column first)");
        if (group_strings) fail(BHIP_ENOTIMPL, "DISTINCT aggregate beside group expressions with a string function (project them to columns first)");
        if (distinct_args_.size() == 8) fail(BHIP_ENOTIMPL, "more than 8 different DISTINCT arguments in one aggregate");
        if (group_.size() + 1 > (size_t)VM_MAX_COLS) fail(BHIP_ENOTIMPL, "more than 15 group expressions with a DISTINCT aggregate");
        {
            ProgramBuilder pb(in);                           // x is hashed like a group key: what a key cannot be, x cannot be
            pb.set_hash_only();
            pb.add_key(a.arg);
        }
        distinct_args_.push_back(a.arg);
    }
    for (size_t i = 0; i < distinct_args_.size(); ++i)
        if (in.index_of(distinct_name(i)) >= 0) fail(BHIP_EINVAL, "column name '" + distinct_name(i) + "' is reserved");
    single_plan_ = final_over_partial(group_, plain, input_);         // (every other plan-time check of the expressions is the pair's)
    auto s = std::make_shared<Schema>(*single_plan_->schema());
    schema_ = s;
}

std::vector<BatchPtr> HashAggregateExec::run_single(int partition, const Exec& ex) const {
    const SchemaPtr in_schema = input_->schema();
    auto reschema = [&](std::vector<BatchPtr> res) {
        for (auto& r : res) {
            auto out = std::make_shared<Batch>(*r);
            out->schema = schema_;
            r = out;
        }
        return res;
    };
    if (distinct_args_.empty() && input_->output_partitioning().count == 1) {
        auto s = single_plan_->execute(0, ex);
        return reschema(drain(*s));
    }
    // this partition alone, as one resident batch
    std::vector<BatchPtr> parts = nonempty_batches(*input_->execute(partition, ex));
    if (distinct_args_.empty()) {
        if (parts.empty() && !group_.empty()) return {};
        auto src = std::make_shared<MemoryExec>(ex.ctx, in_schema, std::vector<std::vector<BatchPtr>>{parts});
        std::vector<AggregateDesc> plain = aggr_;
        auto s = final_over_partial(group_, plain, src)->execute(0, ex);
        return reschema(drain(*s));
    }
    if (parts.empty() && !group_.empty()) return {};
    const BatchPtr in = single_batch(ex, in_schema, parts);
    parts.clear();
    const int64_t n = in->n_rows;
    if (n > 0x7FFFFFF0ll) fail(BHIP_ENOTIMPL, "DISTINCT aggregate over more than 2^31 input rows per partition");
    const LaunchCfg cfg = ex.cfg();

    auto s2 = std::make_shared<Schema>(*in_schema);
    auto aug = std::make_shared<Batch>(*in);
    std::vector<Column> keys;
    for (auto& g : group_) keys.push_back(evaluate_column(ex, *in, g.first));
    for (size_t d = 0; d < distinct_args_.size(); ++d) {
        const ExprPtr& xe = distinct_args_[d];
        Column x = evaluate_column(ex, *in, xe);
        Column marked = x;                                   // x's data and offsets; valid = the first row of every distinct (key, x)
        if (n > 0) {
            Temp tmp(ex);
            std::vector<ExprPtr> cols;
            for (auto& g : group_) cols.push_back(g.first);
            cols.push_back(xe);
            const RowHashes h = hash_rows(ex, tmp, *in_schema, *in, cols);      // the row hash of (group keys ..., x)
            const uint64_t cap = table_capacity((uint64_t)n);
            uint32_t* table = tmp.get<uint32_t>(cap);
            uint32_t* slot_of = tmp.get<uint32_t>((size_t)n);
            HIP_CHECK(hipMemsetAsync(table, 0, cap * 4, ex.stream));
            WideKeyCols K;
            memset(&K, 0, sizeof(K));
            K.n = (int32_t)keys.size() + 1;
            for (size_t i = 0; i < keys.size(); ++i) K.col[i] = keys[i].ref();
            K.col[keys.size()] = x.ref();
            const uint64_t* xvalid = x.validity_words();
            marked.validity = validity_buffer(ex, n);
            TIMED_LAUNCH_N(ex, "distinct_claim", n, launch_distinct_claim(cfg, K, xvalid, h.first, h.second, table, cap - 1, (uint32_t)n, slot_of));
            TIMED_LAUNCH_N(ex, "distinct_mark", n, launch_distinct_mark(cfg, xvalid, table, slot_of, (uint32_t)n, marked.validity->as<uint64_t>()));
        }
        s2->fields.push_back(Field{distinct_name(d), x.dtype, true});
        aug->cols.push_back(std::move(marked));
    }
    aug->schema = s2;
    std::vector<AggregateDesc> plain = aggr_;
    for (auto& a : plain) {
        if (!is_distinct_fn(a.fn)) continue;
        a.fn = distinct_plain_fn(a.fn);
        for (size_t d = 0; d < distinct_args_.size(); ++d)
            if (distinct_args_[d]->to_string() == a.arg->to_string()) { a.arg = make_column(distinct_name(d)); break; }
    }
    auto src = std::make_shared<MemoryExec>(ex.ctx, s2, std::vector<std::vector<BatchPtr>>{{BatchPtr(aug)}});
    auto s = final_over_partial(group_, plain, src)->execute(0, ex);
    return reschema(drain(*s));
}

// ---- string nodes in the keys / arguments, MIN / MAX over Utf8 -------------------------------------------------------
// MIN(s) over strings = the string at the smallest position in the sort order of s: the column is sorted once (the SortExec
// passes), every row gets its rank as an Int64 with the string's validity, the ordinary aggregate takes MIN / MAX of the ranks,
// and the result's strings are gathered through the sort permutation.
std::vector<BatchPtr> HashAggregateExec::run_strings(int partition, const Exec& ex) const {
    const SchemaPtr in_schema = input_->schema();
    const BatchPtr in = single_batch(ex, in_schema, nonempty_batches(*input_->execute(partition, ex)));
    const int64_t n = in->n_rows;
    const LaunchCfg cfg = ex.cfg();

    // the string nodes as columns
    Utf8Lowering low(*in_schema);
    std::vector<std::pair<ExprPtr, std::string>> group2;
    for (auto& g : group_) group2.push_back({low.rewrite(g.first, true), g.second});
    std::vector<AggregateDesc> aggr2 = aggr_;
    if (mode_ == BHIP_AGG_PARTIAL)
        for (auto& a : aggr2) a.arg = low.rewrite(a.arg, true);
    const BatchPtr aug = low.any() ? low.apply(ex, *in) : in;
    auto s2 = std::make_shared<Schema>(*aug->schema);
    auto b2 = std::make_shared<Batch>(*aug);

    // MIN / MAX over Utf8 -> over ranks
    struct Ranked { size_t agg; Column strings; BufferPtr perm; };
    std::vector<Ranked> ranked;
    size_t pos = group_.size();
    for (size_t i = 0; i < aggr2.size(); ++i) {
        AggregateDesc& a = aggr2[i];
        const size_t state_pos = pos;
        pos += a.fn == BHIP_AGG_AVG ? 2 : 1;
        if (a.fn != BHIP_AGG_MIN && a.fn != BHIP_AGG_MAX) continue;
        int ci;
        if (mode_ == BHIP_AGG_PARTIAL) {
            if (expr_type(a.arg, *s2) != DT_UTF8) continue;
            if (a.arg->kind != BHIP_EXPR_COLUMN) fail(BHIP_ENOTIMPL, "MIN/MAX over a Utf8 expression: " + a.arg->to_string());
            ci = s2->index_of(a.arg->name);
        } else {
            ci = (int)state_pos;
            if (s2->fields[ci].dtype != DT_UTF8) continue;
        }
        const Column strings = aug->cols[ci];
        Ranked r;
        r.agg = i;
        r.strings = strings;
        Column rank = alloc_column(ex, DT_INT64, n, false);
        rank.validity = strings.validity;
        if (n > 0) {
            r.perm = sort_permutation(ex, *aug, {SortDesc{make_column(s2->fields[ci].name), false, false}});
            TIMED_LAUNCH_N(ex, "invert_perm", n, launch_invert_perm(cfg, r.perm->as<uint32_t>(), n, rank.data->as<int64_t>()));
        }
        if (mode_ == BHIP_AGG_PARTIAL) {
            const std::string name = "__rank_" + std::to_string(i);
            s2->fields.push_back(Field{name, DT_INT64, s2->fields[ci].nullable});
            b2->cols.push_back(rank);
            a.arg = make_column(name);
        } else {
            s2->fields[ci].dtype = DT_INT64;                  // Final reads its states by position
            b2->cols[ci] = rank;
        }
        ranked.push_back(std::move(r));
    }
    b2->schema = s2;
    auto src = std::make_shared<MemoryExec>(ex.ctx, s2, std::vector<std::vector<BatchPtr>>{{BatchPtr(b2)}});
    auto inner = std::make_shared<HashAggregateExec>(mode_, group2, aggr2, src);
    if (inner->strings_) fail(BHIP_ENOTIMPL, "aggregate over string expressions: " + describe());
    std::vector<BatchPtr> res = inner->run(0, ex);

    std::vector<BatchPtr> outv;
    for (auto& r : res) {
        auto out = std::make_shared<Batch>(*r);
        out->schema = schema_;
        for (auto& rk : ranked) {
            size_t col = group_.size();
            for (size_t i = 0; i < rk.agg; ++i) col += aggr_[i].fn == BHIP_AGG_AVG && mode_ == BHIP_AGG_PARTIAL ? 2 : 1;
            const Column& ranks = r->cols[col];
            BufferPtr idx = index_buffer(ex, r->n_rows);
            TIMED_LAUNCH_N(ex, "rank_to_row", r->n_rows, launch_rank_to_row(cfg, ranks.data->as<int64_t>(), ranks.validity_words(),
                                                                             rk.perm ? rk.perm->as<uint32_t>() : nullptr, r->n_rows, idx->as<uint32_t>()));
            std::vector<const Column*> one{&rk.strings};
            out->cols[col] = take_columns(ex, one, idx->as<uint32_t>(), r->n_rows, /*may_null=*/true, false)[0];
        }
        outv.push_back(out);
    }
    return outv;
}

}  // namespace bhip
