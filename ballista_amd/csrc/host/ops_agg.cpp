// ops_agg.cpp — HashAggregateExec (Partial / Final; Single is the two as one operator, ops_agg_wide.cpp) over the fused scan kernels.
//
// Reference: built at rust/core/src/serde/physical_plan/from_proto.rs:173-252 (mode :181-184,
// aggregates via create_aggregate_expr :230-236; only Sum/Avg/Count are serialisable,
// to_proto.rs:352-363); the stage split Partial | Final is rust/scheduler/src/planner.rs:149-171.
// State layout: SUM -> [sum]; AVG -> [count: UInt64, sum: Float64];
// COUNT -> [count: UInt64].  Final merges by position: state columns follow the group columns
// in aggregate order.
//
// execute() folds the FilterExec / CoalesceBatchesExec / ProjectionExec chain below the
// aggregate into the aggregate's own kernel (predicate fused, projection expressions
// substituted), i.e. the whole of TPC-H Q1/Q6 stage 1 is one kernel launch per input batch.
//
// In this file: the operator's schema and plumbing, and run_packed — program building, the dispatch ladder over the register
// paths (wide-load, register-resident, VM kernel; 1 / 4 / 8 groups per workgroup) and the emit of the group table into the output
// batch.  The hash path the ladder ends in is ops_agg_hash.cpp; keys wider than the packed key and string expressions are
// ops_agg_wide.cpp.
#include "../sort_kernels.h"
#include "../util_kernels.h"
#include "hash_kernels.h"
#include "plan.hpp"
#include "sop.hpp"

namespace bhip {

// sum_return_type of DataFusion 4.0 (physical_plan/aggregates.rs): signed -> Int64, unsigned -> UInt64, Float32 -> Float32, Float64 -> Float64
static int sum_type(int t) {
    if (dt_is_float(t)) return t;
    if (dt_is_unsigned(t)) return DT_UINT64;
    return DT_INT64;
}

// MIN / MAX accumulator of a value type: floats as doubles, unsigned types compare unsigned (a UInt64 at or above 2^63 is no
// negative number), every other type as a signed 64-bit integer
static int minmax_kind(int t, bool is_min) {
    if (dt_is_float(t)) return is_min ? ACC_MIN_F64 : ACC_MAX_F64;
    if (dt_is_unsigned(t)) return is_min ? ACC_MIN_U64 : ACC_MAX_U64;
    return is_min ? ACC_MIN_I64 : ACC_MAX_I64;
}

// the register path's launches by group width, timed at BHIP_KERNEL_TIMING=2 only (the tests read which width ran; the dominant
// launches are timed at level 1 as scan_agg_lowcard_kernel)
static const char* lowcard_launch_name(int gmax, bool batches) {
    if (batches) return gmax == 1 ? "scan_agg_lowcard_g1_batches" : gmax == 4 ? "scan_agg_lowcard_g4_batches" : "scan_agg_lowcard_g8_batches";
    return gmax == 1 ? "scan_agg_lowcard_g1" : gmax == 4 ? "scan_agg_lowcard_g4" : "scan_agg_lowcard_g8";
}

static const char* agg_name(int fn) {
    switch (distinct_plain_fn(fn)) {
        case BHIP_AGG_SUM: return "SUM";
        case BHIP_AGG_AVG: return "AVG";
        case BHIP_AGG_COUNT: return "COUNT";
        case BHIP_AGG_MIN: return "MIN";
        default: return "MAX";
    }
}

HashAggregateExec::HashAggregateExec(int mode, std::vector<std::pair<ExprPtr, std::string>> group_exprs,
                                     std::vector<AggregateDesc> aggr, PlanPtr input)
    : mode_(mode), group_(std::move(group_exprs)), aggr_(std::move(aggr)) {
    input_ = std::move(input);
    ctx_ = input_->context();
    if (mode != BHIP_AGG_PARTIAL && mode != BHIP_AGG_FINAL && mode != BHIP_AGG_SINGLE) fail(BHIP_EINVAL, "Unsupported aggregate mode");
    const Schema& in = *input_->schema();
    if (mode == BHIP_AGG_SINGLE) {
        check_single();                                    // ops_agg_wide.cpp: legality, schema_, single_plan_
        return;
    }
    for (auto& a : aggr_)
        if (is_distinct_fn(a.fn))
            fail(BHIP_ENOTIMPL, std::string(agg_name(a.fn)) + "(DISTINCT " + a.arg->to_string() + ") in a " + (mode == BHIP_AGG_PARTIAL ? "Partial" : "Final") +
                                    " aggregate: the state of a DISTINCT aggregate is a set, not a column; use the Single mode (BHIP_AGG_SINGLE)");
    auto s = std::make_shared<Schema>();
    for (auto& g : group_) {
        const int t = expr_type(g.first, in);
        s->fields.push_back(Field{g.second, t, expr_nullable(g.first, in), t == DT_UTF8 && expr_large(g.first, in), t == DT_UTF8 && expr_binary(g.first, in)});
    }
    size_t state_pos = group_.size();
    for (auto& a : aggr_) {
        if (a.fn < BHIP_AGG_SUM || a.fn > BHIP_AGG_MAX) fail(BHIP_ENOTIMPL, "Unsupported aggregate function");
        if (mode == BHIP_AGG_PARTIAL) {
            const int t = expr_type(a.arg, in);
            if ((a.fn == BHIP_AGG_SUM || a.fn == BHIP_AGG_AVG) && (t == DT_UTF8 || t == DT_BOOLEAN))
                fail(BHIP_EINVAL, std::string(agg_name(a.fn)) + " does not support " + dtype_name(t));
            switch (a.fn) {
                case BHIP_AGG_SUM: s->fields.push_back(Field{a.name + "[sum]", sum_type(t), true}); break;
                case BHIP_AGG_AVG:
                    s->fields.push_back(Field{a.name + "[count]", DT_UINT64, false});
                    s->fields.push_back(Field{a.name + "[sum]", DT_FLOAT64, true});
                    break;
                case BHIP_AGG_COUNT: s->fields.push_back(Field{a.name + "[count]", DT_UINT64, false}); break;
                case BHIP_AGG_MIN: s->fields.push_back(Field{a.name + "[min]", t, true, t == DT_UTF8 && expr_large(a.arg, in)}); break;
                default: s->fields.push_back(Field{a.name + "[max]", t, true, t == DT_UTF8 && expr_large(a.arg, in)}); break;
            }
        } else {
            const size_t need = a.fn == BHIP_AGG_AVG ? 2 : 1;
            if (state_pos + need > in.fields.size()) fail(BHIP_EINVAL, "Final aggregate: input has too few state columns");
            switch (a.fn) {
                case BHIP_AGG_AVG: s->fields.push_back(Field{a.name, DT_FLOAT64, true}); break;
                case BHIP_AGG_COUNT: s->fields.push_back(Field{a.name, DT_UINT64, false}); break;
                default: s->fields.push_back(Field{a.name, in.fields[state_pos].dtype, true, in.fields[state_pos].large}); break;
            }
            state_pos += need;
        }
    }
    schema_ = s;
    // string nodes in the expressions, MIN / MAX over Utf8: run_strings (ops_agg_wide.cpp)
    for (auto& g : group_) strings_ = strings_ || has_lowered_node(g.first, in) || (g.first->kind == BHIP_EXPR_LITERAL && g.first->dtype == DT_UTF8);
    size_t sp = group_.size();
    for (auto& a : aggr_) {
        if (mode == BHIP_AGG_PARTIAL) {
            strings_ = strings_ || has_lowered_node(a.arg, in);
            if ((a.fn == BHIP_AGG_MIN || a.fn == BHIP_AGG_MAX) && expr_type(a.arg, in) == DT_UTF8) strings_ = true;
        } else {
            if ((a.fn == BHIP_AGG_MIN || a.fn == BHIP_AGG_MAX) && in.fields[sp].dtype == DT_UTF8) strings_ = true;
            sp += a.fn == BHIP_AGG_AVG ? 2 : 1;
        }
    }
}

PlanPtr HashAggregateExec::with_new_children(const std::vector<PlanPtr>& c) const {
    if (c.size() != 1) fail(BHIP_EINVAL, "HashAggregateExec wrong number of children");
    return std::make_shared<HashAggregateExec>(mode_, group_, aggr_, c[0]);
}

std::string HashAggregateExec::describe() const {
    std::string s = std::string("HashAggregateExec: mode=") + (mode_ == BHIP_AGG_PARTIAL ? "Partial" : mode_ == BHIP_AGG_FINAL ? "Final" : "Single") + ", gby=[";
    for (size_t i = 0; i < group_.size(); ++i) s += (i ? ", " : "") + group_[i].first->to_string();
    s += "], aggr=[";
    for (size_t i = 0; i < aggr_.size(); ++i)
        s += (i ? ", " : "") + std::string(agg_name(aggr_[i].fn)) + (is_distinct_fn(aggr_[i].fn) ? "(DISTINCT " : "(") + aggr_[i].arg->to_string() + ")";
    return s + "]";
}

StreamPtr HashAggregateExec::execute(int partition, const Exec& ex) const {
    check_partition(*this, partition);
    auto self = std::static_pointer_cast<const HashAggregateExec>(shared_from_this());
    return StreamPtr(new LazyStream(schema_, [self, partition, ex]() { return self->run(partition, ex); }));
}

namespace {

struct FusedInput {
    PlanPtr source;
    ExprPtr predicate;                       // over source schema, may be null
    std::vector<ExprPtr> group;              // over source schema
    std::vector<ExprPtr> args;               // Partial: aggregate arguments; Final: unused
};

FusedInput fuse_below(const PlanPtr& input, std::vector<ExprPtr> group, std::vector<ExprPtr> args) {
    FusedInput f;
    f.source = input;
    f.group = std::move(group);
    f.args = std::move(args);
    for (;;) {
        if (auto* flt = dynamic_cast<const FilterExec*>(f.source.get())) {
            if (has_lowered_node(flt->predicate(), *flt->input()->schema())) break;      // string nodes: the filter runs on its own (utf8_exprs.cpp)
            f.predicate = f.predicate ? make_binary(flt->predicate(), "And", f.predicate) : flt->predicate();
            f.source = flt->input();
        } else if (auto* co = dynamic_cast<const CoalesceBatchesExec*>(f.source.get())) {
            f.source = co->input();
        } else if (auto* pr = dynamic_cast<const ProjectionExec*>(f.source.get())) {
            bool strings = false;
            for (auto& en : pr->exprs()) strings = strings || has_lowered_node(en.first, *pr->input()->schema()) || (en.first->kind == BHIP_EXPR_LITERAL && en.first->dtype == DT_UTF8);
            if (strings) break;
            std::map<std::string, ExprPtr> subst;
            for (auto& en : pr->exprs()) subst[en.second] = en.first;
            for (auto& g : f.group) g = substitute(g, subst);
            for (auto& a : f.args) a = substitute(a, subst);
            if (f.predicate) f.predicate = substitute(f.predicate, subst);
            f.source = pr->input();
        } else {
            break;
        }
    }
    return f;
}

struct TimedLaunches {
    const Exec& ex;
    bool on;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    explicit TimedLaunches(const Exec& e) : ex(e), on(e.ctx->timing_enabled()) {}
    void begin() {
        if (!on) return;
        hipEvent_t a, b;
        HIP_CHECK(hipEventCreate(&a));
        HIP_CHECK(hipEventCreate(&b));
        HIP_CHECK(hipEventRecord(a, ex.stream));
        ev.push_back({a, b});
    }
    void end() {
        if (on) HIP_CHECK(hipEventRecord(ev.back().second, ex.stream));
    }
    const char* kernel = nullptr;
    const char* variant = nullptr;   // which instantiation of `kernel` ran (the lean path: generic or a specialised shape)
    void collect() {   // call after the stream was synchronised
        if (!on) return;
        double ms = 0;
        for (auto& p : ev) {
            float t = 0;
            if (hipEventElapsedTime(&t, p.first, p.second) == hipSuccess) ms += t;
            hipEventDestroy(p.first);
            hipEventDestroy(p.second);
        }
        ex.ctx->add_kernel_time(ms, ev.size(), kernel, variant);
        ev.clear();
    }
};

// ---- group table -> output batch ----------------------------------------------------------------------------------------------
// The output batch allocated for `n` rows, with what the emit kernels need to fill it.  `kinfo`: the packed-key layout of the pass
// that made the table.  A Utf8 key column's value bytes have the packed key's bound (width per group), so the bytes are written
// before their total is known: `utf8_cols` are the columns whose data_bytes finish_table sets once the totals are on the host.
using KeyLayout = std::vector<ProgramBuilder::KeyInfo>;
struct EmitColumns {
    std::shared_ptr<Batch> out;            // cols: the group columns, then the state / value columns
    std::vector<EmitKeySpec> key;
    std::vector<EmitValueSpec> value;      // count_is_rows set
    std::vector<size_t> utf8_cols;
};

EmitColumns alloc_emit_columns(const Exec& ex, const SchemaPtr& out_schema, const KeyLayout& kinfo, size_t n_keys,
                               const std::vector<EmitValueSpec>& emits, bool nullable, int64_t n) {
    EmitColumns E;
    E.out = new_batch(ex.ctx, out_schema, n);
    for (size_t gi = 0; gi < n_keys; ++gi) {
        const int dtype = out_schema->fields[gi].dtype;
        E.key.push_back(EmitKeySpec{kinfo[gi].pos, kinfo[gi].width, kinfo[gi].nullable, dtype});
        if (dtype == DT_UTF8) E.utf8_cols.push_back(gi);
        // Utf8: room for the packed key's bound; finish_table sets data_bytes
        E.out->cols.push_back(alloc_column(ex, dtype, n, kinfo[gi].nullable, n * (int64_t)kinfo[gi].width));
    }
    for (size_t k = 0; k < emits.size(); ++k) {
        const Field& fld = out_schema->fields[n_keys + k];
        E.value.push_back(emits[k]);
        E.value.back().count_is_rows = nullable ? 0 : 1;
        E.out->cols.push_back(alloc_column(ex, fld.dtype, n, fld.nullable));
    }
    return E;
}

// every column in one launch (emit_all_kernel, emit_slots_kernel); totals[gi]: where a Utf8 key column's byte total goes
EmitAllArgs emit_all_args(const EmitColumns& E, uint64_t* totals) {
    EmitAllArgs A;
    memset(&A, 0, sizeof(A));
    A.n_keys = (int32_t)E.key.size();
    A.n_values = (int32_t)E.value.size();
    for (size_t gi = 0; gi < E.key.size(); ++gi) {
        const Column& c = E.out->cols[gi];
        A.key[gi] = E.key[gi];
        A.key_data[gi] = c.data->ptr();
        A.key_validity[gi] = c.validity_words();
        if (c.offsets) { A.key_offsets[gi] = c.offsets->as<int32_t>(); A.key_total[gi] = totals + gi; }
    }
    for (size_t k = 0; k < E.value.size(); ++k) {
        const Column& c = E.out->cols[E.key.size() + k];
        A.value[k] = E.value[k];
        A.value_data[k] = c.data->ptr();
        A.value_validity[k] = c.validity_words();
    }
    return A;
}

// the row count (and the Utf8 byte totals) once the host knows them
void finish_table(const EmitColumns& E, int64_t n, const uint64_t* host_totals) {
    E.out->n_rows = n;
    for (auto& c : E.out->cols) c.length = n;
    for (size_t gi : E.utf8_cols) E.out->cols[gi].data_bytes = (int64_t)host_totals[gi];
}

}  // namespace

std::vector<BatchPtr> HashAggregateExec::run_packed(int partition, const Exec& ex, const HashAggregateExec* as_final) const {
    const Schema& in_schema = *input_->schema();
    const SchemaPtr out_schema = as_final ? as_final->schema_ : schema_;
    // ---- expressions over the (fused) source ---------------------------------------------------
    std::vector<ExprPtr> group, args;
    for (auto& g : group_) group.push_back(g.first);
    if (mode_ == BHIP_AGG_PARTIAL) {
        for (auto& a : aggr_) args.push_back(a.arg);
    } else {
        size_t pos = group_.size();
        for (auto& a : aggr_) {
            args.push_back(make_column(in_schema.fields[pos].name));
            if (a.fn == BHIP_AGG_AVG) args.push_back(make_column(in_schema.fields[pos + 1].name));
            pos += a.fn == BHIP_AGG_AVG ? 2 : 1;
        }
    }
    FusedInput f = fuse_below(input_, group, args);
    const Schema& src_schema = *f.source->schema();

    ProgramBuilder pb(src_schema);
    if (f.predicate) pb.set_predicate(f.predicate);
    for (auto& g : f.group) pb.add_key(g);

    std::vector<SopAccExpr> acc_exprs;  // accumulator index -> (kind, input expression)
    auto add_acc = [&](int kind, const ExprPtr& e) {
        const int idx = pb.add_acc(kind, pb.compile(e));
        if (idx == (int)acc_exprs.size()) acc_exprs.push_back(SopAccExpr{kind, e});
        return idx;
    };
    std::vector<EmitValueSpec> emits;   // one per output state/value column
    auto emit = [&](int kind, int a, int b, int dtype) { emits.push_back(EmitValueSpec{kind, a, b, 0, dtype}); };
    size_t ai = 0;
    for (auto& a : aggr_) {
        if (mode_ == BHIP_AGG_PARTIAL) {
            const ExprPtr& arg = f.args[ai++];
            const int t = expr_type(arg, src_schema);
            const bool lit_nonnull = arg->kind == BHIP_EXPR_LITERAL && !arg->is_null;
            switch (a.fn) {
                case BHIP_AGG_SUM: {
                    // (SUM(Float32) adds doubles and rounds the total to float once: closer to the exact sum than the reference's running float)
                    const int acc = add_acc(dt_is_float(t) ? ACC_SUM_F64 : ACC_SUM_I64, arg);
                    emit(EMIT_VALUE, acc, 0, sum_type(t));
                } break;
                case BHIP_AGG_AVG: {
                    ExprPtr farg = arg;
                    if (t != DT_FLOAT64) {
                        auto c = std::make_shared<Expr>();
                        c->kind = BHIP_EXPR_CAST;
                        c->dtype = DT_FLOAT64;
                        c->args = {arg};
                        farg = c;
                    }
                    const int acc = add_acc(ACC_SUM_F64, farg);
                    if (as_final) {
                        // [count], [sum] of the one partition -> sum / count, NULL without a non-NULL input: what the Final makes of them
                        emit(EMIT_AVG, acc, 0, DT_FLOAT64);
                        break;
                    }
                    emit(EMIT_COUNT, acc, 0, DT_UINT64);
                    emit(EMIT_VALUE, acc, 0, DT_FLOAT64);
                } break;
                case BHIP_AGG_COUNT: {
                    if (lit_nonnull || !expr_nullable(arg, src_schema)) { emit(EMIT_ROWS, 0, 0, DT_UINT64); break; }
                    ExprPtr carg = arg;
                    if (t == DT_UTF8) {
                        // COUNT(s) counts the non-NULL strings: count CASE WHEN s IS NOT NULL THEN 1 END instead,
                        // an Int64 value with the same validity (the VM keeps no per-row Utf8 values)
                        auto nn = std::make_shared<Expr>();
                        nn->kind = BHIP_EXPR_IS_NOT_NULL;
                        nn->args = {arg};
                        auto one = std::make_shared<Expr>();
                        one->kind = BHIP_EXPR_LITERAL;
                        one->dtype = DT_INT64;
                        one->i64 = 1;
                        auto cs = std::make_shared<Expr>();
                        cs->kind = BHIP_EXPR_CASE;
                        cs->args = {ExprPtr(nn), ExprPtr(one)};
                        carg = cs;
                    }
                    Operand x = pb.compile(carg);
                    if (x.is_utf8_col) fail(BHIP_ENOTIMPL, "COUNT over a Utf8-valued expression");
                    const int acc = add_acc(x.vclass == VC_BOOL ? ACC_COUNT_VALID_B : ACC_COUNT_VALID, carg);
                    emit(EMIT_RAW, acc, 0, DT_UINT64);
                } break;
                default: {
                    if (t == DT_UTF8) fail(BHIP_ENOTIMPL, "MIN/MAX over Utf8 on the packed-key path (run_strings handles it)");
                    if (t == DT_BOOLEAN) fail(BHIP_ENOTIMPL, "MIN/MAX over Boolean");
                    const bool is_min = a.fn == BHIP_AGG_MIN;
                    const int kind = minmax_kind(t, is_min);
                    emit(EMIT_VALUE, add_acc(kind, arg), 0, t);
                } break;
            }
        } else {
            const ExprPtr& st0 = f.args[ai++];
            const int t = expr_type(st0, src_schema);
            switch (a.fn) {
                case BHIP_AGG_SUM: {
                    const int acc = add_acc(dt_is_float(t) ? ACC_SUM_F64 : ACC_SUM_I64, st0);
                    emit(EMIT_VALUE, acc, 0, t);
                } break;
                case BHIP_AGG_AVG: {
                    const ExprPtr& st1 = f.args[ai++];
                    const int acc_c = add_acc(ACC_SUM_I64, st0);
                    const int acc_s = add_acc(ACC_SUM_F64, st1);
                    emit(EMIT_AVG_ACC, acc_s, acc_c, DT_FLOAT64);
                } break;
                case BHIP_AGG_COUNT: emit(EMIT_RAW, add_acc(ACC_SUM_I64, st0), 0, DT_UINT64); break;
                default: {
                    const bool is_min = a.fn == BHIP_AGG_MIN;
                    const int kind = minmax_kind(t, is_min);
                    emit(EMIT_VALUE, add_acc(kind, st0), 0, t);
                } break;
            }
        }
    }
    ScanParams P0;
    pb.finish(P0);
    const int n_acc = P0.n_acc;
    // register-resident fast path when the plan has the chain-of-products shape (kernels_sop.hip)
    SopPlan sop;
    static const bool sop_disabled = env_flag("BHIP_NO_SOP");
    bool use_sop = !sop_disabled && !pb.creates_nulls() && (int)acc_exprs.size() == n_acc && n_acc <= SOP_NSTEP &&
                   build_sop(src_schema, f.predicate, f.group, acc_exprs, sop);

    // ---- input ------------------------------------------------------------------------------------
    std::vector<BatchPtr> inputs;
    {
        StreamPtr s;
        if (auto hj = dynamic_cast<const HashJoinExec*>(f.source.get())) {
            // aggregate over a join: the join gathers only the columns the aggregate's program reads
            std::vector<bool> needed(src_schema.fields.size(), false);
            for (int ci : pb.columns()) needed[ci] = true;
            s = hj->execute_needed(partition, ex, needed);
        } else {
            s = f.source->execute(partition, ex);
        }
        while (BatchPtr b = s->next())
            if (b->n_rows > 0) inputs.push_back(b);
    }
    trace_point("aggregate: inputs ready");
    bool nullable = pb.creates_nulls();
    for (auto& b : inputs)
        for (int ci : pb.columns())
            if (b->cols[ci].validity) nullable = true;

    // the fast path packs keys its own way, so it serves either every batch of the run or none.
    // Its wide-load variant (lean_kernel.h) also takes NULLs in the columns the predicate constrains.
    static const bool lean_disabled = env_flag("BHIP_NO_LEAN");
    bool use_lean = use_sop && !lean_disabled && lean_eligible(sop.prog);
    for (auto& b : inputs) {
        if (use_lean && !(sop_columns_bindable(sop, *b, true) && lean_bindable(sop, *b))) use_lean = false;
        if (use_sop && !sop_columns_bindable(sop, *b)) use_sop = false;
    }
    // A Utf8 key longer than the fast paths hold (3 bytes wide-load, 7 bytes register kernel) sends them back empty-handed after a
    // whole pass over the input each.  Short codes (Q1's flags: 1 byte on average) are taken on trust; a key column that averages
    // more than 2 bytes per value has the longest string of its leading 64 Ki rows measured first (one small launch).
    if ((use_lean || use_sop) && !inputs.empty() && inputs[0]->n_rows >= (1 << 17)) {
        const Batch& b0 = *inputs[0];
        uint32_t longest = 0;
        for (auto& g : f.group) {
            if (g->kind != BHIP_EXPR_COLUMN) continue;
            const int ci = src_schema.index_of(g->name);
            if (ci < 0 || b0.cols[ci].dtype != DT_UTF8 || b0.cols[ci].data_bytes <= 2 * b0.n_rows) continue;
            Temp t2(ex);
            uint32_t* dev = t2.get<uint32_t>(1);
            TIMED_LAUNCH(ex, "utf8_max_len", launch_utf8_max_len(ex.cfg(), b0.cols[ci].offsets->as<int32_t>(), std::min<int64_t>(b0.n_rows, 65536), dev));
            longest = std::max(longest, read_device(ex, dev));
        }
        if (longest > 3) use_lean = false;
        if (longest > 7) use_sop = false;
    }
    const KeyLayout* key_layout = &pb.key_info();   // of the pass that produced `table`: the fast paths pack keys their own way (sop.key_info)

    Temp tmp(ex);
    const LaunchCfg cfg = ex.cfg();
    // status of the scan + merge and the byte totals of the Utf8 key columns, side by side: ONE read brings both back
    TailInfo* info = tmp.get<TailInfo>(1);
    ScanStatus* status = &info->st;
    uint64_t* totals = group_.size() <= (size_t)TAIL_TOTALS ? info->totals : tmp.get<uint64_t>(group_.size() + 1);
    GroupRec* table = nullptr;
    int64_t n_groups = 0;
    TimedLaunches timer(ex);

    // ---- group table -> output batch (allocated in ONE place: alloc_emit_columns) ------------------
    // `n_alloc` rows are allocated; dev_n != nullptr: the kernels read the count themselves (<= n_alloc), the host learns it later.
    auto alloc_columns = [&](const KeyLayout& kinfo, int64_t n) { return alloc_emit_columns(ex, out_schema, kinfo, group_.size(), emits, nullable, n); };
    auto emit_table = [&](const GroupRec* tab, int64_t n_alloc, const ScanStatus* dev_n, const KeyLayout& kinfo) {
        EmitColumns E = alloc_columns(kinfo, n_alloc);
        if (dev_n && n_alloc <= EMIT_ALL_MAX_GROUPS && group_.size() <= (size_t)EMIT_ALL_MAX_KEYS && emits.size() <= (size_t)EMIT_ALL_MAX_VALUES) {
            // the small table of the register path: every column in ONE launch, count read on the device
            EmitAllArgs A = emit_all_args(E, totals);
            A.table = tab;
            A.status = dev_n;
            TIMED_LAUNCH(ex, "emit_all", launch_emit_all(cfg, A));
            return E;
        }
        for (size_t gi = 0; gi < group_.size(); ++gi) {
            const Column& c = E.out->cols[gi];
            const EmitKeySpec& ks = E.key[gi];
            uint64_t* vptr = c.validity_words();
            if (c.dtype != DT_UTF8) {
                if (n_alloc) TIMED_LAUNCH(ex, "emit_group_key", launch_emit_group_key(cfg, tab, n_alloc, ks, c.data->ptr(), vptr, nullptr, dev_n));
            } else if (n_alloc > 0 && n_alloc <= EMIT_UTF8_SMALL_MAX) {
                TIMED_LAUNCH(ex, "emit_group_utf8_small", launch_emit_group_utf8_small(cfg, tab, n_alloc, ks, vptr, c.offsets->as<int32_t>(),
                                                       c.data->as<uint8_t>(), totals + gi, dev_n));
            } else {
                uint32_t* lengths = tmp.get<uint32_t>((size_t)n_alloc + 1);
                void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_alloc));
                if (n_alloc) TIMED_LAUNCH(ex, "emit_group_key", launch_emit_group_key(cfg, tab, n_alloc, ks, nullptr, vptr, lengths));
                HIP_CHECK(exclusive_scan_u32_i32(ex.stream, lengths, n_alloc, c.offsets->as<int32_t>(), true, totals + gi, scan_tmp));
                if (n_alloc) TIMED_LAUNCH(ex, "emit_group_utf8", launch_emit_group_utf8(cfg, tab, n_alloc, ks, c.offsets->as<int32_t>(), c.data->as<uint8_t>()));
            }
        }
        // value columns: one launch per EMIT_BATCH_MAX columns
        EmitValueBatch vb;
        vb.n = 0;
        for (size_t k = 0; k < emits.size(); ++k) {
            const Column& c = E.out->cols[group_.size() + k];
            vb.spec[vb.n] = E.value[k];
            vb.data[vb.n] = c.data->ptr();
            vb.validity[vb.n] = c.validity_words();
            if (++vb.n == EMIT_BATCH_MAX || k + 1 == emits.size()) {
                TIMED_LAUNCH(ex, "emit_group_values", launch_emit_group_values(cfg, tab, n_alloc, vb, dev_n));
                vb.n = 0;
            }
        }
        return E;
    };
    // ... and from the run slots of a clustered hash aggregate (kernels_util.hip: emit_slots_kernel), every column in one launch
    // (fixed-width, non-Boolean keys in the VM's layout: the `slot_keys` guard below)
    auto emit_slots = [&](const SlotSource& slots, int64_t n) {
        EmitColumns E = alloc_columns(pb.key_info(), n);
        TIMED_LAUNCH_N(ex, "emit_slots", n, launch_emit_slots(cfg, slots, n, emit_all_args(E, totals)));
        return E;
    };
    SlotSource slots;
    memset(&slots, 0, sizeof(slots));

    int gmax = group_.empty() ? 1 : 4;
    const int hint = path_hint_.load();
    if (hint == 8 || hint == -1) gmax = hint;
    int64_t total_in = 0;
    for (auto& b : inputs) total_in += b->n_rows;
    // more than 8 accumulators: the hash path — except over a tiny input (the Final aggregate over a few partial-state rows
    // per rank), where the 16-accumulator variant of the register kernel is ONE launch instead of a dozen
    const bool wide_acc = n_acc > AGG_NACC;
    if (wide_acc && (total_in > 65536 || hint == -1)) gmax = -1;

    // A plan that has not run yet does not know how many groups there are.  With a large input the ladder below (4 groups per
    // workgroup -> 8 -> hash table) is first walked on the leading 32 Ki rows only: an aggregate with many groups (Q3: one per
    // order) finds out for the price of two tiny launches instead of two passes over the whole input.
    std::vector<BatchPtr> sample;
    // (not for the wide-load path: its plans have at most two 32-bit key parts — flags, short codes — and its launches are the
    // ones the bench's roofline line and the rocprofv3 averages are about)
    // (a mid-sized input — up to 1 Mi rows: one of these launches is ~0.05 ms whatever it reads — is not sampled; with at most four
    // accumulators it starts at 8 groups, whose kernel then holds as many accumulator registers as the 4-group one with eight)
    const bool mid_sized = total_in < (1 << 20);
    if (hint == 0 && gmax == 4 && mid_sized && !wide_acc && n_acc <= 4 && !use_lean) gmax = 8;
    if (hint == 0 && gmax > 0 && !group_.empty() && !use_lean && (!mid_sized || (gmax == 4 && total_in >= (1 << 17)))) {
        auto head = std::make_shared<Batch>(*inputs[0]);
        head->n_rows = std::min<int64_t>(head->n_rows, 32768);
        sample.push_back(head);
    }
    // the head is read at the wider of the two register widths straight away: its group count then picks the width for the whole
    // input (<= 4: the 4-group kernel, which prefetches; <= 8: this one; more: the hash table) — one small launch, not two
    const bool probe8 = !sample.empty() && gmax == 4 && !wide_acc;
    if (probe8) gmax = 8;
    EmitColumns early;                   // early.out: the emit queued behind the merge of the latest round
    TailInfo tail;
    memset(&tail, 0, sizeof(tail));
    static const bool no_early_emit = env_flag("BHIP_NO_EARLY_EMIT");
    while (!inputs.empty()) {
        const bool sampling = !sample.empty();
        const std::vector<BatchPtr>& cur = sampling ? sample : inputs;
        if (gmax == -1) {
            // ---- hash path: one device-wide table, atomics ----------------------------------------
            early = EmitColumns();
            key_layout = &pb.key_info();     // the hash path packs keys with the VM's layout
            // (fixed-width, non-Boolean keys: a clustered input's groups can be emitted straight from their run slots)
            bool slot_keys = group_.size() <= (size_t)EMIT_ALL_MAX_KEYS && emits.size() <= (size_t)EMIT_ALL_MAX_VALUES;
            for (size_t gi = 0; gi < group_.size(); ++gi)
                slot_keys = slot_keys && out_schema->fields[gi].dtype != DT_UTF8 && out_schema->fields[gi].dtype != DT_BOOLEAN;
            const HashAggResult hr = hash_aggregate(ex, tmp, P0, pb, inputs, nullable, status, &clustered_hint_, slot_keys);
            table = hr.table;
            n_groups = hr.n_groups;
            slots = hr.slots;
            break;
        }
        // ---- register path ----------------------------------------------------------------------
        const int max_grid = scan_agg_lowcard_max_grid(cfg);
        const size_t max_parts = cur.size() * (size_t)max_grid;
        GroupRec* partials = tmp.get<GroupRec>(max_parts * gmax);
        uint32_t* partial_ng = tmp.get<uint32_t>(max_parts);
        HIP_CHECK(hipMemsetAsync(status, 0, sizeof(ScanStatus), ex.stream));
        int n_part = 0;
        const bool lean_now = use_lean && (gmax == 1 || gmax == 4);
        const bool sop_now = !lean_now && use_sop;
        key_layout = lean_now || sop_now ? &sop.key_info : &pb.key_info();
        // several SMALL input batches on the VM kernel (the partial states of N ranks under a Final aggregate: one 4-row batch per
        // rank): one launch for all of them — the kernel's fixed cost is ~0.1 ms per launch with 16 accumulators, which a rank of an
        // 8-GPU Q1 would pay eight times per step
        int64_t cur_rows = 0;
        for (auto& b : cur) cur_rows += b->n_rows;
        const bool together = !lean_now && !sop_now && cur.size() > 1 && cur.size() <= 4096 && cur_rows <= (1 << 20);
        bool lens_seen = lean_now && !sampling;        // every launch of this round reports the lengths of all its Utf8 keys' values
        std::vector<ScanParams> Ps;                    // (lives until this round's host wait below: the copy to the device may read it late)
        if (together) {
            Ps.assign(cur.size(), P0);
            for (size_t i = 0; i < cur.size(); ++i) ProgramBuilder::bind(Ps[i], pb.columns(), *cur[i], nullable);
            int grid = 0;
            TIMED_LAUNCH(ex, lowcard_launch_name(gmax, true),
                         launch_scan_agg_lowcard(cfg, Ps[0], tmp.get<ScanParams>(cur.size()), gmax, partials, partial_ng, max_grid, status, &grid, (int)cur.size()));
            n_part = grid;
        }
        for (auto& b : cur) {
            if (together) break;
            ScanParams P = P0;
            ProgramBuilder::bind(P, pb.columns(), *b, nullable);
            int grid = 0;
            // the bench hook times the dominant (large) launches only; BHIP_KERNEL_TIMING=2 names every launch (the tests read the route)
            const bool timed = b->n_rows >= (1 << 16) || ((lean_now || sop_now) && ex.ctx->timing_level() >= 2);
            if (timed) {
                timer.begin();
                timer.kernel = lean_now ? "scan_agg_lean_kernel" : sop_now ? "scan_agg_sop_kernel" : "scan_agg_lowcard_kernel";
                timer.variant = nullptr;
            }
            if (lean_now) {
                bind_sop(sop, *b);
                const char* variant = nullptr;
                bool fixed_keys = false;
                uint32_t step_alias = 0;
                HIP_CHECK(launch_scan_agg_lean(cfg, sop.prog, tmp.get<SopProgram>(1), gmax, partials + (size_t)n_part * gmax,
                                               partial_ng + n_part, max_grid, status, &grid, &variant, &fixed_keys, &step_alias));
                if (timed) timer.variant = variant;
                bool utf8_key = false;
                for (int q = 0; q < sop.prog.n_keys; ++q) utf8_key = utf8_key || sop.prog.keys[q].kind == SOP_KEY_UTF8;
                ex.ctx->set_lean_key_form(fixed_keys ? "fixed" : utf8_key ? "offsets" : "none");
                ex.ctx->set_lean_step_alias(step_alias, sop.prog.n_steps);
                lens_seen = lens_seen && !fixed_keys;
            } else if (sop_now) {
                bind_sop(sop, *b);
                HIP_CHECK(launch_scan_agg_sop(cfg, sop.prog, tmp.get<SopProgram>(1), gmax, partials + (size_t)n_part * gmax,
                                              partial_ng + n_part, max_grid, status, &grid));
            } else
                TIMED_LAUNCH(ex, lowcard_launch_name(gmax, false),
                             launch_scan_agg_lowcard(cfg, P, tmp.get<ScanParams>(1), gmax, partials + (size_t)n_part * gmax,
                                                     partial_ng + n_part, max_grid, status, &grid));
            if (timed) timer.end();
            n_part += grid;
        }
        const int cap = 1024;
        table = tmp.get<GroupRec>(cap);
        uint32_t* entry_group = tmp.get<uint32_t>((size_t)n_part * gmax);
        AccSpec specs[VM_MAX_ACC];
        for (int i = 0; i < n_acc; ++i) specs[i] = P0.acc[i];
        TIMED_LAUNCH(ex, "merge_partials", launch_merge_partials(cfg, partials, partial_ng, n_part, gmax, specs, n_acc, table, cap, entry_group, status));
        // the table has at most `cap` groups: its columns are emitted for that bound straight away, behind the merge and with the
        // count read on the device, so the host waits ONCE per aggregate (the result is dropped if the ladder has to go on)
        early = EmitColumns();
        if (!sampling && !no_early_emit && group_.size() <= (size_t)TAIL_TOTALS) early = emit_table(table, cap, status, *key_layout);
        trace_point("aggregate: scan + merge + emit queued");
        tail = read_device(ex, info);
        const ScanStatus st = tail.st;
        timer.collect();
        if (lean_now && (st.flags & SCAN_ERR_KEY_TOO_LONG)) {
            use_lean = false;                // a string key longer than 3 bytes: the 7-byte variant next
            continue;
        }
        if (sop_now && (st.flags & SCAN_ERR_KEY_TOO_LONG)) {
            use_sop = false;                 // a string key longer than the fast path's 7 bytes: the VM packs up to 15
            continue;
        }
        check_scan_flags(st);
        if (st.flags & SCAN_OVERFLOW_GROUPS) {
            gmax = (gmax == 4 && !wide_acc) ? 8 : -1;       // more groups than the register path holds: widen, then hash
            path_hint_.store(gmax);
            if (gmax == -1) sample.clear();
            continue;
        }
        if (sampling) {                                   // the head fits this width: now the whole input
            if (probe8 && st.n_groups <= 4) gmax = 4;
            sample.clear();
            continue;
        }
        // The scan read the length of every value of its Utf8 key columns (before the range test, so of filtered-out rows
        // too) and ORed / ANDed them per key part.  Equal, and 1..3: every value of those columns has that width, which the
        // next scan of the same buffers then takes as given (Buffer::uniform_width; lean_spec_kernel.h reads no offsets).
        // Only for a column scanned whole: not a head-only launch, not one that gave up on too many groups.
        if (lens_seen) {
            for (int q = 0; q < sop.prog.n_keys && q < 2; ++q) {
                const uint32_t w = sop.prog.keys[q].kind == SOP_KEY_UTF8 ? scan_len_uniform(st.flags, q) : 0;
                if (w < 1 || w > 3) continue;
                for (auto& b : cur) {
                    const Column& c = b->cols[sop.col_map[sop.prog.keys[q].col]];
                    if (c.offsets && c.length == b->n_rows) c.offsets->set_uniform_width(b->n_rows, (int32_t)w);
                }
            }
        }
        n_groups = st.n_groups;
        break;
    }

    if (n_groups == 0 && group_.empty()) {
        early = EmitColumns();
        // no GROUP BY: exactly one output row even for empty input (SUM = NULL, COUNT = 0)
        GroupRec id;
        memset(&id, 0, sizeof(id));
        for (int i = 0; i < n_acc; ++i) {
            switch (P0.acc[i].kind) {
                case ACC_MIN_F64:
                case ACC_MAX_F64: { double v = __builtin_nan(""); memcpy(&id.acc[i], &v, 8); } break;
                case ACC_MIN_I64: id.acc[i] = (uint64_t)INT64_MAX; break;
                case ACC_MAX_I64: id.acc[i] = (uint64_t)INT64_MIN; break;
                case ACC_MIN_U64: id.acc[i] = UINT64_MAX; break;
                case ACC_MAX_U64: id.acc[i] = 0; break;
                default: break;
            }
        }
        table = tmp.get<GroupRec>(1);
        HIP_CHECK(hipMemcpyAsync(table, &id, sizeof(id), hipMemcpyHostToDevice, ex.stream));
        stream_wait(ex);
        n_groups = 1;
    }

    trace_point("aggregate: done");
    if (early.out) {
        // the emit was queued behind the merge; the single read above brought the count and the Utf8 totals
        finish_table(early, n_groups, tail.totals);
        return {early.out};
    }
    const EmitColumns out = slots.valid ? emit_slots(slots, n_groups) : emit_table(table, n_groups, nullptr, *key_layout);
    if (!out.utf8_cols.empty()) {
        std::vector<uint64_t> host(group_.size() + 1);
        if (group_.size() <= (size_t)TAIL_TOTALS) {
            const TailInfo ti = read_device(ex, info);                      // the totals sit in the info block: one pinned-slot read
            for (size_t i = 0; i < group_.size(); ++i) host[i] = ti.totals[i];
        } else {
            HIP_CHECK(hipMemcpyAsync(host.data(), totals, group_.size() * 8, hipMemcpyDeviceToHost, ex.stream));
            stream_wait(ex);
        }
        finish_table(out, n_groups, host.data());
    }
    // (no wait otherwise: everything downstream is queued on the same stream, and scratch is released in stream order)
    return {out.out};
}

}  // namespace bhip
