// ops_window.cpp — WindowAggExec: ranking, LAG / LEAD / FIRST_VALUE / LAST_VALUE and running aggregates over one window
// specification (PARTITION BY ... ORDER BY ...), on the device (kernels_window.hip).
//
// The reference's serde has no window operator (rust/core/src/serde/physical_plan/from_proto.rs:58-346 builds none), so this one is
// reached through bhip_plan_window / bhip_plan_window_frames / bhip_plan_window_frame_specs only, like the join filter and the Semi / Anti joins; semantics: DESIGN.md "Window functions".
//
// The operator sorts its single input partition itself with SortExec's code (sort_permutation + take_batch; stable, so ties keep input
// order) by the partition keys ASC NULLS FIRST and then the order keys, and the rows leave in that order.  After the sort every function
// is a scan or a gather:
//   flags        rows i - 1 and i compared on the evaluated key columns: "starts a partition", "starts a peer group" (two bitmaps)
//   bounds       part_start / peer_start / peers_to (forward scan of the flags), part_end / peer_end (backward scan) — each made once, when
//                a function needs it
//   ranks        elementwise from the bounds; LAG / LEAD / FIRST_VALUE / LAST_VALUE: an index vector, then the outer-join gather
//   aggregates   a segmented inclusive scan of the argument (value + non-NULL count per row), then the finish kernel reads the running
//                state at the frame's last row: the row itself (ROWS), peer_end (RANGE) or part_end (whole partition)
//   sliding      a ROWS frame by offsets: (lo, hi) per row, once per distinct frame.  FIRST_VALUE / LAST_VALUE gather by them; COUNT and
//                the integer SUM take the scan and a difference of two running states; a frame that starts with the partition reads the
//                running state at hi; float SUM, AVG, MIN and MAX between two finite ends are aggregated straight from the argument
//                (window_slide: a bounded neighbourhood of each tile in LDS)
//   by value     a RANGE / GROUPS frame with offsets is another producer of (lo, hi): window_value_bounds searches the order key (RANGE) or
//                the peer-group numbers (GROUPS), once per distinct frame.  The four routes above then apply as they are, except that the
//                aggregates window_slide serves go to window_slide_value (the tile's span comes from the data), after ONE host read of the
//                widest frame found: beyond WINDOW_SLIDE_MAX_ROWS rows the query is refused there, when it runs
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../window_kernels.h"
#include "plan.hpp"

namespace bhip {

namespace {
const char* window_fn_name(int fn) {
    switch (fn) {
        case BHIP_WIN_ROW_NUMBER: return "ROW_NUMBER";
        case BHIP_WIN_RANK: return "RANK";
        case BHIP_WIN_DENSE_RANK: return "DENSE_RANK";
        case BHIP_WIN_LAG: return "LAG";
        case BHIP_WIN_LEAD: return "LEAD";
        case BHIP_WIN_FIRST_VALUE: return "FIRST_VALUE";
        case BHIP_WIN_LAST_VALUE: return "LAST_VALUE";
        case BHIP_WIN_SUM: return "SUM";
        case BHIP_WIN_AVG: return "AVG";
        case BHIP_WIN_COUNT: return "COUNT";
        case BHIP_WIN_MIN: return "MIN";
        default: return "MAX";
    }
}
const char* frame_name(int frame) {
    switch (frame) {
        case BHIP_FRAME_PARTITION: return "PARTITION";
        case BHIP_FRAME_ROWS_TO_CURRENT: return "ROWS_TO_CURRENT";
        default: return "RANGE_TO_CURRENT";
    }
}
bool is_ranking(int fn) { return fn == BHIP_WIN_ROW_NUMBER || fn == BHIP_WIN_RANK || fn == BHIP_WIN_DENSE_RANK; }
bool is_aggregate(int fn) { return fn >= BHIP_WIN_SUM && fn <= BHIP_WIN_MAX; }
bool has_frame(int fn) { return is_aggregate(fn) || fn == BHIP_WIN_LAST_VALUE; }
// a rows frame moves FIRST_VALUE too (a named frame always starts with the partition)
bool takes_rows_frame(int fn) { return has_frame(fn) || fn == BHIP_WIN_FIRST_VALUE; }

std::string bound_name(bool unbounded, int64_t offset, bool is_start) {
    if (unbounded) return is_start ? "UNBOUNDED PRECEDING" : "UNBOUNDED FOLLOWING";
    if (offset == 0) return "CURRENT ROW";
    // (the magnitude of INT64_MIN has no Int64)
    return offset < 0 ? std::to_string(0 - (uint64_t)offset) + " PRECEDING" : std::to_string(offset) + " FOLLOWING";
}
std::string rows_frame_name(const WindowRowsFrame& r) {
    return "ROWS BETWEEN " + bound_name(r.start_unbounded, r.start, true) + " AND " + bound_name(r.end_unbounded, r.end, false);
}
// the aggregates a prefix scan cannot slide: a difference of running Float64 sums cancels, MIN / MAX have no inverse
bool slides(int fn, int arg_dtype) { return fn == BHIP_WIN_AVG || fn == BHIP_WIN_MIN || fn == BHIP_WIN_MAX || (fn == BHIP_WIN_SUM && dt_is_float(arg_dtype)); }

// ---- frames in any units (bhip_frame_spec) ------------------------------------------------------------------------------------------
const char* units_name(int units) { return units == BHIP_FRAME_UNITS_RANGE ? "RANGE" : units == BHIP_FRAME_UNITS_GROUPS ? "GROUPS" : "ROWS"; }
// the shortest decimal that reads back to the same double, with a point so it does not read as an integer
std::string double_text(double v) {
    char buf[40];
    for (int digits = 1; digits <= 17; ++digits) {
        snprintf(buf, sizeof(buf), "%.*g", digits, v);
        if (strtod(buf, nullptr) == v) break;
    }
    std::string s = buf;
    if (s.find_first_of(".en") == std::string::npos) s += ".0";
    return s;
}
bool is_offset(const WindowFrameBound& b) { return b.kind == BHIP_BOUND_OFFSET; }
bool offset_positive(const WindowFrameBound& b) { return is_offset(b) && (b.is_float ? b.f > 0 : b.i > 0); }
bool offset_negative(const WindowFrameBound& b) { return is_offset(b) && (b.is_float ? b.f < 0 : b.i < 0); }
std::string value_bound_name(int units, const WindowFrameBound& b, bool is_start) {
    if (b.kind == BHIP_BOUND_UNBOUNDED) return is_start ? "UNBOUNDED PRECEDING" : "UNBOUNDED FOLLOWING";
    if (b.kind == BHIP_BOUND_CURRENT_ROW || (units == BHIP_FRAME_UNITS_GROUPS && b.i == 0)) return "CURRENT ROW";
    // RANGE: an offset of zero is not CURRENT ROW (it takes -0.0 and +0.0 together); it reads as the side it stands on
    const bool preceding = offset_negative(b) || (!offset_positive(b) && is_start);
    if (b.is_float) return double_text(std::fabs(b.f)) + (preceding ? " PRECEDING" : " FOLLOWING");
    return (b.i < 0 ? std::to_string(0 - (uint64_t)b.i) : std::to_string(b.i)) + (preceding ? " PRECEDING" : " FOLLOWING");
}
std::string value_frame_name(const WindowValueFrame& v) {
    return std::string(units_name(v.units)) + " BETWEEN " + value_bound_name(v.units, v.start, true) + " AND " + value_bound_name(v.units, v.end, false);
}
bool same_bound(const WindowFrameBound& a, const WindowFrameBound& b) { return a.kind == b.kind && a.is_float == b.is_float && a.i == b.i && a.f == b.f; }
bool range_key_type(int t) { return (dt_is_integer(t) || dt_is_float(t)) && dt_width(t) != 0; }
}  // namespace

WindowAggExec::WindowAggExec(std::vector<ExprPtr> partition_by, std::vector<SortDesc> order_by, std::vector<WindowFnDesc> fns, PlanPtr input)
    : partition_by_(std::move(partition_by)), order_by_(std::move(order_by)), fns_(std::move(fns)) {
    input_ = std::move(input);
    ctx_ = input_->context();
    const Schema& in = *input_->schema();
    if (partition_by_.size() > (size_t)WINDOW_MAX_KEYS || order_by_.size() > (size_t)WINDOW_MAX_KEYS)
        fail(BHIP_ENOTIMPL, "WindowAggExec takes at most " + std::to_string(WINDOW_MAX_KEYS) + " partition keys and " + std::to_string(WINDOW_MAX_KEYS) +
                                " order keys");
    if (fns_.empty()) fail(BHIP_EINVAL, "WindowAggExec needs at least one window expression");
    Utf8Lowering low(in);                  // a key or an argument like lower(s) is evaluated as a column first (utf8_exprs.cpp)
    for (auto& e : partition_by_) { expr_type(e, in); low.rewrite(e, true); }
    std::vector<int> order_types;
    for (auto& s : order_by_) { order_types.push_back(expr_type(s.expr, in)); low.rewrite(s.expr, true); }
    auto sch = std::make_shared<Schema>(in);
    for (auto& f : fns_) {
        if (f.fn < BHIP_WIN_ROW_NUMBER || f.fn > BHIP_WIN_MAX) fail(BHIP_EINVAL, "Unknown window function " + std::to_string(f.fn));
        if (f.frame < BHIP_FRAME_DEFAULT || f.frame > BHIP_FRAME_RANGE_TO_CURRENT) fail(BHIP_EINVAL, "Unknown window frame " + std::to_string(f.frame));
        const std::string fname = window_fn_name(f.fn);
        if (f.value.has) {
            // checked for every function, then ignored by those without a frame; ROWS units leave as a rows frame, the forms that are
            // named frames as those
            WindowValueFrame& v = f.value;
            v.slides = false;
            if (f.frame != BHIP_FRAME_DEFAULT)
                fail(BHIP_EINVAL, fname + ": a frame spec goes with BHIP_FRAME_DEFAULT, not with " + frame_name(f.frame));
            if (v.units < BHIP_FRAME_UNITS_ROWS || v.units > BHIP_FRAME_UNITS_GROUPS) fail(BHIP_EINVAL, fname + ": unknown frame units " + std::to_string(v.units));
            for (WindowFrameBound* b : {&v.start, &v.end}) {
                if (b->kind < BHIP_BOUND_UNBOUNDED || b->kind > BHIP_BOUND_OFFSET) fail(BHIP_EINVAL, fname + ": unknown frame bound kind " + std::to_string(b->kind));
                if (!is_offset(*b)) { *b = WindowFrameBound{b->kind, false, 0, 0.0}; continue; }    // (only an OFFSET reads its numbers)
                if (b->is_float) {
                    if (!std::isfinite(b->f)) fail(BHIP_EINVAL, fname + ": a frame offset must be a finite number, got " + (std::isnan(b->f) ? "NaN" : "an infinity"));
                    if (v.units != BHIP_FRAME_UNITS_RANGE) fail(BHIP_EINVAL, fname + ": a " + units_name(v.units) + " frame takes Int64 offsets, got a Float64");
                    b->i = 0;
                } else {
                    b->f = 0.0;
                }
            }
            if (v.units == BHIP_FRAME_UNITS_ROWS) {
                f.rows = WindowRowsFrame{true, v.start.kind == BHIP_BOUND_UNBOUNDED, v.end.kind == BHIP_BOUND_UNBOUNDED, v.start.i, v.end.i};
                v = WindowValueFrame{};
            } else {
                if (v.units == BHIP_FRAME_UNITS_RANGE && (is_offset(v.start) || is_offset(v.end))) {
                    const std::string what = fname + " " + value_frame_name(v);
                    if (order_by_.size() != 1)
                        fail(BHIP_EINVAL, what + ": a RANGE frame with an offset needs exactly one order key, got " + std::to_string(order_by_.size()));
                    const int kt = order_types[0];
                    if (!range_key_type(kt))
                        fail(BHIP_EINVAL, what + ": a RANGE frame with an offset needs an integer, float, date or timestamp order key, not " + dtype_name(kt));
                    for (WindowFrameBound* b : {&v.start, &v.end}) {
                        if (!is_offset(*b)) continue;
                        if (!dt_is_float(kt) && b->is_float)
                            fail(BHIP_EINVAL, what + ": the " + dtype_name(kt) + " order key takes Int64 offsets, got a Float64");
                        if (dt_is_float(kt) && !b->is_float) {
                            const double d = (double)b->i;          // (2^63 itself is no Int64: it cannot be cast back)
                            if (!(d < 9223372036854775808.0) || (int64_t)d != b->i)
                                fail(BHIP_EINVAL, what + ": the offset " + std::to_string(b->i) + " over the " + dtype_name(kt) + " order key is not exactly a Float64");
                            *b = WindowFrameBound{BHIP_BOUND_OFFSET, true, 0, d};
                        }
                    }
                }
                if (v.units == BHIP_FRAME_UNITS_GROUPS)
                    for (WindowFrameBound* b : {&v.start, &v.end})
                        if (b->kind == BHIP_BOUND_CURRENT_ROW) *b = WindowFrameBound{BHIP_BOUND_OFFSET, false, 0, 0.0};
                if (v.start.kind != BHIP_BOUND_UNBOUNDED && v.end.kind != BHIP_BOUND_UNBOUNDED &&
                    (v.start.is_float || v.end.is_float ? (v.start.is_float ? v.start.f : (double)v.start.i) > (v.end.is_float ? v.end.f : (double)v.end.i)
                                                        : v.start.i > v.end.i))     // (CURRENT ROW holds 0; beside a float only that 0 is an integer)
                    fail(BHIP_EINVAL, fname + " " + value_frame_name(v) + ": frame start lies after its end");
                const bool to_current = v.end.kind == BHIP_BOUND_CURRENT_ROW || (v.units == BHIP_FRAME_UNITS_GROUPS && is_offset(v.end) && v.end.i == 0);
                if (!takes_rows_frame(f.fn)) v = WindowValueFrame{};
                else if (v.start.kind == BHIP_BOUND_UNBOUNDED && v.end.kind == BHIP_BOUND_UNBOUNDED) { v = WindowValueFrame{}; f.frame = BHIP_FRAME_PARTITION; }
                else if (v.start.kind == BHIP_BOUND_UNBOUNDED && to_current) { v = WindowValueFrame{}; f.frame = BHIP_FRAME_RANGE_TO_CURRENT; }
            }
        }
        if (f.rows.has) {
            WindowRowsFrame& r = f.rows;
            if (f.frame != BHIP_FRAME_DEFAULT)
                fail(BHIP_EINVAL, fname + ": a rows frame goes with BHIP_FRAME_DEFAULT, not with " + frame_name(f.frame));
            if (r.start_unbounded) r.start = 0;                     // (an unbounded side's offset is not read)
            if (r.end_unbounded) r.end = 0;
            if (!r.start_unbounded && !r.end_unbounded && r.start > r.end)
                fail(BHIP_EINVAL, fname + " " + rows_frame_name(r) + ": frame start lies after its end");
            if (!takes_rows_frame(f.fn)) r = WindowRowsFrame{};     // ignored, as a named frame is
            else if (r.start_unbounded && r.end_unbounded) { r = WindowRowsFrame{}; f.frame = BHIP_FRAME_PARTITION; }
            else if (r.start_unbounded && r.end == 0) { r = WindowRowsFrame{}; f.frame = BHIP_FRAME_ROWS_TO_CURRENT; }
        }
        // (under a rows frame that stays one, `frame` is not read and stays DEFAULT: with_new_children hands the descriptions back in)
        if (f.frame == BHIP_FRAME_DEFAULT && !f.rows.has && !f.value.has) f.frame = order_by_.empty() ? BHIP_FRAME_PARTITION : BHIP_FRAME_RANGE_TO_CURRENT;      // SQL's default
        if (is_ranking(f.fn)) {
            f.arg = nullptr;
            sch->fields.push_back(Field{f.name, DT_UINT64, false});
            continue;
        }
        if (!f.arg) fail(BHIP_EINVAL, fname + " needs an argument");
        const int t = expr_type(f.arg, in);
        low.rewrite(f.arg, true);
        const bool large = t == DT_UTF8 && expr_large(f.arg, in), binary = t == DT_UTF8 && expr_binary(f.arg, in);
        if (f.rows.has && slides(f.fn, t) && t != DT_UTF8 && t != DT_BOOLEAN) {
            const WindowRowsFrame& r = f.rows;
            const std::string what = fname + "(" + dtype_name(t) + ") over " + rows_frame_name(r);
            if (r.end_unbounded)
                fail(BHIP_ENOTIMPL, what + ": a frame from an offset to UNBOUNDED FOLLOWING is supported for COUNT, integer SUM, FIRST_VALUE and LAST_VALUE only");
            // end - start as unsigned: exact for any two Int64 with start <= end
            if (!r.start_unbounded && (uint64_t)r.end - (uint64_t)r.start >= (uint64_t)WINDOW_SLIDE_MAX_ROWS)
                fail(BHIP_ENOTIMPL, what + ": a frame wider than " + std::to_string(WINDOW_SLIDE_MAX_ROWS) +
                                        " rows is supported for COUNT, integer SUM, FIRST_VALUE and LAST_VALUE only");
        }
        if (f.value.has && slides(f.fn, t) && t != DT_UTF8 && t != DT_BOOLEAN) {
            // (how wide a RANGE / GROUPS frame is lies in the data: run() refuses one wider than WINDOW_SLIDE_MAX_ROWS)
            if (f.value.end.kind == BHIP_BOUND_UNBOUNDED)
                fail(BHIP_ENOTIMPL, fname + "(" + dtype_name(t) + ") over " + value_frame_name(f.value) +
                                        ": a frame from an offset to UNBOUNDED FOLLOWING is supported for COUNT, integer SUM, FIRST_VALUE and LAST_VALUE only");
            f.value.slides = true;
        }
        const bool value_may_be_empty = f.value.has && (offset_positive(f.value.start) || offset_negative(f.value.end));
        switch (f.fn) {
            case BHIP_WIN_LAG: case BHIP_WIN_LEAD:
                if (f.offset < 0) fail(BHIP_EINVAL, fname + " offset must not be negative, got " + std::to_string(f.offset));
                sch->fields.push_back(Field{f.name, t, true, large, binary});
                break;
            case BHIP_WIN_FIRST_VALUE: case BHIP_WIN_LAST_VALUE:
                // a rows frame that can lie wholly before or after the partition's rows is empty there
                sch->fields.push_back(Field{f.name, t, expr_nullable(f.arg, in) || value_may_be_empty || (f.rows.has && ((!f.rows.start_unbounded && f.rows.start > 0) ||
                                                                                                                         (!f.rows.end_unbounded && f.rows.end < 0))),
                                            large, binary});
                break;
            case BHIP_WIN_SUM: case BHIP_WIN_AVG:
                if (t == DT_UTF8 || t == DT_BOOLEAN) fail(BHIP_EINVAL, fname + " does not support " + dtype_name(t));
                sch->fields.push_back(Field{f.name, f.fn == BHIP_WIN_AVG || dt_is_float(t) ? DT_FLOAT64 : dt_is_unsigned(t) ? DT_UINT64 : DT_INT64, true});
                break;
            case BHIP_WIN_COUNT:
                sch->fields.push_back(Field{f.name, DT_UINT64, false});
                break;
            default:
                if (t == DT_UTF8 || t == DT_BOOLEAN) fail(BHIP_ENOTIMPL, fname + " over " + dtype_name(t) + " is not supported as a window function");
                sch->fields.push_back(Field{f.name, t, true});
                break;
        }
    }
    low.validate();
    schema_ = sch;
}

PlanPtr WindowAggExec::with_new_children(const std::vector<PlanPtr>& c) const {
    if (c.size() != 1) fail(BHIP_EINVAL, "WindowAggExec wrong number of children");
    return std::make_shared<WindowAggExec>(partition_by_, order_by_, fns_, c[0]);
}

std::string WindowAggExec::describe() const {
    std::string s = "WindowAggExec: partition_by=[";
    for (size_t i = 0; i < partition_by_.size(); ++i) s += (i ? ", " : "") + partition_by_[i]->to_string();
    s += "], order_by=[";
    for (size_t i = 0; i < order_by_.size(); ++i)
        s += (i ? ", " : "") + order_by_[i].expr->to_string() + (order_by_[i].descending ? " DESC" : " ASC") +
             (order_by_[i].nulls_first ? " NULLS FIRST" : " NULLS LAST");
    s += "], fns=[";
    for (size_t i = 0; i < fns_.size(); ++i) {
        const WindowFnDesc& f = fns_[i];
        s += (i ? ", " : "") + std::string(window_fn_name(f.fn)) + "(" + (f.arg ? f.arg->to_string() : "");
        if (f.fn == BHIP_WIN_LAG || f.fn == BHIP_WIN_LEAD) s += ", " + std::to_string(f.offset);
        s += ")";
        if (f.rows.has) s += " " + rows_frame_name(f.rows);
        else if (f.value.has) s += " " + value_frame_name(f.value);
        else if (has_frame(f.fn)) s += std::string(" ") + frame_name(f.frame);
        s += " as " + f.name;
    }
    return s + "]";
}

StreamPtr WindowAggExec::execute(int partition, const Exec& ex) const {
    if (partition != 0) fail(BHIP_EINVAL, "WindowAggExec invalid partition " + std::to_string(partition));
    if (input_->output_partitioning().count != 1) fail(BHIP_EINVAL, "WindowAggExec requires a single input partition: put a MergeExec below it");
    auto self = std::static_pointer_cast<const WindowAggExec>(shared_from_this());
    return StreamPtr(new LazyStream(schema(), [self, ex]() -> std::vector<BatchPtr> {
        const std::vector<BatchPtr> parts = nonempty_batches(*self->input_->execute(0, ex));
        if (parts.empty()) return {};
        return {self->run(ex, concat_batches(ex, self->input_->schema(), parts))};
    }));
}

BatchPtr WindowAggExec::run(const Exec& ex, const BatchPtr& whole) const {
    const LaunchCfg cfg = ex.cfg();
    const int64_t n = whole->n_rows;
    // ---- the order: SortExec's own code over (partition keys ASC NULLS FIRST, order keys) -------------------------------------------
    std::vector<SortDesc> keys;
    for (auto& e : partition_by_) keys.push_back(SortDesc{e, false, true});
    for (auto& s : order_by_) keys.push_back(s);
    BatchPtr sorted = materialize_batch(ex, whole);
    if (!keys.empty() && n > 1) {
        BufferPtr perm = sort_permutation(ex, *sorted, keys);
        sorted = take_batch(ex, *sorted, perm->as<uint32_t>(), n, nullptr, /*permutation=*/true);
    }
    // ---- boundary flags from the key columns of the sorted rows ---------------------------------------------------------------------
    Temp tmp(ex);
    std::vector<Column> key_cols;                                  // keeps computed key columns alive until the launch is queued
    WindowKeys K;
    memset(&K, 0, sizeof(K));
    K.n_part = (int32_t)partition_by_.size();
    K.n_order = (int32_t)order_by_.size();
    for (size_t k = 0; k < keys.size(); ++k) {
        key_cols.push_back(evaluate_column(ex, *sorted, keys[k].expr));
        const Column& c = key_cols.back();
        if (!c.data || (c.dtype == DT_UTF8 && !c.offsets)) fail(BHIP_EEXEC, "WindowAggExec: a key column without buffers");
        K.col[k] = c.ref();
    }
    const size_t words = (size_t)((n + 63) / 64);
    uint64_t* part_flags = tmp.get<uint64_t>(words);
    uint64_t* peer_flags = tmp.get<uint64_t>(words);
    TIMED_LAUNCH_N(ex, "window_flags", n, launch_window_flags(cfg, K, n, part_flags, peer_flags));
    void* scan_temp = tmp.get<uint8_t>(window_scan_temp_bytes(n));  // one scan at a time uses it (stream order)
    // ---- bounds, each made when the first function asks for it ----------------------------------------------------------------------
    uint32_t *part_start = nullptr, *peer_start = nullptr, *peers_to = nullptr, *part_end = nullptr, *peer_end = nullptr;
    auto need_forward = [&]() {
        if (part_start) return;
        part_start = tmp.get<uint32_t>((size_t)n);
        peer_start = tmp.get<uint32_t>((size_t)n);
        peers_to = tmp.get<uint32_t>((size_t)n);
        TIMED_LAUNCH_N(ex, "window_bounds_forward_tiles", n, launch_window_bounds_forward_tiles(cfg, part_flags, peer_flags, n, scan_temp));
        TIMED_LAUNCH_N(ex, "window_bounds_forward_summaries", n, launch_window_bounds_forward_summaries(cfg, n, scan_temp));
        TIMED_LAUNCH_N(ex, "window_bounds_forward_apply", n,
                       launch_window_bounds_forward_apply(cfg, part_flags, peer_flags, n, scan_temp, part_start, peer_start, peers_to));
    };
    auto need_backward = [&]() {
        if (part_end) return;
        part_end = tmp.get<uint32_t>((size_t)n);
        peer_end = tmp.get<uint32_t>((size_t)n);
        TIMED_LAUNCH_N(ex, "window_bounds_backward_tiles", n, launch_window_bounds_backward_tiles(cfg, part_flags, peer_flags, n, scan_temp));
        TIMED_LAUNCH_N(ex, "window_bounds_backward_summaries", n, launch_window_bounds_backward_summaries(cfg, n, scan_temp));
        TIMED_LAUNCH_N(ex, "window_bounds_backward_apply", n,
                       launch_window_bounds_backward_apply(cfg, part_flags, peer_flags, n, scan_temp, part_end, peer_end));
    };
    // the last row of row i's frame: null = the row itself
    auto frame_end = [&](int frame) -> const uint32_t* {
        if (frame == BHIP_FRAME_ROWS_TO_CURRENT) return nullptr;
        need_backward();
        return frame == BHIP_FRAME_PARTITION ? part_end : peer_end;
    };
    // the (lo, hi) of every row under a rows frame, made once per distinct frame of the operator
    struct FrameRows { WindowRowsFrame r; const uint32_t *lo, *hi; };
    std::vector<FrameRows> frames;
    auto frame_rows = [&](const WindowRowsFrame& given) -> FrameRows {
        WindowRowsFrame r = given;                                  // offsets clamped to +-n: i + offset stays far from overflow on the device,
        r.start = std::max(-n, std::min(n, r.start));               // and a row n or more away lies outside every partition either way
        r.end = std::max(-n, std::min(n, r.end));
        for (const FrameRows& f : frames)
            if (f.r.start_unbounded == r.start_unbounded && f.r.end_unbounded == r.end_unbounded && f.r.start == r.start && f.r.end == r.end) return f;
        // a near frame is cut by the partition heads among the rows it reaches over: the flags, not the two bounds scans
        const bool near = window_frame_is_near(r.start_unbounded, r.start, r.end_unbounded, r.end);
        if (!near) {
            need_forward();
            need_backward();
        }
        uint32_t *lo = tmp.get<uint32_t>((size_t)n), *hi = tmp.get<uint32_t>((size_t)n);
        TIMED_LAUNCH_N(ex, "window_frame_bounds", n,
                       launch_window_frame_bounds(cfg, near ? part_flags : nullptr, near ? nullptr : part_start, near ? nullptr : part_end, r.start_unbounded,
                                                  r.start, r.end_unbounded, r.end, n, lo, hi));
        frames.push_back(FrameRows{r, lo, hi});
        return frames.back();
    };
    // ... and under a RANGE / GROUPS frame: the same (lo, hi), found by searching the order key / the peer-group numbers.  When a function
    // that window_slide_value serves uses the frame, the launch also leaves the widest frame in one word, read once (the only wait here).
    struct ValueRows { WindowValueFrame v; const uint32_t *lo, *hi; uint32_t* widest_dev; int64_t widest; };
    std::vector<ValueRows> value_frames;
    auto value_rows = [&](const WindowValueFrame& v) -> size_t {
        for (size_t k = 0; k < value_frames.size(); ++k)
            if (value_frames[k].v.units == v.units && same_bound(value_frames[k].v.start, v.start) && same_bound(value_frames[k].v.end, v.end)) return k;
        bool slides_here = false;
        for (const WindowFnDesc& g : fns_)
            slides_here = slides_here || (g.value.has && g.value.slides && g.value.units == v.units && same_bound(g.value.start, v.start) && same_bound(g.value.end, v.end));
        need_forward();
        need_backward();
        WindowValueFrameArgs a;
        memset(&a, 0, sizeof(a));
        a.units = v.units == BHIP_FRAME_UNITS_GROUPS ? WINDOW_UNITS_GROUPS : WINDOW_UNITS_RANGE;
        a.start_kind = v.start.kind;
        a.end_kind = v.end.kind;
        a.start_i = v.start.i; a.end_i = v.end.i;
        a.start_f = v.start.f; a.end_f = v.end.f;
        a.part_start = part_start; a.part_end = part_end; a.peer_start = peer_start; a.peer_end = peer_end;
        if (a.units == WINDOW_UNITS_GROUPS) a.peers_to = peers_to;
        else if (is_offset(v.start) || is_offset(v.end)) {          // (the constructor saw to exactly one order key of a type that has numbers)
            a.key = K.col[K.n_part];
            a.descending = order_by_[0].descending;
            a.nulls_first = order_by_[0].nulls_first;
        }
        uint32_t *lo = tmp.get<uint32_t>((size_t)n), *hi = tmp.get<uint32_t>((size_t)n), *widest = nullptr;
        if (slides_here) {
            widest = tmp.get<uint32_t>(1);
            HIP_CHECK(hipMemsetAsync(widest, 0, sizeof(uint32_t), ex.stream));
        }
        TIMED_LAUNCH_N(ex, "window_value_bounds", n, launch_window_value_bounds(cfg, a, n, lo, hi, widest));
        value_frames.push_back(ValueRows{v, lo, hi, widest, -1});
        return value_frames.size() - 1;
    };
    static_assert((int)BHIP_BOUND_UNBOUNDED == (int)WINDOW_BOUND_UNBOUNDED && (int)BHIP_BOUND_CURRENT_ROW == (int)WINDOW_BOUND_CURRENT_ROW &&
                      (int)BHIP_BOUND_OFFSET == (int)WINDOW_BOUND_OFFSET,
                  "the kernels take the ABI's bound kinds as they are");

    auto out = new_batch(sorted->ctx, schema_, n);
    out->cols = sorted->cols;
    for (const WindowFnDesc& f : fns_) {
        Column o;
        if (is_ranking(f.fn)) {
            need_forward();
            o = alloc_column(ex, DT_UINT64, n, false);
            const int kind = f.fn == BHIP_WIN_ROW_NUMBER ? WINDOW_ROW_NUMBER : f.fn == BHIP_WIN_RANK ? WINDOW_RANK : WINDOW_DENSE_RANK;
            TIMED_LAUNCH_N(ex, "window_rank", n, launch_window_rank(cfg, kind, part_start, peer_start, peers_to, n, o.data->as<uint64_t>()));
        } else if (!is_aggregate(f.fn) && f.rows.has) {
            // FIRST_VALUE / LAST_VALUE of a rows frame: lo / hi are the index vector (an empty frame: the NULL index)
            const FrameRows fr = frame_rows(f.rows);
            const uint32_t* idx = f.fn == BHIP_WIN_FIRST_VALUE ? fr.lo : fr.hi;
            const Column arg = evaluate_column(ex, *sorted, f.arg);
            const bool may_be_empty = (!fr.r.start_unbounded && f.rows.start > 0) || (!fr.r.end_unbounded && f.rows.end < 0);
            o = may_be_empty ? take_column_nullable(ex, arg, idx, n) : take_batch_column(ex, arg, idx, n);
        } else if (!is_aggregate(f.fn) && f.value.has) {
            // ... and of a RANGE / GROUPS frame
            const ValueRows& vr = value_frames[value_rows(f.value)];
            const uint32_t* idx = f.fn == BHIP_WIN_FIRST_VALUE ? vr.lo : vr.hi;
            const Column arg = evaluate_column(ex, *sorted, f.arg);
            const bool may_be_empty = offset_positive(f.value.start) || offset_negative(f.value.end);
            o = may_be_empty ? take_column_nullable(ex, arg, idx, n) : take_batch_column(ex, arg, idx, n);
        } else if (!is_aggregate(f.fn)) {
            // the row to read, then the gather the outer joins use (an index outside the partition is its NULL index)
            const uint32_t* fe = nullptr;
            int kind;
            switch (f.fn) {
                case BHIP_WIN_LAG: need_forward(); kind = WINDOW_LAG; break;
                case BHIP_WIN_LEAD: need_backward(); kind = WINDOW_LEAD; break;
                case BHIP_WIN_FIRST_VALUE: need_forward(); kind = WINDOW_FIRST; break;
                default: fe = frame_end(f.frame); kind = WINDOW_LAST; break;
            }
            BufferPtr idx = index_buffer(ex, n);
            TIMED_LAUNCH_N(ex, "window_index", n, launch_window_index(cfg, kind, f.offset, part_start, part_end, fe, n, idx->as<uint32_t>()));
            const Column arg = evaluate_column(ex, *sorted, f.arg);
            o = f.fn == BHIP_WIN_LAG || f.fn == BHIP_WIN_LEAD ? take_column_nullable(ex, arg, idx->as<uint32_t>(), n)
                                                              : take_batch_column(ex, arg, idx->as<uint32_t>(), n);
        } else {
            // COUNT of a non-NULL literal (COUNT(*)) reads no column at all
            const bool count_rows = f.fn == BHIP_WIN_COUNT && f.arg->kind == BHIP_EXPR_LITERAL && !f.arg->is_null;
            Column arg;
            if (!count_rows) arg = evaluate_column(ex, *sorted, f.arg);
            ColumnRef ref = arg.ref();
            const int t = count_rows ? DT_UINT8 : arg.dtype;
            int op, kind = WINDOW_FINISH_VALUE, dtype;
            switch (f.fn) {
                case BHIP_WIN_SUM: op = dt_is_float(t) ? WINDOW_OP_ADD_F64 : WINDOW_OP_ADD_I64; dtype = dt_is_float(t) ? DT_FLOAT64 : dt_is_unsigned(t) ? DT_UINT64 : DT_INT64; break;
                case BHIP_WIN_AVG: op = WINDOW_OP_ADD_F64; kind = WINDOW_FINISH_AVG; dtype = DT_FLOAT64; break;
                case BHIP_WIN_COUNT: op = WINDOW_OP_ADD_I64; kind = WINDOW_FINISH_COUNT; dtype = DT_UINT64; ref.data = nullptr; break;
                case BHIP_WIN_MIN: op = dt_is_float(t) ? WINDOW_OP_MIN_F64 : dt_is_unsigned(t) ? WINDOW_OP_MIN_U64 : WINDOW_OP_MIN_I64; dtype = t; break;
                default: op = dt_is_float(t) ? WINDOW_OP_MAX_F64 : dt_is_unsigned(t) ? WINDOW_OP_MAX_U64 : WINDOW_OP_MAX_I64; dtype = t; break;
            }
            if (kind != WINDOW_FINISH_COUNT && !ref.data) fail(BHIP_EEXEC, "WindowAggExec: an argument column without buffers");
            if (f.rows.has && !f.rows.start_unbounded && op != WINDOW_OP_ADD_I64) {
                // two finite ends (the constructor refused the rest): straight from the argument, no scan
                const FrameRows fr = frame_rows(f.rows);
                o = alloc_column(ex, dtype, n, true);
                TIMED_LAUNCH_N(ex, "window_slide", n,
                               launch_window_slide(cfg, op, kind, o.dtype, ref, fr.lo, fr.hi, fr.r.start, fr.r.end, n, o.data->ptr(), o.validity_words()));
                out->cols.push_back(std::move(o));
                continue;
            }
            if (f.value.has && f.value.start.kind != BHIP_BOUND_UNBOUNDED && op != WINDOW_OP_ADD_I64) {
                // the same over a RANGE / GROUPS frame, whose width is known only now
                ValueRows& vr = value_frames[value_rows(f.value)];
                if (vr.widest < 0) vr.widest = vr.widest_dev ? (int64_t)read_device(ex, vr.widest_dev) : 0;
                if (vr.widest > WINDOW_SLIDE_MAX_ROWS)
                    fail(BHIP_ENOTIMPL, std::string(window_fn_name(f.fn)) + "(" + dtype_name(t) + ") over " + value_frame_name(f.value) + ": the widest frame holds " +
                                            std::to_string(vr.widest) + " rows; a frame wider than " + std::to_string(WINDOW_SLIDE_MAX_ROWS) +
                                            " rows is supported for COUNT, integer SUM, FIRST_VALUE and LAST_VALUE only");
                o = alloc_column(ex, dtype, n, true);
                TIMED_LAUNCH_N(ex, "window_slide_value", n,
                               launch_window_slide_value(cfg, op, kind, o.dtype, ref, vr.lo, vr.hi, n, o.data->ptr(), o.validity_words()));
                out->cols.push_back(std::move(o));
                continue;
            }
            uint64_t* run_value = tmp.get<uint64_t>((size_t)n);
            uint32_t* run_count = tmp.get<uint32_t>((size_t)n);
            TIMED_LAUNCH_N(ex, "window_scan_tiles", n, launch_window_scan_tiles(cfg, op, ref, part_flags, n, scan_temp));
            TIMED_LAUNCH_N(ex, "window_scan_summaries", n, launch_window_scan_summaries(cfg, op, n, scan_temp));
            TIMED_LAUNCH_N(ex, "window_scan_apply", n, launch_window_scan_apply(cfg, op, ref, part_flags, n, scan_temp, run_value, run_count));
            o = alloc_column(ex, dtype, n, kind != WINDOW_FINISH_COUNT);
            if (f.rows.has) {
                // the running state at hi; COUNT and the wrapping SUM of a frame that starts at an offset: less the state before lo
                const FrameRows fr = frame_rows(f.rows);
                TIMED_LAUNCH_N(ex, "window_finish_frame", n,
                               launch_window_finish_frame(cfg, kind, o.dtype, run_value, run_count, fr.r.start_unbounded ? nullptr : part_flags, fr.lo, fr.hi,
                                                          n, o.data->ptr(), o.validity_words()));
            } else if (f.value.has) {
                const ValueRows& vr = value_frames[value_rows(f.value)];
                TIMED_LAUNCH_N(ex, "window_finish_frame", n,
                               launch_window_finish_frame(cfg, kind, o.dtype, run_value, run_count, f.value.start.kind == BHIP_BOUND_UNBOUNDED ? nullptr : part_flags,
                                                          vr.lo, vr.hi, n, o.data->ptr(), o.validity_words()));
            } else {
                const uint32_t* fe = frame_end(f.frame);
                TIMED_LAUNCH_N(ex, "window_finish", n,
                               launch_window_finish(cfg, kind, o.dtype, run_value, run_count, fe, n, o.data->ptr(), o.validity_words()));
            }
        }
        out->cols.push_back(std::move(o));
    }
    return out;                                                     // (no wait: scratch is released in stream order)
}

}  // namespace bhip
