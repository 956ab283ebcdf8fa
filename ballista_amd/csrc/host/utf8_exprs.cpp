// utf8_exprs.cpp — expressions that produce Utf8 values, as temporary columns.
//
// Reference: the serde ships lower / upper / trim / ltrim / rtrim (rust/core/src/serde/logical_plan/from_proto.rs:910-918),
// CASE with string branches (ballista.proto LogicalExprNode.case_) and string literals in projections.  DataFusion evaluates
// each as an arrow kernel producing a StringArray; here each such node becomes ONE extra Utf8 column of the input batch
// (kernels_str.hip: lengths -> scan -> bytes), and the expression around it — comparisons, LIKE, group / sort keys, the other
// output columns — goes to the expression VM with the node replaced by a reference to that column.
//
// CAST to and from Utf8 (kernels_cast.hip; the grammar: cast_text.h) takes the same road in both directions:
// CAST(x AS Utf8) of a fixed-width x is one more string-producing node, and CAST(<Utf8 expression> AS T) is an extra column too —
// of type T.  So a lowered node is "an expression evaluated as an extra column of its own type".
//
// concat is one more string-producing node; to_timestamp (Utf8 -> Timestamp(Nanosecond)) and date_trunc (Timestamp -> Timestamp)
// are lowered nodes of a fixed-width type, like CAST(<Utf8> AS T).  Over literals alone the two fold in the VM's compiler instead.
//
// substr / left / right are string-producing nodes too; char_length, strpos, starts_with and date_part are lowered nodes of type
// Int32 / Boolean.  Their rules are str_text.h and temporal_text.h; a call over literals alone folds by the same functions.
#include "../cast_kernels.h"
#include "../cast_text.h"
#include "../temporal_text.h"
#include "../str_kernels.h"
#include "../str_text.h"
#include "../util_kernels.h"
#include "plan.hpp"

namespace bhip {

// CAST(x AS Utf8), x of another type
static bool cast_to_utf8(const ExprPtr& e, const Schema& schema) {
    return e->kind == BHIP_EXPR_CAST && e->dtype == DT_UTF8 && expr_type(e->args[0], schema) != DT_UTF8;
}
// CAST(<Utf8 expression> AS T), T another type.  (A Utf8 literal folds in the VM's compiler instead: host/expr.cpp.)
static bool cast_from_utf8(const ExprPtr& e, const Schema& schema) {
    if (e->kind != BHIP_EXPR_CAST || e->dtype == DT_UTF8 || expr_type(e->args[0], schema) != DT_UTF8) return false;
    const Expr& x = *e->args[0];
    return !(x.kind == BHIP_EXPR_LITERAL && !x.is_null);
}

// to_timestamp(<Utf8 expression>) / date_trunc(g, <Timestamp expression>) / date_part(p, <temporal expression>) and
// char_length / strpos / starts_with: a fixed-width result evaluated as a column, unless the call folds to a literal
static bool typed_fn(const ExprPtr& e, const Schema& schema) {
    if (e->kind != BHIP_EXPR_SCALAR_FN) return false;
    if (e->name == "to_timestamp" || e->name == "date_trunc" || e->name == "date_part") return fold_temporal_literal(e, schema) == nullptr;
    return str_typed_fn(e->name) && fold_string_literal(e, schema) == nullptr;
}

static bool produces_utf8(const ExprPtr& e, const Schema& schema) {
    if (e->kind == BHIP_EXPR_SCALAR_FN) return str_fn(e->name) >= 0 || sha_fn(e->name) != 0 || e->name == "concat" || str_range_fn(e->name) >= 0;
    if (e->kind == BHIP_EXPR_CASE) return expr_type(e, schema) == DT_UTF8;
    return cast_to_utf8(e, schema);
}

bool has_lowered_node(const ExprPtr& e, const Schema& schema) {
    if (produces_utf8(e, schema) || cast_from_utf8(e, schema) || typed_fn(e, schema)) return true;
    for (auto& a : e->args)
        if (has_lowered_node(a, schema)) return true;
    return false;
}

static std::string cast_name(int from, int to) { return std::string("cast ") + dtype_name(from) + " -> " + dtype_name(to); }

Utf8Lowering::Utf8Lowering(const Schema& in) : in_(in) {}

ExprPtr Utf8Lowering::rewrite(const ExprPtr& e, bool output) {
    const bool lit = output && e->kind == BHIP_EXPR_LITERAL && e->dtype == DT_UTF8;
    if (lit || produces_utf8(e, in_) || cast_from_utf8(e, in_) || typed_fn(e, in_)) {
        const std::string text = e->to_string();
        for (size_t i = 0; i < nodes_.size(); ++i)
            if (nodes_[i]->to_string() == text) return make_column(names_[i]);
        nodes_.push_back(e);
        names_.push_back("__utf8_" + std::to_string(nodes_.size() - 1));
        if (in_.index_of(names_.back()) >= 0) fail(BHIP_EINVAL, "column name '" + names_.back() + "' is reserved");
        return make_column(names_.back());
    }
    if (e->args.empty()) return e;
    auto c = std::make_shared<Expr>(*e);
    for (auto& a : c->args) a = rewrite(a, false);
    return c;
}

SchemaPtr Utf8Lowering::schema() const {
    auto s = std::make_shared<Schema>(in_);
    for (size_t i = 0; i < nodes_.size(); ++i) s->fields.push_back(Field{names_[i], expr_type(nodes_[i], in_), expr_nullable(nodes_[i], in_)});
    return s;
}

namespace {

Column utf8_from_lengths(const Exec& ex, Temp& tmp, uint32_t* lengths, int64_t n, uint64_t** total_dev) {
    Column out;
    out.dtype = DT_UTF8;
    out.length = n;
    out.offsets = make_buffer(ex, (size_t)(n + 1) * 4);
    uint64_t* total = tmp.get<uint64_t>(1);
    void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n));
    HIP_CHECK(exclusive_scan_u32_i32(ex.stream, lengths, n, out.offsets->as<int32_t>(), true, total, scan_tmp));
    *total_dev = total;
    return out;
}

Column eval_utf8(const Exec& ex, const Batch& in, const ExprPtr& e);

Column eval_literal(const Exec& ex, const Expr& e, int64_t n) {
    Column out;
    out.dtype = DT_UTF8;
    out.length = n;
    out.offsets = make_buffer(ex, (size_t)(n + 1) * 4);
    if (e.is_null) {
        HIP_CHECK(hipMemsetAsync(out.offsets->ptr(), 0, (size_t)(n + 1) * 4, ex.stream));
        out.data = make_buffer(ex, 8);
        out.validity = make_buffer(ex, bitmap_bytes(n) + 8);
        HIP_CHECK(hipMemsetAsync(out.validity->ptr(), 0, bitmap_bytes(n) + 8, ex.stream));
        return out;
    }
    if (e.name.size() > (size_t)STR_LITERAL_MAX) fail(BHIP_ENOTIMPL, "Utf8 literal longer than 240 bytes as a column value");
    if ((uint64_t)n * e.name.size() > 0x7FFFFFFFull) fail(BHIP_EEXEC, "Utf8 column exceeds 2 GiB of value bytes");
    StrLiteral lit;
    lit.len = (int32_t)e.name.size();
    memcpy(lit.bytes, e.name.data(), e.name.size());
    out.data_bytes = n * lit.len;
    out.data = make_buffer(ex, (size_t)out.data_bytes + 8);
    TIMED_LAUNCH_N(ex, "str_broadcast", n, launch_str_broadcast(ex.cfg(), lit, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    out.offsets->set_uniform_width(n, lit.len);      // n copies of one value (an empty literal: width unknown, as for every 0)
    return out;
}

Column eval_transform(const Exec& ex, const Batch& in, const Expr& e) {
    const int kind = str_fn(e.name);
    const Column arg = eval_utf8(ex, in, e.args[0]);
    const int64_t n = in.n_rows;
    Temp tmp(ex);
    uint32_t* lengths = tmp.get<uint32_t>((size_t)n + 1);
    const ColumnRef cr = arg.ref();
    TIMED_LAUNCH_N(ex, "str_transform_lengths", n, launch_str_transform_lengths(ex.cfg(), kind, cr, n, lengths));
    uint64_t* total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, &total);
    // lower / upper keep the byte count, a trim can only shrink it: the argument's byte count bounds the result
    out.data = make_buffer(ex, (size_t)arg.data_bytes + 8);
    uint32_t* flags = tmp.get<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(flags, 0, 4, ex.stream));
    TIMED_LAUNCH_N(ex, "str_transform_write", n, launch_str_transform_write(ex.cfg(), kind, cr, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>(), flags));
    struct Back { uint64_t total; uint32_t flags, pad; };
    static_assert(sizeof(Back) == 16, "one read");
    Back* back = tmp.get<Back>(1);
    HIP_CHECK(hipMemcpyAsync(&back->total, total, 8, hipMemcpyDeviceToDevice, ex.stream));
    HIP_CHECK(hipMemcpyAsync(&back->flags, flags, 4, hipMemcpyDeviceToDevice, ex.stream));
    const Back b = read_device(ex, back);
    if (b.flags)
        fail(BHIP_ENOTIMPL, e.name + "() over text with non-ASCII characters (Unicode case mapping is not on the GPU path)");
    out.data_bytes = (int64_t)b.total;
    out.validity = arg.validity;
    return out;
}

// sha224 / sha256 / sha384 / sha512: fixed-length digests, one per row, NULL where the argument is
Column eval_sha(const Exec& ex, const Batch& in, const Expr& e) {
    const int bits = sha_fn(e.name);
    const Column arg = eval_utf8(ex, in, e.args[0]);
    const int64_t n = in.n_rows;
    if ((uint64_t)n * (bits / 8) > 0x7FFFFFFFull) fail(BHIP_EEXEC, "Binary column exceeds 2 GiB of value bytes");
    Column out;
    out.dtype = DT_UTF8;
    out.length = n;
    out.offsets = make_buffer(ex, (size_t)(n + 1) * 4);
    out.data_bytes = n * (bits / 8);
    out.data = make_buffer(ex, (size_t)out.data_bytes + 8);
    if (arg.validity) HIP_CHECK(hipMemsetAsync(out.data->ptr(), 0, (size_t)out.data_bytes + 8, ex.stream));    // a NULL row's bytes stay defined
    TIMED_LAUNCH_N(ex, "sha2", n, launch_sha2(ex.cfg(), bits, arg.ref(), n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    out.offsets->set_uniform_width(n, bits / 8);     // a digest per row, a NULL row's (zeroed) one included
    out.validity = arg.validity;
    return out;
}

Column eval_case(const Exec& ex, const Batch& in, const Expr& e) {
    const size_t fw = e.has_base ? 1 : 0;
    const size_t np = (e.args.size() - fw - (e.has_else ? 1 : 0)) / 2;
    if (np > (size_t)STR_SELECT_MAX) fail(BHIP_ENOTIMPL, "CASE producing Utf8 with more than 8 WHEN branches");
    const int64_t n = in.n_rows;
    // the conditions as Boolean columns, in one projection (they may hold string nodes of their own)
    std::vector<std::pair<ExprPtr, std::string>> conds;
    auto cs = std::make_shared<Schema>();
    for (size_t i = 0; i < np; ++i) {
        ExprPtr c = e.args[fw + 2 * i];
        if (e.has_base) c = make_binary(e.args[0], "Eq", c);
        if (expr_type(c, *in.schema) != DT_BOOLEAN) fail(BHIP_EINVAL, "CASE WHEN condition must be Boolean");
        conds.push_back({c, "c" + std::to_string(i)});
        cs->fields.push_back(Field{conds.back().second, DT_BOOLEAN, true});
    }
    BatchPtr cb = project_batch(ex, in, conds, cs);
    std::vector<Column> vals;
    for (size_t i = 0; i < np; ++i) vals.push_back(eval_utf8(ex, in, e.args[fw + 2 * i + 1]));
    if (e.has_else) vals.push_back(eval_utf8(ex, in, e.args.back()));
    StrSelectArgs A;
    memset(&A, 0, sizeof(A));
    A.n_when = (int32_t)np;
    A.has_else = e.has_else ? 1 : 0;
    for (size_t i = 0; i < np; ++i) A.cond[i] = cb->cols[i].ref();
    int64_t bound = 0;
    for (size_t i = 0; i < vals.size(); ++i) { A.val[i] = vals[i].ref(); bound += vals[i].data_bytes; }
    Temp tmp(ex);
    uint32_t* lengths = tmp.get<uint32_t>((size_t)n + 1);
    BufferPtr validity = make_buffer(ex, bitmap_bytes(n) + 8);
    TIMED_LAUNCH_N(ex, "str_select_lengths", n, launch_str_select_lengths(ex.cfg(), A, n, lengths, validity->as<uint64_t>()));
    uint64_t* total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, &total);
    // a row takes its value from ONE branch: the sum of the branches' byte counts bounds the result when it is small; else read it
    if (bound > (64 << 20)) bound = (int64_t)read_device(ex, total);
    out.data = make_buffer(ex, (size_t)bound + 8);
    TIMED_LAUNCH_N(ex, "str_select_write", n, launch_str_select_write(ex.cfg(), A, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    out.data_bytes = (int64_t)read_device(ex, total);
    out.validity = validity;
    return out;
}

// CAST(x AS Utf8): x as a temporary fixed-width column (any expression the VM evaluates, lowered nodes of its own included),
// then lengths -> scan -> bytes.  A literal is written on the host, by the same cast_format.
Column eval_cast_format(const Exec& ex, const Batch& in, const Expr& e) {
    const ExprPtr& x = e.args[0];
    const int from = expr_type(x, *in.schema);
    if (!cast_format_supported(from)) fail(BHIP_ENOTIMPL, cast_name(from, DT_UTF8));
    const int64_t n = in.n_rows;
    if (x->kind == BHIP_EXPR_LITERAL) {
        Expr lit;
        lit.kind = BHIP_EXPR_LITERAL;
        lit.dtype = DT_UTF8;
        uint8_t buf[CAST_TEXT_MAX];
        const int len = x->is_null ? -1 : cast_format(from, (uint64_t)x->i64, buf);
        lit.is_null = len < 0;
        if (len > 0) lit.name.assign(reinterpret_cast<const char*>(buf), (size_t)len);
        return eval_literal(ex, lit, n);
    }
    const Column arg = materialize_column(ex, evaluate_column(ex, in, x));
    const ColumnRef cr = arg.ref();
    Temp tmp(ex);
    uint32_t* lengths = tmp.get<uint32_t>((size_t)n + 1);
    // only a Date32 can have no text (outside 0000 .. 9999): every other result is NULL exactly where its argument is
    BufferPtr validity = from == DT_DATE32 ? make_buffer(ex, bitmap_bytes(n) + 8) : nullptr;
    TIMED_LAUNCH_N(ex, "cast_format_lengths", n, launch_cast_format_lengths(ex.cfg(), cr, n, lengths, validity ? validity->as<uint64_t>() : nullptr));
    uint64_t* total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, &total);
    // the longest text of the type bounds the result when that is small; else read the total first
    int64_t bound = n * cast_format_max(from);
    if (bound > (64 << 20)) bound = (int64_t)read_device(ex, total);
    if ((uint64_t)bound > 0x7FFFFFFFull) fail(BHIP_EEXEC, "Utf8 column exceeds 2 GiB of value bytes");
    out.data = make_buffer(ex, (size_t)bound + 8);
    TIMED_LAUNCH_N(ex, "cast_format_write", n, launch_cast_format_write(ex.cfg(), cr, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    out.data_bytes = (int64_t)read_device(ex, total);
    out.validity = validity ? validity : arg.validity;
    return out;
}

// CAST(<Utf8 expression> AS T): one thread per row parses its value; the result is nullable whatever the argument is
Column eval_cast_parse(const Exec& ex, const Batch& in, const Expr& e) {
    const int to = e.dtype;
    if (!cast_parse_supported(to)) fail(BHIP_ENOTIMPL, cast_name(DT_UTF8, to));
    const Column arg = eval_utf8(ex, in, e.args[0]);
    const int64_t n = in.n_rows;
    Column out;
    out.dtype = to;
    out.length = n;
    out.data = make_buffer(ex, (to == DT_BOOLEAN ? bitmap_bytes(n) : (size_t)n * dtype_width(to)) + 8);
    out.validity = make_buffer(ex, bitmap_bytes(n) + 8);
    Temp tmp(ex);
    uint32_t* status = tmp.get<uint32_t>(1);
    const bool can_decline = dt_is_float(to);
    if (can_decline) HIP_CHECK(hipMemsetAsync(status, 0, 4, ex.stream));
    TIMED_LAUNCH_N(ex, "cast_parse", n, launch_cast_parse(ex.cfg(), arg.ref(), n, to, out.data->ptr(), out.validity->as<uint64_t>(), status));
    // integer, Boolean and Date32 targets cannot decline: handed on in stream order, no host wait
    if (can_decline && (read_device(ex, status) & CAST_STATUS_DECLINED))
        fail(BHIP_ENOTIMPL, cast_name(DT_UTF8, to) + ": a value outside the exactly rounded range (more than 15 significant digits, or a "
                            "power of ten beyond 10^22) is not converted on the GPU path");
    return out;
}

// concat(a1, ..., ak): lengths -> scan -> bytes.  Short literal arguments travel in the kernels' argument struct; a literal that does
// not fit there becomes a column first, and a NULL literal makes every row NULL.
Column eval_concat(const Exec& ex, const Batch& in, const Expr& e) {
    const int64_t n = in.n_rows;
    if (e.args.size() > (size_t)STR_CONCAT_MAX) fail(BHIP_ENOTIMPL, "concat with more than 8 arguments");
    for (auto& a : e.args)
        if (a->kind == BHIP_EXPR_LITERAL && a->is_null) return eval_literal(ex, *a, n);
    StrConcatArgs A;
    memset(&A, 0, sizeof(A));
    A.n_args = (int32_t)e.args.size();
    std::vector<Column> cols(e.args.size());
    int64_t bound = 0;
    int32_t lit_used = 0;
    bool any_validity = false;
    for (size_t j = 0; j < e.args.size(); ++j) {
        const Expr& a = *e.args[j];
        if (a.kind == BHIP_EXPR_LITERAL && a.dtype == DT_UTF8 && lit_used + (int64_t)a.name.size() <= STR_CONCAT_LIT_BYTES) {
            A.is_lit[j] = 1;
            A.lit_off[j] = lit_used;
            A.lit_len[j] = (int32_t)a.name.size();
            memcpy(A.lit_bytes + lit_used, a.name.data(), a.name.size());
            lit_used += A.lit_len[j];
            bound += n * A.lit_len[j];
            continue;
        }
        cols[j] = eval_utf8(ex, in, e.args[j]);
        A.col[j] = cols[j].ref();
        bound += cols[j].data_bytes;
        any_validity = any_validity || (bool)cols[j].validity;
    }
    Temp tmp(ex);
    uint32_t* lengths = tmp.get<uint32_t>((size_t)n + 1);
    BufferPtr validity = any_validity ? make_buffer(ex, bitmap_bytes(n) + 8) : nullptr;
    TIMED_LAUNCH_N(ex, "concat_lengths", n, launch_concat_lengths(ex.cfg(), A, n, lengths, validity ? validity->as<uint64_t>() : nullptr));
    uint64_t* total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, &total);
    // a row holds every argument's bytes: the sum of their byte counts bounds the result when it is small; else read the total
    int64_t total_bytes = -1;
    if (bound > (64 << 20)) bound = total_bytes = (int64_t)read_device(ex, total);
    if ((uint64_t)bound > 0x7FFFFFFFull) fail(BHIP_EEXEC, "Utf8 column exceeds 2 GiB of value bytes");
    out.data = make_buffer(ex, (size_t)bound + 8);
    TIMED_LAUNCH_N(ex, "concat_write", n, launch_concat_write(ex.cfg(), A, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    out.data_bytes = total_bytes >= 0 ? total_bytes : (int64_t)read_device(ex, total);
    out.validity = validity;
    return out;
}

// to_timestamp(<Utf8 expression>): one thread per row parses its value; NULL exactly where the argument is, and a non-NULL value
// that is no timestamp fails the batch
Column eval_to_timestamp(const Exec& ex, const Batch& in, const Expr& e) {
    const Column arg = eval_utf8(ex, in, e.args[0]);
    const int64_t n = in.n_rows;
    Column out;
    out.dtype = DT_TIMESTAMP_NS;
    out.length = n;
    out.data = make_buffer(ex, (size_t)n * 8 + 8);
    out.validity = arg.validity;
    Temp tmp(ex);
    uint32_t* status = tmp.get<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(status, 0, 4, ex.stream));
    TIMED_LAUNCH_N(ex, "to_timestamp_parse", n, launch_to_timestamp_parse(ex.cfg(), arg.ref(), n, out.data->as<int64_t>(), status));
    if (read_device(ex, status) & TO_TIMESTAMP_STATUS_INVALID)
        fail(BHIP_EEXEC, "to_timestamp: a value is not a timestamp (YYYY-MM-DD[T ]hh:mm:ss[.fraction][Z|+hh:mm] within the range of "
                         "Timestamp(Nanosecond))");
    return out;
}

// date_trunc(g, t): t as a temporary column (any expression the VM evaluates, lowered nodes of its own included), then one streaming kernel
Column eval_date_trunc(const Exec& ex, const Batch& in, const Expr& e) {
    const int gran = date_trunc_granularity(e, *in.schema);
    const Column arg = materialize_column(ex, evaluate_column(ex, in, e.args[1]));
    const int64_t n = in.n_rows;
    Column out;
    out.dtype = arg.dtype;
    out.length = n;
    out.data = make_buffer(ex, (size_t)n * 8 + 8);
    out.validity = make_buffer(ex, bitmap_bytes(n) + 8);
    TIMED_LAUNCH_N(ex, "date_trunc", n, launch_date_trunc(ex.cfg(), arg.ref(), n, gran, out.data->as<int64_t>(), out.validity->as<uint64_t>()));
    return out;
}

// an integer argument of substr / left / right: a literal travels in the struct, anything else is evaluated as an Int64 column
// (kept alive in `keep`)
StrIntArg int_argument(const Exec& ex, const Batch& in, const ExprPtr& a, std::vector<Column>& keep, bool& any_validity) {
    StrIntArg r;
    memset(&r, 0, sizeof(r));
    if (a->kind == BHIP_EXPR_LITERAL) {
        r.is_lit = 1;
        r.lit = a->i64;
        return r;
    }
    keep.push_back(materialize_column(ex, evaluate_column(ex, in, a)));
    if (keep.back().dtype != DT_INT64) fail(BHIP_EINVAL, "expected an Int64 argument: " + a->to_string());
    r.col = keep.back().ref();
    any_validity = any_validity || (bool)keep.back().validity;
    return r;
}

// substr(s, start[, count]) / left(s, n) / right(s, n): lengths -> scan -> bytes; the result is a byte range of the argument, so the
// argument's byte count bounds it.  One status word says that a row asked for a negative count.
Column eval_str_range(const Exec& ex, const Batch& in, const ExprPtr& ep) {
    const Expr& e = *ep;
    const int64_t n = in.n_rows;
    if (const ExprPtr l = fold_string_literal(ep, *in.schema)) return eval_literal(ex, *l, n);       // (it checks the call as well)
    const Column arg = eval_utf8(ex, in, e.args[0]);
    std::vector<Column> ints;
    bool any_validity = (bool)arg.validity;
    StrRangeArgs A;
    memset(&A, 0, sizeof(A));
    A.fn = str_range_fn(e.name);
    A.has_count = e.args.size() == 3 ? 1 : 0;
    A.s = arg.ref();
    A.a = int_argument(ex, in, e.args[1], ints, any_validity);
    if (A.has_count) A.b = int_argument(ex, in, e.args[2], ints, any_validity);
    Temp tmp(ex);
    uint32_t* lengths = tmp.get<uint32_t>((size_t)n + 1);
    uint32_t* status = tmp.get<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(status, 0, 4, ex.stream));
    BufferPtr validity = any_validity ? make_buffer(ex, bitmap_bytes(n) + 8) : nullptr;
    TIMED_LAUNCH_N(ex, "str_range_lengths", n, launch_str_range_lengths(ex.cfg(), A, n, lengths, validity ? validity->as<uint64_t>() : nullptr, status));
    uint64_t* total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, &total);
    out.data = make_buffer(ex, (size_t)arg.data_bytes + 8);
    TIMED_LAUNCH_N(ex, "str_range_write", n, launch_str_range_write(ex.cfg(), A, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    struct Back { uint64_t total; uint32_t status, pad; };
    static_assert(sizeof(Back) == 16, "one read");
    Back* back = tmp.get<Back>(1);
    HIP_CHECK(hipMemcpyAsync(&back->total, total, 8, hipMemcpyDeviceToDevice, ex.stream));
    HIP_CHECK(hipMemcpyAsync(&back->status, status, 4, hipMemcpyDeviceToDevice, ex.stream));
    const Back b = read_device(ex, back);
    if (b.status & STR_RANGE_STATUS_NEGATIVE) fail(BHIP_EEXEC, "negative substring length not allowed");
    out.data_bytes = (int64_t)b.total;
    out.validity = validity;
    return out;
}

// char_length(<Utf8 expression>): one thread per row counts its code points; NULL exactly where the argument is
Column eval_char_length(const Exec& ex, const Batch& in, const Expr& e) {
    const Column arg = eval_utf8(ex, in, e.args[0]);
    const int64_t n = in.n_rows;
    Column out;
    out.dtype = DT_INT32;
    out.length = n;
    out.data = make_buffer(ex, (size_t)n * 4 + 8);
    out.validity = arg.validity;
    TIMED_LAUNCH_N(ex, "char_length", n, launch_char_length(ex.cfg(), arg.ref(), n, out.data->as<int32_t>()));
    return out;
}

// strpos(s, sub) -> Int32 / starts_with(s, prefix) -> Boolean: the second argument a literal in the struct, or a column
Column eval_str_search(const Exec& ex, const Batch& in, const Expr& e) {
    const bool pos = e.name == "strpos";
    const Column arg = eval_utf8(ex, in, e.args[0]);
    const int64_t n = in.n_rows;
    StrSearchArgs A;
    memset(&A, 0, sizeof(A));
    A.s = arg.ref();
    Column sub;
    const Expr& x = *e.args[1];
    if (x.kind == BHIP_EXPR_LITERAL) {
        A.sub_is_lit = 1;
        A.lit.len = (int32_t)x.name.size();
        memcpy(A.lit.bytes, x.name.data(), x.name.size());
    } else {
        sub = eval_utf8(ex, in, e.args[1]);
        A.sub = sub.ref();
    }
    Column out;
    out.dtype = pos ? DT_INT32 : DT_BOOLEAN;
    out.length = n;
    out.data = make_buffer(ex, (pos ? (size_t)n * 4 : bitmap_bytes(n)) + 8);
    if (arg.validity || sub.validity) out.validity = make_buffer(ex, bitmap_bytes(n) + 8);
    uint64_t* validity = out.validity ? out.validity->as<uint64_t>() : nullptr;
    if (pos) TIMED_LAUNCH_N(ex, "strpos", n, launch_strpos(ex.cfg(), A, n, out.data->as<int32_t>(), validity));
    else TIMED_LAUNCH_N(ex, "starts_with", n, launch_starts_with(ex.cfg(), A, n, out.data->as<uint64_t>(), validity));
    return out;
}

// date_part(p, x): x as a temporary column, then one streaming kernel, as date_trunc
Column eval_date_part(const Exec& ex, const Batch& in, const Expr& e) {
    const int part = date_part_of(e, *in.schema);
    const Column arg = materialize_column(ex, evaluate_column(ex, in, e.args[1]));
    const int64_t n = in.n_rows;
    Column out;
    out.dtype = DT_INT32;
    out.length = n;
    out.data = make_buffer(ex, (size_t)n * 4 + 8);
    out.validity = make_buffer(ex, bitmap_bytes(n) + 8);
    TIMED_LAUNCH_N(ex, "date_part", n, launch_date_part(ex.cfg(), arg.ref(), n, part, out.data->as<int32_t>(), out.validity->as<uint64_t>()));
    return out;
}

Column eval_utf8(const Exec& ex, const Batch& in, const ExprPtr& e) {
    switch (e->kind) {
        case BHIP_EXPR_COLUMN: {
            const int i = in.schema->index_of(e->name);
            if (i < 0) fail(BHIP_EINVAL, "No field named '" + e->name + "'");
            if (in.cols[i].dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 column: " + e->name);
            return in.cols[i];
        }
        case BHIP_EXPR_LITERAL:
            if (e->dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 literal");
            return eval_literal(ex, *e, in.n_rows);
        case BHIP_EXPR_SCALAR_FN:
            if (str_fn(e->name) >= 0) return eval_transform(ex, in, *e);
            if (sha_fn(e->name)) return eval_sha(ex, in, *e);
            if (e->name == "concat") return eval_concat(ex, in, *e);
            if (str_range_fn(e->name) >= 0) return eval_str_range(ex, in, e);
            break;
        case BHIP_EXPR_CASE: return eval_case(ex, in, *e);
        case BHIP_EXPR_CAST:
            if (e->dtype != DT_UTF8) break;
            if (expr_type(e->args[0], *in.schema) == DT_UTF8) return eval_utf8(ex, in, e->args[0]);
            return eval_cast_format(ex, in, *e);
        default: break;
    }
    fail(BHIP_ENOTIMPL, "expression producing Utf8: " + e->to_string());
}

}  // namespace

BatchPtr Utf8Lowering::apply(const Exec& ex, const Batch& in) const {
    auto out = std::make_shared<Batch>(in);
    out->schema = schema();
    for (auto& node : nodes_) {
        const int t = expr_type(node, in_);
        if (in.n_rows == 0) {
            Column c;
            c.dtype = t;
            if (t == DT_UTF8) {
                c.offsets = make_buffer(ex, 8);
                HIP_CHECK(hipMemsetAsync(c.offsets->ptr(), 0, 8, ex.stream));
            }
            c.data = make_buffer(ex, 8);
            out->cols.push_back(c);
        } else {
            if (t == DT_UTF8) out->cols.push_back(eval_utf8(ex, in, node));
            else if (node->kind == BHIP_EXPR_CAST) out->cols.push_back(eval_cast_parse(ex, in, *node));
            else if (node->name == "to_timestamp") out->cols.push_back(eval_to_timestamp(ex, in, *node));
            else if (node->name == "date_trunc") out->cols.push_back(eval_date_trunc(ex, in, *node));
            else if (node->name == "date_part") out->cols.push_back(eval_date_part(ex, in, *node));
            else if (node->name == "char_length") out->cols.push_back(eval_char_length(ex, in, *node));
            else out->cols.push_back(eval_str_search(ex, in, *node));
        }
    }
    return out;
}

// plan-time check: every string node is one this file evaluates (BHIP_ENOTIMPL otherwise, before anything runs)
void Utf8Lowering::validate() const {
    // an argument that is a projection of its own (evaluate_column): its lowered nodes and its VM program are checked as ProjectionExec does
    auto check_projected = [&](const ExprPtr& x) {
        Utf8Lowering inner(in_);
        const ExprPtr lowered = inner.rewrite(x, true);
        inner.validate();
        const SchemaPtr aug = inner.schema();
        ProgramBuilder pb(*aug);
        if (lowered->kind != BHIP_EXPR_COLUMN) pb.add_output(lowered);
    };
    std::function<void(const ExprPtr&)> walk = [&](const ExprPtr& e) {
        switch (e->kind) {
            case BHIP_EXPR_COLUMN: {
                const int i = in_.index_of(e->name);
                if (i < 0) fail(BHIP_EINVAL, "No field named '" + e->name + "'");
                if (in_.fields[i].dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 column: " + e->name);
            } break;
            case BHIP_EXPR_LITERAL:
                if (e->dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 literal");
                break;
            case BHIP_EXPR_SCALAR_FN:
                if (e->name == "concat") {
                    if (e->args.size() > (size_t)STR_CONCAT_MAX) fail(BHIP_ENOTIMPL, "concat with more than 8 arguments");
                    for (auto& a : e->args) {
                        const int t = expr_type(a, in_);
                        if (t != DT_UTF8) fail(BHIP_EINVAL, std::string("concat requires Utf8 arguments, not ") + dtype_name(t));
                        walk(a);
                    }
                    break;
                }
                if (str_range_fn(e->name) >= 0) {
                    check_string_fn(*e, in_);
                    walk(e->args[0]);
                    for (size_t k = 1; k < e->args.size(); ++k)
                        if (e->args[k]->kind != BHIP_EXPR_LITERAL) check_projected(e->args[k]);
                    break;
                }
                if (str_fn(e->name) < 0 && !sha_fn(e->name)) fail(BHIP_ENOTIMPL, "expression producing Utf8: " + e->to_string());
                walk(e->args[0]);
                break;
            case BHIP_EXPR_CASE: {
                const size_t fw = e->has_base ? 1 : 0;
                const size_t np = (e->args.size() - fw - (e->has_else ? 1 : 0)) / 2;
                if (np > (size_t)STR_SELECT_MAX) fail(BHIP_ENOTIMPL, "CASE producing Utf8 with more than 8 WHEN branches");
                for (size_t i = 0; i < np; ++i) walk(e->args[fw + 2 * i + 1]);
                if (e->has_else) walk(e->args.back());
            } break;
            case BHIP_EXPR_CAST: {
                if (e->dtype != DT_UTF8) fail(BHIP_ENOTIMPL, "expression producing Utf8: " + e->to_string());
                const ExprPtr& x = e->args[0];
                const int from = expr_type(x, in_);
                if (from == DT_UTF8) { walk(x); break; }
                if (!cast_format_supported(from)) fail(BHIP_ENOTIMPL, cast_name(from, DT_UTF8));
                check_projected(x);
            } break;
            default: fail(BHIP_ENOTIMPL, "expression producing Utf8: " + e->to_string());
        }
    };
    for (auto& n : nodes_) {
        if (expr_type(n, in_) == DT_UTF8) { walk(n); continue; }
        if (n->kind == BHIP_EXPR_SCALAR_FN && n->name == "date_trunc") {
            (void)date_trunc_granularity(*n, in_);
            check_projected(n->args[1]);
            continue;
        }
        if (n->kind == BHIP_EXPR_SCALAR_FN && n->name == "date_part") {
            (void)date_part_of(*n, in_);
            check_projected(n->args[1]);
            continue;
        }
        if (n->kind == BHIP_EXPR_SCALAR_FN && str_typed_fn(n->name)) {
            check_string_fn(*n, in_);
            for (auto& a : n->args) walk(a);
            continue;
        }
        if (n->kind == BHIP_EXPR_SCALAR_FN) {          // to_timestamp
            if (expr_type(n->args[0], in_) != DT_UTF8) fail(BHIP_EINVAL, std::string("to_timestamp requires a Utf8 argument, not ") + dtype_name(expr_type(n->args[0], in_)));
            walk(n->args[0]);
            continue;
        }
        if (!cast_parse_supported(n->dtype)) fail(BHIP_ENOTIMPL, cast_name(DT_UTF8, n->dtype));
        walk(n->args[0]);
    }
}

}  // namespace bhip
