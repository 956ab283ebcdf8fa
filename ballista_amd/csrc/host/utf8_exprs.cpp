// utf8_exprs.cpp — expressions that produce Utf8 values, as temporary columns; and the table of scalar functions.
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
// What evaluates a lowered node is a ScalarFn row (expr.hpp): a row of SCALAR_FNS at the end of this file for a scalar function, one of
// the three rows beside it for CASE and the two CASTs.  A row holds the node's plan-time check and its evaluator, so what validate()
// accepts is what apply() evaluates.  The functions of a fixed-width type (to_timestamp, date_trunc, date_part, char_length, strpos,
// starts_with) fold in the VM's compiler instead when they stand over literals alone; their rules are str_text.h and temporal_text.h.
#include "../cast_kernels.h"
#include "../cast_text.h"
#include "../temporal_text.h"
#include "../str_kernels.h"
#include "../str_text.h"
#include "../util_kernels.h"
#include "plan.hpp"

namespace bhip {

namespace {

// the row that evaluates `e` as a column of its own; null where the VM evaluates `e` (or its compiler folds it to a literal)
const ScalarFn* lowered_by(const ExprPtr& e, const Schema& schema);
Column eval_utf8(const Exec& ex, const Batch& in, const ExprPtr& e);
void check_utf8(const ExprPtr& e, const Schema& in);

std::string cast_name(int from, int to) { return std::string("cast ") + dtype_name(from) + " -> " + dtype_name(to); }

// ---- plan-time checks: every lowered node is one this file evaluates (before anything runs) -----------------------------------------

// an argument that is a projection of its own (evaluate_column): its lowered nodes and its VM program are checked as ProjectionExec does
void check_projected(const ExprPtr& x, const Schema& in) {
    Utf8Lowering inner(in);
    const ExprPtr lowered = inner.rewrite(x, true);
    inner.validate();
    const SchemaPtr aug = inner.schema();
    ProgramBuilder pb(*aug);
    if (lowered->kind != BHIP_EXPR_COLUMN) pb.add_output(lowered);
}

// Utf8 arguments alone: lower .. rtrim, sha224 .. sha512; char_length, strpos, starts_with
void validate_strings(const ExprPtr& e, const Schema& in, const ScalarFn& f) {
    if (f.check) (void)f.check(*e, in);
    for (auto& a : e->args) check_utf8(a, in);
}

void validate_concat(const ExprPtr& e, const Schema& in, const ScalarFn&) {
    for (auto& a : e->args) {
        const int t = expr_type(a, in);
        if (t != DT_UTF8) fail(BHIP_EINVAL, std::string("concat requires Utf8 arguments, not ") + dtype_name(t));
        check_utf8(a, in);
    }
}

void validate_str_range(const ExprPtr& e, const Schema& in, const ScalarFn& f) {
    (void)f.check(*e, in);
    check_utf8(e->args[0], in);
    for (size_t k = 1; k < e->args.size(); ++k)
        if (e->args[k]->kind != BHIP_EXPR_LITERAL) check_projected(e->args[k], in);
}

void validate_to_timestamp(const ExprPtr& e, const Schema& in, const ScalarFn&) {
    const int t = expr_type(e->args[0], in);
    if (t != DT_UTF8) fail(BHIP_EINVAL, std::string("to_timestamp requires a Utf8 argument, not ") + dtype_name(t));
    check_utf8(e->args[0], in);
}

// date_trunc(g, t), date_part(p, x): the first argument is the literal that `check` reads
void validate_temporal(const ExprPtr& e, const Schema& in, const ScalarFn& f) {
    (void)f.check(*e, in);
    check_projected(e->args[1], in);
}

// WHEN branches of a CASE that produces Utf8
size_t case_branches(const Expr& e) {
    const size_t np = (e.args.size() - (e.has_base ? 1 : 0) - (e.has_else ? 1 : 0)) / 2;
    if (np > (size_t)STR_SELECT_MAX) fail(BHIP_ENOTIMPL, "CASE producing Utf8 with more than " + std::to_string(STR_SELECT_MAX) + " WHEN branches");
    return np;
}

void validate_case(const ExprPtr& e, const Schema& in, const ScalarFn&) {
    const size_t fw = e->has_base ? 1 : 0, np = case_branches(*e);
    for (size_t i = 0; i < np; ++i) check_utf8(e->args[fw + 2 * i + 1], in);
    if (e->has_else) check_utf8(e->args.back(), in);
}

void validate_cast_format(const ExprPtr& e, const Schema& in, const ScalarFn&) {
    const int from = expr_type(e->args[0], in);
    if (!cast_format_supported(from)) fail(BHIP_ENOTIMPL, cast_name(from, DT_UTF8));
    check_projected(e->args[0], in);
}

void validate_cast_parse(const ExprPtr& e, const Schema& in, const ScalarFn&) {
    if (!cast_parse_supported(e->dtype)) fail(BHIP_ENOTIMPL, cast_name(DT_UTF8, e->dtype));
    check_utf8(e->args[0], in);
}

// ---- evaluators ----------------------------------------------------------------------------------------------------------------------

Column eval_literal(const Exec& ex, const Expr& e, int64_t n) {
    if (e.is_null) return null_column(ex, DT_UTF8, n);
    if (e.name.size() > (size_t)STR_LITERAL_MAX) fail(BHIP_ENOTIMPL, "Utf8 literal longer than " + std::to_string(STR_LITERAL_MAX) + " bytes as a column value");
    StrLiteral lit;
    lit.len = (int32_t)e.name.size();
    memcpy(lit.bytes, e.name.data(), e.name.size());
    Column out = alloc_column(ex, DT_UTF8, n, false, n * lit.len);
    TIMED_LAUNCH_N(ex, "str_broadcast", n, launch_str_broadcast(ex.cfg(), lit, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    out.offsets->set_uniform_width(n, lit.len);      // n copies of one value (an empty literal: width unknown, as for every 0)
    return out;
}

Column eval_transform(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn& f) {
    const Column arg = eval_utf8(ex, in, e->args[0]);
    const int64_t n = in.n_rows;
    Temp tmp(ex);
    uint32_t* lengths = tmp.get<uint32_t>((size_t)n + 1);
    const ColumnRef cr = arg.ref();
    TIMED_LAUNCH_N(ex, "str_transform_lengths", n, launch_str_transform_lengths(ex.cfg(), f.param, cr, n, lengths));
    Utf8Total total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, total);
    // lower / upper keep the byte count, a trim can only shrink it: the argument's byte count bounds the result, and it is a column's own
    utf8_alloc_data(ex, out, arg.data_bytes);
    uint32_t* flags = tmp.get<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(flags, 0, 4, ex.stream));
    TIMED_LAUNCH_N(ex, "str_transform_write", n, launch_str_transform_write(ex.cfg(), f.param, cr, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>(), flags));
    if (utf8_read_total(ex, tmp, out, total, flags))
        fail(BHIP_ENOTIMPL, e->name + "() over text with non-ASCII characters (Unicode case mapping is not on the GPU path)");
    out.validity = arg.validity;
    return out;
}

// sha224 / sha256 / sha384 / sha512: fixed-length digests, one per row, NULL where the argument is
Column eval_sha(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn& f) {
    const int bits = f.param;
    const Column arg = eval_utf8(ex, in, e->args[0]);
    const int64_t n = in.n_rows;
    if ((uint64_t)n * (bits / 8) > 0x7FFFFFFFull) fail(BHIP_EEXEC, "Binary column exceeds 2 GiB of value bytes");
    Column out = alloc_column(ex, DT_UTF8, n, false, n * (bits / 8));
    if (arg.validity) HIP_CHECK(hipMemsetAsync(out.data->ptr(), 0, out.data->bytes(), ex.stream));    // a NULL row's bytes stay defined
    TIMED_LAUNCH_N(ex, "sha2", n, launch_sha2(ex.cfg(), bits, arg.ref(), n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    out.offsets->set_uniform_width(n, bits / 8);     // a digest per row, a NULL row's (zeroed) one included
    out.validity = arg.validity;
    return out;
}

Column eval_case(const Exec& ex, const Batch& in, const ExprPtr& ep, const ScalarFn&) {
    const Expr& e = *ep;
    const size_t fw = e.has_base ? 1 : 0, np = case_branches(e);
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
    BufferPtr validity = validity_buffer(ex, n);
    TIMED_LAUNCH_N(ex, "str_select_lengths", n, launch_str_select_lengths(ex.cfg(), A, n, lengths, validity->as<uint64_t>()));
    Utf8Total total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, total);
    utf8_size_data(ex, out, bound, total);           // a row takes its value from ONE branch: the sum of the branches' byte counts bounds it
    TIMED_LAUNCH_N(ex, "str_select_write", n, launch_str_select_write(ex.cfg(), A, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    utf8_read_total(ex, tmp, out, total);
    out.validity = validity;
    return out;
}

// CAST(x AS Utf8): x as a temporary fixed-width column (any expression the VM evaluates, lowered nodes of its own included),
// then lengths -> scan -> bytes.  A literal is written on the host, by the same cast_format.
Column eval_cast_format(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn&) {
    const ExprPtr& x = e->args[0];
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
    BufferPtr validity = from == DT_DATE32 ? validity_buffer(ex, n) : nullptr;
    TIMED_LAUNCH_N(ex, "cast_format_lengths", n, launch_cast_format_lengths(ex.cfg(), cr, n, lengths, validity ? validity->as<uint64_t>() : nullptr));
    Utf8Total total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, total);
    utf8_size_data(ex, out, n * cast_format_max(from), total);       // the longest text of the type bounds the result
    TIMED_LAUNCH_N(ex, "cast_format_write", n, launch_cast_format_write(ex.cfg(), cr, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    utf8_read_total(ex, tmp, out, total);
    out.validity = validity ? validity : arg.validity;
    return out;
}

// CAST(<Utf8 expression> AS T): one thread per row parses its value; the result is nullable whatever the argument is
Column eval_cast_parse(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn&) {
    const int to = e->dtype;
    if (!cast_parse_supported(to)) fail(BHIP_ENOTIMPL, cast_name(DT_UTF8, to));
    const Column arg = eval_utf8(ex, in, e->args[0]);
    const int64_t n = in.n_rows;
    Column out = alloc_column(ex, to, n, true);
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
Column eval_concat(const Exec& ex, const Batch& in, const ExprPtr& ep, const ScalarFn&) {
    const Expr& e = *ep;
    const int64_t n = in.n_rows;
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
    BufferPtr validity = any_validity ? validity_buffer(ex, n) : nullptr;
    TIMED_LAUNCH_N(ex, "concat_lengths", n, launch_concat_lengths(ex.cfg(), A, n, lengths, validity ? validity->as<uint64_t>() : nullptr));
    Utf8Total total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, total);
    utf8_size_data(ex, out, bound, total);           // a row holds every argument's bytes: the sum of their byte counts bounds the result
    TIMED_LAUNCH_N(ex, "concat_write", n, launch_concat_write(ex.cfg(), A, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    utf8_read_total(ex, tmp, out, total);
    out.validity = validity;
    return out;
}

// to_timestamp(<Utf8 expression>): one thread per row parses its value; NULL exactly where the argument is, and a non-NULL value
// that is no timestamp fails the batch
Column eval_to_timestamp(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn&) {
    const Column arg = eval_utf8(ex, in, e->args[0]);
    const int64_t n = in.n_rows;
    Column out = alloc_column(ex, DT_TIMESTAMP_NS, n, false);
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
Column eval_date_trunc(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn& f) {
    const int gran = f.check(*e, *in.schema);
    const Column arg = materialize_column(ex, evaluate_column(ex, in, e->args[1]));
    const int64_t n = in.n_rows;
    Column out = alloc_column(ex, arg.dtype, n, true);
    TIMED_LAUNCH_N(ex, "date_trunc", n, launch_date_trunc(ex.cfg(), arg.ref(), n, gran, out.data->as<int64_t>(), out.validity->as<uint64_t>()));
    return out;
}

// date_part(p, x): x as a temporary column, then one streaming kernel, as date_trunc
Column eval_date_part(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn& f) {
    const int part = f.check(*e, *in.schema);
    const Column arg = materialize_column(ex, evaluate_column(ex, in, e->args[1]));
    const int64_t n = in.n_rows;
    Column out = alloc_column(ex, DT_INT32, n, true);
    TIMED_LAUNCH_N(ex, "date_part", n, launch_date_part(ex.cfg(), arg.ref(), n, part, out.data->as<int32_t>(), out.validity->as<uint64_t>()));
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
Column eval_str_range(const Exec& ex, const Batch& in, const ExprPtr& ep, const ScalarFn& f) {
    const Expr& e = *ep;
    const int64_t n = in.n_rows;
    if (const ExprPtr l = f.fold(ep, *in.schema)) return eval_literal(ex, *l, n);       // (it checks the call as well)
    const Column arg = eval_utf8(ex, in, e.args[0]);
    std::vector<Column> ints;
    bool any_validity = (bool)arg.validity;
    StrRangeArgs A;
    memset(&A, 0, sizeof(A));
    A.fn = f.param;
    A.has_count = e.args.size() == 3 ? 1 : 0;
    A.s = arg.ref();
    A.a = int_argument(ex, in, e.args[1], ints, any_validity);
    if (A.has_count) A.b = int_argument(ex, in, e.args[2], ints, any_validity);
    Temp tmp(ex);
    uint32_t* lengths = tmp.get<uint32_t>((size_t)n + 1);
    uint32_t* status = tmp.get<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(status, 0, 4, ex.stream));
    BufferPtr validity = any_validity ? validity_buffer(ex, n) : nullptr;
    TIMED_LAUNCH_N(ex, "str_range_lengths", n, launch_str_range_lengths(ex.cfg(), A, n, lengths, validity ? validity->as<uint64_t>() : nullptr, status));
    Utf8Total total;
    Column out = utf8_from_lengths(ex, tmp, lengths, n, total);
    utf8_alloc_data(ex, out, arg.data_bytes);
    TIMED_LAUNCH_N(ex, "str_range_write", n, launch_str_range_write(ex.cfg(), A, n, out.offsets->as<int32_t>(), out.data->as<uint8_t>()));
    if (utf8_read_total(ex, tmp, out, total, status) & STR_RANGE_STATUS_NEGATIVE) fail(BHIP_EEXEC, "negative substring length not allowed");
    out.validity = validity;
    return out;
}

// char_length(<Utf8 expression>): one thread per row counts its code points; NULL exactly where the argument is
Column eval_char_length(const Exec& ex, const Batch& in, const ExprPtr& e, const ScalarFn&) {
    const Column arg = eval_utf8(ex, in, e->args[0]);
    const int64_t n = in.n_rows;
    Column out = alloc_column(ex, DT_INT32, n, false);
    out.validity = arg.validity;
    TIMED_LAUNCH_N(ex, "char_length", n, launch_char_length(ex.cfg(), arg.ref(), n, out.data->as<int32_t>()));
    return out;
}

// strpos(s, sub) -> Int32 / starts_with(s, prefix) -> Boolean: the second argument a literal in the struct, or a column
Column eval_str_search(const Exec& ex, const Batch& in, const ExprPtr& ep, const ScalarFn& f) {
    const Expr& e = *ep;
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
    Column out = alloc_column(ex, f.result, n, arg.validity || sub.validity);
    uint64_t* validity = out.validity_words();
    if (f.param == STR_STRPOS) TIMED_LAUNCH_N(ex, "strpos", n, launch_strpos(ex.cfg(), A, n, out.data->as<int32_t>(), validity));
    else TIMED_LAUNCH_N(ex, "starts_with", n, launch_starts_with(ex.cfg(), A, n, out.data->as<uint64_t>(), validity));
    return out;
}

// ---- the lowered forms that are no scalar functions, as rows of their own -----------------------------------------------------------
const ScalarFn CASE_UTF8 = {"CASE", 0, 0, FN_UTF8, 0, DT_UTF8, COERCE_NONE, LARGE_NEVER, false, false, {}, nullptr, nullptr, validate_case, eval_case};
const ScalarFn CAST_TO_UTF8 = {"CAST", 1, 1, FN_UTF8, 0, DT_UTF8, COERCE_NONE, LARGE_NEVER, false, false, {}, nullptr, nullptr, validate_cast_format, eval_cast_format};
const ScalarFn CAST_FROM_UTF8 = {"CAST", 1, 1, FN_FIXED, 0, 0, COERCE_NONE, LARGE_NEVER, false, false, {}, nullptr, nullptr, validate_cast_parse, eval_cast_parse};

const ScalarFn* lowered_by(const ExprPtr& e, const Schema& schema) {
    switch (e->kind) {
        case BHIP_EXPR_SCALAR_FN: {
            const ScalarFn& f = scalar_fn(*e);
            return f.where == FN_UTF8 || (f.where == FN_FIXED && f.fold(e, schema) == nullptr) ? &f : nullptr;
        }
        case BHIP_EXPR_CASE: return expr_type(e, schema) == DT_UTF8 ? &CASE_UTF8 : nullptr;
        case BHIP_EXPR_CAST: {
            const Expr& x = *e->args[0];
            const bool from_utf8 = expr_type(e->args[0], schema) == DT_UTF8;
            if (from_utf8 == (e->dtype == DT_UTF8)) return nullptr;
            if (!from_utf8) return &CAST_TO_UTF8;
            return x.kind == BHIP_EXPR_LITERAL && !x.is_null ? nullptr : &CAST_FROM_UTF8;       // (a Utf8 literal folds in the VM's compiler: host/expr.cpp)
        }
        default: return nullptr;
    }
}

// the row that evaluates a Utf8-valued `e` that is neither a column nor a literal, null if there is none
const ScalarFn* utf8_form(const ExprPtr& e, const Schema& schema) {
    if (e->kind == BHIP_EXPR_CASE) return &CASE_UTF8;
    const ScalarFn* f = lowered_by(e, schema);
    return f && f->where == FN_UTF8 ? f : nullptr;
}
bool utf8_to_utf8_cast(const ExprPtr& e, const Schema& schema) { return e->kind == BHIP_EXPR_CAST && e->dtype == DT_UTF8 && expr_type(e->args[0], schema) == DT_UTF8; }

Column eval_utf8(const Exec& ex, const Batch& in, const ExprPtr& e) {
    if (e->kind == BHIP_EXPR_COLUMN) {
        const int i = in.schema->index_of(e->name);
        if (i < 0) fail(BHIP_EINVAL, "No field named '" + e->name + "'");
        if (in.cols[i].dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 column: " + e->name);
        return in.cols[i];
    }
    if (e->kind == BHIP_EXPR_LITERAL) {
        if (e->dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 literal");
        return eval_literal(ex, *e, in.n_rows);
    }
    if (utf8_to_utf8_cast(e, *in.schema)) return eval_utf8(ex, in, e->args[0]);
    if (const ScalarFn* f = utf8_form(e, *in.schema)) return f->eval(ex, in, e, *f);
    fail(BHIP_ENOTIMPL, "expression producing Utf8: " + e->to_string());
}

void check_utf8(const ExprPtr& e, const Schema& in) {
    if (e->kind == BHIP_EXPR_COLUMN) {
        const int i = in.index_of(e->name);
        if (i < 0) fail(BHIP_EINVAL, "No field named '" + e->name + "'");
        if (in.fields[i].dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 column: " + e->name);
    } else if (e->kind == BHIP_EXPR_LITERAL) {
        if (e->dtype != DT_UTF8) fail(BHIP_EINVAL, "expected a Utf8 literal");
    } else if (utf8_to_utf8_cast(e, in)) {
        check_utf8(e->args[0], in);
    } else if (const ScalarFn* f = utf8_form(e, in)) {
        f->validate(e, in, *f);
    } else {
        fail(BHIP_ENOTIMPL, "expression producing Utf8: " + e->to_string());
    }
}

}  // namespace

bool has_lowered_node(const ExprPtr& e, const Schema& schema) {
    if (lowered_by(e, schema)) return true;
    for (auto& a : e->args)
        if (has_lowered_node(a, schema)) return true;
    return false;
}

Utf8Lowering::Utf8Lowering(const Schema& in) : in_(in) {}

ExprPtr Utf8Lowering::rewrite(const ExprPtr& e, bool output) {
    const bool lit = output && e->kind == BHIP_EXPR_LITERAL && e->dtype == DT_UTF8;
    if (lit || lowered_by(e, in_)) {
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

// a node is what lowered_by() says, or a bare Utf8 literal that is an output column: check_utf8 / eval_utf8 take that one
BatchPtr Utf8Lowering::apply(const Exec& ex, const Batch& in) const {
    auto out = std::make_shared<Batch>(in);
    out->schema = schema();
    for (auto& node : nodes_) {
        if (in.n_rows == 0) {
            out->cols.push_back(alloc_column(ex, expr_type(node, in_), 0, false));
        } else {
            const ScalarFn* f = lowered_by(node, in_);
            out->cols.push_back(f ? f->eval(ex, in, node, *f) : eval_utf8(ex, in, node));
        }
    }
    return out;
}

void Utf8Lowering::validate() const {
    for (auto& n : nodes_) {
        if (const ScalarFn* f = lowered_by(n, in_)) f->validate(n, in_, *f);
        else check_utf8(n, in_);
    }
}

// ---- the table ----------------------------------------------------------------------------------------------------------------------
// name, arguments (min, max), where, param, result, coercion, LargeUtf8 from, Binary, own NULLs, aliases, fold, check, validate, eval
static const ScalarFn SCALAR_FNS[] = {
    {"sqrt", 1, 1, FN_VM_MATH, 0, DT_FLOAT64, COERCE_FLOAT64},
    {"abs", 1, 1, FN_VM_MATH, 1, DT_FLOAT64, COERCE_FLOAT64},
    {"floor", 1, 1, FN_VM_MATH, 2, DT_FLOAT64, COERCE_FLOAT64},
    {"ceil", 1, 1, FN_VM_MATH, 3, DT_FLOAT64, COERCE_FLOAT64},
    {"round", 1, 1, FN_VM_MATH, 4, DT_FLOAT64, COERCE_FLOAT64},
    {"trunc", 1, 1, FN_VM_MATH, 5, DT_FLOAT64, COERCE_FLOAT64},
    {"signum", 1, 1, FN_VM_MATH, 6, DT_FLOAT64, COERCE_FLOAT64},
    {"exp", 1, 1, FN_VM_MATH, 7, DT_FLOAT64, COERCE_FLOAT64},
    {"ln", 1, 1, FN_VM_MATH, 8, DT_FLOAT64, COERCE_FLOAT64},
    {"log2", 1, 1, FN_VM_MATH, 9, DT_FLOAT64, COERCE_FLOAT64},
    {"log10", 1, 1, FN_VM_MATH, 10, DT_FLOAT64, COERCE_FLOAT64},
    {"sin", 1, 1, FN_VM_MATH, 11, DT_FLOAT64, COERCE_FLOAT64},
    {"cos", 1, 1, FN_VM_MATH, 12, DT_FLOAT64, COERCE_FLOAT64},
    {"tan", 1, 1, FN_VM_MATH, 13, DT_FLOAT64, COERCE_FLOAT64},
    {"asin", 1, 1, FN_VM_MATH, 14, DT_FLOAT64, COERCE_FLOAT64},
    {"acos", 1, 1, FN_VM_MATH, 15, DT_FLOAT64, COERCE_FLOAT64},
    {"atan", 1, 1, FN_VM_MATH, 16, DT_FLOAT64, COERCE_FLOAT64},
    {"octet_length", 1, 1, FN_VM, VM_OCTET_LENGTH, DT_INT32},
    {"nullif", 2, 2, FN_VM, VM_NULLIF, TYPE_OF_ARG(0), COERCE_LIKE_EQ, LARGE_NEVER, false, true},
    {"lower", 1, 1, FN_UTF8, STR_LOWER, DT_UTF8, COERCE_NONE, LARGE_ARG0, false, false, {}, nullptr, nullptr, validate_strings, eval_transform},
    {"upper", 1, 1, FN_UTF8, STR_UPPER, DT_UTF8, COERCE_NONE, LARGE_ARG0, false, false, {}, nullptr, nullptr, validate_strings, eval_transform},
    {"trim", 1, 1, FN_UTF8, STR_TRIM, DT_UTF8, COERCE_NONE, LARGE_ARG0, false, false, {}, nullptr, nullptr, validate_strings, eval_transform},
    {"ltrim", 1, 1, FN_UTF8, STR_LTRIM, DT_UTF8, COERCE_NONE, LARGE_ARG0, false, false, {}, nullptr, nullptr, validate_strings, eval_transform},
    {"rtrim", 1, 1, FN_UTF8, STR_RTRIM, DT_UTF8, COERCE_NONE, LARGE_ARG0, false, false, {}, nullptr, nullptr, validate_strings, eval_transform},
    {"sha224", 1, 1, FN_UTF8, 224, DT_UTF8, COERCE_NONE, LARGE_NEVER, true, false, {}, nullptr, nullptr, validate_strings, eval_sha},
    {"sha256", 1, 1, FN_UTF8, 256, DT_UTF8, COERCE_NONE, LARGE_NEVER, true, false, {}, nullptr, nullptr, validate_strings, eval_sha},
    {"sha384", 1, 1, FN_UTF8, 384, DT_UTF8, COERCE_NONE, LARGE_NEVER, true, false, {}, nullptr, nullptr, validate_strings, eval_sha},
    {"sha512", 1, 1, FN_UTF8, 512, DT_UTF8, COERCE_NONE, LARGE_NEVER, true, false, {}, nullptr, nullptr, validate_strings, eval_sha},
    {"concat", 1, STR_CONCAT_MAX, FN_UTF8, 0, DT_UTF8, COERCE_NONE, LARGE_ANY_ARG, false, false, {}, nullptr, nullptr, validate_concat, eval_concat},
    {"substr", 2, 3, FN_UTF8, STR_SUBSTR, DT_UTF8, COERCE_INT64_REST, LARGE_ARG0, false, false, {"substring"}, fold_string_literal, check_string_fn, validate_str_range, eval_str_range},
    {"left", 2, 2, FN_UTF8, STR_LEFT, DT_UTF8, COERCE_INT64_REST, LARGE_ARG0, false, false, {}, fold_string_literal, check_string_fn, validate_str_range, eval_str_range},
    {"right", 2, 2, FN_UTF8, STR_RIGHT, DT_UTF8, COERCE_INT64_REST, LARGE_ARG0, false, false, {}, fold_string_literal, check_string_fn, validate_str_range, eval_str_range},
    {"char_length", 1, 1, FN_FIXED, STR_CHAR_LENGTH, DT_INT32, COERCE_NONE, LARGE_NEVER, false, false, {"length", "character_length"}, fold_string_literal, check_string_fn, validate_strings, eval_char_length},
    {"strpos", 2, 2, FN_FIXED, STR_STRPOS, DT_INT32, COERCE_NONE, LARGE_NEVER, false, false, {}, fold_string_literal, check_string_fn, validate_strings, eval_str_search},
    {"starts_with", 2, 2, FN_FIXED, STR_STARTS_WITH, DT_BOOLEAN, COERCE_NONE, LARGE_NEVER, false, false, {}, fold_string_literal, check_string_fn, validate_strings, eval_str_search},
    {"to_timestamp", 1, 1, FN_FIXED, 0, DT_TIMESTAMP_NS, COERCE_NONE, LARGE_NEVER, false, false, {}, fold_to_timestamp, check_to_timestamp, validate_to_timestamp, eval_to_timestamp},
    {"date_trunc", 2, 2, FN_FIXED, 0, TYPE_OF_ARG(1), COERCE_NONE, LARGE_NEVER, false, true, {}, fold_date_trunc, date_trunc_granularity, validate_temporal, eval_date_trunc},
    {"date_part", 2, 2, FN_FIXED, 0, DT_INT32, COERCE_NONE, LARGE_NEVER, false, true, {}, fold_date_part, date_part_of, validate_temporal, eval_date_part},
};

const ScalarFn* find_scalar_fn(const std::string& name) {
    for (const ScalarFn& f : SCALAR_FNS) {
        if (name == f.name) return &f;
        for (const char* a : f.aliases)
            if (a && name == a) return &f;
    }
    return nullptr;
}

}  // namespace bhip
