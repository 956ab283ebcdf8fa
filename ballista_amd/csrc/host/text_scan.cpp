// text_scan.cpp — host side of the two text scans, `.tbl` (kernels_tbl.hip) and general CSV (kernels_csv.hip): the leaf where the
// reference has CsvExec with the `has_header` and `delimiter` of the wire plan — rust/benchmarks/tpch/src/main.rs:129-150
// (`--format tbl` / `--format csv`), rust/core/src/serde/physical_plan/from_proto.rs:93-110.  The text crosses PCIe once;
// records (quote-aware in CSV), fields, values and NULLs are found on the device.  Every value the device needs arrives as a
// kernel argument or is written by a kernel: no hipMemcpyAsync reads a host variable here.
//
// `.tbl` is the '|', quote-free, NULL-free, header-free case with count, starts and parse kernels of its own.  Where the CSV scan
// does more, it says so at that point: the count pass, the starts kernel, the header, three more per-slot buffers, the flags.
#include <cstring>

#include "../util_kernels.h"
#include "core.hpp"
#include "text_scan.hpp"

namespace bhip {

namespace {

// flag bit of the parse pass -> what the caller is told; the first set bit of a table wins, a zero bit ends it
struct FlagError { uint32_t bit; int status; const char* message; };
const FlagError TBL_ERRORS[] = {
    {TBL_ERR_MISSING_FIELD, BHIP_EEXEC, "tbl: a line has fewer fields than the schema"},
    {TBL_ERR_BLANK_LINE, BHIP_EEXEC, "tbl: blank line"},
    {TBL_ERR_BAD_VALUE, BHIP_EEXEC, "tbl: a field is not a value of its column's type"},
    {TBL_ERR_PRECISION, BHIP_ENOTIMPL, "tbl: a decimal with more than 15 significant digits"},
    {0, 0, nullptr},
};
const FlagError CSV_ERRORS[] = {
    {CSV_ERR_STRAY_QUOTE, BHIP_ENOTIMPL, "csv: a quote inside an unquoted field, bytes behind a closing quote, or a bare carriage return"},
    {TBL_ERR_MISSING_FIELD, BHIP_EEXEC, "csv: a record has fewer fields than the schema"},
    {TBL_ERR_BLANK_LINE, BHIP_EEXEC, "csv: blank line"},
    {TBL_ERR_BAD_VALUE, BHIP_EEXEC, "csv: a field is not a value of its column's type"},
    {CSV_ERR_NULL, BHIP_EEXEC, "csv: an empty field in a column that is not nullable"},
    {TBL_ERR_PRECISION, BHIP_ENOTIMPL, "csv: a decimal with more than 15 significant digits"},
    {0, 0, nullptr},
};

const char* format_name(int format) { return format == BHIP_TEXT_CSV ? "csv" : "tbl"; }
const char* record_word(int format) { return format == BHIP_TEXT_CSV ? "record" : "line"; }

}  // namespace

void check_csv_delimiter(uint8_t delimiter) {
    if (delimiter == '"' || delimiter == '\n' || delimiter == '\r')
        fail(BHIP_EINVAL, "csv delimiter must be one byte other than '\"', '\\n' and '\\r'");
}

TextScanSpec make_text_spec(int format, int n_fields, const bhip_column_desc* fields, int n_proj, const int32_t* projection,
                            const bhip_csv_opts& csv_opts) {
    const bool csv = format == BHIP_TEXT_CSV;
    const std::string name = format_name(format);
    if (n_fields < 1 || n_fields > TBL_MAX_FIELDS) fail(BHIP_EINVAL, name + " schema must have 1.." + std::to_string(TBL_MAX_FIELDS) + " fields");
    if (csv) check_csv_delimiter(csv_opts.delimiter);

    // which fields to materialise, in which order
    std::vector<int> proj;
    if (projection) {
        for (int i = 0; i < n_proj; ++i) {
            if (projection[i] < 0 || projection[i] >= n_fields) fail(BHIP_EINVAL, name + " projection index out of range");
            proj.push_back(projection[i]);
        }
    } else {
        for (int i = 0; i < n_fields; ++i) proj.push_back(i);
    }
    for (int f = 0; f < n_fields; ++f)
        if (!fields[f].name) fail(BHIP_EINVAL, name + " field without a name");
    TextScanSpec spec;
    spec.format = format;
    std::vector<int> out(n_fields, -1);
    int last_needed = -1;
    auto schema = std::make_shared<Schema>();
    for (size_t s = 0; s < proj.size(); ++s) {
        const int f = proj[s];
        const int dt = fields[f].dtype;
        if (dt != DT_INT32 && dt != DT_INT64 && dt != DT_FLOAT64 && dt != DT_DATE32 && dt != DT_UTF8 && !(csv && dt == DT_BOOLEAN))
            fail(BHIP_ENOTIMPL, name + " scan of a " + dtype_name(dt) + " column: " + fields[f].name);
        if (out[f] >= 0) fail(BHIP_EINVAL, name + " projection names a field twice: " + fields[f].name);
        out[f] = (int)s;
        schema->fields.push_back(Field{fields[f].name, dt, fields[f].nullable != 0});
        spec.dtype.push_back(dt);
        spec.nullable.push_back(fields[f].nullable != 0);
        if (f > last_needed) last_needed = f;
    }
    spec.schema = schema;

    // the field walk of the parse kernel; fields behind the last projected one are never walked
    memset(&spec.plan, 0, sizeof(spec.plan));
    spec.plan.n_fields = last_needed + 1;
    spec.plan.delimiter = csv_opts.delimiter;
    for (int f = 0; f < n_fields; ++f) {
        spec.plan.dtype[f] = fields[f].dtype;
        spec.plan.out[f] = out[f];
        spec.plan.nullable[f] = fields[f].nullable != 0;
    }
    return spec;
}

BatchPtr batch_from_text(const ContextPtr& ctx, int format, const void* text_host, int64_t n_bytes, int n_fields,
                         const bhip_column_desc* fields, int n_proj, const int32_t* projection, const bhip_csv_opts& csv_opts) {
    const std::string name = format_name(format);
    if (n_bytes < 0 || n_bytes > 0xFFFFFFF0ll)
        fail(BHIP_EINVAL, name + " text must be < 4 GiB per call (split the file on " + record_word(format) + " boundaries)");
    const TextScanSpec spec = make_text_spec(format, n_fields, fields, n_proj, projection, csv_opts);
    if (n_bytes > 0 && !text_host) fail(BHIP_EINVAL, name + " text is null");
    ctx->set_device();
    Exec ex{ctx, nullptr};

    Temp tmp(ex);
    uint8_t* text = tmp.get<uint8_t>((size_t)n_bytes + 64);
    if (n_bytes) HIP_CHECK(hipMemcpyAsync(text, text_host, (size_t)n_bytes, hipMemcpyHostToDevice, ex.stream));
    TextSlab slab;
    slab.text = text;
    slab.n_bytes = n_bytes;
    slab.unterminated = n_bytes > 0 && static_cast<const uint8_t*>(text_host)[n_bytes - 1] != '\n';
    slab.header_here = format == BHIP_TEXT_CSV && csv_opts.has_header != 0;
    return parse_text_slab(ex, spec, slab).batch;
}

TextParsed parse_text_slab(const Exec& ex, const TextScanSpec& spec, const TextSlab& slab) {
    const bool csv = spec.format == BHIP_TEXT_CSV;
    const std::string name = format_name(spec.format);
    const LaunchCfg cfg = ex.cfg();
    const uint8_t* text = slab.text;
    const int64_t n_bytes = slab.n_bytes;
    const size_t n_slots = spec.dtype.size();

    auto batch = new_batch(ex.ctx, spec.schema, 0);           // n_rows: once the records are counted

    Temp tmp(ex);

    // ---- records: newlines per chunk -> each chunk's first record rank.  CSV: quotes and both newline counters per chunk ->
    // parity of every chunk, which picks the counter that lies outside quotes
    const int64_t n_chunks = (n_bytes + TBL_CHUNK - 1) / TBL_CHUNK;
    struct Totals { uint64_t quotes, newlines; };
    Totals totals{0, 0};
    uint64_t* quotes_before = nullptr;
    uint64_t* chunk_base = nullptr;
    if (!csv) {
        uint32_t* chunk_lines = tmp.get<uint32_t>((size_t)n_chunks + 1);
        chunk_base = tmp.get<uint64_t>((size_t)n_chunks + 1);
        uint64_t* total = tmp.get<uint64_t>(1);
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_chunks > 0 ? n_chunks : 1));
        if (n_chunks) {
            HIP_CHECK(launch_tbl_count(cfg, text, n_bytes, chunk_lines));
            HIP_CHECK(exclusive_scan_u32_u64(ex.stream, chunk_lines, n_chunks, chunk_base, false, total, scan_tmp));
            totals.newlines = read_device(ex, total);
        }
    } else {
        uint32_t* chunk_quotes = tmp.get<uint32_t>((size_t)n_chunks + 1);
        uint32_t* chunk_newlines = tmp.get<uint32_t>(2 * (size_t)n_chunks + 2);
        uint32_t* chunk_records = tmp.get<uint32_t>((size_t)n_chunks + 1);
        quotes_before = tmp.get<uint64_t>((size_t)n_chunks + 1);
        chunk_base = tmp.get<uint64_t>((size_t)n_chunks + 1);
        Totals* totals_dev = tmp.get<Totals>(1);
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_chunks > 0 ? n_chunks : 1));
        if (n_chunks) {
            HIP_CHECK(launch_csv_count(cfg, text, n_bytes, chunk_quotes, chunk_newlines));
            HIP_CHECK(exclusive_scan_u32_u64(ex.stream, chunk_quotes, n_chunks, quotes_before, false, &totals_dev->quotes, scan_tmp));
            HIP_CHECK(launch_csv_pick(cfg, quotes_before, chunk_newlines, n_chunks, chunk_records));
            HIP_CHECK(exclusive_scan_u32_u64(ex.stream, chunk_records, n_chunks, chunk_base, false, &totals_dev->newlines, scan_tmp));
            totals = read_device(ex, totals_dev);
        }
    }
    // a slab that is not the last yields its complete records only; what lies behind the last record end is the next slab's
    // carry, and a quote may still be open there
    if (slab.last && (totals.quotes & 1)) fail(BHIP_ENOTIMPL, "csv: a quoted field is not closed");
    const bool quoted = totals.quotes != 0;
    const bool unterminated = slab.last && slab.unterminated;
    const int64_t n_records = (int64_t)totals.newlines + (unterminated ? 1 : 0);
    if (n_records > 0xFFFFFFF0ll) fail(BHIP_EINVAL, name + " text holds more than 2^32-16 " + record_word(spec.format) + "s");
    if (!slab.last && n_records == 0) return TextParsed{nullptr, slab.first_record};       // no record ends here: all of it is carry
    const int64_t header = slab.header_here && n_records > 0 ? 1 : 0;                       // CSV only
    const int64_t n_rows = n_records - header;
    batch->n_rows = n_rows;

    // ---- starts
    uint64_t* starts = tmp.get<uint64_t>((size_t)n_records + 2);
    if (n_records) {
        FillMany fill;                                          // the two ends the starts pass does not write (values < 2^32)
        fill.add(starts, 4, (uint32_t)slab.first_record);
        fill.add(reinterpret_cast<uint32_t*>(starts) + 1, 4, 0);
        if (unterminated) {                                     // an unterminated last record "ends" one past the text
            fill.add(starts + n_records, 4, (uint32_t)(n_bytes + 1));
            fill.add(reinterpret_cast<uint32_t*>(starts + n_records) + 1, 4, 0);
        }
        HIP_CHECK(launch_fill_many(cfg, fill));
        // a text without a single quote takes the quote-free line pass of the `.tbl` scan
        if (quoted) HIP_CHECK(launch_csv_starts(cfg, text, n_bytes, quotes_before, chunk_base, starts));
        else HIP_CHECK(launch_tbl_starts(cfg, text, n_bytes, chunk_base, starts));
    }

    // ---- columns.  CSV: a mark per row whose string holds "" pairs, a validity bitmap per nullable column, Boolean as a bitmap
    uint32_t* flags = tmp.get<uint32_t>(2);
    HIP_CHECK(hipMemsetAsync(flags, 0, 8, ex.stream));
    TextPlan plan = spec.plan;
    for (size_t s = 0; s < n_slots; ++s) {
        const int dt = spec.dtype[s];
        // a Utf8 column: offsets now, the bytes once the lengths are summed (below)
        Column c = alloc_column(ex, dt, n_rows, dt != DT_UTF8 && csv && spec.nullable[s], /*utf8_data_bytes: later*/ -1);
        if (dt == DT_UTF8) {
            plan.str_start[s] = tmp.get<uint32_t>((size_t)n_rows + 1);
            plan.str_len[s] = tmp.get<uint32_t>((size_t)n_rows + 1);
            if (quoted) plan.str_esc[s] = tmp.get<uint64_t>(bitmap_bytes(n_rows) / 8 + 1);
        } else {
            plan.data[s] = c.data->ptr();
            plan.validity[s] = c.validity_words();
        }
        batch->cols.push_back(std::move(c));
    }

    // ---- parse
    if (csv) HIP_CHECK(launch_csv_parse(cfg, text, starts + header, n_rows, n_bytes, plan, quoted, flags));
    else HIP_CHECK(launch_tbl_parse(cfg, text, starts, n_rows, n_bytes, plan, flags));

    // ---- strings: lengths -> offsets -> bytes
    uint64_t* totals_str = tmp.get<uint64_t>(n_slots + 1);
    std::vector<size_t> utf8;
    for (size_t s = 0; s < n_slots; ++s)
        if (plan.str_len[s]) {
            void* st = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_rows > 0 ? n_rows : 1));
            HIP_CHECK(exclusive_scan_u32_i32(ex.stream, plan.str_len[s], n_rows, batch->cols[s].offsets->as<int32_t>(), true, totals_str + s, st));
            utf8.push_back(s);
        }

    // ---- read-back: the cut, all string totals and the flags at once
    std::vector<uint64_t> host_totals(n_slots + 1, 0);
    uint32_t host_flags[2] = {0, 0};                            // [1], CSV: the slots in which a NULL occurred
    uint64_t cut = (uint64_t)n_bytes;
    if (!slab.last) HIP_CHECK(hipMemcpyAsync(&cut, starts + n_records, 8, hipMemcpyDeviceToHost, ex.stream));  // behind the last complete record
    if (!utf8.empty()) HIP_CHECK(hipMemcpyAsync(host_totals.data(), totals_str, n_slots * 8, hipMemcpyDeviceToHost, ex.stream));
    HIP_CHECK(hipMemcpyAsync(host_flags, flags, csv ? 8 : 4, hipMemcpyDeviceToHost, ex.stream));
    HIP_CHECK(hipStreamSynchronize(ex.stream));
    for (const FlagError* e = csv ? CSV_ERRORS : TBL_ERRORS; e->bit; ++e)
        if (host_flags[0] & e->bit) fail(e->status, e->message);
    for (size_t s = 0; s < n_slots; ++s)
        if (!(host_flags[1] >> s & 1u)) batch->cols[s].validity.reset();        // no NULL occurred: no validity buffer
    for (size_t s : utf8) {
        Column& c = batch->cols[s];
        utf8_alloc_data(ex, c, (int64_t)host_totals[s]);
        c.data_bytes = (int64_t)host_totals[s];
        const int32_t* offsets = c.offsets->as<int32_t>();
        HIP_CHECK(launch_text_copy_strings(cfg, text, plan.str_start[s], plan.str_len[s], plan.str_esc[s], offsets, n_rows, c.data->as<uint8_t>()));
    }
    HIP_CHECK(hipStreamSynchronize(ex.stream));
    return TextParsed{batch, (int64_t)cut};
}

}  // namespace bhip
