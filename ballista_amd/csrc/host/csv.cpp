// csv.cpp — host side of the general CSV scan (kernels_csv.hip): the leaf where the reference has CsvExec with the `has_header`
// and `delimiter` of the wire plan — rust/benchmarks/tpch/src/main.rs:129-150 (`--format csv`),
// rust/core/src/serde/physical_plan/from_proto.rs:93-110.  The text crosses PCIe once; records (quote-aware), fields, values and
// NULLs are found on the device.  Every value the device needs arrives as a kernel argument or is written by a kernel: no
// hipMemcpyAsync reads a host variable here.
#include <cstring>

#include "../csv_kernels.h"
#include "../util_kernels.h"
#include "core.hpp"
#include "text_scan.hpp"

namespace bhip {

CsvScanSpec make_csv_spec(int n_fields, const bhip_column_desc* fields, int n_proj, const int32_t* projection, const bhip_csv_opts& opts) {
    if (n_fields < 1 || n_fields > TBL_MAX_FIELDS) fail(BHIP_EINVAL, "csv schema must have 1.." + std::to_string(TBL_MAX_FIELDS) + " fields");
    if (opts.delimiter == '"' || opts.delimiter == '\n' || opts.delimiter == '\r')
        fail(BHIP_EINVAL, "csv delimiter must be one byte other than '\"', '\\n' and '\\r'");

    // which fields to materialise, in which order
    std::vector<int> proj;
    if (projection) {
        for (int i = 0; i < n_proj; ++i) {
            if (projection[i] < 0 || projection[i] >= n_fields) fail(BHIP_EINVAL, "csv projection index out of range");
            proj.push_back(projection[i]);
        }
    } else {
        for (int i = 0; i < n_fields; ++i) proj.push_back(i);
    }
    CsvScanSpec spec;
    CsvPlan& plan = spec.plan;
    memset(&plan, 0, sizeof(plan));
    plan.delimiter = opts.delimiter;
    int last_needed = -1;
    for (int f = 0; f < n_fields; ++f) {
        if (!fields[f].name) fail(BHIP_EINVAL, "csv field without a name");
        plan.dtype[f] = fields[f].dtype;
        plan.nullable[f] = fields[f].nullable != 0;
        plan.out[f] = -1;
    }
    auto schema = std::make_shared<Schema>();
    for (size_t s = 0; s < proj.size(); ++s) {
        const int f = proj[s];
        const int dt = fields[f].dtype;
        if (dt != DT_INT32 && dt != DT_INT64 && dt != DT_FLOAT64 && dt != DT_DATE32 && dt != DT_UTF8 && dt != DT_BOOLEAN)
            fail(BHIP_ENOTIMPL, std::string("csv scan of a ") + dtype_name(dt) + " column: " + fields[f].name);
        if (plan.out[f] >= 0) fail(BHIP_EINVAL, std::string("csv projection names a field twice: ") + fields[f].name);
        plan.out[f] = (int)s;
        schema->fields.push_back(Field{fields[f].name, dt, fields[f].nullable != 0});
        spec.dtype.push_back(dt);
        spec.nullable.push_back(fields[f].nullable != 0);
        if (f > last_needed) last_needed = f;
    }
    plan.n_fields = last_needed + 1;                     // fields behind the last projected one are never walked
    spec.schema = schema;
    return spec;
}

BatchPtr batch_from_csv(const ContextPtr& ctx, const void* text_host, int64_t n_bytes, int n_fields, const bhip_column_desc* fields,
                        int n_proj, const int32_t* projection, const bhip_csv_opts& opts) {
    if (n_bytes < 0 || n_bytes > 0xFFFFFFF0ll) fail(BHIP_EINVAL, "csv text must be < 4 GiB per call (split the file on record boundaries)");
    if (n_fields < 1 || n_fields > TBL_MAX_FIELDS) fail(BHIP_EINVAL, "csv schema must have 1.." + std::to_string(TBL_MAX_FIELDS) + " fields");
    if (n_bytes > 0 && !text_host) fail(BHIP_EINVAL, "csv text is null");
    const CsvScanSpec spec = make_csv_spec(n_fields, fields, n_proj, projection, opts);
    ctx->set_device();
    Exec ex{ctx, nullptr};

    Temp tmp(ex);
    uint8_t* text = tmp.get<uint8_t>((size_t)n_bytes + 64);
    if (n_bytes) HIP_CHECK(hipMemcpyAsync(text, text_host, (size_t)n_bytes, hipMemcpyHostToDevice, ex.stream));
    TextSlab slab;
    slab.text = text;
    slab.n_bytes = n_bytes;
    slab.unterminated = n_bytes > 0 && static_cast<const uint8_t*>(text_host)[n_bytes - 1] != '\n';
    slab.header_here = opts.has_header != 0;
    return parse_csv_slab(ex, spec, slab).batch;
}

TextParsed parse_csv_slab(const Exec& ex, const CsvScanSpec& spec, const TextSlab& slab) {
    const LaunchCfg cfg = ex.cfg();
    const uint8_t* text = slab.text;
    const int64_t n_bytes = slab.n_bytes;
    CsvPlan plan = spec.plan;
    const size_t n_slots = spec.dtype.size();

    auto batch = std::make_shared<Batch>();
    batch->ctx = ex.ctx;
    batch->schema = spec.schema;

    Temp tmp(ex);

    // ---- records: quotes and both newline counters per chunk -> parity of every chunk -> its first record rank
    const int64_t n_chunks = (n_bytes + TBL_CHUNK - 1) / TBL_CHUNK;
    uint32_t* chunk_quotes = tmp.get<uint32_t>((size_t)n_chunks + 1);
    uint32_t* chunk_newlines = tmp.get<uint32_t>(2 * (size_t)n_chunks + 2);
    uint32_t* chunk_records = tmp.get<uint32_t>((size_t)n_chunks + 1);
    uint64_t* quotes_before = tmp.get<uint64_t>((size_t)n_chunks + 1);
    uint64_t* chunk_base = tmp.get<uint64_t>((size_t)n_chunks + 1);
    struct Totals { uint64_t quotes, newlines; };
    Totals* totals_dev = tmp.get<Totals>(1);
    void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_chunks > 0 ? n_chunks : 1));
    Totals totals{0, 0};
    if (n_chunks) {
        HIP_CHECK(launch_csv_count(cfg, text, n_bytes, chunk_quotes, chunk_newlines));
        HIP_CHECK(exclusive_scan_u32_u64(ex.stream, chunk_quotes, n_chunks, quotes_before, false, &totals_dev->quotes, scan_tmp));
        HIP_CHECK(launch_csv_pick(cfg, quotes_before, chunk_newlines, n_chunks, chunk_records));
        HIP_CHECK(exclusive_scan_u32_u64(ex.stream, chunk_records, n_chunks, chunk_base, false, &totals_dev->newlines, scan_tmp));
        totals = read_device(ex, totals_dev);
    }
    // a slab that is not the last yields its complete records only; what lies behind the last '\n' outside quotes is the next
    // slab's carry, and a quote may still be open there
    if (slab.last && (totals.quotes & 1)) fail(BHIP_ENOTIMPL, "csv: a quoted field is not closed");
    const bool quoted = totals.quotes != 0;
    const bool unterminated = slab.last && slab.unterminated;
    const int64_t n_records = (int64_t)totals.newlines + (unterminated ? 1 : 0);
    if (n_records > 0xFFFFFFF0ll) fail(BHIP_EINVAL, "csv text holds more than 2^32-16 records");
    if (!slab.last && n_records == 0) return TextParsed{nullptr, slab.first_record};       // no record ends here: all of it is carry
    const int64_t header = slab.header_here && n_records > 0 ? 1 : 0;
    const int64_t n_rows = n_records - header;
    batch->n_rows = n_rows;

    uint64_t* starts = tmp.get<uint64_t>((size_t)n_records + 2);
    if (n_records) {
        FillMany fill;
        fill.add(starts, 4, (uint32_t)slab.first_record);
        fill.add(reinterpret_cast<uint32_t*>(starts) + 1, 4, 0);
        if (unterminated) {                                     // an unterminated last record "ends" one past the text (< 2^32)
            fill.add(starts + n_records, 4, (uint32_t)(n_bytes + 1));
            fill.add(reinterpret_cast<uint32_t*>(starts + n_records) + 1, 4, 0);
        }
        HIP_CHECK(launch_fill_many(cfg, fill));
        // a text without a single quote takes the quote-free line pass of the `.tbl` scan
        if (quoted) HIP_CHECK(launch_csv_starts(cfg, text, n_bytes, quotes_before, chunk_base, starts));
        else HIP_CHECK(launch_tbl_starts(cfg, text, n_bytes, chunk_base, starts));
    }

    // ---- values
    uint32_t* flags = tmp.get<uint32_t>(2);
    HIP_CHECK(hipMemsetAsync(flags, 0, 8, ex.stream));
    std::vector<uint32_t*> lens(n_slots, nullptr);
    for (size_t s = 0; s < n_slots; ++s) {
        const int dt = spec.dtype[s];
        Column c;
        c.dtype = dt;
        c.length = n_rows;
        if (dt == DT_UTF8) {
            plan.str_start[s] = tmp.get<uint32_t>((size_t)n_rows + 1);
            plan.str_len[s] = lens[s] = tmp.get<uint32_t>((size_t)n_rows + 1);
            if (quoted) plan.str_esc[s] = tmp.get<uint64_t>(bitmap_bytes(n_rows) / 8 + 1);
            c.offsets = make_buffer(ex, (size_t)(n_rows + 1) * 4);
        } else {
            c.data = make_buffer(ex, (dt == DT_BOOLEAN ? bitmap_bytes(n_rows) : (size_t)n_rows * dtype_width(dt)) + 8);
            plan.data[s] = c.data->ptr();
            if (spec.nullable[s]) {
                c.validity = make_buffer(ex, bitmap_bytes(n_rows) + 8);
                plan.validity[s] = c.validity->as<uint64_t>();
            }
        }
        batch->cols.push_back(std::move(c));
    }
    HIP_CHECK(launch_csv_parse(cfg, text, starts + header, n_rows, n_bytes, plan, quoted, flags));

    // ---- strings: lengths -> offsets -> bytes; all totals and the flags in one read-back
    uint64_t* totals_str = tmp.get<uint64_t>(n_slots + 1);
    std::vector<size_t> utf8;
    for (size_t s = 0; s < n_slots; ++s)
        if (lens[s]) {
            void* st = tmp.get<uint8_t>(exclusive_scan_temp_bytes(n_rows > 0 ? n_rows : 1));
            HIP_CHECK(exclusive_scan_u32_i32(ex.stream, lens[s], n_rows, batch->cols[s].offsets->as<int32_t>(), true, totals_str + s, st));
            utf8.push_back(s);
        }
    std::vector<uint64_t> host_totals(n_slots + 1, 0);
    uint32_t host_flags[2] = {0, 0};
    uint64_t cut = (uint64_t)n_bytes;
    if (!slab.last) HIP_CHECK(hipMemcpyAsync(&cut, starts + n_records, 8, hipMemcpyDeviceToHost, ex.stream));  // behind the last complete record
    if (!utf8.empty()) HIP_CHECK(hipMemcpyAsync(host_totals.data(), totals_str, n_slots * 8, hipMemcpyDeviceToHost, ex.stream));
    HIP_CHECK(hipMemcpyAsync(host_flags, flags, 8, hipMemcpyDeviceToHost, ex.stream));
    HIP_CHECK(hipStreamSynchronize(ex.stream));
    if (host_flags[0] & CSV_ERR_STRAY_QUOTE)
        fail(BHIP_ENOTIMPL, "csv: a quote inside an unquoted field, bytes behind a closing quote, or a bare carriage return");
    if (host_flags[0] & TBL_ERR_MISSING_FIELD) fail(BHIP_EEXEC, "csv: a record has fewer fields than the schema");
    if (host_flags[0] & TBL_ERR_BLANK_LINE) fail(BHIP_EEXEC, "csv: blank line");
    if (host_flags[0] & TBL_ERR_BAD_VALUE) fail(BHIP_EEXEC, "csv: a field is not a value of its column's type");
    if (host_flags[0] & CSV_ERR_NULL) fail(BHIP_EEXEC, "csv: an empty field in a column that is not nullable");
    if (host_flags[0] & TBL_ERR_PRECISION) fail(BHIP_ENOTIMPL, "csv: a decimal with more than 15 significant digits");
    for (size_t s = 0; s < n_slots; ++s)
        if (!(host_flags[1] >> s & 1u)) batch->cols[s].validity.reset();        // no NULL occurred: no validity buffer
    for (size_t s : utf8) {
        if (host_totals[s] > 0x7FFFFFFFull) fail(BHIP_EEXEC, "Utf8 column exceeds 2 GiB of value bytes");
        Column& c = batch->cols[s];
        c.data_bytes = (int64_t)host_totals[s];
        c.data = make_buffer(ex, (size_t)c.data_bytes + 8);
        HIP_CHECK(launch_csv_copy_strings(cfg, text, plan.str_start[s], lens[s], plan.str_esc[s], c.offsets->as<int32_t>(), n_rows,
                                          c.data->as<uint8_t>()));
    }
    HIP_CHECK(hipStreamSynchronize(ex.stream));
    return TextParsed{batch, (int64_t)cut};
}

}  // namespace bhip
