// text_scan.hpp — the `.tbl` and CSV scans (text_scan.cpp) as one function over text that is already on the device, so that the
// one-shot entry points (bhip_batch_from_tbl / _csv: the whole text in one call) and the slab pipeline of the scan leaf
// (text_stream.cpp: a file of any size, one batch per slab) run the same passes.
#pragma once
#include "../csv_kernels.h"
#include "../tbl_kernels.h"
#include "core.hpp"

namespace bhip {

// One piece of a text on the device.  The kernels index the text from `text` with 32-bit offsets and load 16-byte pieces at
// multiples of 16, so `text` is 256-byte aligned and n_bytes < 4 GiB.  A slab that continues a file starts with the carry of the
// slab before it (the bytes behind that slab's last record end); the carry ends where the new bytes begin, which is aligned, so
// it begins at `first_record` >= 0 bytes behind `text`, and the bytes before it are NUL: neither a quote nor a newline.
struct TextSlab {
    const uint8_t* text = nullptr;
    int64_t n_bytes = 0;
    int64_t first_record = 0;       // offset of the first record's first byte (0 for a whole text; < 256 in a slab)
    bool last = true;               // the text ends with this slab: an unterminated last record counts, an open quote is an error
    bool unterminated = false;      // last slab: its last byte is not '\n'
    bool header_here = false;       // CSV: the first record of this slab is the header
};

// the batch of the slab's complete records, and `cut`: the offset behind the last of them (n_bytes in the last slab).  The bytes
// [cut, n_bytes) of a slab that is not the last are the carry of the next one.  No batch (null) and cut = first_record when no
// record ends in a slab that is not the last.
struct TextParsed {
    BatchPtr batch;
    int64_t cut = 0;
};

// what one scan reads: the schema and the projection, validated once.  The plan is the parse kernels' own argument; its per-slot
// pointers are filled per slab.
struct TextScanSpec {
    int format = BHIP_TEXT_TBL;     // BHIP_TEXT_TBL | BHIP_TEXT_CSV
    TextPlan plan;                  // field walk; CSV: with the delimiter and which fields may be NULL
    SchemaPtr schema;
    std::vector<int> dtype;         // [slot]
    std::vector<char> nullable;     // [slot]
};
// validate the schema and the projection (BHIP_EINVAL / BHIP_ENOTIMPL as the one-shot entry points report them); csv_opts: CSV only
TextScanSpec make_text_spec(int format, int n_fields, const bhip_column_desc* fields, int n_proj, const int32_t* projection,
                            const bhip_csv_opts& csv_opts);
// the one place that says which bytes cannot separate fields (BHIP_EINVAL); the scan leaf asks when the plan is built
void check_csv_delimiter(uint8_t delimiter);

// records -> starts -> columns -> parse -> strings -> read-back.  Everything runs on ex.stream; returns once the batch is complete.
TextParsed parse_text_slab(const Exec& ex, const TextScanSpec& spec, const TextSlab& slab);

}  // namespace bhip
