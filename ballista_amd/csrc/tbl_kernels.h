// tbl_kernels.h — launchers of kernels_tbl.hip ('|'-separated TPC-H text -> Arrow columns on the device), and what the CSV scan
// (csv_kernels.h) shares with it: the field plan, the error bits, the string copy
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace bhip {

constexpr int TBL_CHUNK = 16384;          // bytes of text per workgroup in the line passes
constexpr int TBL_MAX_FIELDS = 32;

enum TblErr : uint32_t {
    TBL_ERR_MISSING_FIELD = 1u,           // a line has fewer fields than the schema
    TBL_ERR_BAD_VALUE = 2u,               // not a number / date of the declared type
    TBL_ERR_PRECISION = 4u,               // a decimal with more than 15-16 significant digits (not converted exactly)
    TBL_ERR_BLANK_LINE = 8u
};

// what to do with each field of a record.  The `.tbl` walk ('|', no quotes, no NULLs) ignores delimiter, nullable, validity, str_esc.
struct TextPlan {
    int32_t n_fields;
    int32_t delimiter;
    int32_t dtype[TBL_MAX_FIELDS];        // DType of the field
    int32_t out[TBL_MAX_FIELDS];          // output slot, or -1: skipped
    int32_t nullable[TBL_MAX_FIELDS];     // [field] an empty field is NULL (else CSV_ERR_NULL)
    void* data[TBL_MAX_FIELDS];           // [slot] fixed-width values | Boolean bitmap (64-bit words)
    uint64_t* validity[TBL_MAX_FIELDS];   // [slot] validity bitmap of a nullable non-Utf8 column, or null
    uint32_t* str_start[TBL_MAX_FIELDS];  // [slot] Utf8: offset of the field's content in the text (behind an opening quote)
    uint32_t* str_len[TBL_MAX_FIELDS];    // [slot] Utf8: its length with every "" counted once
    uint64_t* str_esc[TBL_MAX_FIELDS];    // [slot] Utf8: bit i = the content of row i holds "" pairs (null: the text has no quotes)
};

hipError_t launch_tbl_count(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, uint32_t* chunk_lines);
hipError_t launch_tbl_starts(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, const uint64_t* chunk_base, uint64_t* starts);
hipError_t launch_tbl_parse(const LaunchCfg& cfg, const uint8_t* text, const uint64_t* starts, int64_t n_lines, int64_t n_bytes,
                            const TextPlan& plan, uint32_t* flags);
// both formats: the bytes of one Utf8 column behind its offsets; str_esc may be null (no row holds "" pairs)
hipError_t launch_text_copy_strings(const LaunchCfg& cfg, const uint8_t* text, const uint32_t* str_start, const uint32_t* str_len,
                                    const uint64_t* str_esc, const int32_t* offsets, int64_t n, uint8_t* out);

}  // namespace bhip
