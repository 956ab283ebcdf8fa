// csv_kernels.h — launchers of kernels_csv.hip (general CSV text: any one-byte delimiter, quoted fields, NULLs -> Arrow columns
// on the device).  The `.tbl` scan (tbl_kernels.h) is the '|', quote-free, NULL-free special case and keeps its own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "tbl_kernels.h"

namespace bhip {

// error flags of the parse pass: the TblErr bits, plus
enum CsvErr : uint32_t {
    CSV_ERR_STRAY_QUOTE = 16u,            // a '"' inside an unquoted field, bytes behind a closing quote, a bare '\r': readers disagree
    CSV_ERR_NULL = 32u                    // an empty field in a non-nullable, non-Utf8 column
};

// what to do with each field of a record
struct CsvPlan {
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

// per chunk of TBL_CHUNK bytes: quotes[c] = number of '"'; newlines[2c] / [2c + 1] = '\n' seen at even / odd quote parity counted
// from the chunk's first byte
hipError_t launch_csv_count(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, uint32_t* quotes, uint32_t* newlines);
// records[c] = the counter of chunk c that lies outside quotes, given the quotes before the chunk
hipError_t launch_csv_pick(const LaunchCfg& cfg, const uint64_t* quotes_before, const uint32_t* newlines, int64_t n_chunks, uint32_t* records);
// starts[1 + r] = offset behind the r-th '\n' outside quotes (starts[0] belongs to the host)
hipError_t launch_csv_starts(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, const uint64_t* quotes_before,
                             const uint64_t* chunk_base, uint64_t* starts);
// flags[0] |= TblErr | CsvErr bits; flags[1] |= 1 << slot for every slot in which a NULL occurred.  quoted = false: the text holds
// no '"' at all (the count pass says so) and the walk does not look for any.
hipError_t launch_csv_parse(const LaunchCfg& cfg, const uint8_t* text, const uint64_t* starts, int64_t n_records, int64_t n_bytes,
                            const CsvPlan& plan, bool quoted, uint32_t* flags);
hipError_t launch_csv_copy_strings(const LaunchCfg& cfg, const uint8_t* text, const uint32_t* str_start, const uint32_t* str_len,
                                   const uint64_t* str_esc, const int32_t* offsets, int64_t n, uint8_t* out);

}  // namespace bhip
