// csv_kernels.h — launchers of kernels_csv.hip (general CSV text: any one-byte delimiter, quoted fields, NULLs -> Arrow columns
// on the device).  The `.tbl` scan (tbl_kernels.h) is the '|', quote-free, NULL-free special case with count, starts and parse
// kernels of its own; the field plan (TextPlan) and the string copy are declared there, for both.
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
                            const TextPlan& plan, bool quoted, uint32_t* flags);

}  // namespace bhip
