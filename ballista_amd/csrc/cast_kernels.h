// cast_kernels.h — launchers of kernels_cast.hip (internal C++ interface): CAST between Utf8 and the fixed-width types.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace bhip {

constexpr uint32_t CAST_STATUS_DECLINED = 1u;       // a float string outside the exactly rounded path (cast_text.h)

// CAST(<Utf8 column> AS to): n values at `out` (a Boolean target: the bitmap) and n validity bits.  Both bitmaps are written as
// whole 64-bit words, (n + 63) / 64 of them.  *status gets CAST_STATUS_DECLINED OR-ed in; only a float target can set it.
hipError_t launch_cast_parse(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int to, void* out, uint64_t* validity, uint32_t* status);

// CAST(<fixed-width column> AS Utf8): lengths first, then — after a scan — the bytes.  validity_out (may be null): the result's
// validity in whole 64-bit words, for the one source type whose values can have no text (a Date32 outside 0000 .. 9999).
hipError_t launch_cast_format_lengths(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, uint32_t* lengths, uint64_t* validity_out);
hipError_t launch_cast_format_write(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, const int32_t* out_offsets, uint8_t* out);

// to_timestamp(<Utf8 column>): n Timestamp(Nanosecond) values at `out` (0 for a NULL row; the result's validity is the argument's).
// *status gets TO_TIMESTAMP_STATUS_INVALID OR-ed in when a non-NULL value is outside the grammar of temporal_text.h.
constexpr uint32_t TO_TIMESTAMP_STATUS_INVALID = 1u;
hipError_t launch_to_timestamp_parse(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int64_t* out, uint32_t* status);

// date_trunc(granularity, <Timestamp column>): n values of the column's own type at `out` and n validity bits, written as whole
// 64-bit words: NULL where the argument is, or where the floor does not fit int64 in the unit.  granularity: TruncGranularity.
hipError_t launch_date_trunc(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int granularity, int64_t* out, uint64_t* validity);

// date_part(part, <Date32 / Date64 / Timestamp column>): n Int32 values at `out` and n validity bits, written as whole 64-bit words:
// NULL where the argument is, or where the field does not fit Int32.  part: DatePart (temporal_text.h).
hipError_t launch_date_part(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int part, int32_t* out, uint64_t* validity);

}  // namespace bhip
