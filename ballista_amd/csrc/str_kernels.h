// str_kernels.h — launchers of kernels_str.hip (internal C++ interface).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace bhip {

enum StrFn : int { STR_LOWER = 0, STR_UPPER = 1, STR_TRIM = 2, STR_LTRIM = 3, STR_RTRIM = 4 };

// lower / upper (ASCII letters; *non_ascii is set when a byte >= 0x80 went through unchanged) and the three trims
// (Unicode White_Space, as Rust's str::trim / trim_start / trim_end): lengths first, then — after a scan — the bytes
hipError_t launch_str_transform_lengths(const LaunchCfg& cfg, int kind, const ColumnRef& c, int64_t n, uint32_t* lengths);
hipError_t launch_str_transform_write(const LaunchCfg& cfg, int kind, const ColumnRef& c, int64_t n, const int32_t* out_offsets, uint8_t* out,
                                      uint32_t* non_ascii);

// a string literal as a column of n equal values
constexpr int STR_LITERAL_MAX = 240;
struct StrLiteral { int32_t len; uint8_t bytes[STR_LITERAL_MAX]; };
hipError_t launch_str_broadcast(const LaunchCfg& cfg, const StrLiteral& lit, int64_t n, int32_t* offsets, uint8_t* out);

// CASE WHEN cond[0] THEN val[0] ... [ELSE val[n_when]] END over Utf8 values
constexpr int STR_SELECT_MAX = 8;
struct StrSelectArgs {
    int32_t n_when, has_else;
    ColumnRef cond[STR_SELECT_MAX];          // Boolean columns
    ColumnRef val[STR_SELECT_MAX + 1];       // Utf8 columns; val[n_when] = the ELSE value
};
hipError_t launch_str_select_lengths(const LaunchCfg& cfg, const StrSelectArgs& A, int64_t n, uint32_t* lengths, uint64_t* validity);
hipError_t launch_str_select_write(const LaunchCfg& cfg, const StrSelectArgs& A, int64_t n, const int32_t* out_offsets, uint8_t* out);

// concat(a1, ..., ak): NULL where any argument is (SQL ||).  An argument is a Utf8 column, or a literal carried in the struct
// (is_lit[j] != 0: lit_len[j] bytes at lit_bytes + lit_off[j]; its ColumnRef is unused).
constexpr int STR_CONCAT_MAX = 8;
constexpr int STR_CONCAT_LIT_BYTES = 256;        // all literal arguments together
constexpr int STR_CONCAT_WAVE_BYTES = 1024;      // a row whose result is longer is copied by its whole wave, not by one lane
struct StrConcatArgs {
    int32_t n_args;
    int32_t is_lit[STR_CONCAT_MAX], lit_off[STR_CONCAT_MAX], lit_len[STR_CONCAT_MAX];
    ColumnRef col[STR_CONCAT_MAX];
    uint8_t lit_bytes[STR_CONCAT_LIT_BYTES];
};
// lengths[i] = the sum of the arguments' lengths (0 for a NULL row; saturated at 2^32 - 1, which the 2 GiB check of the caller
// catches).  validity (may be null when no argument has a validity buffer): written as whole 64-bit words, (n + 63) / 64 of them.
hipError_t launch_concat_lengths(const LaunchCfg& cfg, const StrConcatArgs& A, int64_t n, uint32_t* lengths, uint64_t* validity);
hipError_t launch_concat_write(const LaunchCfg& cfg, const StrConcatArgs& A, int64_t n, const int32_t* out_offsets, uint8_t* out);

// substr(s, start[, count]) / left(s, n) / right(s, n) (str_text.h: StrRangeFn and the rules).  An integer argument is an Int64
// column or a literal carried in the struct; left / right keep n in `a`.  NULL where any argument is.
struct StrIntArg { int32_t is_lit, pad; int64_t lit; ColumnRef col; };
struct StrRangeArgs {
    int32_t fn, has_count;
    ColumnRef s;
    StrIntArg a, b;
};
constexpr uint32_t STR_RANGE_STATUS_NEGATIVE = 1u;      // a non-NULL row of substr with count < 0
// lengths[i] = the result's byte count (0 for a NULL row).  validity (may be null when no argument has a validity buffer): whole
// 64-bit words, (n + 63) / 64 of them.  *status gets STR_RANGE_STATUS_NEGATIVE OR-ed in.
hipError_t launch_str_range_lengths(const LaunchCfg& cfg, const StrRangeArgs& A, int64_t n, uint32_t* lengths, uint64_t* validity, uint32_t* status);
// the bytes: a row whose result is longer than STR_CONCAT_WAVE_BYTES is copied by its whole wave, a shorter one by its lane
hipError_t launch_str_range_write(const LaunchCfg& cfg, const StrRangeArgs& A, int64_t n, const int32_t* out_offsets, uint8_t* out);

// char_length(s): n Int32 code-point counts (0 for a NULL row; the result's validity is the argument's)
hipError_t launch_char_length(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int32_t* out);
// strpos(s, sub) -> n Int32 values, starts_with(s, prefix) -> n bits.  `sub` is a Utf8 column, or a literal carried in the struct.
// validity (may be null when neither argument has a validity buffer) and the bits of starts_with: whole 64-bit words.
struct StrSearchArgs {
    int32_t sub_is_lit, pad;
    ColumnRef s, sub;
    StrLiteral lit;
};
hipError_t launch_strpos(const LaunchCfg& cfg, const StrSearchArgs& A, int64_t n, int32_t* out, uint64_t* validity);
hipError_t launch_starts_with(const LaunchCfg& cfg, const StrSearchArgs& A, int64_t n, uint64_t* out_bits, uint64_t* validity);

// sha224 / sha256 / sha384 / sha512 of every string: n digests of bits / 8 bytes at out + row * (bits / 8), offsets written too
hipError_t launch_sha2(const LaunchCfg& cfg, int bits, const ColumnRef& c, int64_t n, int32_t* out_offsets, uint8_t* out);

// MIN / MAX over Utf8 through sort ranks
hipError_t launch_invert_perm(const LaunchCfg& cfg, const uint32_t* perm, int64_t n, int64_t* rank);
hipError_t launch_rank_to_row(const LaunchCfg& cfg, const int64_t* rank, const uint64_t* validity, const uint32_t* perm, int64_t n, uint32_t* idx);

}  // namespace bhip
