// text_device.h — what the `.tbl` scan (kernels_tbl.hip) and the CSV scan (kernels_csv.hip) have in common on the device, once:
// the staging of a chunk and of a span of records in LDS, the rank scan of the starts passes, the byte readers of the field walk
// and the conversion of a fixed-width value (text_convert).  The count, starts and record-walk kernels are each format's own; the
// string copy is one kernel for both (kernels_tbl.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cast_text.h"
#include "kernels.h"
#include "tbl_kernels.h"
#include "vm_device.h"
#include "vm_isa.h"

namespace bhip {

constexpr int TEXT_THREAD_BYTES = TBL_CHUNK / BLOCK;      // 64 consecutive bytes per thread and chunk in the starts passes
constexpr int TEXT_PIECES = TBL_CHUNK / (BLOCK * 16);     // 16-byte pieces per thread in the coalesced passes
constexpr int TEXT_STAGE = 48 * 1024;                     // LDS bytes for the records of one workgroup in the parse passes

// 16 bytes at p as four dwords; bytes at and behind n_bytes read as 0: neither a quote nor a newline
__device__ inline uint4 load_piece(const uint8_t* text, int64_t p, int64_t n_bytes) {
    if (p + 16 <= n_bytes) return *reinterpret_cast<const uint4*>(text + p);        // text is 256-byte aligned, p a multiple of 16
    uint32_t w[4] = {0, 0, 0, 0};
    for (int64_t q = p; q < n_bytes && q < p + 16; ++q) w[(q - p) >> 2] |= (uint32_t)text[q] << (8 * ((q - p) & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// starts passes: the chunk at chunk0 into s_text[BLOCK * 17] with coalesced 16-byte loads.  Thread t then owns the 64 CONSECUTIVE
// bytes of row t: rows of 16 dwords padded to 17, so the 64 lanes of a wave read 64 different banks.  The caller synchronises.
__device__ inline void stage_chunk_rows(uint32_t* s_text, int tid, const uint8_t* text, int64_t chunk0, int64_t n_bytes) {
#pragma unroll
    for (int k = 0; k < TEXT_PIECES; ++k) {
        const int piece = k * BLOCK + tid;               // 16-byte piece of the chunk
        const uint4 v = load_piece(text, chunk0 + (int64_t)piece * 16, n_bytes);
        const int row = piece >> 2, col = (piece & 3) * 4;       // row = owning thread (64 bytes = 4 pieces)
        s_text[row * 17 + col + 0] = v.x; s_text[row * 17 + col + 1] = v.y;
        s_text[row * 17 + col + 2] = v.z; s_text[row * 17 + col + 3] = v.w;
    }
}

// parse passes: the text of records [i0, i0 + n_here) is one contiguous span.  It goes into s_buf[TEXT_STAGE] with coalesced
// 16-byte loads from span0 (16-byte aligned: the text buffer is) and every thread then walks its own record in LDS (a thread
// walking byte by byte in HBM issues one dependent load per byte); false: the span does not fit (very long records) and is walked
// in HBM.  The caller synchronises.
__device__ inline bool stage_span(uint8_t* s_buf, int tid, const uint8_t* text, const uint64_t* starts, int64_t i0, int64_t n_here,
                                  int64_t n_bytes, int64_t& span0) {
    span0 = (int64_t)starts[i0] & ~(int64_t)15;
    int64_t span1 = (int64_t)starts[i0 + n_here];
    if (span1 > n_bytes) span1 = n_bytes;
    const bool staged = span1 - span0 <= TEXT_STAGE - 16;      // the copy below moves whole 16-byte pieces
    if (staged) {
        for (int64_t k = (int64_t)tid * 16; k < span1 - span0; k += BLOCK * 16) {
            const int64_t g = span0 + k;
            if (g + 16 <= n_bytes) *reinterpret_cast<uint4*>(s_buf + k) = *reinterpret_cast<const uint4*>(text + g);
            else
                for (int64_t b = g; b < n_bytes; ++b) s_buf[b - span0] = text[b];
        }
    }
    return staged;
}

// byte sources of the field walk: the text in HBM, or the records of one workgroup staged in LDS
struct TextGlobalReader {
    const uint8_t* text;
    __device__ uint8_t operator()(int64_t pos) const { return text[pos]; }
};
struct TextLdsReader {
    const uint8_t* buf;          // LDS copy of text[origin, origin + ...)
    int64_t origin;
    __device__ uint8_t operator()(int64_t pos) const { return buf[pos - origin]; }
};

// starts passes: inclusive Hillis-Steele scan of the per-thread counts `c` in s_scan[BLOCK]; returns the count of the threads before
// this one.  Every thread of the workgroup calls it.
__device__ inline uint32_t block_rank_base(uint32_t c, uint32_t* s_scan, int tid) {
    s_scan[tid] = c;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {
        const uint32_t v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    return s_scan[tid] - c;
}

// the value [a, b) of a fixed-width column -> row i of `data`; returns the TBL_ERR_* bits.  The grammar of both scans:
//   Int32 / Int64   [-]digits
//   Float64         [-]digits[.digits]  =  M / 10^k with M < 2^53 and k <= 22: both exact in double, so the one
//                   division is the correctly rounded value of the decimal text (what str::parse::<f64> returns)
//   Date32          YYYY-MM-DD -> days since 1970-01-01 (proleptic Gregorian; days_from_civil is cast_text.h's, the host folds
//                   date literals with it)
// A '+' is read like no sign.  An empty value is TBL_ERR_BAD_VALUE.  A value is stored even when a flag is raised: 0 days, +-0.0
// or the wrapped integer.
template <class R>
__device__ inline uint32_t text_convert(const R& rd, int64_t a, int64_t b, int dt, void* data, int64_t i) {
    uint32_t err = 0;
    if (dt == DT_DATE32) {
        bool ok = (b - a) == 10 && rd(a + 4) == '-' && rd(a + 7) == '-';
        int v[8];
        const int pos[8] = {0, 1, 2, 3, 5, 6, 8, 9};
        for (int k = 0; k < 8 && ok; ++k) {
            const int c = (int)rd(a + pos[k]) - '0';
            ok = c >= 0 && c <= 9;
            v[k] = c;
        }
        int32_t days = 0;
        if (ok) {
            const int y = v[0] * 1000 + v[1] * 100 + v[2] * 10 + v[3], m = v[4] * 10 + v[5], d = v[6] * 10 + v[7];
            ok = m >= 1 && m <= 12 && d >= 1 && d <= 31;
            days = (int32_t)days_from_civil(y, (unsigned)m, (unsigned)d);
        }
        if (!ok) err |= TBL_ERR_BAD_VALUE;
        reinterpret_cast<int32_t*>(data)[i] = days;
        return err;
    }
    int64_t r = a;
    bool neg = false;
    if (r < b && (rd(r) == '-' || rd(r) == '+')) { neg = rd(r) == '-'; ++r; }
    uint64_t m = 0;
    int digits = 0, frac = 0;
    bool seen_dot = false, ok = r < b;
    for (; r < b; ++r) {
        const uint8_t ch = rd(r);
        if (ch >= '0' && ch <= '9') {
            if (digits >= 19) {                                  // 19 digits still fit 64 bits
                if (dt == DT_FLOAT64) { err |= TBL_ERR_PRECISION; m = 0; frac = 0; r = b; break; }
                ok = false;
                break;
            }
            m = m * 10 + (uint64_t)(ch - '0');
            if (m != 0 || seen_dot) ++digits;             // leading zeros of the integer part are free
            if (seen_dot) ++frac;
        } else if (ch == '.' && !seen_dot && dt == DT_FLOAT64) {
            seen_dot = true;
        } else { ok = false; break; }
    }
    if (dt == DT_FLOAT64) {
        if (!ok) err |= TBL_ERR_BAD_VALUE;
        else if (m >= (1ull << 53) || frac > 22) { err |= TBL_ERR_PRECISION; ok = false; }
        const double v = ok ? (double)m / cast_pow10(frac) : 0.0;
        reinterpret_cast<double*>(data)[i] = neg ? -v : v;
    } else {
        if (!ok || seen_dot) err |= TBL_ERR_BAD_VALUE;
        if (m > (neg ? (1ull << 63) : (1ull << 63) - 1ull)) err |= TBL_ERR_BAD_VALUE;      // beyond Int64
        const int64_t v = neg ? (int64_t)(0ull - m) : (int64_t)m;
        if (dt == DT_INT32) {
            if (v > 2147483647ll || v < -2147483648ll) err |= TBL_ERR_BAD_VALUE;
            reinterpret_cast<int32_t*>(data)[i] = (int32_t)v;
        } else {
            reinterpret_cast<int64_t*>(data)[i] = v;
        }
    }
    return err;
}

// workgroups of a pass with one thread per row
static inline int grid_rows(const LaunchCfg& cfg, int64_t n) {
    int64_t g = (n + BLOCK - 1) / BLOCK;
    const int64_t cap = (int64_t)cfg.device_cus * 16;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace bhip
