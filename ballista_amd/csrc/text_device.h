// text_device.h — what the `.tbl` scan (kernels_tbl.hip) and the CSV scan (kernels_csv.hip) have in common on the device, once:
// the staging of a chunk and of a span of records in LDS, the byte readers of the field walk, the date and power-of-ten helpers of
// the value grammar.  The count, starts, record-walk and copy kernels are each format's own, and so is, for now, the conversion
// of a fixed-width value (see tbl_parse_line in kernels_tbl.hip).
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

// days_from_civil: cast_text.h (the host folds date literals with the same function)

static __constant__ double TEXT_POW10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                                             1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// workgroups of a pass with one thread per row
static inline int grid_rows(const LaunchCfg& cfg, int64_t n) {
    int64_t g = (n + BLOCK - 1) / BLOCK;
    const int64_t cap = (int64_t)cfg.device_cus * 16;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace bhip
