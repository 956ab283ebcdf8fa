// kernels_tbl.hip — TPC-H `.tbl` text (dbgen: '|'-separated fields, '|' before the newline) -> Arrow columns on the
// device.  Stands where the reference's scan leaf stands: CsvExec with delimiter '|', no header, explicit schema
// (rust/benchmarks/tpch/src/main.rs:129-150, schemas :267-360; rust/core/src/serde/physical_plan/from_proto.rs:93-110).
// with `--format tbl` the CPU spends its time here, upstream of every operator.
//
// Byte work, three passes over the text:
//   1. newlines per 16 KiB chunk                          (count)  -> exclusive scan
//   2. start offset of every line                          (stable ranks inside a chunk: thread-local counts + LDS scan)
//   3. one thread per line walks its fields; projected fields are converted in place (text_convert), a Utf8 field leaves as
//      (offset, length); a second pass copies the bytes behind an exclusive scan of the lengths
// The LDS staging, the byte readers and the conversion with its grammar are shared with the CSV scan: text_device.h.
// Anything else in the text (exponents, > 15 significant digits, missing fields, blank lines) raises a flag and the
// host reports BHIP_EEXEC / BHIP_ENOTIMPL: the caller keeps its CPU reader for that file.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "tbl_kernels.h"
#include "text_device.h"
#include "vm_device.h"
#include "vm_isa.h"

namespace bhip {

// newlines among the four bytes of `w` (byte by byte: the subtract-and-mask zero-byte trick can flag a 0x0B byte that
// sits right above a newline, and these counts must equal the line count exactly)
__device__ inline uint32_t newlines_exact(uint32_t w) {
    uint32_t c = 0;
    c += (w & 0xFFu) == 0x0Au;
    c += ((w >> 8) & 0xFFu) == 0x0Au;
    c += ((w >> 16) & 0xFFu) == 0x0Au;
    c += (w >> 24) == 0x0Au;
    return c;
}

// pass 1: newlines per chunk.  Lanes read adjacent 16-byte pieces (coalesced), order does not matter for a count.
__global__ void __launch_bounds__(BLOCK)
tbl_count_kernel(const uint8_t* text, int64_t n_bytes, uint32_t* chunk_lines) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int64_t chunk0 = (int64_t)blockIdx.x * TBL_CHUNK;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < TBL_CHUNK / (BLOCK * 16); ++k) {
        const int64_t p = chunk0 + ((int64_t)k * BLOCK + threadIdx.x) * 16;
        if (p + 16 <= n_bytes) {
            const uint4 v = *reinterpret_cast<const uint4*>(text + p);            // text is 256-byte aligned, p a multiple of 16
            c += newlines_exact(v.x) + newlines_exact(v.y) + newlines_exact(v.z) + newlines_exact(v.w);
        } else {
            for (int64_t q = p; q < n_bytes && q < p + 16; ++q) c += text[q] == '\n';
        }
    }
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) chunk_lines[blockIdx.x] = s_cnt;
}

// pass 2: starts[i] = offset of the first byte of line i (starts[0] = 0 is written by the host).  The chunk is staged
// in LDS (stage_chunk_rows); each thread then owns 64 CONSECUTIVE bytes, which keeps the newline ranks in text order.
__global__ void __launch_bounds__(BLOCK)
tbl_starts_kernel(const uint8_t* text, int64_t n_bytes, const uint64_t* chunk_base, uint64_t* starts) {
    __shared__ uint32_t s_text[BLOCK * 17];
    __shared__ uint32_t s_scan[BLOCK];
    const int tid = threadIdx.x;
    const int64_t chunk0 = (int64_t)blockIdx.x * TBL_CHUNK;
    stage_chunk_rows(s_text, tid, text, chunk0, n_bytes);          // bytes past the text read as 0: never a newline
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (int d = 0; d < 16; ++d) c += newlines_exact(s_text[tid * 17 + d]);
    const uint32_t before = block_rank_base(c, s_scan, tid);
    if (c == 0) return;
    uint64_t rank = chunk_base[blockIdx.x] + before;
    const int64_t base = chunk0 + (int64_t)tid * TEXT_THREAD_BYTES;
    for (int d = 0; d < 16; ++d) {
        const uint32_t w = s_text[tid * 17 + d];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (((w >> (8 * b)) & 0xFFu) == 0x0Au) starts[++rank] = (uint64_t)(base + d * 4 + b) + 1;
    }
}

// one line [p, e): walk the fields, convert the projected ones.  Returns the error flags.
template <class R>
__device__ inline uint32_t tbl_parse_line(const R& rd, int64_t p, int64_t e, int64_t i, const TextPlan& plan) {
    uint32_t err = 0;
    if (e > p && rd(e - 1) == '\r') --e;
    if (e <= p) return TBL_ERR_BLANK_LINE;
    for (int f = 0; f < plan.n_fields; ++f) {
        if (p > e) { err |= TBL_ERR_MISSING_FIELD; break; }
        int64_t q = p;
        while (q < e && rd(q) != '|') ++q;              // field = [p, q)
        const int out = plan.out[f];
        if (out >= 0) {
            const int dt = plan.dtype[f];
            if (dt == DT_UTF8) {
                plan.str_start[out][i] = (uint32_t)p;
                plan.str_len[out][i] = (uint32_t)(q - p);
            } else {
                err |= text_convert(rd, p, q, dt, plan.data[out], i);
            }
        }
        p = q + 1;
    }
    return err;
}

// pass 3: a workgroup takes 256 consecutive lines and walks them in LDS (stage_span), or in HBM when they do not fit.
__global__ void __launch_bounds__(BLOCK)
tbl_parse_kernel(const uint8_t* text, const uint64_t* starts, int64_t n_lines, int64_t n_bytes, TextPlan plan, uint32_t* flags) {
    __shared__ __align__(16) uint8_t s_buf[TEXT_STAGE];
    uint32_t err = 0;
    const int tid = threadIdx.x;
    for (int64_t i0 = (int64_t)blockIdx.x * BLOCK; i0 < n_lines; i0 += (int64_t)gridDim.x * BLOCK) {
        const int64_t n_here = n_lines - i0 < BLOCK ? n_lines - i0 : BLOCK;
        int64_t span0;
        const bool staged = stage_span(s_buf, tid, text, starts, i0, n_here, n_bytes, span0);
        __syncthreads();
        if (tid < n_here) {
            const int64_t i = i0 + tid;
            const int64_t p = (int64_t)starts[i];
            const int64_t e = (int64_t)starts[i + 1] - 1;       // the newline (or one past the text for an unterminated last line)
            if (staged) err |= tbl_parse_line(TextLdsReader{s_buf, span0}, p, e, i, plan);
            else err |= tbl_parse_line(TextGlobalReader{text}, p, e, i, plan);
        }
        __syncthreads();
    }
    if (err) atomicOr(flags, err);
}

// pass 4, both formats: one thread per row.  A set bit of str_esc (CSV; null: no row has any) marks a quoted field with "" pairs:
// every '"' inside it is the first of a pair, and the second is skipped.
__global__ void __launch_bounds__(BLOCK)
text_copy_strings_kernel(const uint8_t* text, const uint32_t* str_start, const uint32_t* str_len, const uint64_t* str_esc,
                         const int32_t* offsets, int64_t n, uint8_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const uint8_t* s = text + str_start[i];
        uint8_t* d = out + offsets[i];
        const uint32_t len = str_len[i];
        if (str_esc && ((str_esc[i >> 6] >> (i & 63)) & 1ull)) {
            for (uint32_t b = 0; b < len; ++b) {
                const uint8_t ch = *s;
                d[b] = ch;
                s += ch == '"' ? 2 : 1;
            }
        } else {
            for (uint32_t b = 0; b < len; ++b) d[b] = s[b];
        }
    }
}

hipError_t launch_tbl_count(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, uint32_t* chunk_lines) {
    const int64_t n_chunks = (n_bytes + TBL_CHUNK - 1) / TBL_CHUNK;
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(tbl_count_kernel, dim3((unsigned)n_chunks), dim3(BLOCK), 0, cfg.stream, text, n_bytes, chunk_lines);
    return hipGetLastError();
}
hipError_t launch_tbl_starts(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, const uint64_t* chunk_base, uint64_t* starts) {
    const int64_t n_chunks = (n_bytes + TBL_CHUNK - 1) / TBL_CHUNK;
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(tbl_starts_kernel, dim3((unsigned)n_chunks), dim3(BLOCK), 0, cfg.stream, text, n_bytes, chunk_base, starts);
    return hipGetLastError();
}
hipError_t launch_tbl_parse(const LaunchCfg& cfg, const uint8_t* text, const uint64_t* starts, int64_t n_lines, int64_t n_bytes,
                            const TextPlan& plan, uint32_t* flags) {
    if (n_lines == 0) return hipSuccess;
    hipLaunchKernelGGL(tbl_parse_kernel, dim3(grid_rows(cfg, n_lines)), dim3(BLOCK), 0, cfg.stream, text, starts, n_lines, n_bytes, plan,
                       flags);
    return hipGetLastError();
}
hipError_t launch_text_copy_strings(const LaunchCfg& cfg, const uint8_t* text, const uint32_t* str_start, const uint32_t* str_len,
                                    const uint64_t* str_esc, const int32_t* offsets, int64_t n, uint8_t* out) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(text_copy_strings_kernel, dim3(grid_rows(cfg, n)), dim3(BLOCK), 0, cfg.stream, text, str_start, str_len, str_esc,
                       offsets, n, out);
    return hipGetLastError();
}

}  // namespace bhip
