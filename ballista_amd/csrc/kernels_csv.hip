// kernels_csv.hip — general CSV text -> Arrow columns on the device: one-byte delimiter of the caller's choice, fields quoted
// with '"' ("" inside is one '"'; delimiter, '\r' and '\n' inside are data), records ended by '\n' or '\r\n' outside quotes, an
// empty field of a nullable column is NULL.  Stands where the reference has CsvExec with `has_header` / `delimiter` from the wire
// plan (rust/core/src/serde/physical_plan/from_proto.rs:93-110; `--format csv`, rust/benchmarks/tpch/src/main.rs:129-150).
//
// A '\n' ends a record only when the number of '"' before it is even, and that parity is a prefix property of the whole text:
//   1. count   per 16 KiB chunk: '"' count, and '\n' counts at even and at odd quote parity counted from the chunk's first byte.
//              A scan of the quote counts gives the parity each chunk starts in, which picks one of the two counters; a scan of
//              the picked counters gives each chunk's first record rank.
//   2. starts  the chunk staged in LDS, 64 consecutive bytes per thread as bit masks; the thread's parity is carried across the
//              wave by a ballot + masked popcount, across the waves through LDS; '\n' outside quotes are ranked and written.
//   3. parse   one thread per record, fields found quote-aware; validity, Boolean and ""-mark bits leave as one ballot word per
//              wave.
//   4. copy    Utf8 bytes behind an exclusive scan of the lengths, "" collapsed where marked (text_copy_strings_kernel,
//              kernels_tbl.hip).
// The value grammar is the `.tbl` scan's plus Boolean.  The LDS staging, the byte readers and the conversion of a fixed-width
// value (text_convert) are shared with that scan: text_device.h.  What two CSV readers would read differently (a '"' inside an
// unquoted field, bytes behind a closing quote, a bare '\r') raises CSV_ERR_STRAY_QUOTE: the caller keeps its CPU reader.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "csv_kernels.h"
#include "text_device.h"
#include "vm_device.h"
#include "vm_isa.h"

namespace bhip {

constexpr int CSV_WAVES = BLOCK / 64;
static_assert(TEXT_THREAD_BYTES == 64, "a thread's bytes are one 64-bit mask");

// bit b = byte b of `w` equals the byte replicated in `rep`.  Exact: 0x80 is left in every zero byte of x and in no other (the
// per-byte sum cannot carry into the next byte), and the multiply gathers the four bits without two of them meeting.
__device__ inline uint32_t eq_mask4(uint32_t w, uint32_t rep) {
    const uint32_t x = w ^ rep;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}
constexpr uint32_t REP_QUOTE = 0x22222222u, REP_NL = 0x0A0A0A0Au;

// lanes below this one whose bit is set in `ballot`
__device__ inline uint32_t lanes_below(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// pass 1.  Piece order is text order: (k, wave, lane).  A lane turns its 16 bytes into a quote mask and a newline mask; the prefix
// XOR of the quote mask is the parity at every byte, counted from the lane's first byte; the lanes before it in the wave (one
// ballot) flip it.  That leaves one pair of counters per 1 KiB segment, relative to the segment's start; thread 0 chains the 16
// segments of the chunk.
__global__ void __launch_bounds__(BLOCK)
csv_count_kernel(const uint8_t* text, int64_t n_bytes, uint32_t* quotes, uint32_t* newlines) {
    __shared__ uint32_t s_quotes, s_odd;
    __shared__ uint32_t s_seg[TEXT_PIECES * CSV_WAVES];           // even | odd << 16 (at most 1024 each)
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid < TEXT_PIECES * CSV_WAVES) s_seg[tid] = 0;
    if (tid == 0) { s_quotes = 0; s_odd = 0; }
    __syncthreads();
    const int64_t chunk0 = (int64_t)blockIdx.x * TBL_CHUNK;
    uint32_t nq = 0;
#pragma unroll
    for (int k = 0; k < TEXT_PIECES; ++k) {
        const uint4 v = load_piece(text, chunk0 + ((int64_t)k * BLOCK + tid) * 16, n_bytes);
        const uint32_t qm = eq_mask4(v.x, REP_QUOTE) | eq_mask4(v.y, REP_QUOTE) << 4 | eq_mask4(v.z, REP_QUOTE) << 8 | eq_mask4(v.w, REP_QUOTE) << 12;
        const uint32_t nm = eq_mask4(v.x, REP_NL) | eq_mask4(v.y, REP_NL) << 4 | eq_mask4(v.z, REP_NL) << 8 | eq_mask4(v.w, REP_NL) << 12;
        const uint32_t q = __popc(qm);
        nq += q;
        uint32_t pm = qm ^ (qm << 1);                            // bit b = parity of the quotes in bytes 0..b
        pm ^= pm << 2;
        pm ^= pm << 4;
        pm ^= pm << 8;
        const uint64_t odd = __ballot(q & 1u);
        if (lanes_below(odd) & 1u) pm = ~pm;
        const uint32_t c = __popc(nm & ~pm & 0xFFFFu) | __popc(nm & pm & 0xFFFFu) << 16;
        const int seg = k * CSV_WAVES + wave;
        if (c) atomicAdd(&s_seg[seg], c);
        if ((tid & 63) == 0 && (__popcll(odd) & 1)) atomicOr(&s_odd, 1u << seg);
    }
    if (nq) atomicAdd(&s_quotes, nq);
    __syncthreads();
    if (tid == 0) {
        uint32_t even = 0, odd = 0, parity = 0;
        for (int s = 0; s < TEXT_PIECES * CSV_WAVES; ++s) {
            const uint32_t a = s_seg[s] & 0xFFFFu, b = s_seg[s] >> 16;
            even += parity ? b : a;
            odd += parity ? a : b;
            parity ^= (s_odd >> s) & 1u;
        }
        quotes[blockIdx.x] = s_quotes;
        newlines[2 * (int64_t)blockIdx.x] = even;
        newlines[2 * (int64_t)blockIdx.x + 1] = odd;
    }
}

__global__ void __launch_bounds__(BLOCK)
csv_pick_kernel(const uint64_t* quotes_before, const uint32_t* newlines, int64_t n_chunks, uint32_t* records) {
    const int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (c < n_chunks) records[c] = newlines[2 * c + (int64_t)(quotes_before[c] & 1u)];
}

// pass 2: the staging of tbl_starts_kernel (stage_chunk_rows); a thread's 64 bytes become a quote mask and a newline mask, and
// the parity it starts in is
//   chunk (scan of pass 1) ^ waves before it (LDS) ^ lanes before it (ballot + masked popcount).
__global__ void __launch_bounds__(BLOCK)
csv_starts_kernel(const uint8_t* text, int64_t n_bytes, const uint64_t* quotes_before, const uint64_t* chunk_base, uint64_t* starts) {
    __shared__ uint32_t s_text[BLOCK * 17];
    __shared__ uint32_t s_scan[BLOCK];
    __shared__ uint32_t s_wave_odd[CSV_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t chunk0 = (int64_t)blockIdx.x * TBL_CHUNK;
    stage_chunk_rows(s_text, tid, text, chunk0, n_bytes);
    __syncthreads();
    uint64_t qm = 0, nm = 0;
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const uint32_t w = s_text[tid * 17 + d];
        qm |= (uint64_t)eq_mask4(w, REP_QUOTE) << (4 * d);
        nm |= (uint64_t)eq_mask4(w, REP_NL) << (4 * d);
    }
    const uint64_t odd = __ballot(__popcll(qm) & 1);
    if ((tid & 63) == 0) s_wave_odd[wave] = (uint32_t)__popcll(odd) & 1u;
    uint64_t pm = qm ^ (qm << 1);                               // bit b = parity of the quotes in bytes 0..b of this thread
    pm ^= pm << 2;
    pm ^= pm << 4;
    pm ^= pm << 8;
    pm ^= pm << 16;
    pm ^= pm << 32;
    __syncthreads();
    uint32_t in = (uint32_t)(quotes_before[blockIdx.x] & 1u) ^ (lanes_below(odd) & 1u);
    for (int w = 0; w < wave; ++w) in ^= s_wave_odd[w];
    if (in) pm = ~pm;
    uint64_t ends = nm & ~pm;                                   // '\n' outside quotes
    const uint32_t c = (uint32_t)__popcll(ends);
    const uint32_t before = block_rank_base(c, s_scan, tid);
    if (c == 0) return;
    uint64_t rank = chunk_base[blockIdx.x] + before;
    const int64_t base = chunk0 + (int64_t)tid * TEXT_THREAD_BYTES;
    while (ends) {
        const int b = __ffsll((unsigned long long)ends) - 1;
        starts[++rank] = (uint64_t)(base + b) + 1;
        ends &= ends - 1;
    }
}

// a non-empty Boolean value [a, b): "true" / "false" in any letter case.  The value comes back in `truth` and leaves as a ballot bit.
template <class R>
__device__ inline uint32_t csv_convert_bool(const R& rd, int64_t a, int64_t b, bool& truth) {
    const char* word = (b - a) == 4 ? "true" : "false";
    bool ok = (b - a) == 4 || (b - a) == 5;
    for (int k = 0; ok && k < (int)(b - a); ++k) ok = (rd(a + k) | 0x20) == (uint8_t)word[k];
    truth = ok && (b - a) == 4;
    return ok ? 0u : (uint32_t)TBL_ERR_BAD_VALUE;
}

// one record [p, e) per lane.  Every lane of the wave walks all the fields, with or without a record (`active`), because the bits
// of a column leave as one ballot word per wave: `word` is the wave's word in every bitmap, or -1 when the wave has no record.
template <bool QUOTED, class R>
__device__ inline uint32_t csv_parse_record(const R& rd, bool active, int64_t p, int64_t e, int64_t i, int64_t word, const TextPlan& plan,
                                            uint32_t& null_slots) {
    uint32_t err = 0;
    const bool writer = (threadIdx.x & 63) == 0 && word >= 0;
    const uint8_t delim = (uint8_t)plan.delimiter;
    if (active) {
        if (e > p && rd(e - 1) == '\r') --e;
        if (e <= p) { err |= TBL_ERR_BLANK_LINE; active = false; }
    }
    for (int f = 0; f < plan.n_fields; ++f) {
        if (active && p > e) { err |= TBL_ERR_MISSING_FIELD; active = false; }
        int64_t a = p, b = p;                            // content of the field
        uint32_t pairs = 0;                              // "" inside it
        if (active) {
            if (QUOTED && p < e && rd(p) == '"') {
                int64_t q = p + 1;
                bool closed = false;
                while (q < e) {
                    if (rd(q) != '"') { ++q; continue; }
                    if (q + 1 < e && rd(q + 1) == '"') { ++pairs; q += 2; continue; }
                    closed = true;
                    break;
                }
                a = p + 1;
                b = q;
                if (!closed) { err |= CSV_ERR_STRAY_QUOTE; b = a; active = false; }
                else if (q + 1 < e && rd(q + 1) != delim) { err |= CSV_ERR_STRAY_QUOTE; active = false; }
                p = q + 2;                               // behind the closing quote and the delimiter (or the record's end)
            } else {
                int64_t q = p;
                for (; q < e; ++q) {
                    const uint8_t ch = rd(q);
                    if (ch == delim) break;
                    if ((QUOTED && ch == '"') || ch == '\r') err |= CSV_ERR_STRAY_QUOTE;
                }
                b = q;
                p = q + 1;
            }
        }
        const int out = plan.out[f];
        if (out < 0) continue;
        const int dt = plan.dtype[f];
        if (dt == DT_UTF8) {
            if (active) {
                plan.str_start[out][i] = (uint32_t)a;
                plan.str_len[out][i] = (uint32_t)(b - a) - pairs;
            }
            if (QUOTED) {
                const uint64_t marks = __ballot(active && pairs != 0);
                if (writer) plan.str_esc[out][word] = marks;
            }
            continue;
        }
        bool valid = false, truth = false;
        if (active) {
            if (b == a) {
                if (!plan.nullable[f]) err |= CSV_ERR_NULL;
                if (dt == DT_FLOAT64 || dt == DT_INT64) reinterpret_cast<uint64_t*>(plan.data[out])[i] = 0;
                else if (dt != DT_BOOLEAN) reinterpret_cast<uint32_t*>(plan.data[out])[i] = 0;
            } else {
                valid = true;
                if (pairs) err |= TBL_ERR_BAD_VALUE;
                // a constant type per call, so one instance of the conversion per type: 0.16 ms per GiB of text faster than one
                // call with `dt` passed through (profiles/text_convert_shared.txt).  The host admits no other type.
                switch (dt) {
                    case DT_BOOLEAN: err |= csv_convert_bool(rd, a, b, truth); break;
                    case DT_DATE32: err |= text_convert(rd, a, b, DT_DATE32, plan.data[out], i); break;
                    case DT_FLOAT64: err |= text_convert(rd, a, b, DT_FLOAT64, plan.data[out], i); break;
                    case DT_INT64: err |= text_convert(rd, a, b, DT_INT64, plan.data[out], i); break;
                    default: err |= text_convert(rd, a, b, DT_INT32, plan.data[out], i); break;
                }
            }
        }
        if (plan.validity[out]) {
            const uint64_t bits = __ballot(valid);
            if (__ballot(active && !valid)) null_slots |= 1u << out;
            if (writer) plan.validity[out][word] = bits;
        }
        if (dt == DT_BOOLEAN) {
            const uint64_t bits = __ballot(truth);
            if (writer) reinterpret_cast<uint64_t*>(plan.data[out])[word] = bits;
        }
    }
    return err;
}

// pass 3: a workgroup takes 256 consecutive records and walks them in LDS (stage_span), or in HBM when they do not fit.
// Record i0 is a multiple of 256, so wave w of the workgroup owns bitmap word i0 / 64 + w of every column.
template <bool QUOTED>
__global__ void __launch_bounds__(BLOCK)
csv_parse_kernel(const uint8_t* text, const uint64_t* starts, int64_t n_records, int64_t n_bytes, TextPlan plan, uint32_t* flags) {
    __shared__ __align__(16) uint8_t s_buf[TEXT_STAGE];
    uint32_t err = 0, null_slots = 0;
    const int tid = threadIdx.x;
    for (int64_t i0 = (int64_t)blockIdx.x * BLOCK; i0 < n_records; i0 += (int64_t)gridDim.x * BLOCK) {
        const int64_t n_here = n_records - i0 < BLOCK ? n_records - i0 : BLOCK;
        int64_t span0;
        const bool staged = stage_span(s_buf, tid, text, starts, i0, n_here, n_bytes, span0);
        __syncthreads();
        const bool active = tid < n_here;
        const int64_t i = i0 + tid;
        const int64_t p = active ? (int64_t)starts[i] : 0;
        const int64_t e = active ? (int64_t)starts[i + 1] - 1 : 0;     // the newline (or one past the text for an unterminated last record)
        const int64_t word = (tid & ~63) < n_here ? (i0 + (tid & ~63)) >> 6 : -1;
        if (staged) err |= csv_parse_record<QUOTED>(TextLdsReader{s_buf, span0}, active, p, e, i, word, plan, null_slots);
        else err |= csv_parse_record<QUOTED>(TextGlobalReader{text}, active, p, e, i, word, plan, null_slots);
        __syncthreads();
    }
    if (err) atomicOr(flags, err);
    if (null_slots && (tid & 63) == 0) atomicOr(flags + 1, null_slots);
}

hipError_t launch_csv_count(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, uint32_t* quotes, uint32_t* newlines) {
    const int64_t n_chunks = (n_bytes + TBL_CHUNK - 1) / TBL_CHUNK;
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(csv_count_kernel, dim3((unsigned)n_chunks), dim3(BLOCK), 0, cfg.stream, text, n_bytes, quotes, newlines);
    return hipGetLastError();
}
hipError_t launch_csv_pick(const LaunchCfg& cfg, const uint64_t* quotes_before, const uint32_t* newlines, int64_t n_chunks, uint32_t* records) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(csv_pick_kernel, dim3((unsigned)((n_chunks + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, cfg.stream, quotes_before, newlines,
                       n_chunks, records);
    return hipGetLastError();
}
hipError_t launch_csv_starts(const LaunchCfg& cfg, const uint8_t* text, int64_t n_bytes, const uint64_t* quotes_before,
                             const uint64_t* chunk_base, uint64_t* starts) {
    const int64_t n_chunks = (n_bytes + TBL_CHUNK - 1) / TBL_CHUNK;
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(csv_starts_kernel, dim3((unsigned)n_chunks), dim3(BLOCK), 0, cfg.stream, text, n_bytes, quotes_before, chunk_base, starts);
    return hipGetLastError();
}
hipError_t launch_csv_parse(const LaunchCfg& cfg, const uint8_t* text, const uint64_t* starts, int64_t n_records, int64_t n_bytes,
                            const TextPlan& plan, bool quoted, uint32_t* flags) {
    if (n_records == 0) return hipSuccess;
    const dim3 grid(grid_rows(cfg, n_records));
    if (quoted) hipLaunchKernelGGL(csv_parse_kernel<true>, grid, dim3(BLOCK), 0, cfg.stream, text, starts, n_records, n_bytes, plan, flags);
    else hipLaunchKernelGGL(csv_parse_kernel<false>, grid, dim3(BLOCK), 0, cfg.stream, text, starts, n_records, n_bytes, plan, flags);
    return hipGetLastError();
}

}  // namespace bhip
