// kernels_window.hip — WindowAggExec on the device (host/ops_window.cpp; declarations and the tile constants: window_kernels.h).
//
// The input is already in (partition keys, order keys) order.  Every kernel is one row per lane over 4-byte and 8-byte streams,
// lane i of a wave at row base + i (coalesced loads and stores), wave64:
//   window_flags_kernel                  rows i - 1 and i compared on the key columns -> "starts a partition" / "starts a peer group"
//   window_{tiles,summaries,apply}       ONE three-launch inclusive scan, instantiated for the partition / peer bounds (forward max +
//                                        sum, backward min) and for the segmented scans of an argument (add, min, max)
//   window_rank / window_index           ROW_NUMBER, RANK, DENSE_RANK; the row LAG / LEAD / FIRST_VALUE / LAST_VALUE gather from
//   window_finish                        the running state at the frame's last row -> the output column and its validity
//   window_frame_bounds / _finish_frame  sliding ROWS frames: every row's (lo, hi); the finish over it (a difference for COUNT and integer SUM)
//   window_slide                         the aggregate of a frame with two finite ends, out of a tile's neighbourhood staged in LDS
//   window_value_bounds                  RANGE / GROUPS frames: every row's (lo, hi) by a gallop-and-bisect search of the order key / peer count
//   window_slide_value                   window_slide for those (lo, hi): the tile's span comes from the data (LDS when it fits, else global)
//
// The scan: a tile is WINDOW_TILE_ROWS rows = WINDOW_ROUNDS rounds of one row per thread.  Inside a round the scan is scan_device.h's
// block_scan_inclusive over the policies below (wave-level shuffles, the four wave totals cross through LDS).  Launch 1 leaves one summary per
// tile, launch 2 (one workgroup) scans the summaries WINDOW_SUMMARY_STEP at a time with a running carry, launch 3 redoes the
// tile-local scan with the summary of the tiles before it as carry.  Nothing waits on another workgroup.  The combine tree is a
// function of the row positions alone (not of the grid or the device), so floating-point sums are reproducible bit for bit.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "window_kernels.h"
#include "scan_device.h"

namespace bhip {

namespace {

__device__ inline bool bit_at(const uint64_t* words, int64_t i) { return (words[i >> 6] >> (i & 63)) & 1; }

// =============================================================================================
// boundary flags
// =============================================================================================
// rows a and b of one key column are the same key: validity first (NULL equals NULL, whatever lies under it), then the bits
__device__ inline bool key_equal(const ColumnRef& c, int64_t a, int64_t b) {
    if (c.validity) {
        const bool va = bit_at(c.validity, a), vb = bit_at(c.validity, b);
        if (va != vb) return false;
        if (!va) return true;
    }
    if (c.dtype == DT_UTF8) {
        const int32_t a0 = c.offsets[a], a1 = c.offsets[a + 1], b0 = c.offsets[b], b1 = c.offsets[b + 1];
        if (a1 - a0 != b1 - b0) return false;
        const uint8_t* bytes = static_cast<const uint8_t*>(c.data);
        for (int32_t k = 0; k < a1 - a0; ++k)
            if (bytes[a0 + k] != bytes[b0 + k]) return false;
        return true;
    }
    if (c.dtype == DT_BOOLEAN) return bit_at(static_cast<const uint64_t*>(c.data), a) == bit_at(static_cast<const uint64_t*>(c.data), b);
    switch (dt_width(c.dtype)) {
        case 1: return static_cast<const uint8_t*>(c.data)[a] == static_cast<const uint8_t*>(c.data)[b];
        case 2: return static_cast<const uint16_t*>(c.data)[a] == static_cast<const uint16_t*>(c.data)[b];
        case 4: return static_cast<const uint32_t*>(c.data)[a] == static_cast<const uint32_t*>(c.data)[b];       // floats: by bit pattern
        default: return static_cast<const uint64_t*>(c.data)[a] == static_cast<const uint64_t*>(c.data)[b];
    }
}

__global__ void __launch_bounds__(WINDOW_BLOCK)
window_flags_kernel(WindowKeys K, int64_t n, uint64_t* __restrict__ part_flags, uint64_t* __restrict__ peer_flags) {
    const int64_t i = (int64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    bool part = false, peer = false;
    if (i < n) {
        part = i == 0;
        for (int k = 0; k < K.n_part && !part; ++k) part = !key_equal(K.col[k], i - 1, i);
        peer = part;
        for (int k = 0; k < K.n_order && !peer; ++k) peer = !key_equal(K.col[K.n_part + k], i - 1, i);
    }
    // a wave covers 64 consecutive rows starting at a multiple of 64: one word of each bitmap
    const uint64_t part_word = __ballot(part), peer_word = __ballot(peer);
    if ((threadIdx.x & 63) == 0 && i < n) {
        part_flags[i >> 6] = part_word;
        peer_flags[i >> 6] = peer_word;
    }
}

// =============================================================================================
// the three-launch inclusive scan over a policy P: what scan_device.h asks of one (P::State, P::identity(), P::combine(left, right),
//   P::shfl_up(state, d)) and p.load(position), p.store(position, state)
// positions run 0 .. n in SCAN order (the backward policy maps them to rows from the right)
// =============================================================================================
template <class P>
__global__ void __launch_bounds__(WINDOW_BLOCK)
window_tiles_kernel(P p, int64_t n, typename P::State* __restrict__ summaries) {
    using S = typename P::State;
    __shared__ S s_wave[WINDOW_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * WINDOW_TILE_ROWS;
    S carry = P::identity();
#pragma unroll
    for (int r = 0; r < WINDOW_ROUNDS; ++r) {
        const int64_t pos = base + r * WINDOW_BLOCK + threadIdx.x;
        S total;
        block_scan_inclusive<P, WINDOW_BLOCK / 64>(pos < n ? p.load(pos, n) : P::identity(), s_wave, total);
        carry = P::combine(carry, total);
    }
    if (threadIdx.x == 0) summaries[blockIdx.x] = carry;
}

// one workgroup, in place: summaries[t] = combine(summaries[0 .. t])
template <class P>
__global__ void __launch_bounds__(WINDOW_BLOCK)
window_summaries_kernel(typename P::State* summaries, int64_t n_tiles) {
    using S = typename P::State;
    static_assert(WINDOW_SUMMARY_STEP == WINDOW_BLOCK, "one summary per thread and step");
    __shared__ S s_wave[WINDOW_BLOCK / 64];
    S carry = P::identity();
    for (int64_t b = 0; b < n_tiles; b += WINDOW_SUMMARY_STEP) {
        const int64_t t = b + threadIdx.x;
        S total;
        const S incl = block_scan_inclusive<P, WINDOW_BLOCK / 64>(t < n_tiles ? summaries[t] : P::identity(), s_wave, total);
        if (t < n_tiles) summaries[t] = P::combine(carry, incl);
        carry = P::combine(carry, total);
    }
}

template <class P>
__global__ void __launch_bounds__(WINDOW_BLOCK)
window_apply_kernel(P p, int64_t n, const typename P::State* __restrict__ summaries) {
    using S = typename P::State;
    __shared__ S s_wave[WINDOW_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * WINDOW_TILE_ROWS;
    S carry = blockIdx.x > 0 ? summaries[blockIdx.x - 1] : P::identity();
#pragma unroll
    for (int r = 0; r < WINDOW_ROUNDS; ++r) {
        const int64_t pos = base + r * WINDOW_BLOCK + threadIdx.x;
        S total;
        const S incl = block_scan_inclusive<P, WINDOW_BLOCK / 64>(pos < n ? p.load(pos, n) : P::identity(), s_wave, total);
        if (pos < n) p.store(pos, n, P::combine(carry, incl));
        carry = P::combine(carry, total);
    }
}

// ---- partition / peer bounds -------------------------------------------------------------------------------------------------
struct ForwardBounds {
    struct State { uint32_t part_start, peer_start, peers; };
    const uint64_t* part_flags;
    const uint64_t* peer_flags;
    uint32_t* part_start;
    uint32_t* peer_start;
    uint32_t* peers_to;
    __device__ static State identity() { return State{0u, 0u, 0u}; }
    __device__ static State combine(const State& a, const State& b) {
        return State{a.part_start > b.part_start ? a.part_start : b.part_start, a.peer_start > b.peer_start ? a.peer_start : b.peer_start,
                     a.peers + b.peers};
    }
    __device__ static State shfl_up(const State& x, int d) {
        return State{__shfl_up(x.part_start, d, 64), __shfl_up(x.peer_start, d, 64), __shfl_up(x.peers, d, 64)};
    }
    __device__ State load(int64_t i, int64_t) const {
        const bool part = bit_at(part_flags, i), peer = bit_at(peer_flags, i);
        return State{part ? (uint32_t)i : 0u, peer ? (uint32_t)i : 0u, peer ? 1u : 0u};
    }
    __device__ void store(int64_t i, int64_t, const State& s) const {
        part_start[i] = s.part_start;
        peer_start[i] = s.peer_start;
        peers_to[i] = s.peers;
    }
};

// scan position p is row n - 1 - p: the last row of a segment is the row before the next head (or row n - 1)
struct BackwardBounds {
    struct State { uint32_t part_end, peer_end; };
    const uint64_t* part_flags;
    const uint64_t* peer_flags;
    uint32_t* part_end;
    uint32_t* peer_end;
    __device__ static State identity() { return State{0xFFFFFFFFu, 0xFFFFFFFFu}; }
    __device__ static State combine(const State& a, const State& b) {
        return State{a.part_end < b.part_end ? a.part_end : b.part_end, a.peer_end < b.peer_end ? a.peer_end : b.peer_end};
    }
    __device__ static State shfl_up(const State& x, int d) { return State{__shfl_up(x.part_end, d, 64), __shfl_up(x.peer_end, d, 64)}; }
    __device__ State load(int64_t p, int64_t n) const {
        const int64_t i = n - 1 - p;
        const bool last_of_part = i == n - 1 || bit_at(part_flags, i + 1), last_of_peers = i == n - 1 || bit_at(peer_flags, i + 1);
        return State{last_of_part ? (uint32_t)i : 0xFFFFFFFFu, last_of_peers ? (uint32_t)i : 0xFFFFFFFFu};
    }
    __device__ void store(int64_t p, int64_t n, const State& s) const {
        const int64_t i = n - 1 - p;
        part_end[i] = s.part_end;
        peer_end[i] = s.peer_end;
    }
};

// ---- segmented scan of an argument ---------------------------------------------------------------------------------------------------
constexpr uint32_t ARG_HEAD = 1, ARG_HAS_NUMBER = 2, ARG_SAW_NAN = 4;
constexpr uint64_t F64_QUIET_NAN = 0x7FF8000000000000ull;

__device__ inline double f64_of(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ inline uint64_t bits_of(double d) { return (uint64_t)__double_as_longlong(d); }

template <int OP>
struct ArgScan {
    static constexpr bool FLOAT_MINMAX = OP == WINDOW_OP_MIN_F64 || OP == WINDOW_OP_MAX_F64;
    // value, non-NULL arguments, ARG_HEAD (a partition starts inside the span) | ARG_HAS_NUMBER | ARG_SAW_NAN (float MIN / MAX)
    struct State { uint64_t value; uint32_t count, flags; };
    ColumnRef arg;
    const uint64_t* part_flags;
    uint64_t* run_value;
    uint32_t* run_count;
    __device__ static State identity() { return State{0ull, 0u, 0u}; }
    __device__ static State shfl_up(const State& x, int d) { return State{shfl_up_u64(x.value, d), __shfl_up(x.count, d, 64), __shfl_up(x.flags, d, 64)}; }
    // a side that holds nothing (count 0; float MIN / MAX: no number) contributes nothing: the other side's value stands
    __device__ static uint64_t merge(const State& a, const State& b) {
        if (OP == WINDOW_OP_ADD_I64) return a.value + b.value;                      // an empty side holds 0
        const bool has_a = FLOAT_MINMAX ? (a.flags & ARG_HAS_NUMBER) != 0 : a.count != 0;
        const bool has_b = FLOAT_MINMAX ? (b.flags & ARG_HAS_NUMBER) != 0 : b.count != 0;
        uint64_t both;
        if (OP == WINDOW_OP_ADD_F64) both = bits_of(f64_of(a.value) + f64_of(b.value));
        else if (OP == WINDOW_OP_MIN_I64) both = (int64_t)b.value < (int64_t)a.value ? b.value : a.value;
        else if (OP == WINDOW_OP_MAX_I64) both = (int64_t)b.value > (int64_t)a.value ? b.value : a.value;
        else if (OP == WINDOW_OP_MIN_U64) both = b.value < a.value ? b.value : a.value;
        else if (OP == WINDOW_OP_MAX_U64) both = b.value > a.value ? b.value : a.value;
        else if (OP == WINDOW_OP_MIN_F64) both = f64_of(b.value) < f64_of(a.value) ? b.value : a.value;
        else both = f64_of(b.value) > f64_of(a.value) ? b.value : a.value;
        return !has_a ? b.value : !has_b ? a.value : both;
    }
    // the segmented operator: a head on the right cuts the left side off
    __device__ static State combine(const State& a, const State& b) {
        const bool cut = (b.flags & ARG_HEAD) != 0;
        const uint64_t merged = merge(a, b);
        return State{cut ? b.value : merged, cut ? b.count : a.count + b.count, cut ? b.flags : a.flags | b.flags};
    }
    __device__ State load(int64_t i, int64_t) const {
        State s = load_arg(arg, i);
        if (bit_at(part_flags, i)) s.flags |= ARG_HEAD;
        return s;
    }
    __device__ static State load_arg(const ColumnRef& arg, int64_t i) {
        const bool valid = !arg.validity || bit_at(arg.validity, i);
        // sign- / zero-extended; Float32 as a double's bits (COUNT: no data, the validity is all that is read)
        return state_of(arg.dtype, arg.data != nullptr, valid, valid && arg.data ? dt_load(arg.dtype, arg.data, i) : 0ull);
    }
    // one row's argument, `v` its 64-bit image (dt_load), as a state of one row without the head flag
    __device__ static State state_of(int dtype, bool has_data, bool valid, uint64_t v) {
        uint64_t value = 0;
        uint32_t count = 0, flags = 0u;
        if (valid) {
            count = 1;
            if (has_data) {
                if (OP == WINDOW_OP_ADD_F64 && !dt_is_float(dtype)) v = bits_of(dt_is_unsigned(dtype) ? (double)v : (double)(int64_t)v);
                if (FLOAT_MINMAX) {
                    const double d = f64_of(v);
                    const bool nan = d != d;
                    flags |= nan ? ARG_SAW_NAN : ARG_HAS_NUMBER;
                    v = nan ? 0ull : v;
                }
                value = v;
            }
        }
        return State{value, count, flags};
    }
    __device__ void store(int64_t i, int64_t, const State& s) const {
        run_value[i] = FLOAT_MINMAX && !(s.flags & ARG_HAS_NUMBER) ? F64_QUIET_NAN : s.value;     // NaNs alone: a NaN
        run_count[i] = s.count;
    }
};

// =============================================================================================
// elementwise: ranks, gather indices, finish
// =============================================================================================
__global__ void __launch_bounds__(WINDOW_BLOCK)
window_rank_kernel(int kind, const uint32_t* __restrict__ part_start, const uint32_t* __restrict__ peer_start, const uint32_t* __restrict__ peers_to,
                   int64_t n, uint64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t p0 = part_start[i];
    uint64_t v;
    if (kind == WINDOW_ROW_NUMBER) v = (uint64_t)i - p0 + 1;
    else if (kind == WINDOW_RANK) v = (uint64_t)peer_start[i] - p0 + 1;
    else v = (uint64_t)peers_to[i] - peers_to[p0] + 1;              // p0 starts a peer group: it is counted on both sides
    out[i] = v;
}

__global__ void __launch_bounds__(WINDOW_BLOCK)
window_index_kernel(int kind, int64_t offset, const uint32_t* __restrict__ part_start, const uint32_t* __restrict__ part_end,
                    const uint32_t* __restrict__ frame_end, int64_t n, uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t r;
    if (kind == WINDOW_LAG) r = offset <= i - (int64_t)part_start[i] ? (uint32_t)(i - offset) : WINDOW_NULL_INDEX;
    else if (kind == WINDOW_LEAD) r = offset <= (int64_t)part_end[i] - i ? (uint32_t)(i + offset) : WINDOW_NULL_INDEX;
    else if (kind == WINDOW_FIRST) r = part_start[i];
    else r = frame_end ? frame_end[i] : (uint32_t)i;
    idx[i] = r;
}

__global__ void __launch_bounds__(WINDOW_BLOCK)
window_finish_kernel(int kind, int out_dtype, const uint64_t* __restrict__ run_value, const uint32_t* __restrict__ run_count,
                     const uint32_t* __restrict__ frame_end, int64_t n, void* __restrict__ out, uint64_t* __restrict__ validity) {
    const int64_t i = (int64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    bool valid = false;
    if (i < n) {
        const int64_t j = frame_end ? (int64_t)frame_end[i] : i;
        const uint32_t count = run_count[j];
        valid = count != 0;
        if (kind == WINDOW_FINISH_COUNT) {
            static_cast<uint64_t*>(out)[i] = count;
        } else if (kind == WINDOW_FINISH_AVG) {
            static_cast<double*>(out)[i] = valid ? f64_of(run_value[j]) / (double)count : 0.0;
        } else {
            dt_store(out_dtype, out, i, valid ? run_value[j] : 0ull);
        }
    }
    const uint64_t word = __ballot(valid);                          // 64 consecutive rows from a multiple of 64: one validity word
    if (validity && (threadIdx.x & 63) == 0 && i < n) validity[i >> 6] = word;
}

// =============================================================================================
// sliding ROWS frames: the frame of every row, the finish over it, and the aggregate of a bounded neighbourhood
// =============================================================================================
// the last / first partition head among rows a .. b (0 <= a, b < n), or -1.  Bits past n are 0 (window_flags).
__device__ inline int64_t last_head_in(const uint64_t* __restrict__ part_flags, int64_t a, int64_t b) {
    for (int64_t w = b >> 6; w >= (a >> 6); --w) {
        uint64_t x = part_flags[w];
        if (w == (b >> 6)) x &= ~0ull >> (63 - (b & 63));
        if (w == (a >> 6)) x &= ~0ull << (a & 63);
        if (x) return (w << 6) + 63 - __clzll((long long)x);
    }
    return -1;
}
__device__ inline int64_t first_head_in(const uint64_t* __restrict__ part_flags, int64_t a, int64_t b) {
    for (int64_t w = a >> 6; w <= (b >> 6); ++w) {
        uint64_t x = part_flags[w];
        if (w == (b >> 6)) x &= ~0ull >> (63 - (b & 63));
        if (w == (a >> 6)) x &= ~0ull << (a & 63);
        if (x) return (w << 6) + __ffsll((unsigned long long)x) - 1;
    }
    return -1;
}

// With `part_flags` (two finite ends that reach at most WINDOW_SLIDE_MAX_ROWS rows away) the partition's bounds are not needed: only a
// head among the rows the frame reaches over cuts it, and the flags of those rows are a few words.  Otherwise from part_start / part_end.
__global__ void __launch_bounds__(WINDOW_BLOCK)
window_frame_bounds_kernel(const uint64_t* __restrict__ part_flags, const uint32_t* __restrict__ part_start, const uint32_t* __restrict__ part_end,
                           bool start_unbounded, int64_t start, bool end_unbounded, int64_t end, int64_t n, uint32_t* __restrict__ lo,
                           uint32_t* __restrict__ hi) {
    const int64_t i = (int64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    if (i >= n) return;
    int64_t l, h;                                                    // |start|, |end| <= n: no overflow
    if (part_flags) {
        // a frame that lies past the partition's end (start > 0) or before its start (end < 0) comes out with l > h: the other side is
        // cut at the head that lies between
        l = i + start;
        if (start < 0) {                                             // the last head in (i + start, i]; row 0 is one
            const int64_t q = last_head_in(part_flags, l + 1 > 0 ? l + 1 : 0, i);
            if (q >= 0) l = q;
        }
        h = i + end < n - 1 ? i + end : n - 1;
        if (end > 0 && i + 1 < n) {                                  // the first head in (i, i + end]: the partition ends before it
            const int64_t q = first_head_in(part_flags, i + 1, h);
            if (q >= 0) h = q - 1;
        }
    } else {
        const int64_t ps = part_start[i], pe = part_end[i];
        l = start_unbounded || i + start < ps ? ps : i + start;
        h = end_unbounded || i + end > pe ? pe : i + end;
    }
    const bool empty = l > h;
    lo[i] = empty ? WINDOW_NULL_INDEX : (uint32_t)l;
    hi[i] = empty ? WINDOW_NULL_INDEX : (uint32_t)h;
}

__global__ void __launch_bounds__(WINDOW_BLOCK)
window_finish_frame_kernel(int kind, int out_dtype, const uint64_t* __restrict__ run_value, const uint32_t* __restrict__ run_count,
                           const uint64_t* __restrict__ part_flags, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, int64_t n,
                           void* __restrict__ out, uint64_t* __restrict__ validity) {
    const int64_t i = (int64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    bool valid = false;
    if (i < n) {
        const uint32_t h = hi[i];
        uint32_t count = 0;
        uint64_t value = 0;
        if (h != WINDOW_NULL_INDEX) {
            count = run_count[h];
            value = run_value[h];
            if (part_flags) {                                       // wrapping differences are exact
                const uint32_t l = lo[i];
                if (!bit_at(part_flags, l)) {                       // (a frame that starts with its partition has nothing before it)
                    count -= run_count[l - 1];
                    value -= run_value[l - 1];
                }
            }
        }
        valid = count != 0;
        if (kind == WINDOW_FINISH_COUNT) {
            static_cast<uint64_t*>(out)[i] = count;
        } else if (kind == WINDOW_FINISH_AVG) {
            static_cast<double*>(out)[i] = valid ? f64_of(value) / (double)count : 0.0;
        } else {
            dt_store(out_dtype, out, i, valid ? value : 0ull);
        }
    }
    const uint64_t word = __ballot(valid);
    if (validity && (threadIdx.x & 63) == 0 && i < n) validity[i >> 6] = word;
}

// a raw element of an Arrow buffer, zero-extended by its load -> the 64-bit image dt_load gives
__device__ inline uint64_t dt_widen(int t, uint64_t raw) {
    switch (t) {
        case DT_INT8: return (uint64_t)(int64_t)(int8_t)raw;
        case DT_INT16: return (uint64_t)(int64_t)(int16_t)raw;
        case DT_INT32: case DT_DATE32: return (uint64_t)(int64_t)(int32_t)raw;
        case DT_FLOAT32: return bits_of((double)__uint_as_float((uint32_t)raw));
        default: return raw;
    }
}

// One workgroup per tile.  LDS: the argument of rows span_first .. span_last as 64-bit values, then one byte per row: bit 0 = not
// NULL, ARG_HAS_NUMBER / ARG_SAW_NAN as the scan's state has them.  Lane k of a wave walks row base + k, so at every step of the
// walk consecutive lanes read consecutive 8-byte slots (away from a partition's edge).
constexpr uint32_t SLIDE_NOT_NULL = 1;
static_assert((SLIDE_NOT_NULL & (ARG_HAS_NUMBER | ARG_SAW_NAN)) == 0, "one flag byte per staged row");

// rows span_first .. span_first + span - 1 of the argument into LDS, WINDOW_ROUNDS rows per thread and round: the raw values and the
// validity words, coalesced and unconditional (a lane past the span re-reads the span's last row and stores nothing), so all of a
// round's loads are issued before the first LDS write waits for one
template <int OP, class T, bool NULLABLE>
__device__ inline void slide_stage(const ColumnRef& arg, int64_t span_first, int span, uint64_t* s_value, uint8_t* s_flag) {
    using A = ArgScan<OP>;
    const T* __restrict__ data = static_cast<const T*>(arg.data);
    for (int base = 0; base < span; base += WINDOW_TILE_ROWS) {
        T raw[WINDOW_ROUNDS];
        uint64_t word[WINDOW_ROUNDS];
#pragma unroll
        for (int r = 0; r < WINDOW_ROUNDS; ++r) {
            const int s = base + r * WINDOW_BLOCK + (int)threadIdx.x;
            const int64_t row = span_first + (s < span ? s : span - 1);
            raw[r] = data[row];
            word[r] = NULLABLE ? arg.validity[row >> 6] : ~0ull;
        }
#pragma unroll
        for (int r = 0; r < WINDOW_ROUNDS; ++r) {
            const int s = base + r * WINDOW_BLOCK + (int)threadIdx.x;
            if (s < span) {
                const typename A::State v = A::state_of(arg.dtype, true, (word[r] >> ((span_first + s) & 63)) & 1, dt_widen(arg.dtype, raw[r]));
                s_value[s] = v.value;
                s_flag[s] = (uint8_t)((v.count ? SLIDE_NOT_NULL : 0u) | v.flags);
            }
        }
    }
}

// the element type and "has a validity" are chosen here, outside the staging loop: chosen per load, each load would wait for the last
template <int OP>
__device__ inline void slide_stage_span(const ColumnRef& arg, int64_t span_first, int span, uint64_t* s_value, uint8_t* s_flag) {
#define STAGE(T) (arg.validity ? slide_stage<OP, T, true>(arg, span_first, span, s_value, s_flag) : slide_stage<OP, T, false>(arg, span_first, span, s_value, s_flag))
    switch (dt_width(arg.dtype)) {
        case 1: STAGE(uint8_t); break;
        case 2: STAGE(uint16_t); break;
        case 4: STAGE(uint32_t); break;
        default: STAGE(uint64_t); break;
    }
#undef STAGE
}

// where the walk reads a row's state (no head flag) from: the staged span, by slot, or the argument itself, by row
template <int OP>
struct SlideStaged {
    const uint64_t* value;
    const uint8_t* flag;
    __device__ typename ArgScan<OP>::State at(int s) const {
        const uint32_t f = flag[s];
        return typename ArgScan<OP>::State{value[s], f & SLIDE_NOT_NULL, f & ~SLIDE_NOT_NULL};
    }
};
template <int OP>
struct SlideGlobal {
    ColumnRef arg;
    __device__ typename ArgScan<OP>::State at(int64_t row) const { return ArgScan<OP>::load_arg(arg, row); }
};

// the aggregate of positions from .. to (none when from > to), in ascending order from the identity (value 0: the bits of +0.0)
template <int OP, class Rows, class Index>
__device__ inline typename ArgScan<OP>::State slide_walk(const Rows& rows, Index from, Index to) {
    using A = ArgScan<OP>;
    using S = typename A::State;
    S acc = A::identity();
    for (Index s = from; s <= to; ++s) {
        const S b = rows.at(s);
        if (OP == WINDOW_OP_ADD_F64) {
            if (b.count) acc.value = bits_of(f64_of(acc.value) + f64_of(b.value));
        } else {
            acc.value = A::merge(acc, b);
            acc.flags |= b.flags;
        }
        acc.count += b.count;
    }
    return acc;
}

// row i's output and, per wave, its validity word (every lane of the wave calls this, a row past n included)
template <int OP>
__device__ inline void slide_finish(const typename ArgScan<OP>::State& acc, int64_t i, int64_t n, int kind, int out_dtype, void* __restrict__ out,
                                    uint64_t* __restrict__ validity) {
    using A = ArgScan<OP>;
    const bool valid = acc.count != 0;
    if (i < n) {
        const uint64_t value = A::FLOAT_MINMAX && !(acc.flags & ARG_HAS_NUMBER) ? F64_QUIET_NAN : acc.value;      // NaNs alone: a NaN
        if (kind == WINDOW_FINISH_AVG) static_cast<double*>(out)[i] = valid ? f64_of(value) / (double)acc.count : 0.0;
        else dt_store(out_dtype, out, i, valid ? value : 0ull);
    }
    const uint64_t word = __ballot(valid);                          // 64 consecutive rows from a multiple of 64: one validity word
    if (validity && (threadIdx.x & 63) == 0 && i < n) validity[i >> 6] = word;
}

template <int OP>
__global__ void __launch_bounds__(WINDOW_BLOCK)
window_slide_kernel(ColumnRef arg, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, int64_t start, int64_t end, int64_t n, int kind,
                    int out_dtype, void* __restrict__ out, uint64_t* __restrict__ validity) {
    using A = ArgScan<OP>;
    using S = typename A::State;
    extern __shared__ uint64_t s_slide[];
    const int t = threadIdx.x;
    const int64_t tile_first = (int64_t)blockIdx.x * WINDOW_TILE_ROWS;
    const int64_t tile_last = tile_first + WINDOW_TILE_ROWS - 1 < n - 1 ? tile_first + WINDOW_TILE_ROWS - 1 : n - 1;
    const int64_t span_first = tile_first + start > 0 ? tile_first + start : 0;
    const int64_t span_last = tile_last + end < n - 1 ? tile_last + end : n - 1;
    const int span = span_last >= span_first ? (int)(span_last - span_first + 1) : 0;    // <= cap: the launch sized the LDS for cap rows
    const int cap = WINDOW_TILE_ROWS + (int)(end - start);
    uint8_t* s_flag = reinterpret_cast<uint8_t*>(s_slide + cap);

    uint32_t l[WINDOW_ROUNDS], h[WINDOW_ROUNDS];
#pragma unroll
    for (int r = 0; r < WINDOW_ROUNDS; ++r) {
        const int64_t i = tile_first + r * WINDOW_BLOCK + t;
        l[r] = i < n ? lo[i] : WINDOW_NULL_INDEX;
        h[r] = i < n ? hi[i] : WINDOW_NULL_INDEX;
    }
    slide_stage_span<OP>(arg, span_first, span, s_slide, s_flag);
    __syncthreads();
    const SlideStaged<OP> staged{s_slide, s_flag};
#pragma unroll
    for (int r = 0; r < WINDOW_ROUNDS; ++r) {
        const int64_t i = tile_first + r * WINDOW_BLOCK + t;
        S acc = A::identity();
        if (h[r] != WINDOW_NULL_INDEX) {
            // the row's own frame; the clamp to the staged span changes nothing for a (lo, hi) made with this start / end
            const int64_t jl = (int64_t)l[r] > span_first ? (int64_t)l[r] : span_first, jh = (int64_t)h[r] < span_last ? (int64_t)h[r] : span_last;
            acc = slide_walk<OP>(staged, (int)(jl - span_first), (int)(jh - span_first));
        }
        slide_finish<OP>(acc, i, n, kind, out_dtype, out, validity);
    }
}

// window_slide over frames whose span no offset bounds: the tile's span is the smallest lo .. the largest hi of its non-empty rows.
// Staged and walked in LDS when it fits WINDOW_SLIDE_STAGE_ROWS, else walked in global memory (uniform per workgroup).
template <int OP>
__global__ void __launch_bounds__(WINDOW_BLOCK)
window_slide_value_kernel(ColumnRef arg, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, int64_t n, int kind, int out_dtype,
                          void* __restrict__ out, uint64_t* __restrict__ validity) {
    using A = ArgScan<OP>;
    using S = typename A::State;
    extern __shared__ uint64_t s_slide[];
    __shared__ uint32_t s_span[2 * (WINDOW_BLOCK / 64)];
    const int t = threadIdx.x;
    const int64_t tile_first = (int64_t)blockIdx.x * WINDOW_TILE_ROWS;
    uint8_t* s_flag = reinterpret_cast<uint8_t*>(s_slide + WINDOW_SLIDE_STAGE_ROWS);

    uint32_t l[WINDOW_ROUNDS], h[WINDOW_ROUNDS];
    uint32_t first = WINDOW_NULL_INDEX, last = 0;                   // over the non-empty rows (an empty one: lo = hi = WINDOW_NULL_INDEX)
#pragma unroll
    for (int r = 0; r < WINDOW_ROUNDS; ++r) {
        const int64_t i = tile_first + r * WINDOW_BLOCK + t;
        l[r] = i < n ? lo[i] : WINDOW_NULL_INDEX;
        h[r] = i < n ? hi[i] : WINDOW_NULL_INDEX;
        if (h[r] != WINDOW_NULL_INDEX) {
            first = l[r] < first ? l[r] : first;
            last = h[r] > last ? h[r] : last;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t of = __shfl_xor(first, d, 64), ol = __shfl_xor(last, d, 64);
        first = of < first ? of : first;
        last = ol > last ? ol : last;
    }
    if ((t & 63) == 0) {
        s_span[2 * (t >> 6)] = first;
        s_span[2 * (t >> 6) + 1] = last;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WINDOW_BLOCK / 64; ++w) {
        first = s_span[2 * w] < first ? s_span[2 * w] : first;
        last = s_span[2 * w + 1] > last ? s_span[2 * w + 1] : last;
    }
    // the same in every lane of the workgroup from here on
    const bool any = first != WINDOW_NULL_INDEX;
    const int64_t span_first = any ? (int64_t)first : 0;
    const int64_t rows = any ? (int64_t)last - (int64_t)first + 1 : 0;
    const bool fits = rows <= (int64_t)WINDOW_SLIDE_STAGE_ROWS;
    if (fits) {
        slide_stage_span<OP>(arg, span_first, (int)rows, s_slide, s_flag);
        __syncthreads();
    }
    const SlideStaged<OP> staged{s_slide, s_flag};
    const SlideGlobal<OP> global{arg};
#pragma unroll
    for (int r = 0; r < WINDOW_ROUNDS; ++r) {
        const int64_t i = tile_first + r * WINDOW_BLOCK + t;
        S acc = A::identity();
        if (h[r] != WINDOW_NULL_INDEX) {
            if (fits) acc = slide_walk<OP>(staged, (int)((int64_t)l[r] - span_first), (int)((int64_t)h[r] - span_first));
            else acc = slide_walk<OP>(global, (int64_t)l[r], (int64_t)h[r]);
        }
        slide_finish<OP>(acc, i, n, kind, out_dtype, out, validity);
    }
}

// =============================================================================================
// RANGE / GROUPS frames: the two ends of every row's frame, by a search of the sorted rows
// =============================================================================================
// a - b >= bound / a - b <= bound for two 64-bit unsigned images and a signed bound, as if in unbounded integers
__device__ inline bool diff_at_least(uint64_t a, uint64_t b, int64_t bound) {
    if (a >= b) return bound <= 0 || a - b >= (uint64_t)bound;
    return bound < 0 && b - a <= 0 - (uint64_t)bound;                // (the magnitude of INT64_MIN: 2^63, as unsigned)
}
__device__ inline bool diff_at_most(uint64_t a, uint64_t b, int64_t bound) {
    if (a >= b) return bound >= 0 && a - b <= (uint64_t)bound;
    return bound >= 0 || b - a >= 0 - (uint64_t)bound;
}

// One OFFSET side of row i's frame as a predicate over the rows of its partition that is false up to some row and true from it on:
//   START  "row j lies at or after the frame's first row": its class is after the numbers, or it is a number that qualifies
//   END    "row j lies after the frame's last row":        its class is after the numbers, or it is a number that does not qualify
// Classes in row order: 0 = before the numbers, 1 = a number, 2 = after them (NULLs where the sort put them; ascending, -NaN sorts
// first and +NaN last, descending the other way round).  GROUPS: every row is a number, its peer-group count, ascending.
struct ValueSide {
    ColumnRef key;                       // RANGE
    const uint32_t* peers_to;            // GROUPS (key.data unused)
    bool is_end, groups, is_float, descending, nulls_first;
    int64_t offset;                      // integer keys and GROUPS
    double target;                       // float keys: key_i + s * offset
    uint64_t mine;                       // integer keys and GROUPS: row i's ordered image

    __device__ int cls(int64_t j, uint64_t& image) const {
        if (groups) { image = peers_to[j]; return 1; }
        if (key.validity && !bit_at(key.validity, j)) return nulls_first ? 0 : 2;
        image = dt_load(key.dtype, key.data, j);
        if (is_float) {
            const double d = f64_of(image);
            if (d != d) return ((image >> 63) != 0) != descending ? 0 : 2;
            return 1;
        }
        if (!dt_is_unsigned(key.dtype)) image ^= 0x8000000000000000ull;       // signed order as unsigned order
        return 1;
    }
    __device__ bool qualifies(uint64_t image) const {
        if (is_float) {
            const double d = f64_of(image);
            return is_end != descending ? d <= target : d >= target;           // start asc / end desc: key_j >= t; the other two: <=
        }
        const uint64_t a = descending ? mine : image, b = descending ? image : mine;   // s * (key_j - key_i) = a - b
        return is_end ? diff_at_most(a, b, offset) : diff_at_least(a, b, offset);
    }
    __device__ bool operator()(int64_t j) const {
        uint64_t image = 0;
        const int c = cls(j, image);
        if (c != 1) return c == 2;
        return qualifies(image) != is_end;
    }
};

// the first row of ps .. pe at which the predicate holds (pe + 1: nowhere), galloping outward from row i and then bisecting
template <class P>
__device__ inline int64_t first_true_from(const P& p, int64_t ps, int64_t pe, int64_t i) {
    int64_t no, yes;                                                 // p(no) is false (or no = ps - 1), p(yes) true (or yes = pe + 1)
    if (p(i)) {
        yes = i;
        no = ps - 1;
        for (int64_t step = 1; yes - step >= ps; step <<= 1) {
            if (p(yes - step)) yes -= step;
            else { no = yes - step; break; }
        }
    } else {
        no = i;
        yes = pe + 1;
        for (int64_t step = 1; no + step <= pe; step <<= 1) {
            if (!p(no + step)) no += step;
            else { yes = no + step; break; }
        }
    }
    while (yes - no > 1) {
        const int64_t mid = no + ((yes - no) >> 1);
        if (p(mid)) yes = mid;
        else no = mid;
    }
    return yes;
}

__global__ void __launch_bounds__(WINDOW_BLOCK)
window_value_bounds_kernel(WindowValueFrameArgs a, int64_t n, uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t* __restrict__ widest) {
    const int64_t i = (int64_t)blockIdx.x * WINDOW_BLOCK + threadIdx.x;
    uint32_t width = 0;
    if (i < n) {
        const int64_t ps = a.part_start[i], pe = a.part_end[i];
        const bool groups = a.units == WINDOW_UNITS_GROUPS;
        const bool search_start = a.start_kind == WINDOW_BOUND_OFFSET, search_end = a.end_kind == WINDOW_BOUND_OFFSET;
        ValueSide side;
        side.key = a.key;
        side.peers_to = a.peers_to;
        side.groups = groups;
        side.is_float = !groups && dt_is_float(a.key.dtype);
        side.descending = !groups && a.descending != 0;
        side.nulls_first = a.nulls_first != 0;
        side.is_end = false;
        side.offset = 0;
        side.target = 0.0;
        side.mine = 0;
        int own = 1;                                                 // the class of row i's own key
        double own_f = 0.0;
        if (search_start || search_end) {
            own = side.cls(i, side.mine);
            own_f = f64_of(side.mine);
        }
        int64_t l, h;                                                // l = pe + 1 / h = ps - 1: the side has no row
        if (a.start_kind == WINDOW_BOUND_UNBOUNDED) l = ps;
        else if (a.start_kind == WINDOW_BOUND_CURRENT_ROW || own != 1) l = a.peer_start[i];
        else {
            side.is_end = false;
            side.offset = a.start_i;
            side.target = side.descending ? own_f - a.start_f : own_f + a.start_f;
            l = first_true_from(side, ps, pe, i);
            uint64_t image;
            if (l <= pe && side.cls(l, image) != 1) l = pe + 1;      // no number qualifies
        }
        if (a.end_kind == WINDOW_BOUND_UNBOUNDED) h = pe;
        else if (a.end_kind == WINDOW_BOUND_CURRENT_ROW || own != 1) h = a.peer_end[i];
        else {
            side.is_end = true;
            side.offset = a.end_i;
            side.target = side.descending ? own_f - a.end_f : own_f + a.end_f;
            h = first_true_from(side, ps, pe, i) - 1;
            uint64_t image;
            if (h >= ps && side.cls(h, image) != 1) h = ps - 1;
        }
        const bool empty = l > pe || h < ps || l > h;
        lo[i] = empty ? WINDOW_NULL_INDEX : (uint32_t)l;
        hi[i] = empty ? WINDOW_NULL_INDEX : (uint32_t)h;
        width = empty ? 0u : (uint32_t)(h - l + 1);
    }
    if (widest) {                                                    // (uniform: a kernel argument)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t o = __shfl_xor(width, d, 64);
            width = o > width ? o : width;
        }
        if ((threadIdx.x & 63) == 0 && width) atomicMax(widest, width);
    }
}

inline unsigned row_blocks(int64_t n) { return (unsigned)((n + WINDOW_BLOCK - 1) / WINDOW_BLOCK); }

template <class P>
hipError_t run_tiles(const LaunchCfg& cfg, const P& p, int64_t n, void* temp) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((window_tiles_kernel<P>), dim3((unsigned)window_tiles(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, p, n,
                       static_cast<typename P::State*>(temp));
    return hipGetLastError();
}
template <class P>
hipError_t run_summaries(const LaunchCfg& cfg, int64_t n, void* temp) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((window_summaries_kernel<P>), dim3(1), dim3(WINDOW_BLOCK), 0, cfg.stream, static_cast<typename P::State*>(temp), window_tiles(n));
    return hipGetLastError();
}
template <class P>
hipError_t run_apply(const LaunchCfg& cfg, const P& p, int64_t n, const void* temp) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((window_apply_kernel<P>), dim3((unsigned)window_tiles(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, p, n,
                       static_cast<const typename P::State*>(temp));
    return hipGetLastError();
}

}  // namespace

// the widest state (ArgScan: 16 bytes) sizes the scratch of every scan
size_t window_scan_temp_bytes(int64_t n) { return (size_t)(window_tiles(n) > 0 ? window_tiles(n) : 1) * 16; }
static_assert(sizeof(ArgScan<WINDOW_OP_ADD_I64>::State) == 16 && sizeof(ForwardBounds::State) <= 16 && sizeof(BackwardBounds::State) <= 16,
              "window_scan_temp_bytes counts 16 bytes per tile summary");

hipError_t launch_window_flags(const LaunchCfg& cfg, const WindowKeys& K, int64_t n, uint64_t* part_flags, uint64_t* peer_flags) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(window_flags_kernel, dim3(row_blocks(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, K, n, part_flags, peer_flags);
    return hipGetLastError();
}

hipError_t launch_window_bounds_forward_tiles(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, void* temp) {
    return run_tiles(cfg, ForwardBounds{part_flags, peer_flags, nullptr, nullptr, nullptr}, n, temp);
}
hipError_t launch_window_bounds_forward_summaries(const LaunchCfg& cfg, int64_t n, void* temp) { return run_summaries<ForwardBounds>(cfg, n, temp); }
hipError_t launch_window_bounds_forward_apply(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, const void* temp,
                                              uint32_t* part_start, uint32_t* peer_start, uint32_t* peers_to) {
    return run_apply(cfg, ForwardBounds{part_flags, peer_flags, part_start, peer_start, peers_to}, n, temp);
}
hipError_t launch_window_bounds_backward_tiles(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, void* temp) {
    return run_tiles(cfg, BackwardBounds{part_flags, peer_flags, nullptr, nullptr}, n, temp);
}
hipError_t launch_window_bounds_backward_summaries(const LaunchCfg& cfg, int64_t n, void* temp) { return run_summaries<BackwardBounds>(cfg, n, temp); }
hipError_t launch_window_bounds_backward_apply(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, const void* temp,
                                               uint32_t* part_end, uint32_t* peer_end) {
    return run_apply(cfg, BackwardBounds{part_flags, peer_flags, part_end, peer_end}, n, temp);
}

hipError_t launch_window_rank(const LaunchCfg& cfg, int kind, const uint32_t* part_start, const uint32_t* peer_start, const uint32_t* peers_to,
                              int64_t n, uint64_t* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(window_rank_kernel, dim3(row_blocks(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, kind, part_start, peer_start, peers_to, n, out);
    return hipGetLastError();
}
hipError_t launch_window_index(const LaunchCfg& cfg, int kind, int64_t offset, const uint32_t* part_start, const uint32_t* part_end,
                               const uint32_t* frame_end, int64_t n, uint32_t* idx) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(window_index_kernel, dim3(row_blocks(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, kind, offset, part_start, part_end, frame_end, n, idx);
    return hipGetLastError();
}

#define WINDOW_OP_DISPATCH(op, CALL)                                           \
    switch (op) {                                                              \
        case WINDOW_OP_ADD_I64: return CALL(WINDOW_OP_ADD_I64);                \
        case WINDOW_OP_ADD_F64: return CALL(WINDOW_OP_ADD_F64);                \
        case WINDOW_OP_MIN_I64: return CALL(WINDOW_OP_MIN_I64);                \
        case WINDOW_OP_MAX_I64: return CALL(WINDOW_OP_MAX_I64);                \
        case WINDOW_OP_MIN_U64: return CALL(WINDOW_OP_MIN_U64);                \
        case WINDOW_OP_MAX_U64: return CALL(WINDOW_OP_MAX_U64);                \
        case WINDOW_OP_MIN_F64: return CALL(WINDOW_OP_MIN_F64);                \
        case WINDOW_OP_MAX_F64: return CALL(WINDOW_OP_MAX_F64);                \
        default: return hipErrorInvalidValue;                                  \
    }

hipError_t launch_window_scan_tiles(const LaunchCfg& cfg, int op, const ColumnRef& arg, const uint64_t* part_flags, int64_t n, void* temp) {
#define CALL(OP) run_tiles(cfg, ArgScan<OP>{arg, part_flags, nullptr, nullptr}, n, temp)
    WINDOW_OP_DISPATCH(op, CALL)
#undef CALL
}
hipError_t launch_window_scan_summaries(const LaunchCfg& cfg, int op, int64_t n, void* temp) {
#define CALL(OP) run_summaries<ArgScan<OP>>(cfg, n, temp)
    WINDOW_OP_DISPATCH(op, CALL)
#undef CALL
}
hipError_t launch_window_scan_apply(const LaunchCfg& cfg, int op, const ColumnRef& arg, const uint64_t* part_flags, int64_t n, const void* temp,
                                    uint64_t* run_value, uint32_t* run_count) {
#define CALL(OP) run_apply(cfg, ArgScan<OP>{arg, part_flags, run_value, run_count}, n, temp)
    WINDOW_OP_DISPATCH(op, CALL)
#undef CALL
}

hipError_t launch_window_finish(const LaunchCfg& cfg, int kind, int out_dtype, const uint64_t* run_value, const uint32_t* run_count,
                                const uint32_t* frame_end, int64_t n, void* out, uint64_t* validity) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(window_finish_kernel, dim3(row_blocks(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, kind, out_dtype, run_value, run_count, frame_end, n,
                       out, validity);
    return hipGetLastError();
}

hipError_t launch_window_frame_bounds(const LaunchCfg& cfg, const uint64_t* part_flags, const uint32_t* part_start, const uint32_t* part_end,
                                      bool start_unbounded, int64_t start, bool end_unbounded, int64_t end, int64_t n, uint32_t* lo, uint32_t* hi) {
    if (n <= 0) return hipSuccess;
    if (start < -n || start > n || end < -n || end > n) return hipErrorInvalidValue;
    if (part_flags ? !window_frame_is_near(start_unbounded, start, end_unbounded, end) || start > end : !part_start || !part_end) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_frame_bounds_kernel, dim3(row_blocks(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, part_flags, part_start, part_end, start_unbounded,
                       start, end_unbounded, end, n, lo, hi);
    return hipGetLastError();
}

hipError_t launch_window_finish_frame(const LaunchCfg& cfg, int kind, int out_dtype, const uint64_t* run_value, const uint32_t* run_count,
                                      const uint64_t* part_flags, const uint32_t* lo, const uint32_t* hi, int64_t n, void* out, uint64_t* validity) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(window_finish_frame_kernel, dim3(row_blocks(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, kind, out_dtype, run_value, run_count,
                       part_flags, lo, hi, n, out, validity);
    return hipGetLastError();
}

template <int OP>
static hipError_t run_slide(const LaunchCfg& cfg, int kind, int out_dtype, const ColumnRef& arg, const uint32_t* lo, const uint32_t* hi, int64_t start,
                     int64_t end, int64_t n, void* out, uint64_t* validity) {
    const size_t cap = (size_t)WINDOW_TILE_ROWS + (size_t)(end - start);               // rows a workgroup stages at most
    const size_t lds = cap * 8 + ((cap + 7) & ~(size_t)7);
    hipLaunchKernelGGL((window_slide_kernel<OP>), dim3((unsigned)window_tiles(n)), dim3(WINDOW_BLOCK), lds, cfg.stream, arg, lo, hi, start, end, n, kind,
                       out_dtype, out, validity);
    return hipGetLastError();
}

hipError_t launch_window_slide(const LaunchCfg& cfg, int op, int kind, int out_dtype, const ColumnRef& arg, const uint32_t* lo, const uint32_t* hi,
                               int64_t start, int64_t end, int64_t n, void* out, uint64_t* validity) {
    if (n <= 0) return hipSuccess;
    if (start < -n || start > n || end < start || end > n || end - start >= WINDOW_SLIDE_MAX_ROWS) return hipErrorInvalidValue;
    if ((kind != WINDOW_FINISH_VALUE && kind != WINDOW_FINISH_AVG) || !arg.data || arg.dtype == DT_UTF8 || arg.dtype == DT_BOOLEAN) return hipErrorInvalidValue;
#define CALL(OP) run_slide<OP>(cfg, kind, out_dtype, arg, lo, hi, start, end, n, out, validity)
    switch (op) {
        case WINDOW_OP_ADD_F64: return CALL(WINDOW_OP_ADD_F64);
        case WINDOW_OP_MIN_I64: return CALL(WINDOW_OP_MIN_I64);
        case WINDOW_OP_MAX_I64: return CALL(WINDOW_OP_MAX_I64);
        case WINDOW_OP_MIN_U64: return CALL(WINDOW_OP_MIN_U64);
        case WINDOW_OP_MAX_U64: return CALL(WINDOW_OP_MAX_U64);
        case WINDOW_OP_MIN_F64: return CALL(WINDOW_OP_MIN_F64);
        case WINDOW_OP_MAX_F64: return CALL(WINDOW_OP_MAX_F64);
        default: return hipErrorInvalidValue;                       // the wrapping add takes the scan and a difference
    }
#undef CALL
}

hipError_t launch_window_value_bounds(const LaunchCfg& cfg, const WindowValueFrameArgs& a, int64_t n, uint32_t* lo, uint32_t* hi, uint32_t* widest) {
    if (n <= 0) return hipSuccess;
    if ((a.units != WINDOW_UNITS_RANGE && a.units != WINDOW_UNITS_GROUPS) || !a.part_start || !a.part_end) return hipErrorInvalidValue;
    const int kinds[2] = {a.start_kind, a.end_kind};
    for (int k : kinds) {
        if (k < WINDOW_BOUND_UNBOUNDED || k > WINDOW_BOUND_OFFSET) return hipErrorInvalidValue;
        if (k == WINDOW_BOUND_CURRENT_ROW && (!a.peer_start || !a.peer_end)) return hipErrorInvalidValue;
        if (k != WINDOW_BOUND_OFFSET) continue;
        if (a.units == WINDOW_UNITS_GROUPS ? !a.peers_to : !a.key.data || dt_width(a.key.dtype) == 0 || !a.peer_start || !a.peer_end) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(window_value_bounds_kernel, dim3(row_blocks(n)), dim3(WINDOW_BLOCK), 0, cfg.stream, a, n, lo, hi, widest);
    return hipGetLastError();
}

template <int OP>
static hipError_t run_slide_value(const LaunchCfg& cfg, int kind, int out_dtype, const ColumnRef& arg, const uint32_t* lo, const uint32_t* hi, int64_t n,
                                  void* out, uint64_t* validity) {
    const size_t lds = (size_t)WINDOW_SLIDE_STAGE_ROWS * 9;
    hipLaunchKernelGGL((window_slide_value_kernel<OP>), dim3((unsigned)window_tiles(n)), dim3(WINDOW_BLOCK), lds, cfg.stream, arg, lo, hi, n, kind, out_dtype,
                       out, validity);
    return hipGetLastError();
}

hipError_t launch_window_slide_value(const LaunchCfg& cfg, int op, int kind, int out_dtype, const ColumnRef& arg, const uint32_t* lo,
                                     const uint32_t* hi, int64_t n, void* out, uint64_t* validity) {
    if (n <= 0) return hipSuccess;
    if ((kind != WINDOW_FINISH_VALUE && kind != WINDOW_FINISH_AVG) || !arg.data || arg.dtype == DT_UTF8 || arg.dtype == DT_BOOLEAN) return hipErrorInvalidValue;
#define CALL(OP) run_slide_value<OP>(cfg, kind, out_dtype, arg, lo, hi, n, out, validity)
    switch (op) {
        case WINDOW_OP_ADD_F64: return CALL(WINDOW_OP_ADD_F64);
        case WINDOW_OP_MIN_I64: return CALL(WINDOW_OP_MIN_I64);
        case WINDOW_OP_MAX_I64: return CALL(WINDOW_OP_MAX_I64);
        case WINDOW_OP_MIN_U64: return CALL(WINDOW_OP_MIN_U64);
        case WINDOW_OP_MAX_U64: return CALL(WINDOW_OP_MAX_U64);
        case WINDOW_OP_MIN_F64: return CALL(WINDOW_OP_MIN_F64);
        case WINDOW_OP_MAX_F64: return CALL(WINDOW_OP_MAX_F64);
        default: return hipErrorInvalidValue;
    }
#undef CALL
}

}  // namespace bhip
