// kernels_topk.hip — ORDER BY ... LIMIT k as a selection: the rows of one batch that can be among the first k of SortExec's order.
//
// An MSB-first radix select over the FIRST sort key's order-preserving 64-bit image (sort_device.h: the very functions the sort's
// key kernels use, NULL rows and DESC folded the same way, so "smaller image" is "earlier in the output" by construction).  A
// nullable key is ordered by the composite (NULL rank, image).  Each pass histograms one image byte over the rows that still match
// the prefix chosen so far, reading the key column itself (16-byte loads for 4- and 8-byte types), never a materialised image
// buffer; a one-workgroup pick then chooses the bin that holds the k-th row and updates a small state block in device memory that
// the next pass reads — the host queues every pass up front and waits once, for the candidate count.  Bytes on which all images
// agree are skipped on the device (the launch returns at once), as radix_key_diff does for the sort.
//
// Candidates = rows with composite < T plus EVERY row == T (the later keys decide among the ties); the mark kernel writes them as
// the bitmap + tile counts launch_select_indices compacts, which keeps input order — so sorting the candidates with the stable
// sort and cutting at k IS the head of the full stable sort.
#include <hip/hip_runtime.h>
#include "sort_device.h"
#include "topk_kernels.h"

namespace bhip {

constexpr int TK_BLOCK = 256;
constexpr int TK_WAVES = TK_BLOCK / 64;

struct TopkState {
    uint64_t prefix, mask;       // image bits chosen so far / the bytes they cover
    uint64_t diff;               // image bits that differ between any two rows
    uint64_t want;               // rank (1-based) of the k-th row among the rows that match the prefix
    TopkCount count;             // rows strictly before the prefix / rows that match it
    uint32_t null_rank, pad;     // the NULL rank that holds the k-th row (0 where the key has no validity bitmap)
    unsigned long long hist[TOPK_NULL_BYTE + 1][256];     // one histogram per pass, zeroed once; [TOPK_NULL_BYTE][1] = rows of NULL rank 1
};

size_t topk_state_bytes() { return sizeof(TopkState); }
const TopkCount* topk_state_count(const void* state) { return &static_cast<const TopkState*>(state)->count; }

static int topk_width(int dtype) {
    switch (dtype) {
        case DT_UTF8: return 0;
        case DT_INT32: case DT_DATE32: case DT_UINT32: case DT_FLOAT32: return 4;
        case DT_INT64: case DT_UINT64: case DT_FLOAT64: case DT_DATE64:
        case DT_TIMESTAMP_S: case DT_TIMESTAMP_MS: case DT_TIMESTAMP_US: case DT_TIMESTAMP_NS: return 8;
        default: return -1;
    }
}
bool topk_key_supported(int dtype) { return topk_width(dtype) >= 0; }
uint32_t topk_key_bytes(int dtype) {
    switch (dtype) {
        case DT_INT32: case DT_DATE32: return 0x8F;      // sign-extended: bytes 4..6 repeat what byte 7 says
        case DT_UINT32: case DT_FLOAT32: return 0x0F;    // zero-extended
        default: return 0xFF;
    }
}

// the image as the sort sees it: 0 for a NULL row, then the descending flip
__device__ inline uint64_t topk_finish(uint64_t raw, bool valid, int descending) {
    const uint64_t k = valid ? raw : 0ull;
    return descending ? ~k : k;
}
// nulls_first -> NULL = 0, valid = 1 ; nulls last -> NULL = 1, valid = 0 (sort_key_null_kernel)
__device__ inline uint32_t topk_null_rank(bool valid, int nulls_first) { return nulls_first ? (valid ? 1u : 0u) : (valid ? 0u : 1u); }

// W: bytes per value (0: Utf8, image = its first 8 bytes).  VEC rows per thread and step: 16 / W through one 16-byte load where the
// column starts on a 16-byte boundary, else 1.  Rows at or beyond n give 0 and are never read.
template <int W>
__device__ inline uint64_t topk_raw_image(const ColumnRef& c, uint32_t row) {
    return W == 0 ? utf8_key_image(c, row, 0) : fixed_key_image(c, row);
}
template <int W, int VEC>
__device__ inline void topk_load_group(const ColumnRef& c, int64_t g, int64_t n, uint64_t (&raw)[VEC]) {
    const int64_t r0 = g * VEC;
    if (VEC > 1 && r0 + VEC <= n) {
        const uint4 v = reinterpret_cast<const uint4*>(c.data)[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (W == 8) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) raw[i] = key_image_bits8(c.dtype, (uint64_t)w[(2 * i) & 3] | ((uint64_t)w[(2 * i + 1) & 3] << 32));
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) raw[i] = key_image_bits4(c.dtype, w[i & 3]);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) raw[i] = r0 + i < n ? topk_raw_image<W>(c, (uint32_t)(r0 + i)) : 0ull;
}

// diff |= image XOR row 0's image over all rows; hist[NULL byte][1] = rows of NULL rank 1; the first thread arms the state
template <int W, int VEC>
__global__ void __launch_bounds__(TK_BLOCK)
topk_diff_kernel(TopkKey K, int64_t n, int64_t k, TopkState* st) {
    const ColumnRef& c = K.col;
    const uint64_t first = topk_finish(topk_raw_image<W>(c, 0u), row_valid(c.validity, 0u), K.descending);
    uint64_t acc = 0;
    uint32_t rank1 = 0;
    const int64_t n_groups = (n + VEC - 1) / VEC;
    for (int64_t g = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * TK_BLOCK) {
        uint64_t raw[VEC];
        topk_load_group<W, VEC>(c, g, n, raw);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int64_t row = g * VEC + i;
            if (row < n) {
                const bool valid = row_valid(c.validity, (uint32_t)row);
                acc |= topk_finish(raw[i], valid, K.descending) ^ first;
                rank1 += topk_null_rank(valid, K.nulls_first);
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_down((uint32_t)acc, d, 64), hi = __shfl_down((uint32_t)(acc >> 32), d, 64);
        acc |= ((uint64_t)hi << 32) | lo;
        rank1 += __shfl_down(rank1, d, 64);
    }
    __shared__ uint64_t s_acc[TK_WAVES];
    __shared__ uint32_t s_rank1[TK_WAVES];
    if ((threadIdx.x & 63) == 0) { s_acc[threadIdx.x >> 6] = acc; s_rank1[threadIdx.x >> 6] = rank1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0;
        uint32_t r1 = 0;
        for (int w = 0; w < TK_WAVES; ++w) { all |= s_acc[w]; r1 += s_rank1[w]; }
        // only a workgroup that adds a bit sends an atomic (a stale read costs a redundant atomic, never a missing bit)
        if (all & ~__hip_atomic_load(&st->diff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr((unsigned long long*)&st->diff, (unsigned long long)all);
        if (c.validity != nullptr && r1) atomicAdd(&st->hist[TOPK_NULL_BYTE][1], (unsigned long long)r1);
        if (blockIdx.x == 0) { st->want = (uint64_t)k; st->count.equal = (uint64_t)n; }      // (the state was zeroed before the launch)
    }
}

template <int W, int VEC>
__global__ void __launch_bounds__(TK_BLOCK)
topk_hist_kernel(TopkKey K, int64_t n, int byte, TopkState* st) {
    const int shift = 8 * byte;
    if (((st->diff >> shift) & 0xFF) == 0) return;          // every image has the same byte here: no order in it
    const ColumnRef& c = K.col;
    const uint64_t prefix = st->prefix, mask = st->mask;
    const uint32_t null_rank = st->null_rank;
    __shared__ uint32_t s_hist[TK_WAVES][256];                // one private histogram per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < TK_WAVES; ++w) s_hist[w][tid] = 0;
    __syncthreads();
    // whole waves step together (the ballots below): the group count is rounded up to the wave size, rows beyond n match nothing
    const int64_t n_groups = (n + VEC - 1) / VEC, n_round = (n_groups + 63) & ~(int64_t)63;
    const int64_t stride = (int64_t)gridDim.x * TK_BLOCK;
    int64_t g = (int64_t)blockIdx.x * TK_BLOCK + tid;
    uint64_t cur[VEC] = {}, nxt[VEC] = {};
    if (g < n_round) topk_load_group<W, VEC>(c, g, n, cur);
    for (; g < n_round; g += stride) {
        if (g + stride < n_round) topk_load_group<W, VEC>(c, g + stride, n, nxt);     // the next step's loads go out before this step's ballots
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int64_t row = g * VEC + i;
            const bool in = row < n;
            const bool valid = in && row_valid(c.validity, (uint32_t)row);
            const uint64_t img = topk_finish(cur[i], valid, K.descending);
            const bool match = in && ((img ^ prefix) & mask) == 0 && (c.validity == nullptr || topk_null_rank(valid, K.nulls_first) == null_rank);
            const uint32_t digit = (uint32_t)(img >> shift) & 0xFF;
            // the lanes of this wave that hit the same bin add once
            uint64_t same = __ballot(match);
            if (same == 0) continue;                                                      // wave-uniform
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint64_t m = __ballot((digit >> b) & 1);
                same &= ((digit >> b) & 1) ? m : ~m;
            }
            if (match && (same & ((1ull << lane) - 1ull)) == 0) atomicAdd(&s_hist[wave][digit], (uint32_t)__popcll(same));
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) cur[i] = nxt[i];
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < TK_WAVES; ++w) sum += s_hist[w][tid];
    if (sum) atomicAdd(&st->hist[byte][tid], (unsigned long long)sum);                   // one flush per workgroup, non-zero bins only
}

// one workgroup: the bin that holds row `want` of the rows matching the prefix
__global__ void __launch_bounds__(TK_BLOCK)
topk_pick_kernel(int byte, TopkState* st) {
    if (byte < TOPK_NULL_BYTE && ((st->diff >> (8 * byte)) & 0xFF) == 0) return;
    __shared__ uint64_t s_bin[256];
    const int tid = threadIdx.x;
    if (byte == TOPK_NULL_BYTE) {
        const uint64_t r1 = st->hist[TOPK_NULL_BYTE][1];
        s_bin[tid] = tid == 0 ? st->count.equal - r1 : tid == 1 ? r1 : 0ull;
    } else {
        s_bin[tid] = st->hist[byte][tid];
    }
    __syncthreads();
    if (tid != 0) return;
    const uint64_t want = st->want;
    uint64_t before = 0;
    int bin = 0;
    for (; bin < 255; ++bin) {
        if (before + s_bin[bin] >= want) break;
        before += s_bin[bin];
    }
    st->count.less += before;
    st->count.equal = s_bin[bin];
    st->want = want - before;
    if (byte == TOPK_NULL_BYTE) st->null_rank = (uint32_t)bin;
    else { st->prefix |= (uint64_t)bin << (8 * byte); st->mask |= 0xFFull << (8 * byte); }
}

// bit i = row i's composite <= the threshold; tile_counts[t] = candidates of tile t (SEL_TILE rows, one workgroup)
template <int W>
__global__ void __launch_bounds__(TK_BLOCK)
topk_mark_kernel(TopkKey K, int64_t n, const TopkState* st, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ tile_counts) {
    static_assert(SEL_TILE % TK_BLOCK == 0 && TK_WAVES == 4, "a tile is a whole number of steps of 4 waves");
    const ColumnRef& c = K.col;
    const uint64_t prefix = st->prefix, mask = st->mask;      // bytes outside the mask agree in every row of the threshold's NULL rank
    const uint32_t null_rank = st->null_rank;
    __shared__ uint32_t s_cnt[TK_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile_base = (int64_t)blockIdx.x * SEL_TILE;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < SEL_TILE / TK_BLOCK; ++k) {
        const int64_t row0 = tile_base + wave * (SEL_TILE / TK_WAVES) + k * 64, row = row0 + lane;
        bool keep = false;
        if (row < n) {
            const bool valid = row_valid(c.validity, (uint32_t)row);
            const uint64_t img = topk_finish(topk_raw_image<W>(c, (uint32_t)row), valid, K.descending);
            const uint32_t rank = c.validity == nullptr ? 0u : topk_null_rank(valid, K.nulls_first);
            keep = rank < null_rank || (rank == null_rank && (img & mask) <= prefix);
        }
        const uint64_t w = __ballot(keep);
        if (lane == 0 && row0 < n) bitmap[row0 >> 6] = w;
        cnt += (uint32_t)__popcll(w);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
static bool topk_args_ok(const TopkKey& key, int64_t n) {
    const int w = topk_width(key.col.dtype);
    return w >= 0 && n >= 1 && n <= 0xFFFFFFF0ll && key.col.data != nullptr && (w != 0 || key.col.offsets != nullptr);
}
// rows per thread and step: 16-byte loads need the column on a 16-byte boundary (a slice of a larger buffer may start anywhere)
static int topk_vec(const TopkKey& key) {
    const int w = topk_width(key.col.dtype);
    return w > 0 && (reinterpret_cast<uintptr_t>(key.col.data) & 15) == 0 ? 16 / w : 1;
}
int topk_rows_per_load(const TopkKey& key) { return topk_vec(key); }
static bool topk_vec_ok(const TopkKey& key, int vec) { return vec == 1 || vec == topk_vec(key); }
static unsigned topk_grid(const LaunchCfg& cfg, int64_t n, int vec) {
    const int64_t groups = (n + vec - 1) / vec;
    int64_t g = (groups + TK_BLOCK - 1) / TK_BLOCK;
    const int64_t cap = (int64_t)cfg.device_cus * 4;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}
#define TOPK_LAUNCH(KERNEL, grid, ...)                                                                                             \
    switch (topk_width(key.col.dtype) * 8 + vec) {                                                                                 \
        case 0 * 8 + 1: hipLaunchKernelGGL((KERNEL<0, 1>), dim3(grid), dim3(TK_BLOCK), 0, cfg.stream, __VA_ARGS__); break;       \
        case 4 * 8 + 1: hipLaunchKernelGGL((KERNEL<4, 1>), dim3(grid), dim3(TK_BLOCK), 0, cfg.stream, __VA_ARGS__); break;       \
        case 4 * 8 + 4: hipLaunchKernelGGL((KERNEL<4, 4>), dim3(grid), dim3(TK_BLOCK), 0, cfg.stream, __VA_ARGS__); break;       \
        case 8 * 8 + 1: hipLaunchKernelGGL((KERNEL<8, 1>), dim3(grid), dim3(TK_BLOCK), 0, cfg.stream, __VA_ARGS__); break;       \
        default: hipLaunchKernelGGL((KERNEL<8, 2>), dim3(grid), dim3(TK_BLOCK), 0, cfg.stream, __VA_ARGS__); break;              \
    }

hipError_t launch_topk_diff(const LaunchCfg& cfg, const TopkKey& key, int vec, int64_t n, int64_t k, void* state) {
    if (!topk_args_ok(key, n) || !topk_vec_ok(key, vec) || k < 1 || k > n) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(state, 0, sizeof(TopkState), cfg.stream);
    if (e != hipSuccess) return e;
    TOPK_LAUNCH(topk_diff_kernel, topk_grid(cfg, n, vec), key, n, k, static_cast<TopkState*>(state));
    return hipGetLastError();
}

hipError_t launch_topk_hist(const LaunchCfg& cfg, const TopkKey& key, int vec, int64_t n, int byte, void* state) {
    if (!topk_args_ok(key, n) || !topk_vec_ok(key, vec) || byte < 0 || byte >= TOPK_NULL_BYTE) return hipErrorInvalidValue;
    TOPK_LAUNCH(topk_hist_kernel, topk_grid(cfg, n, vec), key, n, byte, static_cast<TopkState*>(state));
    return hipGetLastError();
}

hipError_t launch_topk_pick(const LaunchCfg& cfg, int byte, void* state) {
    if (byte < 0 || byte > TOPK_NULL_BYTE) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(TK_BLOCK), 0, cfg.stream, byte, static_cast<TopkState*>(state));
    return hipGetLastError();
}

hipError_t launch_topk_mark(const LaunchCfg& cfg, const TopkKey& key, int64_t n, const void* state, uint64_t* bitmap, uint32_t* tile_counts) {
    if (!topk_args_ok(key, n)) return hipErrorInvalidValue;
    const unsigned n_tiles = (unsigned)((n + SEL_TILE - 1) / SEL_TILE);
    const TopkState* st = static_cast<const TopkState*>(state);
    switch (topk_width(key.col.dtype)) {
        case 0: hipLaunchKernelGGL(topk_mark_kernel<0>, dim3(n_tiles), dim3(TK_BLOCK), 0, cfg.stream, key, n, st, bitmap, tile_counts); break;
        case 4: hipLaunchKernelGGL(topk_mark_kernel<4>, dim3(n_tiles), dim3(TK_BLOCK), 0, cfg.stream, key, n, st, bitmap, tile_counts); break;
        default: hipLaunchKernelGGL(topk_mark_kernel<8>, dim3(n_tiles), dim3(TK_BLOCK), 0, cfg.stream, key, n, st, bitmap, tile_counts); break;
    }
    return hipGetLastError();
}

}  // namespace bhip
