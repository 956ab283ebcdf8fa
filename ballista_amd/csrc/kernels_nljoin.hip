// kernels_nljoin.hip — NestedLoopJoinExec on the device (host/ops_join.cpp "nested loop join"; declarations and constants: nljoin_kernels.h).
//
// The fused route (nlj_compare_count / nlj_compare_emit).  Probe rows sit on lanes, one row per lane, 256 rows per workgroup; a row's
// operands (up to NLJ_MAX_TERMS) are loaded once, widened to the VM's 64-bit images (vm_isa.h dt_load) and kept in registers with one
// valid bit per term.  The build rows pass through LDS in tiles of NLJ_BUILD_TILE rows, structure of arrays: vals[term][row] and one
// mask word per row (bit t: the row's operand of term t is not NULL).  Staging is one build row per thread per round, so consecutive
// lanes read consecutive values of each column (coalesced) and write consecutive LDS words.  In the inner loop every lane of a wave
// reads the SAME LDS address (build row j's operand): identical addresses broadcast, no bank conflict.  The compare is the VM's
// cmp_vals<T> (vm_device.h), so NaN, -0.0 and signed / unsigned order mean here what they mean in a FilterExec.
//
// Two passes, as the hash join's enumerate_pairs: count, exclusive scan (kernels_util.hip), emit.  A probe row's pairs are consecutive,
// build rows ascending: the output order is a function of the input alone.  Every workgroup loops over all build tiles on its own:
// nothing waits on another workgroup, every loop bound is a kernel argument.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "nljoin_kernels.h"
#include "vm_device.h"

namespace bhip {

namespace {

__device__ inline bool nlj_bit(const uint64_t* words, uint32_t i) { return !words || ((words[i >> 6] >> (i & 63)) & 1); }

// one term over one pair: a = the build row's image, b = the probe row's
__device__ inline bool nlj_term(uint64_t a, uint64_t b, int vclass, int cmp) {
    if (vclass == NLJ_F64) return cmp_vals<double>(u2d(a), u2d(b), cmp);
    if (vclass == NLJ_U64) return cmp_vals<uint64_t>(a, b, cmp);
    return cmp_vals<int64_t>((int64_t)a, (int64_t)b, cmp);
}

// the loop both passes run.  EMIT: write the pairs at `pos`; else count them, and (MARK) collect the build rows' matched bits.
// LDS: vals[T.n][NLJ_BUILD_TILE] (8 B each), then mask[NLJ_BUILD_TILE] (4 B each)
template <bool EMIT, bool MARK>
__device__ inline uint32_t nlj_scan(const NljTerms& T, uint32_t n_build, uint32_t n_probe, uint32_t* matched, uint64_t pos, uint32_t* lidx,
                                    uint32_t* ridx) {
    extern __shared__ uint64_t nlj_lds[];
    uint64_t* vals = nlj_lds;
    uint32_t* mask = reinterpret_cast<uint32_t*>(nlj_lds + (size_t)T.n * NLJ_BUILD_TILE);
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t row = blockIdx.x * NLJ_BLOCK + tid;
    const bool live = row < n_probe;
    uint64_t pv[NLJ_MAX_TERMS];
    uint32_t pk = 0;                                  // bit t: this lane's operand of term t is there (a row past the batch: none)
#pragma unroll
    for (int t = 0; t < NLJ_MAX_TERMS; ++t) {
        pv[t] = 0;
        if (t < T.n && live) {
            pv[t] = dt_load(T.t[t].probe.dtype, T.t[t].probe.data, row);
            if (nlj_bit(T.t[t].probe.validity, row)) pk |= 1u << t;
        }
    }
    const uint32_t all = (1u << T.n) - 1u;
    uint32_t count = 0;
    for (uint32_t base = 0; base < n_build; base += NLJ_BUILD_TILE) {
        const uint32_t rows = n_build - base < (uint32_t)NLJ_BUILD_TILE ? n_build - base : (uint32_t)NLJ_BUILD_TILE;
        __syncthreads();                              // the tile before this one has been read by every wave
        for (uint32_t i = tid; i < rows; i += NLJ_BLOCK) {
            uint32_t m = 0;
#pragma unroll
            for (int t = 0; t < NLJ_MAX_TERMS; ++t) {
                if (t < T.n) {
                    vals[t * NLJ_BUILD_TILE + i] = dt_load(T.t[t].build.dtype, T.t[t].build.data, base + i);
                    if (nlj_bit(T.t[t].build.validity, base + i)) m |= 1u << t;
                }
            }
            mask[i] = m;
        }
        __syncthreads();
        // a lane without all its operands has no partner: it still walks the tile (the barriers above are the workgroup's)
        const bool can = (pk & all) == all && live;
        for (uint32_t j0 = 0; j0 < rows; j0 += 64) {
            const uint32_t j1 = rows - j0 < 64u ? rows - j0 : 64u;
            bool mine = false;                        // MARK: build row j0 + lane has a partner among this wave's probe rows
            for (uint32_t k = 0; k < j1; ++k) {
                const uint32_t j = j0 + k;
                bool ok = can && mask[j] == all;
#pragma unroll
                for (int t = 0; t < NLJ_MAX_TERMS; ++t)
                    if (t < T.n) ok = ok && nlj_term(vals[t * NLJ_BUILD_TILE + j], pv[t], T.t[t].vclass, T.t[t].cmp);
                if (EMIT) {
                    if (ok) { lidx[pos] = base + j; ridx[pos] = row; ++pos; }
                } else {
                    count += ok ? 1u : 0u;
                    if (MARK) {
                        const bool any = __ballot(ok) != 0ull;
                        if ((uint32_t)lane == k) mine = any;
                    }
                }
            }
            if (MARK) {
                // 64 build rows' bits in one word of the wave; two 32-bit words of `matched`, read before they are written
                const unsigned long long w = __ballot(mine);
                if (lane == 0 && w) {
                    const uint32_t wi = (base + j0) >> 5, lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
                    if (lo && (matched[wi] & lo) != lo) atomicOr(&matched[wi], lo);
                    if (hi && (matched[wi + 1] & hi) != hi) atomicOr(&matched[wi + 1], hi);
                }
            }
        }
    }
    return count;
}

__global__ void __launch_bounds__(NLJ_BLOCK)
nlj_compare_count_kernel(NljTerms T, uint32_t n_build, uint32_t n_probe, uint32_t* counts, uint32_t* matched, unsigned long long* hit) {
    const uint32_t count = matched ? nlj_scan<false, true>(T, n_build, n_probe, matched, 0, nullptr, nullptr)
                                   : nlj_scan<false, false>(T, n_build, n_probe, nullptr, 0, nullptr, nullptr);
    const uint32_t row = blockIdx.x * NLJ_BLOCK + threadIdx.x;
    if (row < n_probe) counts[row] = count;
    if (hit) {
        // this wave's 64 probe rows are one word of `hit`, and its own: a plain store (rows past the batch counted nothing)
        const unsigned long long h = __ballot(count != 0);
        const uint32_t row0 = row & ~63u;
        if ((threadIdx.x & 63) == 0 && row0 < n_probe) hit[row0 >> 6] = h;
    }
}

__global__ void __launch_bounds__(NLJ_BLOCK)
nlj_compare_emit_kernel(NljTerms T, uint32_t n_build, uint32_t n_probe, const uint64_t* offsets, uint32_t* lidx, uint32_t* ridx) {
    const uint32_t row = blockIdx.x * NLJ_BLOCK + threadIdx.x;
    nlj_scan<true, false>(T, n_build, n_probe, nullptr, row < n_probe ? offsets[row] : 0, lidx, ridx);
}

__global__ void __launch_bounds__(NLJ_BLOCK)
nlj_cross_pairs_kernel(uint32_t n_build, uint64_t p0, uint64_t n, uint32_t* lidx, uint32_t* ridx) {
    for (uint64_t k = (uint64_t)blockIdx.x * NLJ_BLOCK + threadIdx.x; k < n; k += (uint64_t)gridDim.x * NLJ_BLOCK) {
        const uint64_t p = p0 + k, r = p / n_build;
        lidx[k] = (uint32_t)(p - r * n_build);
        ridx[k] = (uint32_t)r;
    }
}

size_t nlj_lds_bytes(const NljTerms& T) { return (size_t)T.n * NLJ_BUILD_TILE * 8 + (size_t)NLJ_BUILD_TILE * 4; }

}  // namespace

hipError_t launch_nlj_cross_pairs(const LaunchCfg& cfg, uint32_t n_build, uint64_t p0, uint64_t p1, uint32_t* lidx, uint32_t* ridx) {
    if (p1 <= p0 || n_build == 0) return hipSuccess;
    const uint64_t n = p1 - p0;
    uint64_t grid = (n + NLJ_BLOCK - 1) / NLJ_BLOCK;
    const uint64_t cap = (uint64_t)cfg.device_cus * 16;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(nlj_cross_pairs_kernel, dim3((unsigned)grid), dim3(NLJ_BLOCK), 0, cfg.stream, n_build, p0, n, lidx, ridx);
    return hipGetLastError();
}

hipError_t launch_nlj_compare_count(const LaunchCfg& cfg, const NljTerms& T, uint32_t n_build, uint32_t n_probe, uint32_t* counts, uint32_t* matched,
                                    uint64_t* hit) {
    if (n_probe == 0) return hipSuccess;
    if (T.n < 1 || T.n > NLJ_MAX_TERMS) return hipErrorInvalidValue;
    const unsigned grid = (n_probe + NLJ_BLOCK - 1) / NLJ_BLOCK;
    hipLaunchKernelGGL(nlj_compare_count_kernel, dim3(grid), dim3(NLJ_BLOCK), nlj_lds_bytes(T), cfg.stream, T, n_build, n_probe, counts, matched,
                       reinterpret_cast<unsigned long long*>(hit));
    return hipGetLastError();
}

hipError_t launch_nlj_compare_emit(const LaunchCfg& cfg, const NljTerms& T, uint32_t n_build, uint32_t n_probe, const uint64_t* offsets, uint32_t* lidx,
                                   uint32_t* ridx) {
    if (n_probe == 0) return hipSuccess;
    if (T.n < 1 || T.n > NLJ_MAX_TERMS) return hipErrorInvalidValue;
    const unsigned grid = (n_probe + NLJ_BLOCK - 1) / NLJ_BLOCK;
    hipLaunchKernelGGL(nlj_compare_emit_kernel, dim3(grid), dim3(NLJ_BLOCK), nlj_lds_bytes(T), cfg.stream, T, n_build, n_probe, offsets, lidx, ridx);
    return hipGetLastError();
}

}  // namespace bhip
