// scan_device.h — the project's one prefix-scan primitive: the wave-level __shfl_up ladder and the workgroup scan on top of it
// (the wave totals cross through LDS), over a policy.  Beside reduce_device.h, which holds the fixed-order reductions.
//
// A policy P states  P::State,  P::identity(),  P::combine(left, right) (associative),  P::shfl_up(state, d).  The combine tree is
// a function of the thread positions alone, so floating-point scans are reproducible bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace bhip {

__device__ inline uint64_t shfl_up_u64(uint64_t x, int d) {
    const uint32_t lo = __shfl_up((uint32_t)x, d, 64), hi = __shfl_up((uint32_t)(x >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive scan over the 64 lanes of a wave
template <class P>
__device__ inline typename P::State wave_scan_inclusive(typename P::State x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const typename P::State y = P::shfl_up(x, d);
        if (lane >= d) x = P::combine(y, x);
    }
    return x;
}

// inclusive scan over a workgroup of NWAVES waves; s_wave[NWAVES] is LDS of the caller's, free again on return; `total` is the
// combine of the whole workgroup.  Every thread of the workgroup calls it.
template <class P, int NWAVES>
__device__ inline typename P::State block_scan_inclusive(typename P::State x, typename P::State* s_wave, typename P::State& total) {
    using S = typename P::State;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = wave_scan_inclusive<P>(x);
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    S before = P::identity(), tot = P::identity();
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const S s = s_wave[w];
        if (w < wave) before = P::combine(before, s);
        tot = P::combine(tot, s);
    }
    __syncthreads();                       // the next call overwrites s_wave
    total = tot;
    return P::combine(before, x);
}

// ---- the additive instance (uint32_t / uint64_t) ----------------------------------------------------------------------------------
template <class T>
struct SumScan {
    using State = T;
    __device__ static T identity() { return 0; }
    __device__ static T combine(T a, T b) { return a + b; }
    __device__ static uint32_t shfl_up(uint32_t x, int d) { return __shfl_up(x, d, 64); }
    __device__ static uint64_t shfl_up(uint64_t x, int d) { return shfl_up_u64(x, d); }
};

template <class T>
__device__ inline T wave_inclusive_sum(T v) { return wave_scan_inclusive<SumScan<T>>(v); }

// the sum of the threads before this one (the inclusive sum less the thread's own value: no second shuffle)
template <int NWAVES, class T>
__device__ inline T block_exclusive_sum(T v, T* s_wave, T& total) {
    return block_scan_inclusive<SumScan<T>, NWAVES>(v, s_wave, total) - v;
}

}  // namespace bhip
