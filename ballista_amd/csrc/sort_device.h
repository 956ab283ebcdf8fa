// sort_device.h — the order-preserving u64 images of SortExec's keys (device side), shared by the sort (kernels_sort.hip) and the
// top-k select (kernels_topk.hip): one definition, so "smaller image" means "earlier in the sorted output" in both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vm_isa.h"

namespace bhip {

// image of the raw bits of a 4-byte / 8-byte fixed-width value: unsigned order of the images == the type's order
// (floats: total order by sign-magnitude flip, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
__device__ inline uint64_t key_image_bits4(int dtype, uint32_t b) {
    constexpr uint64_t SIGN = 0x8000000000000000ull;
    switch (dtype) {
        case DT_UINT32: return b;
        case DT_FLOAT32: return (b >> 31) ? (uint32_t)~b : (b | 0x80000000u);
        default: return (uint64_t)(int64_t)(int32_t)b ^ SIGN;          // Int32, Date32
    }
}
__device__ inline uint64_t key_image_bits8(int dtype, uint64_t b) {
    constexpr uint64_t SIGN = 0x8000000000000000ull;
    switch (dtype) {
        case DT_UINT64: return b;
        case DT_FLOAT64: return (b >> 63) ? ~b : (b | SIGN);
        default: return b ^ SIGN;                                      // Int64, Date64, Timestamp*
    }
}

__device__ inline uint64_t fixed_key_image(const ColumnRef& c, uint32_t row) {
    constexpr uint64_t SIGN = 0x8000000000000000ull;
    switch (c.dtype) {
        case DT_INT8: return (uint64_t)(int64_t) reinterpret_cast<const int8_t*>(c.data)[row] ^ SIGN;
        case DT_INT16: return (uint64_t)(int64_t) reinterpret_cast<const int16_t*>(c.data)[row] ^ SIGN;
        case DT_INT32:
        case DT_DATE32:
        case DT_UINT32:
        case DT_FLOAT32: return key_image_bits4(c.dtype, reinterpret_cast<const uint32_t*>(c.data)[row]);
        case DT_UINT8: return reinterpret_cast<const uint8_t*>(c.data)[row];
        case DT_UINT16: return reinterpret_cast<const uint16_t*>(c.data)[row];
        case DT_BOOLEAN: return (reinterpret_cast<const uint8_t*>(c.data)[row >> 3] >> (row & 7)) & 1u;
        default: return key_image_bits8(c.dtype, reinterpret_cast<const uint64_t*>(c.data)[row]);   // Int64, UInt64, Date64, Timestamp*, Float64
    }
}
__device__ inline bool row_valid(const uint64_t* validity, uint32_t row) {
    return validity == nullptr || ((validity[row >> 6] >> (row & 63)) & 1ull);
}

// Utf8: chunk `chunk` = bytes [8*chunk, 8*chunk+8) big-endian, zero padded; chunk == -1: the length
__device__ inline uint64_t utf8_key_image(const ColumnRef& c, uint32_t row, int chunk) {
    const int32_t o0 = c.offsets[row], len = c.offsets[row + 1] - o0;
    if (chunk < 0) return (uint64_t)(uint32_t)len;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(c.data) + o0;
    uint64_t k = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int p = chunk * 8 + b;
        k = (k << 8) | (p < len ? s[p] : 0u);
    }
    return k;
}

}  // namespace bhip
