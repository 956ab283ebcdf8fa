// kernels_cast.hip — CAST between Utf8 and the fixed-width types (integers, Boolean, Date32, floats) on the device.
//
// The reference hands a `Cast` expression to arrow's cast kernel (rust/core/src/serde/physical_plan/from_proto.rs:348-364 via
// DataFusion's create_physical_expr); the value grammar is restated once in cast_text.h and shared with the host's literal folding.
// Like every string-producing node (kernels_str.hip) a cast is a new column, not a VM instruction: the host
// (host/utf8_exprs.cpp) evaluates it as an extra column of the batch and the rest of the expression goes to the VM.
//
//   Utf8 -> T     one thread per row walks its bytes in HBM; value, and the validity as one ballot word per wave64
//   T -> Utf8     lengths -> exclusive scan (offsets) -> bytes, the shape of str_transform_*
//
// to_timestamp (Utf8 -> Timestamp(Nanosecond)), date_trunc (Timestamp -> Timestamp) and date_part (Date32 / Date64 / Timestamp ->
// Int32) are lowered the same way and live here; their grammar and calendar arithmetic are temporal_text.h.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "cast_kernels.h"
#include "cast_text.h"
#include "temporal_text.h"

namespace bhip {

namespace {
constexpr int BLOCK = 256;       // 4 waves; a wave's 64 rows start at a multiple of 64: one validity word

__device__ inline bool bit_at(const uint64_t* bits, int64_t i) { return bits == nullptr || ((bits[i >> 6] >> (i & 63)) & 1ull); }

// the value of parse result `bits` in the column's storage type
template <typename T> __device__ inline T stored(uint64_t bits) { return (T)bits; }
template <> __device__ inline double stored<double>(uint64_t bits) { return cast_bits_f64(bits); }
template <> __device__ inline float stored<float>(uint64_t bits) { return cast_bits_f32((uint32_t)bits); }

// T = the target's storage type; bool: the values are a bitmap, written like the validity.  Rows are taken 64 at a time by whole
// waves (the loop runs to n rounded up), so the lanes past n still vote — with `false` — and the last wave writes its partial word.
template <typename T>
__global__ void __launch_bounds__(BLOCK)
cast_parse_kernel(ColumnRef c, int64_t n, int to, T* out, uint64_t* out_bits, uint64_t* validity, uint32_t* status) {
    const int64_t n_round = (n + 63) & ~(int64_t)63;
    bool declined = false;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * BLOCK) {
        bool valid = false;
        uint64_t bits = 0;
        if (i < n) {
            if (bit_at(c.validity, i)) {
                const CastPtrReader rd{reinterpret_cast<const uint8_t*>(c.data)};
                const int r = cast_parse(rd, (int64_t)c.offsets[i], (int64_t)c.offsets[i + 1], to, bits);
                valid = r == CAST_VALUE;
                declined |= r == CAST_DECLINED;
                if (!valid) bits = 0;
            }
            if constexpr (!std::is_same<T, bool>::value) out[i] = stored<T>(bits);       // 0 for a NULL: the bytes stay defined
        }
        const uint64_t vw = __ballot(valid);
        if constexpr (std::is_same<T, bool>::value) {
            const uint64_t bw = __ballot(valid && bits != 0);
            if ((threadIdx.x & 63) == 0) out_bits[i >> 6] = bw;
        }
        if ((threadIdx.x & 63) == 0) validity[i >> 6] = vw;
    }
    if (dt_is_float(to)) {
        const uint64_t any = __ballot(declined);
        if (any != 0 && (threadIdx.x & 63) == 0) atomicOr(status, CAST_STATUS_DECLINED);
    }
}

// value i of a fixed-width column as the VM holds it: sign- or zero-extended, Boolean 0 / 1
__device__ inline uint64_t load_value(const ColumnRef& c, int64_t i) {
    switch (c.dtype) {
        case DT_BOOLEAN: return (reinterpret_cast<const uint64_t*>(c.data)[i >> 6] >> (i & 63)) & 1ull;
        case DT_INT8: return (uint64_t)(int64_t) reinterpret_cast<const int8_t*>(c.data)[i];
        case DT_UINT8: return reinterpret_cast<const uint8_t*>(c.data)[i];
        case DT_INT16: return (uint64_t)(int64_t) reinterpret_cast<const int16_t*>(c.data)[i];
        case DT_UINT16: return reinterpret_cast<const uint16_t*>(c.data)[i];
        case DT_INT32: case DT_DATE32: return (uint64_t)(int64_t) reinterpret_cast<const int32_t*>(c.data)[i];
        case DT_UINT32: return reinterpret_cast<const uint32_t*>(c.data)[i];
        default: return reinterpret_cast<const uint64_t*>(c.data)[i];
    }
}

__global__ void __launch_bounds__(BLOCK)
cast_format_lengths_kernel(ColumnRef c, int64_t n, uint32_t* lengths, uint64_t* validity_out) {
    const int64_t n_round = (n + 63) & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * BLOCK) {
        bool valid = false;
        if (i < n) {
            int len = -1;
            if (bit_at(c.validity, i)) len = cast_format(c.dtype, load_value(c, i), nullptr);
            valid = len >= 0;
            lengths[i] = valid ? (uint32_t)len : 0u;
        }
        const uint64_t vw = __ballot(valid);
        if (validity_out != nullptr && (threadIdx.x & 63) == 0) validity_out[i >> 6] = vw;
    }
}

__global__ void __launch_bounds__(BLOCK)
cast_format_write_kernel(ColumnRef c, int64_t n, const int32_t* out_offsets, uint8_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const int32_t d0 = out_offsets[i];
        const int len = out_offsets[i + 1] - d0;
        if (len == 0) continue;                     // a NULL row (no value has an empty text)
        uint8_t buf[CAST_TEXT_MAX];
        cast_format(c.dtype, load_value(c, i), buf);
        for (int k = 0; k < len; ++k) out[d0 + k] = buf[k];
    }
}

// to_timestamp: one thread per row walks its bytes, as cast_parse_kernel does.  A NULL row stays NULL (the result shares the
// argument's validity) and gets a defined 0; a non-NULL text outside the grammar raises the status bit — the query fails.
__global__ void __launch_bounds__(BLOCK)
to_timestamp_parse_kernel(ColumnRef c, int64_t n, int64_t* out, uint32_t* status) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        int64_t v = 0;
        if (bit_at(c.validity, i)) {
            const CastPtrReader rd{reinterpret_cast<const uint8_t*>(c.data)};
            bad |= !to_timestamp_parse(rd, (int64_t)c.offsets[i], (int64_t)c.offsets[i + 1], v);
        }
        out[i] = v;
    }
    if (bad) atomicOr(status, TO_TIMESTAMP_STATUS_INVALID);
}

// date_trunc: a streaming kernel, 8 bytes in and 8 bytes out per row plus the validity — one ballot word per wave64, the lanes
// past n voting `false` (the loop runs to n rounded up)
__global__ void __launch_bounds__(BLOCK)
date_trunc_kernel(ColumnRef c, int64_t n, int g, int64_t* out, uint64_t* validity) {
    const int64_t n_round = (n + 63) & ~(int64_t)63;
    const int64_t* in = reinterpret_cast<const int64_t*>(c.data);
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * BLOCK) {
        bool valid = false;
        if (i < n) {
            int64_t v = 0;
            valid = bit_at(c.validity, i) && temporal_trunc(c.dtype, g, in[i], v);
            out[i] = valid ? v : 0;                     // 0 for a NULL: the bytes stay defined
        }
        const uint64_t vw = __ballot(valid);
        if ((threadIdx.x & 63) == 0) validity[i >> 6] = vw;
    }
}

// date_part: one Int32 field per row of a Date32 / Date64 / Timestamp column, the validity as date_trunc_kernel writes it: NULL
// where the argument is, or where the field does not fit Int32
__global__ void __launch_bounds__(BLOCK)
date_part_kernel(ColumnRef c, int64_t n, int part, int32_t* out, uint64_t* validity) {
    const int64_t n_round = (n + 63) & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * BLOCK) {
        bool valid = false;
        if (i < n) {
            int32_t v = 0;
            valid = bit_at(c.validity, i) && temporal_part(c.dtype, part, (int64_t)load_value(c, i), v);
            out[i] = valid ? v : 0;                     // 0 for a NULL: the bytes stay defined
        }
        const uint64_t vw = __ballot(valid);
        if ((threadIdx.x & 63) == 0) validity[i >> 6] = vw;
    }
}

inline int grid_of(const LaunchCfg& cfg, int64_t n) {
    const int64_t want = (n + BLOCK - 1) / BLOCK, cap = (int64_t)cfg.device_cus * 8;
    return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

template <typename T>
hipError_t parse_as(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int to, void* out, uint64_t* validity, uint32_t* status) {
    hipLaunchKernelGGL(cast_parse_kernel<T>, dim3(grid_of(cfg, n)), dim3(BLOCK), 0, cfg.stream, c, n, to, reinterpret_cast<T*>(out),
                       reinterpret_cast<uint64_t*>(out), validity, status);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_cast_parse(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int to, void* out, uint64_t* validity, uint32_t* status) {
    if (!cast_parse_supported(to) || c.dtype != DT_UTF8) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (to == DT_BOOLEAN) return parse_as<bool>(cfg, c, n, to, out, validity, status);
    if (to == DT_FLOAT64) return parse_as<double>(cfg, c, n, to, out, validity, status);
    if (to == DT_FLOAT32) return parse_as<float>(cfg, c, n, to, out, validity, status);
    switch (dt_width(to)) {
        case 1: return parse_as<uint8_t>(cfg, c, n, to, out, validity, status);
        case 2: return parse_as<uint16_t>(cfg, c, n, to, out, validity, status);
        case 4: return parse_as<uint32_t>(cfg, c, n, to, out, validity, status);
        default: return parse_as<uint64_t>(cfg, c, n, to, out, validity, status);
    }
}

hipError_t launch_to_timestamp_parse(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int64_t* out, uint32_t* status) {
    if (c.dtype != DT_UTF8) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(to_timestamp_parse_kernel, dim3(grid_of(cfg, n)), dim3(BLOCK), 0, cfg.stream, c, n, out, status);
    return hipGetLastError();
}

hipError_t launch_date_trunc(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int granularity, int64_t* out, uint64_t* validity) {
    if (timestamp_units_per_second(c.dtype) == 0 || granularity < 0 || granularity >= TRUNC_COUNT) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(date_trunc_kernel, dim3(grid_of(cfg, n)), dim3(BLOCK), 0, cfg.stream, c, n, granularity, out, validity);
    return hipGetLastError();
}

hipError_t launch_date_part(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, int part, int32_t* out, uint64_t* validity) {
    if (temporal_units_per_day(c.dtype) == 0 || part < 0 || part >= PART_COUNT) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(date_part_kernel, dim3(grid_of(cfg, n)), dim3(BLOCK), 0, cfg.stream, c, n, part, out, validity);
    return hipGetLastError();
}

hipError_t launch_cast_format_lengths(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, uint32_t* lengths, uint64_t* validity_out) {
    if (!cast_format_supported(c.dtype)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cast_format_lengths_kernel, dim3(grid_of(cfg, n)), dim3(BLOCK), 0, cfg.stream, c, n, lengths, validity_out);
    return hipGetLastError();
}

hipError_t launch_cast_format_write(const LaunchCfg& cfg, const ColumnRef& c, int64_t n, const int32_t* out_offsets, uint8_t* out) {
    if (!cast_format_supported(c.dtype)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cast_format_write_kernel, dim3(grid_of(cfg, n)), dim3(BLOCK), 0, cfg.stream, c, n, out_offsets, out);
    return hipGetLastError();
}

}  // namespace bhip
