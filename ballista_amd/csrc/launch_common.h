// launch_common.h — launch-geometry helpers shared by the kernels_*.hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "kernels.h"
#include "sop.h"
#include "vm_device.h"

namespace bhip {

template <int R>
static size_t host_tile_bytes(const VmProgram& G) {
    constexpr int TILE = BLOCK * R;
    size_t b = (size_t)G.n_vslots * TILE * 8;
    if (G.nullable) b += (size_t)G.n_vslots * TILE;
    b += (size_t)G.n_bslots * TILE;
    return (b + 15) & ~(size_t)15;
}

constexpr size_t LDS_PER_CU = 160 * 1024;

template <class K>
static hipError_t set_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// rows per thread: 4 when at least two workgroups still fit a CU's LDS, else 2.
// BHIP_SCAN_R=2|4 overrides (tuning experiments).
static int choose_r(const VmProgram& G, size_t extra) {
    static const int forced = env_int("BHIP_SCAN_R", 0);
    if (forced == 2) return 2;
    if (forced == 4 && host_tile_bytes<4>(G) + extra <= LDS_PER_CU) return 4;
    return (host_tile_bytes<4>(G) + extra) * 2 <= LDS_PER_CU ? 4 : 2;
}

static int pick_grid(const LaunchCfg& cfg, int64_t n_tiles, size_t lds_bytes, int vgpr_blocks_per_cu) {
    int by_lds = (int)(LDS_PER_CU / (lds_bytes ? lds_bytes : 1));
    if (by_lds < 1) by_lds = 1;
    int per_cu = by_lds < vgpr_blocks_per_cu ? by_lds : vgpr_blocks_per_cu;
    int64_t g = (int64_t)cfg.device_cus * per_cu;
    if (g > n_tiles) g = n_tiles;
    if (g < 1) g = 1;
    return (int)g;
}

// ---- the register-path aggregate kernels: one resident wave of workgroups, every workgroup strides over the tiles -------------
// grid: the CUs x the blocks per CU the kernel's resources admit (BHIP_AGG_BLOCKS_PER_CU overrides), at most one workgroup per
// tile and at most max_grid
static hipError_t agg_grid(const void* kernel, size_t lds_bytes, int64_t n_tiles, int max_grid, int device_cus, int64_t* grid_out) {
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, BLOCK, lds_bytes);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    static const int forced_per_cu = env_int("BHIP_AGG_BLOCKS_PER_CU", 0);
    if (forced_per_cu > 0) per_cu = forced_per_cu;
    int64_t grid = (int64_t)device_cus * per_cu;
    if (grid > n_tiles) grid = n_tiles;
    if (grid > max_grid) grid = max_grid;
    if (grid < 1) grid = 1;
    *grid_out = grid;
    return hipSuccess;
}

// the kernels over a SopProgram (sop_kernel.h, lean_kernel.h, lean_spec_kernel.h): tiles of `tile` rows, no dynamic LDS
template <typename Kernel>
static hipError_t launch_sop_program(Kernel k, int tile, const LaunchCfg& cfg, const SopProgram& S, SopProgram* dprog, GroupRec* partials,
                                     uint32_t* partial_ng, int max_grid, ScanStatus* status, int* grid_out) {
    int64_t grid = 0;
    hipError_t e = agg_grid(reinterpret_cast<const void*>(k), 0, (S.n_rows + tile - 1) / tile, max_grid, cfg.device_cus, &grid);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(dprog, &S, sizeof(SopProgram), hipMemcpyHostToDevice, cfg.stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(BLOCK), 0, cfg.stream, (const SopProgram*)dprog, partials, partial_ng, status);
    *grid_out = (int)grid;
    return hipGetLastError();
}

}  // namespace bhip
