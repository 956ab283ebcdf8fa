// kernels_sop.hip — dispatcher of the register-resident scan + aggregate fast path
// (kernel: sop_kernel.h; instantiations: kernels_sop_g{1,4,8}.hip; plan table: sop.h).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "sop.h"

namespace bhip {

hipError_t launch_scan_agg_sop_g1(const LaunchCfg&, const SopProgram&, SopProgram*, GroupRec*, uint32_t*, int, ScanStatus*, int*);
hipError_t launch_scan_agg_sop_g4(const LaunchCfg&, const SopProgram&, SopProgram*, GroupRec*, uint32_t*, int, ScanStatus*, int*);
hipError_t launch_scan_agg_sop_g8(const LaunchCfg&, const SopProgram&, SopProgram*, GroupRec*, uint32_t*, int, ScanStatus*, int*);

hipError_t launch_scan_agg_sop(const LaunchCfg& cfg, const SopProgram& S, SopProgram* dprog, int gmax, GroupRec* partials,
                               uint32_t* partial_ng, int max_grid, ScanStatus* status, int* grid_out) {
    switch (gmax) {
        case 1: return launch_scan_agg_sop_g1(cfg, S, dprog, partials, partial_ng, max_grid, status, grid_out);
        case 4: return launch_scan_agg_sop_g4(cfg, S, dprog, partials, partial_ng, max_grid, status, grid_out);
        case 8: return launch_scan_agg_sop_g8(cfg, S, dprog, partials, partial_ng, max_grid, status, grid_out);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_agg_lean_g1(const LaunchCfg&, const SopProgram&, SopProgram*, GroupRec*, uint32_t*, int, ScanStatus*, int*);
hipError_t launch_scan_agg_lean_g4(const LaunchCfg&, const SopProgram&, SopProgram*, GroupRec*, uint32_t*, int, ScanStatus*, int*);
hipError_t launch_scan_agg_lean_spec(const LaunchCfg&, const SopProgram&, SopProgram*, int, GroupRec*, uint32_t*, int, ScanStatus*, int*,
                                     bool*, const char**, bool*, uint32_t*);

// wide-load variant: the shape-specialised kernel when S has one of its shapes (lean_spec_kernel.h;
// kernels_lean_spec.hip), else the generic one (lean_kernel.h; kernels_lean_g{1,4}.hip).  BHIP_LEAN_GENERIC=1: always generic.
hipError_t launch_scan_agg_lean(const LaunchCfg& cfg, const SopProgram& S, SopProgram* dprog, int gmax, GroupRec* partials,
                                uint32_t* partial_ng, int max_grid, ScanStatus* status, int* grid_out, const char** variant,
                                bool* fixed_keys, uint32_t* step_alias) {
    static const bool generic_only = env_flag("BHIP_LEAN_GENERIC");
    const char* name = "lean_generic";
    bool fixed = false;
    uint32_t alias = 0;
    if (!variant) variant = &name;
    if (!fixed_keys) fixed_keys = &fixed;
    if (!step_alias) step_alias = &alias;
    *fixed_keys = false;
    if (!generic_only) {
        bool ran = false;
        const hipError_t e = launch_scan_agg_lean_spec(cfg, S, dprog, gmax, partials, partial_ng, max_grid, status, grid_out, &ran, variant, fixed_keys, step_alias);
        if (ran || e != hipSuccess) return e;
    }
    *variant = "lean_generic";
    *step_alias = 0;
    for (int s = 0; s < S.n_steps; ++s) *step_alias |= (uint32_t)s << (4 * s);
    switch (gmax) {
        case 1: return launch_scan_agg_lean_g1(cfg, S, dprog, partials, partial_ng, max_grid, status, grid_out);
        case 4: return launch_scan_agg_lean_g4(cfg, S, dprog, partials, partial_ng, max_grid, status, grid_out);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace bhip
