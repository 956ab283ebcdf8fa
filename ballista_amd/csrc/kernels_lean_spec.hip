// kernels_lean_spec.hip — shape-specialised instantiations of the wide-load scan + aggregate kernel
// (lean_spec_kernel.h) for the hot plans; every other plan the host sends to the lean path runs on lean_kernel.h.
#include <stdlib.h>
#include "lean_spec_kernel.h"

namespace bhip {

// *ran = false (and nothing launched) when S has none of the specialised shapes; *variant names the one that ran, *fixed
// says whether it read its Utf8 keys in the fixed-width form.  BHIP_NO_FIXED_UTF8=1: never (the widths are ignored).
hipError_t launch_scan_agg_lean_spec(const LaunchCfg& cfg, const SopProgram& S, SopProgram* dprog, int gmax, GroupRec* partials,
                                     uint32_t* partial_ng, int max_grid, ScanStatus* status, int* grid_out, bool* ran,
                                     const char** variant, bool* fixed) {
    static const bool no_fixed = env_flag("BHIP_NO_FIXED_UTF8");
#define BHIP_LEAN_SPEC(NAME_, GMAX_, NR_, R32_, K0_, K1_, NS_)                                                            \
    if (gmax == GMAX_ && !(no_fixed && (K0_ == LK_UTF8_FIXED || K1_ == LK_UTF8_FIXED)) &&                                 \
        lean_shape_matches<NR_, R32_, K0_, K1_, NS_>(S)) {                                                                \
        *ran = true;                                                                                                      \
        *variant = NAME_;                                                                                                 \
        *fixed = K0_ == LK_UTF8_FIXED || K1_ == LK_UTF8_FIXED;                                                            \
        return launch_sop_program(scan_agg_lean_spec_kernel<GMAX_, NR_, R32_, K0_, K1_, NS_>, LEAN_TILE, cfg, S, dprog,   \
                                  partials, partial_ng, max_grid, status, grid_out);                                      \
    }
    // TPC-H Q1: l_shipdate range, GROUP BY two 1-byte strings, 5 chain steps.  First the form for key columns whose values
    // all have one known width (every Utf8 key part of the plan: no mixed forms), then the one that reads the offsets.
    BHIP_LEAN_SPEC("lean_spec_q1", 4, 1, 0b1, LK_UTF8_FIXED, LK_UTF8_FIXED, 5)
    BHIP_LEAN_SPEC("lean_spec_q1", 4, 1, 0b1, LK_UTF8, LK_UTF8, 5)
    // the same with one string key part
    BHIP_LEAN_SPEC("lean_spec_key1", 4, 1, 0b1, LK_UTF8_FIXED, LK_NONE, 5)
    BHIP_LEAN_SPEC("lean_spec_key1", 4, 1, 0b1, LK_UTF8, LK_NONE, 5)
    // Not instantiated, measured slower than the generic kernel: TPC-H Q6 (<1, 3, 0b001, none, none, 2>,
    // -4 %: its generic loop already keeps its loads in flight) and Q1's sums without GROUP BY (<1, 1, 1, none, none, 5>:
    // spills to scratch under the 128-VGPR bound of 4 blocks per CU).
#undef BHIP_LEAN_SPEC
    *ran = false;
    return hipSuccess;
}

}  // namespace bhip
