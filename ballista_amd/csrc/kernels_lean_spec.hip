// kernels_lean_spec.hip — shape-specialised instantiations of the wide-load scan + aggregate kernel
// (lean_spec_kernel.h) for the hot plans; every other plan the host sends to the lean path runs on lean_kernel.h.
#include <stdlib.h>
#include "lean_spec_kernel.h"

namespace bhip {

// *ran = false (and nothing launched) when S has none of the specialised shapes; *variant names the one that ran, *fixed
// says whether it read its Utf8 keys in the fixed-width form, *step_alias is the alias pattern it was compiled for (the
// identity: every step loads its own column).  BHIP_NO_FIXED_UTF8=1: never the fixed form (the widths are ignored).
// BHIP_LEAN_NO_ALIAS=1: never an aliased instantiation.
hipError_t launch_scan_agg_lean_spec(const LaunchCfg& cfg, const SopProgram& S, SopProgram* dprog, int gmax, GroupRec* partials,
                                     uint32_t* partial_ng, int max_grid, ScanStatus* status, int* grid_out, bool* ran,
                                     const char** variant, bool* fixed, uint32_t* step_alias) {
    static const bool no_fixed = env_flag("BHIP_NO_FIXED_UTF8");
    static const bool no_alias = env_flag("BHIP_LEAN_NO_ALIAS");
    const uint32_t alias = lean_step_alias(S);
    // an aliased instantiation serves exactly the plans with its pattern; the identity serves every pattern
#define BHIP_LEAN_SPEC_A(NAME_, GMAX_, NR_, R32_, K0_, K1_, NS_, ALIAS_)                                                  \
    if (gmax == GMAX_ && !(no_fixed && (K0_ == LK_UTF8_FIXED || K1_ == LK_UTF8_FIXED)) &&                                 \
        (ALIAS_ == lean_alias_identity(NS_) || (!no_alias && alias == ALIAS_)) &&                                         \
        lean_shape_matches<NR_, R32_, K0_, K1_, NS_>(S)) {                                                                \
        *ran = true;                                                                                                      \
        *variant = NAME_;                                                                                                 \
        *fixed = K0_ == LK_UTF8_FIXED || K1_ == LK_UTF8_FIXED;                                                            \
        *step_alias = ALIAS_;                                                                                             \
        return launch_sop_program(scan_agg_lean_spec_kernel<GMAX_, NR_, R32_, K0_, K1_, NS_, ALIAS_>, LEAN_TILE, cfg, S,  \
                                  dprog, partials, partial_ng, max_grid, status, grid_out);                               \
    }
    // each shape with Q1's pattern (step 4, avg(disc), reads the column of step 2, 1 - disc), then un-aliased
#define BHIP_LEAN_SPEC(NAME_, GMAX_, NR_, R32_, K0_, K1_, NS_)                                                            \
    BHIP_LEAN_SPEC_A(NAME_, GMAX_, NR_, R32_, K0_, K1_, NS_, 0x23210u)                                                    \
    BHIP_LEAN_SPEC_A(NAME_, GMAX_, NR_, R32_, K0_, K1_, NS_, lean_alias_identity(NS_))
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
#undef BHIP_LEAN_SPEC_A
    *ran = false;
    return hipSuccess;
}

}  // namespace bhip
