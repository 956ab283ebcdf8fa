// nljoin_kernels.h — launchers of kernels_nljoin.hip: what NestedLoopJoinExec (host/ops_join.cpp, "nested loop join") runs when a join
// has no equality key.
//
//   nlj_cross_pairs      the pairs p = ri * n_build + li of a range [p0, p1) as two index vectors (the cross product, and the
//                        candidates of the general route, a chunk at a time)
//   nlj_compare_count    the fused route, pass 1: partners per probe row, the build rows' `matched` bits, the probe rows' `hit` words
//   nlj_compare_emit     the fused route, pass 2: the partner pairs at each probe row's offset, build rows ascending
//
// The fused route evaluates an AND of 1 .. NLJ_MAX_TERMS terms `build column OP probe column` per pair in registers: probe rows on
// lanes, build rows staged in LDS NLJ_BUILD_TILE at a time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "vm_isa.h"

namespace bhip {

constexpr int NLJ_BLOCK = 256;                 // threads of a workgroup = probe rows of a workgroup: four waves of 64
constexpr int NLJ_MAX_TERMS = 4;               // terms of a fused predicate
// build rows staged per tile: NLJ_MAX_TERMS x 8 B values + a 4 B mask word a row = 36 KiB at four terms, so four workgroups fit the
// 160 KiB of a CU whatever the term count; fewer terms stage (and allocate) less.  Unmeasured: no other tile size has been tried.
constexpr int NLJ_BUILD_TILE = 1024;
static_assert(NLJ_BUILD_TILE % 64 == 0 && NLJ_BUILD_TILE % NLJ_BLOCK == 0, "a tile is whole `matched` words and whole staging rounds");
// pairs per chunk of the cross and general routes (host: BHIP_NLJ_CHUNK_PAIRS overrides it).  Unmeasured.
constexpr uint64_t NLJ_CHUNK_PAIRS = 1ull << 24;

// how a term's two 64-bit images compare (the VM's OP_CMP_I64 / OP_CMP_U64 / OP_CMP_F64)
enum NljClass : int32_t { NLJ_I64 = 0, NLJ_U64 = 1, NLJ_F64 = 2 };
struct NljTerm {
    ColumnRef build, probe;    // the same fixed-width type of at most 8 bytes on both sides
    int32_t cmp;               // CmpKind of `build OP probe`
    int32_t vclass;            // NljClass
};
struct NljTerms {
    int32_t n;
    NljTerm t[NLJ_MAX_TERMS];
};

// lidx[p - p0] = p % n_build, ridx[p - p0] = p / n_build for p in [p0, p1); n_build >= 1
hipError_t launch_nlj_cross_pairs(const LaunchCfg& cfg, uint32_t n_build, uint64_t p0, uint64_t p1, uint32_t* lidx, uint32_t* ridx);
// counts[r] = build rows l with every term TRUE for (l, r); a NULL on either side of a term makes no partner.
// matched (may be null): bit l of 32-bit words, OR-ed in, for every build row with a partner in this batch.
// hit (may be null): (n_probe + 63) / 64 64-bit words, every one of them written; bit r = probe row r has a partner, bits past n_probe 0.
hipError_t launch_nlj_compare_count(const LaunchCfg& cfg, const NljTerms& T, uint32_t n_build, uint32_t n_probe, uint32_t* counts, uint32_t* matched,
                                    uint64_t* hit);
// the pairs themselves: probe row r's at lidx / ridx [offsets[r] ..), build rows ascending (offsets: the exclusive scan of counts)
hipError_t launch_nlj_compare_emit(const LaunchCfg& cfg, const NljTerms& T, uint32_t n_build, uint32_t n_probe, const uint64_t* offsets, uint32_t* lidx,
                                   uint32_t* ridx);

}  // namespace bhip
