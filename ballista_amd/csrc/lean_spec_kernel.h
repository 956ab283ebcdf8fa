// lean_spec_kernel.h — lean_kernel.h with the plan SHAPE fixed at compile time, for the hot plans
// (instantiated in kernels_lean_spec.hip; picked by launch_scan_agg_lean_spec, else the generic kernel runs).
//
// Same rows per thread, same per-row arithmetic, same per-thread summation order per accumulator, the same grid and the
// same fixed-order workgroup reduction as scan_agg_lean_kernel.  What differs is the main loop.
// The shape facts that decide WHICH loads exist are template parameters — the number of ranges and the width of each
// (NULL-free range columns only), the kind of each key part, the exact number of chain steps — so the loop body is
// straight-line code with no branch around a load.  The generic kernel's loop drains the memory queue at every turn:
// its loads sit behind runtime `if`s, so the values that cross the back edge are phis of "loaded" and "kept", which the
// compiler resolves with register copies, and a copy of a register still being loaded waits for it (s_waitcnt vmcnt(0)).
// Here:
//   * the tile loop is unrolled by two with explicit even / odd register sets for the Float64 step values and the Utf8
//     offsets, so no register that is still being loaded is copied across the back edge;
//   * loads are issued unconditionally; the offsets prefetch two tiles ahead is re-pointed at the workgroup's last own
//     tile instead of running past the end (no extra HBM bytes: that tile was just read);
//   * per tile t: once the ranges and key bytes of t are consumed, ranges(t+1), Int32 keys(t+1), key bytes(t+1) from
//     offsets(t+1) and offsets(t+2); then, step column by step column, the sums of t and the loads of steps(t+1);
//   * the ragged tail and the key-append path of the lookup stay out of the fast path, as in the generic kernel.
//
// Step aliases (ALIAS): where two steps of the plan read one column (Q1: 1 - l_discount inside the products, l_discount
// for its average), only the earlier one has registers and a load.  When it is summed it also forms the later step's
// factor f = sgn*x + add from the same registers, before they are reloaded; the later step takes that f, multiplies it
// into its own chain (or starts one) and adds it to its own accumulator when its turn comes.  Step order, and with it the
// order in which every accumulator receives a thread's rows, is unchanged, so every per-thread partial sum is too.
// launch_scan_agg_lean_spec computes the pattern of a plan (lean_step_alias) and takes an aliased instantiation only
// for exactly its pattern; the identity pattern serves every plan, with one load per step (profiles/isa_lean_alias.txt).
//
// The fixed-width key form (LK_UTF8_FIXED): every value of the key column is w bytes long (SopColumn::width, 1..3), so
// offsets[i] = offsets[0] + i*w and the lengths are the constant w.  The kernel then reads offsets[0] once and no other
// offset: there is no load_offsets, no `ko` register set and no re-pointed prefetch, and the key bytes of tile t+1 are
// loaded straight from data + offsets[0] + row*w where the offsets form issues its (dependent) key-byte load.  Key words
// are still lean_str_word(raw, w), so keys, sums and their order are what the offsets form gives.  Nothing can be too
// long and nothing is learnt about lengths in this form; the ragged tail still goes through the offsets (lean_tail).
#pragma once
#include "lean_kernel.h"

namespace bhip {

enum LeanKeyKind : int { LK_NONE = 0, LK_I32 = 1, LK_UTF8 = 2, LK_UTF8_FIXED = 3 };

// Step aliases, 4 bits per step: a(s) = the earliest step <= s that reads the same column as step s.  a(s) == s: the step
// owns its load.  TPC-H Q1 sums x*(1 - disc) and averages disc: {0, 1, 2, 3, 2}.
constexpr uint32_t lean_alias_of(uint32_t alias, int s) { return (alias >> (4 * s)) & 15u; }
constexpr uint32_t lean_alias_identity(int ns) {
    uint32_t a = 0;
    for (int s = 0; s < ns; ++s) a |= (uint32_t)s << (4 * s);
    return a;
}
constexpr bool lean_alias_valid(uint32_t alias, int ns) {
    for (int s = 0; s < ns; ++s) {
        const uint32_t a = lean_alias_of(alias, s);
        if (a > (uint32_t)s || lean_alias_of(alias, (int)a) != a) return false;
    }
    return true;
}

// The 8- and 16-byte loads of the streamed columns (range, step and Int32 key columns): non-temporal, one instruction each.
// Every byte of those columns is read once per launch, so nothing is lost by passing the L1 by.  The key bytes (whose
// lines neighbouring waves share) and the offsets (prefetched two tiles ahead and read again) keep the default policy.
typedef uint32_t LeanV2 __attribute__((ext_vector_type(2)));
typedef uint32_t LeanV4 __attribute__((ext_vector_type(4)));
__device__ inline LeanU2 lean_stream_ld2(const BHIP_GLOBAL char* p) {
    const LeanV2 v = __builtin_nontemporal_load((const BHIP_GLOBAL LeanV2*)p);
    return LeanU2{v.x, v.y};
}
__device__ inline LeanU4 lean_stream_ld4(const BHIP_GLOBAL char* p) {
    const LeanV4 v = __builtin_nontemporal_load((const BHIP_GLOBAL LeanV4*)p);
    return LeanU4{v.x, v.y, v.z, v.w};
}

// NR ranges (bit p of R32: range p reads a 32-bit integer column, else Float64), key parts K0 / K1, exactly NS steps with
// the alias pattern ALIAS (the plan's own, or the identity: then a repeated column is simply loaded again)
template <int GMAX, int NR, int R32, int K0, int K1, int NS, uint32_t ALIAS = lean_alias_identity(NS)>
__global__ void __launch_bounds__(BLOCK, (GMAX == 1 && NS <= 5) ? 4 : 3)
scan_agg_lean_spec_kernel(const SopProgram* __restrict__ Sp, GroupRec* partials, uint32_t* partial_ng, ScanStatus* status) {
    static_assert(NR >= 1 && NR <= SOP_NRANGE && NS >= 1 && NS <= SOP_NSTEP && (K0 != LK_NONE || K1 == LK_NONE), "lean shape");
    static_assert(lean_alias_valid(ALIAS, NS), "a(s) <= s and a(a(s)) == a(s)");
    const SopProgram& S = *Sp;
    constexpr int U = LEAN_U;
    constexpr int NKEY = 2;
    constexpr int KK[NKEY] = {K0, K1};
    constexpr bool HAS_OFFSETS = K0 == LK_UTF8 || K1 == LK_UTF8;
    constexpr bool HAS_FIXED = K0 == LK_UTF8_FIXED || K1 == LK_UTF8_FIXED;
    static_assert(!(HAS_OFFSETS && HAS_FIXED), "no mixed key forms: one unknown width sends the plan to the offsets form");
    __shared__ LeanLds<GMAX, NS> lds;
    const int tid = threadIdx.x, lane = tid & 63;

    // ---- plan: wave-uniform bases and constants (addresses are rebuilt per tile from the tile index)
    const int64_t n_rows = S.n_rows;
    const int64_t n_tiles = n_rows / LEAN_TILE;
    const int64_t grid = gridDim.x;
    const int64_t my_tiles = (int64_t)blockIdx.x < n_tiles ? (n_tiles - 1 - (int64_t)blockIdx.x) / grid + 1 : 0;

    const BHIP_GLOBAL char* rbase[NR];
    double rlo[NR], rhi[NR];
#pragma unroll
    for (int p = 0; p < NR; ++p) {
        rbase[p] = (const BHIP_GLOBAL char*)S.cols[S.ranges[p].col].data;
        rlo[p] = S.ranges[p].lo; rhi[p] = S.ranges[p].hi;
    }
    const BHIP_GLOBAL char* kbase[NKEY];       // Int32 key: values.  Utf8 key: the offsets
    const BHIP_GLOBAL char* kdat[NKEY];        // Utf8 key: bytes (absolute offsets).  Fixed width: the bytes of row 0
    uint32_t kw[NKEY];                         // fixed-width Utf8 key: the width, 1..3
#pragma unroll
    for (int q = 0; q < NKEY; ++q) {
        kbase[q] = nullptr; kdat[q] = nullptr; kw[q] = 0;
        if (KK[q] != LK_NONE) {
            const SopColumn c = S.cols[S.keys[q].col];
            kbase[q] = KK[q] == LK_UTF8 ? (const BHIP_GLOBAL char*)c.offsets : (const BHIP_GLOBAL char*)c.data;
            kdat[q] = (const BHIP_GLOBAL char*)c.data;
            if (KK[q] == LK_UTF8_FIXED) {
                kdat[q] += (uint32_t)c.offsets[0];            // wave-uniform, read once; not assumed to be 0
                kw[q] = (uint32_t)c.width;
            }
        }
    }
    const BHIP_GLOBAL char* xbase[NS];
    bool xstart[NS], xplain[NS];
    uint32_t xflip[NS];
    double xadd[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const SopStep st = S.steps[s];
        xstart[s] = st.start != 0;
        xplain[s] = st.sgn == 1.0 && st.add == 0.0 && __builtin_signbit(st.add);
        xflip[s] = st.sgn < 0.0 ? 0x80000000u : 0u;
        xadd[s] = st.add;
        xbase[s] = (const BHIP_GLOBAL char*)S.cols[st.col].data;
    }
    const int64_t tile_of0 = blockIdx.x;
    auto tile_row = [&](int64_t k) -> int64_t {   // first row of the workgroup's k-th tile, clamped to its last one
        const int64_t kk = k < my_tiles ? k : my_tiles - 1;
        return (tile_of0 + kk * grid) * LEAN_TILE;
    };

    // ---- accumulators
    double acc[NS];                            // GMAX == 1 only
    uint32_t rows1 = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    if constexpr (GMAX > 1) {
#pragma unroll
        for (int j = 0; j < GMAX * NS; ++j) lds.acc[j * BLOCK + tid] = 0.0;
#pragma unroll
        for (int j = 0; j < GMAX; ++j) lds.cnt[j * BLOCK + tid] = 0;
    }
    if (tid == 0) { lds.ng = 0; lds.overflow = 0; lds.lock = 0; lds.pad = 0; }
    if (tid < AGG_GMAX) lds.keys[tid] = 0;
    __syncthreads();
    LeanLens<(GMAX > 1)> lens;
    LeanKeyTable<GMAX, NS> table;
    auto lookup = [&](const uint64_t (&key)[LEAN_ROWS], const bool (&live)[LEAN_ROWS], int (&lg)[LEAN_ROWS]) -> bool {
        return table.lookup(lds, lane, key, live, lg);
    };
    // one row's value of step s / the row itself into its group's accumulators, without a branch: a filtered-out row
    // adds +0.0 (and a count of 0) to group 0's slot, which leaves it bit-for-bit as it was (the slots start at +0.0,
    // and x + (+0.0) == x for every x other than -0.0, which a sum that starts at +0.0 never holds)
    auto add_step = [&](int lgr, int s, double v) {
        const double a = lgr >= 0 ? v : 0.0;
        if constexpr (GMAX == 1) {
            acc[s] += a;
        } else {
            const int g = lgr >= 0 ? lgr : 0;
            __hip_atomic_fetch_add(&lds.acc[(g * NS + s) * BLOCK + tid], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    auto add_row = [&](int lgr) {
        if constexpr (GMAX == 1) {
            rows1 += lgr >= 0 ? 1u : 0u;
        } else {
            const int g = lgr >= 0 ? lgr : 0;
            __hip_atomic_fetch_add(&lds.cnt[g * BLOCK + tid], lgr >= 0 ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };

    // ---- registers.  Row j of sub-tile u: tile row u*512 + 2*tid + j.
    LeanU4 rv[NR][U];            // 32-bit column: .x .y = rows 0 1; Float64: (.x .y) (.z .w)
    uint32_t kv[NKEY][U][2];     // Int32 key: the two values.  Utf8 key: lengths of the two strings (fixed width: unused)
    uint64_t kb[NKEY][U];        // Utf8 key: 8 bytes at the first string's offset
    LeanU3 ko[2][NKEY][U];       // Utf8 key offsets, by parity of the tile they belong to (fixed width: unused)
    LeanU4 xv[NS][U];            // Float64 step values
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int p = 0; p < NR; ++p) rv[p][u] = LeanU4{0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < NKEY; ++q) {
            kv[q][u][0] = kv[q][u][1] = 0; kb[q][u] = 0;
            ko[0][q][u] = ko[1][q][u] = LeanU3{0, 0, 0};
        }
    }
    const uint32_t t8 = (uint32_t)tid * 8u, t16 = (uint32_t)tid * 16u;
    uint32_t t2w[NKEY];          // fixed-width Utf8 key: byte offset of this thread's row pair within a sub-tile
#pragma unroll
    for (int q = 0; q < NKEY; ++q) t2w[q] = (uint32_t)tid * 2u * kw[q];

    auto load_step = [&](int s, int64_t row) {
#pragma unroll
        for (int u = 0; u < U; ++u) xv[s][u] = lean_stream_ld4(xbase[s] + (row + u * LEAN_SUB) * 8 + t16);
    };
    auto load_ranges = [&](int64_t row) {
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            if ((R32 >> p) & 1) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const LeanU2 v = lean_stream_ld2(rbase[p] + (row + u * LEAN_SUB) * 4 + t8);
                    rv[p][u].x = v.x; rv[p][u].y = v.y;
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) rv[p][u] = lean_stream_ld4(rbase[p] + (row + u * LEAN_SUB) * 8 + t16);
            }
        }
    };
    auto load_int_keys = [&](int64_t row) {
#pragma unroll
        for (int q = 0; q < NKEY; ++q)
            if (KK[q] == LK_I32) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const LeanU2 v = lean_stream_ld2(kbase[q] + (row + u * LEAN_SUB) * 4 + t8);
                    kv[q][u][0] = v.x; kv[q][u][1] = v.y;
                }
            }
    };
    auto load_offsets = [&](LeanU3 (&o)[NKEY][U], int64_t row) {
#pragma unroll
        for (int q = 0; q < NKEY; ++q)
            if (KK[q] == LK_UTF8) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const BHIP_GLOBAL char* a = kbase[q] + (row + u * LEAN_SUB) * 4 + t8;
                    const LeanU2 v = lean_ld2(a);
                    o[q][u].a = v.x; o[q][u].b = v.y;
                    o[q][u].c = *(const BHIP_GLOBAL uint32_t*)(a + 8);
                }
            }
    };
    // Utf8 key: lengths from the offsets + the bytes at the first string
    auto load_key_bytes = [&](const LeanU3 (&o)[NKEY][U]) {
#pragma unroll
        for (int q = 0; q < NKEY; ++q)
            if (KK[q] == LK_UTF8) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t l0 = o[q][u].b - o[q][u].a, l1 = o[q][u].c - o[q][u].b;
                    lens.see(q, l0); lens.see(q, l1);
                    kv[q][u][0] = l0; kv[q][u][1] = l1;
                    kb[q][u] = ((const BHIP_GLOBAL PackedU64*)(kdat[q] + o[q][u].a))->v;   // buffers carry 16 B of slack
                }
            }
    };

    // fixed-width Utf8 key: the bytes of both strings, straight from the row number (64-bit: rows go to 2^32 - 16; a
    // sub-tile's rows * w < 2^31 since Arrow offsets are Int32).  The same 8-byte load as the offsets form issues.
    auto load_key_bytes_fixed = [&](int64_t row) {
#pragma unroll
        for (int q = 0; q < NKEY; ++q)
            if (KK[q] == LK_UTF8_FIXED) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    kb[q][u] = ((const BHIP_GLOBAL PackedU64*)(kdat[q] + (row + u * LEAN_SUB) * (int64_t)kw[q] + t2w[q]))->v;
            }
    };

    auto eval_live = [&](bool (&live)[LEAN_ROWS]) {
#pragma unroll
        for (int r = 0; r < LEAN_ROWS; ++r) live[r] = true;
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            if ((R32 >> p) & 1) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double a = (double)(int32_t)rv[p][u].x, b = (double)(int32_t)rv[p][u].y;
                    live[2 * u] = live[2 * u] && a >= rlo[p] && a <= rhi[p];
                    live[2 * u + 1] = live[2 * u + 1] && b >= rlo[p] && b <= rhi[p];
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double a = u2d(((uint64_t)rv[p][u].y << 32) | rv[p][u].x), b = u2d(((uint64_t)rv[p][u].w << 32) | rv[p][u].z);
                    live[2 * u] = live[2 * u] && a >= rlo[p] && a <= rhi[p];
                    live[2 * u + 1] = live[2 * u + 1] && b >= rlo[p] && b <= rhi[p];
                }
            }
        }
    };
    auto eval_keys = [&](uint64_t (&key)[LEAN_ROWS]) {
        uint32_t w[NKEY][LEAN_ROWS];
#pragma unroll
        for (int q = 0; q < NKEY; ++q) {
#pragma unroll
            for (int r = 0; r < LEAN_ROWS; ++r) w[q][r] = 0;
            if (KK[q] == LK_UTF8) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t l0 = kv[q][u][0] > LEAN_MAX_STR ? LEAN_MAX_STR : kv[q][u][0];
                    const uint32_t l1 = kv[q][u][1] > LEAN_MAX_STR ? LEAN_MAX_STR : kv[q][u][1];
                    w[q][2 * u] = lean_str_word((uint32_t)kb[q][u], l0);
                    w[q][2 * u + 1] = lean_str_word((uint32_t)(kb[q][u] >> (l0 << 3)), l1);
                }
            } else if (KK[q] == LK_UTF8_FIXED) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    w[q][2 * u] = lean_str_word((uint32_t)kb[q][u], kw[q]);
                    w[q][2 * u + 1] = lean_str_word((uint32_t)(kb[q][u] >> (kw[q] << 3)), kw[q]);
                }
            } else if (KK[q] == LK_I32) {
#pragma unroll
                for (int u = 0; u < U; ++u) { w[q][2 * u] = kv[q][u][0]; w[q][2 * u + 1] = kv[q][u][1]; }
            }
        }
#pragma unroll
        for (int r = 0; r < LEAN_ROWS; ++r) key[r] = ((uint64_t)w[1][r] << 32) | w[0][r];
    };
    // ---- one tile: k-th of the workgroup, parity P of its offsets set.  NEXT: issue the loads of tile k+1 (and the
    // offsets of k+2) — ranges and keys once this tile's are consumed, each step column once this tile's is summed
    auto tile = [&](auto P_, auto NEXT_, int64_t k) -> bool {
        constexpr int P = decltype(P_)::value;
        constexpr bool NEXT = decltype(NEXT_)::value;
        const int64_t row1 = tile_row(k + 1);
        bool live[LEAN_ROWS];
        uint64_t key[LEAN_ROWS];
        eval_live(live);
        eval_keys(key);
        if constexpr (NEXT) {
            load_ranges(row1);
            load_int_keys(row1);
            load_key_bytes(ko[P ^ 1]);                                   // offsets(k+1) -> lengths + bytes(k+1)
            load_key_bytes_fixed(row1);                                  // ... or bytes(k+1) from the row number
            if constexpr (HAS_OFFSETS) load_offsets(ko[P], tile_row(k + 2));   // clamped to the last own tile
        }
        int lg[LEAN_ROWS];
        if (!lookup(key, live, lg)) return false;
        // chain values f = sgn*x + add ; t = (start ? 1 : t_prev) * f, summed step by step: each accumulator still
        // receives this thread's rows in row order.  A step that owns its column also forms f (with their sgn / add) for
        // the later steps aliased to it, before its registers are reloaded; an aliased step has no registers and no load.
        double tp[LEAN_ROWS];
        double fa[NS][LEAN_ROWS];                   // f of the aliased steps
        auto factor = [&](int s, const LeanU4 x, double& a, double& b) {
            a = u2d(((uint64_t)x.y << 32) | x.x); b = u2d(((uint64_t)x.w << 32) | x.z);
            if (!xplain[s]) {
                a = u2d(((uint64_t)(x.y ^ xflip[s]) << 32) | x.x) + xadd[s];
                b = u2d(((uint64_t)(x.w ^ xflip[s]) << 32) | x.z) + xadd[s];
            }
        };
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool own = lean_alias_of(ALIAS, s) == (uint32_t)s;
            double tv[LEAN_ROWS];
            if (own) {
#pragma unroll
                for (int u = 0; u < U; ++u) factor(s, xv[s][u], tv[2 * u], tv[2 * u + 1]);
#pragma unroll
                for (int a = s + 1; a < NS; ++a)
                    if (lean_alias_of(ALIAS, a) == (uint32_t)s) {
#pragma unroll
                        for (int u = 0; u < U; ++u) factor(a, xv[s][u], fa[a][2 * u], fa[a][2 * u + 1]);
                    }
            } else {
#pragma unroll
                for (int r = 0; r < LEAN_ROWS; ++r) tv[r] = fa[s][r];
            }
            if (s > 0 && !xstart[s]) {
#pragma unroll
                for (int r = 0; r < LEAN_ROWS; ++r) tv[r] = tp[r] * tv[r];
            }
#pragma unroll
            for (int r = 0; r < LEAN_ROWS; ++r) { add_step(lg[r], s, tv[r]); tp[r] = tv[r]; }
            if constexpr (NEXT) { if (own) load_step(s, row1); }
        }
#pragma unroll
        for (int r = 0; r < LEAN_ROWS; ++r) add_row(lg[r]);
        return true;
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using BT = std::integral_constant<bool, true>;
    using BF = std::integral_constant<bool, false>;

    bool over = false;
    if (my_tiles > 0) {
        const int64_t row0 = tile_row(0);
        if constexpr (HAS_OFFSETS) load_offsets(ko[0], row0);
        load_key_bytes(ko[0]);                                           // the one exposed dependent load
        load_key_bytes_fixed(row0);
        load_ranges(row0);
        load_int_keys(row0);
        if constexpr (HAS_OFFSETS) load_offsets(ko[1], tile_row(1));
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (lean_alias_of(ALIAS, s) == (uint32_t)s) load_step(s, row0);
        // Drain the prologue once.  The loop head is entered from here and from its back edge, and the compiler's wait at
        // a join assumes the worse of the two; with nothing in flight here the prologue's load order (key bytes behind the
        // step loads) cannot lower the head's counts.  (The even tile's head still waits vmcnt(10..8): DESIGN.md §3.1.)
        __builtin_amdgcn_s_waitcnt(0x0F70);                              // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
        int64_t k = 0;
        for (; k + 2 < my_tiles; k += 2) {
            if (!tile(I0{}, BT{}, k) || !tile(I1{}, BT{}, k + 1)) { over = true; break; }
        }
        if (!over) {
            if (my_tiles - k == 2) over = !tile(I0{}, BT{}, k) || !tile(I1{}, BF{}, k + 1);
            else over = !tile(I0{}, BF{}, k);
        }
    }

    // ---- ragged tail (< 1024 rows): the workgroup next in line takes it
    if (!over && (int64_t)blockIdx.x == n_tiles % grid && n_tiles * LEAN_TILE < n_rows) {
        auto accumulate = [&](int lgr, const double (&tv)[NS]) {
#pragma unroll
            for (int s = 0; s < NS; ++s) add_step(lgr, s, tv[s]);
            add_row(lgr);
        };
        // (fixed-width keys: what the tail sees of the lengths is dropped, it is not the whole column)
        LeanLens<(GMAX > 1)> tail_lens;
        over = !lean_tail<GMAX, NS, NR>(S, n_tiles * LEAN_TILE, n_rows, HAS_FIXED ? tail_lens : lens, lookup, accumulate);
    }
    lean_finish<GMAX, NS>(lds, S, acc, rows1, lens, partials, partial_ng, status);
}

// the alias pattern of plan S: for each step the earliest step that reads the same column at the same width
static uint32_t lean_step_alias(const SopProgram& S) {
    uint32_t alias = 0;
    for (int s = 0; s < S.n_steps && s < SOP_NSTEP; ++s) {
        int a = s;
        for (int e = s - 1; e >= 0; --e)
            if (S.steps[e].col == S.steps[s].col && S.steps[e].is32 == S.steps[s].is32) a = e;
        alias |= (uint32_t)a << (4 * s);
    }
    return alias;
}

// does plan S have exactly this shape (range widths, no NULLs in a range column, key kinds, step count)?
template <int NR, int R32, int K0, int K1, int NS>
static bool lean_shape_matches(const SopProgram& S) {
    if (S.n_ranges != NR || S.n_steps != NS) return false;
    for (int p = 0; p < NR; ++p) {
        if ((S.ranges[p].is32 != 0) != (((R32 >> p) & 1) != 0)) return false;
        if (S.cols[S.ranges[p].col].validity) return false;
    }
    const int kk[2] = {K0, K1};
    int n_keys = 0;
    for (int q = 0; q < 2; ++q) {
        if (kk[q] == LK_NONE) continue;
        ++n_keys;
        if (S.n_keys <= q) return false;
        if (S.keys[q].kind != (kk[q] == LK_I32 ? SOP_KEY_I32 : SOP_KEY_UTF8)) return false;
        const int32_t w = S.cols[S.keys[q].col].width;
        if (kk[q] == LK_UTF8_FIXED && (w < 1 || w > (int32_t)LEAN_MAX_STR)) return false;
    }
    return S.n_keys == n_keys;
}

}  // namespace bhip
