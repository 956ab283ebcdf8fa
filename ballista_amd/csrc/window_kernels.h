// window_kernels.h — launchers of kernels_window.hip: what WindowAggExec (host/ops_window.cpp) runs over its SORTED input.
//
// Every window function here is a scan or a gather over 4-byte and 8-byte streams:
//   boundary flags  ->  partition / peer bounds (scans of the flags)  ->  rank or index vectors (elementwise)
//                   ->  segmented inclusive scan of an argument       ->  finish (read the running state at the frame's last row)
// and, for a sliding ROWS frame, the frame's rows (lo, hi)  ->  a gather, a finish over (lo, hi), or window_slide: the aggregate of a
// bounded neighbourhood of each row straight from the argument.
// The scans are the multi-launch form: per-tile summaries, ONE workgroup's scan of the summaries, then the apply pass.  No
// workgroup ever waits for another one.  A tile is WINDOW_TILE_ROWS rows whatever the device and the grid, so the order of every
// floating-point addition is a function of the row positions alone: two runs over the same input give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace bhip {

constexpr int WINDOW_BLOCK = 256;                                  // threads of a workgroup: four waves of 64
constexpr int WINDOW_ROUNDS = 4;                                   // a tile is scanned in rounds of WINDOW_BLOCK consecutive rows
constexpr int WINDOW_TILE_ROWS = 1024;                             // rows per tile summary (mirrored as ballista_amd.plan.WINDOW_TILE_ROWS)
static_assert(WINDOW_TILE_ROWS == WINDOW_BLOCK * WINDOW_ROUNDS, "a tile is WINDOW_ROUNDS rounds of one row per thread");
constexpr int WINDOW_SUMMARY_STEP = 256;                           // tile summaries the second level scans per step (one per thread)
constexpr int WINDOW_MAX_KEYS = 8;                                 // partition keys, and order keys, of one specification
constexpr uint32_t WINDOW_NULL_INDEX = 0xFFFFFFFFu;                // the NULL row of the outer-join gather (take_column_nullable)

// the evaluated key columns of the sorted rows: col[0 .. n_part) partition keys, col[n_part .. n_part + n_order) order keys
struct WindowKeys {
    int32_t n_part, n_order;
    ColumnRef col[2 * WINDOW_MAX_KEYS];
};
// bit i of part_flags: row i starts a partition (a partition key differs from row i - 1's, or i == 0); of peer_flags: row i starts
// a peer group (it starts a partition, or an order key differs).  NULL equals NULL, fixed widths compare by bits, Utf8 by bytes.
// Both bitmaps have (n + 63) / 64 words; the bits past n in the last word are 0.
hipError_t launch_window_flags(const LaunchCfg& cfg, const WindowKeys& K, int64_t n, uint64_t* part_flags, uint64_t* peer_flags);

// bytes of the scratch every scan below needs for its tile summaries
size_t window_scan_temp_bytes(int64_t n);
inline int64_t window_tiles(int64_t n) { return (n + WINDOW_TILE_ROWS - 1) / WINDOW_TILE_ROWS; }

// part_start[i] / peer_start[i]: first row of row i's partition / peer group (inclusive max-scan of flag ? i : 0);
// peers_to[i]: peer groups that start at or before row i (inclusive sum of the peer flags)
hipError_t launch_window_bounds_forward_tiles(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, void* temp);
hipError_t launch_window_bounds_forward_summaries(const LaunchCfg& cfg, int64_t n, void* temp);
hipError_t launch_window_bounds_forward_apply(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, const void* temp,
                                              uint32_t* part_start, uint32_t* peer_start, uint32_t* peers_to);
// part_end[i] / peer_end[i]: last row of row i's partition / peer group (the mirror image: inclusive min-scan from the right)
hipError_t launch_window_bounds_backward_tiles(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, void* temp);
hipError_t launch_window_bounds_backward_summaries(const LaunchCfg& cfg, int64_t n, void* temp);
hipError_t launch_window_bounds_backward_apply(const LaunchCfg& cfg, const uint64_t* part_flags, const uint64_t* peer_flags, int64_t n, const void* temp,
                                               uint32_t* part_end, uint32_t* peer_end);

// ROW_NUMBER / RANK / DENSE_RANK as UInt64
enum WindowRankKind : int32_t { WINDOW_ROW_NUMBER = 0, WINDOW_RANK = 1, WINDOW_DENSE_RANK = 2 };
hipError_t launch_window_rank(const LaunchCfg& cfg, int kind, const uint32_t* part_start, const uint32_t* peer_start, const uint32_t* peers_to,
                              int64_t n, uint64_t* out);
// the row each output row reads, for the outer-join gather: LAG / LEAD by `offset` rows (WINDOW_NULL_INDEX outside the partition),
// the partition's first row, the frame's last row (`frame_end`: part_end, peer_end, or null = the row itself)
enum WindowIndexKind : int32_t { WINDOW_LAG = 0, WINDOW_LEAD = 1, WINDOW_FIRST = 2, WINDOW_LAST = 3 };
hipError_t launch_window_index(const LaunchCfg& cfg, int kind, int64_t offset, const uint32_t* part_start, const uint32_t* part_end,
                               const uint32_t* frame_end, int64_t n, uint32_t* idx);

// segmented inclusive scan of one argument column; the segment heads are the partition flags.  The running state of row i is
// (value, number of non-NULL arguments) over rows part_start[i] .. i; a NULL contributes nothing.  The value is 64 bits wide:
// narrower integers are sign- or zero-extended and Float32 is widened to Float64 on load (exact, and MIN / MAX commute with it).
enum WindowScanOp : int32_t {
    WINDOW_OP_ADD_I64 = 0,      // wrapping 64-bit add (signed and unsigned alike); a null `arg.data`: only the count is kept
    WINDOW_OP_ADD_F64 = 1,      // Float64 add; integer arguments are converted on load (AVG)
    WINDOW_OP_MIN_I64 = 2, WINDOW_OP_MAX_I64 = 3, WINDOW_OP_MIN_U64 = 4, WINDOW_OP_MAX_U64 = 5,
    // state (has a number, value, saw a NaN): a NaN is skipped unless nothing else is there, and the rule stays associative
    WINDOW_OP_MIN_F64 = 6, WINDOW_OP_MAX_F64 = 7
};
hipError_t launch_window_scan_tiles(const LaunchCfg& cfg, int op, const ColumnRef& arg, const uint64_t* part_flags, int64_t n, void* temp);
hipError_t launch_window_scan_summaries(const LaunchCfg& cfg, int op, int64_t n, void* temp);
// run_value[i]: the value as 64 bits (a MIN / MAX over NaNs alone: a NaN); run_count[i]: the non-NULL count
hipError_t launch_window_scan_apply(const LaunchCfg& cfg, int op, const ColumnRef& arg, const uint64_t* part_flags, int64_t n, const void* temp,
                                    uint64_t* run_value, uint32_t* run_count);

// out[i] from the running state at row frame_end[i] (null: at row i itself).  VALUE: the value narrowed to `out_dtype`, NULL when
// the count is 0; AVG: value / (double)count as Float64, NULL when the count is 0; COUNT: the count as UInt64 (validity may be null)
enum WindowFinishKind : int32_t { WINDOW_FINISH_VALUE = 0, WINDOW_FINISH_AVG = 1, WINDOW_FINISH_COUNT = 2 };
hipError_t launch_window_finish(const LaunchCfg& cfg, int kind, int out_dtype, const uint64_t* run_value, const uint32_t* run_count,
                                const uint32_t* frame_end, int64_t n, void* out, uint64_t* validity);

// ---- sliding ROWS frames: rows i + start .. i + end of row i's partition ---------------------------------------------------------
// The widest finite frame (end - start + 1 rows) window_slide takes.  Chosen, not tuned: a tile and the widest frame's neighbourhood,
// WINDOW_TILE_ROWS + WINDOW_SLIDE_MAX_ROWS - 1 rows of 9 bytes (about 46 KB), stay under the 64 KiB of LDS one workgroup may ask
// for.  Mirrored as ballista_amd.plan.WINDOW_SLIDE_MAX_ROWS.
constexpr int WINDOW_SLIDE_MAX_ROWS = 4096;
static_assert((WINDOW_TILE_ROWS + WINDOW_SLIDE_MAX_ROWS - 1) * 9 + 8 <= 64 * 1024, "window_slide stages a tile and its widest frame in LDS");

// lo[i] = max(part_start[i], i + start), hi[i] = min(part_end[i], i + end); an unbounded side takes the partition's bound.  An empty
// frame (lo > hi) is WINDOW_NULL_INDEX in both.  `start` and `end` are already clamped to [-n, n] (all arithmetic is 64-bit signed).
// A NEAR frame — two finite ends, neither more than WINDOW_SLIDE_MAX_ROWS rows from the current row — is given `part_flags` instead
// of the two bounds (null then): only a partition head among the rows it reaches over cuts it, and those flags are a few words, so a
// moving aggregate does not pay for the two bounds scans.  Every other frame: part_flags null, part_start and part_end.
inline bool window_frame_is_near(bool start_unbounded, int64_t start, bool end_unbounded, int64_t end) {
    return !start_unbounded && !end_unbounded && start >= -(int64_t)WINDOW_SLIDE_MAX_ROWS && end <= (int64_t)WINDOW_SLIDE_MAX_ROWS;
}
hipError_t launch_window_frame_bounds(const LaunchCfg& cfg, const uint64_t* part_flags, const uint32_t* part_start, const uint32_t* part_end,
                                      bool start_unbounded, int64_t start, bool end_unbounded, int64_t end, int64_t n, uint32_t* lo, uint32_t* hi);
// window_finish over a frame (lo, hi) of window_frame_bounds: the running state at row hi[i]; with `part_flags` (COUNT and the
// wrapping integer SUM alone) less the running state at row lo[i] - 1 unless lo[i] starts the partition.  An empty frame: count 0.
hipError_t launch_window_finish_frame(const LaunchCfg& cfg, int kind, int out_dtype, const uint64_t* run_value, const uint32_t* run_count,
                                      const uint64_t* part_flags, const uint32_t* lo, const uint32_t* hi, int64_t n, void* out, uint64_t* validity);
// The aggregate of a frame with two finite ends, straight from the argument: one workgroup per tile stages the argument of rows
// tile_first + start .. tile_last + end (clipped to [0, n)) in LDS, then every row walks its own lo .. hi in ascending order.
// ADD_F64: the accumulator starts at +0.0 and takes the non-NULL values in row order, so the bits are those of a plain loop.
// `start` / `end` as window_frame_bounds took them, end - start + 1 <= WINDOW_SLIDE_MAX_ROWS; `kind`: VALUE or AVG.
hipError_t launch_window_slide(const LaunchCfg& cfg, int op, int kind, int out_dtype, const ColumnRef& arg, const uint32_t* lo, const uint32_t* hi,
                               int64_t start, int64_t end, int64_t n, void* out, uint64_t* validity);

// ---- RANGE / GROUPS frames: the frame's ends are found by searching the sorted rows --------------------------------------------------
// One side of a frame.  OFFSET is signed like a rows frame's: -3 = 3 PRECEDING, +2 = 2 FOLLOWING; `f` for a float order key (RANGE).
enum WindowBoundKind : int32_t { WINDOW_BOUND_UNBOUNDED = 0, WINDOW_BOUND_CURRENT_ROW = 1, WINDOW_BOUND_OFFSET = 2 };
enum WindowFrameUnits : int32_t { WINDOW_UNITS_ROWS = 0, WINDOW_UNITS_RANGE = 1, WINDOW_UNITS_GROUPS = 2 };
struct WindowValueFrameArgs {
    int32_t units;                       // RANGE or GROUPS
    int32_t start_kind, end_kind;        // WindowBoundKind
    int32_t descending, nulls_first;     // of the order key (RANGE with an OFFSET side)
    int64_t start_i, end_i;              // OFFSET over an integer-typed key, and every GROUPS offset
    double start_f, end_f;               // OFFSET over a float key
    ColumnRef key;                       // the evaluated order key of the sorted rows: RANGE with an OFFSET side only
    const uint32_t *part_start, *part_end, *peer_start, *peer_end;
    const uint32_t* peers_to;            // GROUPS with an OFFSET side only
};
// lo[i] / hi[i] of row i's frame (WINDOW_NULL_INDEX in both: empty), one row per lane.  UNBOUNDED reads part_*, CURRENT ROW peer_*.
// An OFFSET side is a search inside the row's partition for the first row that qualifies (start) / the last one (end): it gallops
// outward from row i in steps of 1, 2, 4 ... and then bisects, at most about 2 log2(partition) probes and none of them waits on
// another lane.  RANGE compares the order key: rows are classed as the sort laid them (NULLs and the NaNs of one sign before the
// numbers, the rest after) and numbers compare exactly — integers as if unbounded (a key of 2^63 - 1 plus 2^63 - 1 does not wrap),
// floats against t = key_i +- offset, computed once in Float64, by IEEE comparison.  A row whose own key is NULL or NaN takes its peer
// bound.  GROUPS compares peers_to (the row's peer-group number, ascending).  `widest` (null: not kept): one word, zeroed by the
// caller, that receives the largest hi - lo + 1 (an atomic max, at most one per wave).
hipError_t launch_window_value_bounds(const LaunchCfg& cfg, const WindowValueFrameArgs& a, int64_t n, uint32_t* lo, uint32_t* hi, uint32_t* widest);

// Rows a tile of window_slide_value stages in LDS at most (8 bytes of value and one of flags each: 18 KiB, so LDS leaves eight
// workgroups to a CU).  Chosen, not tuned: a tile and as many rows again of neighbourhood.
constexpr int WINDOW_SLIDE_STAGE_ROWS = 2048;
static_assert(WINDOW_SLIDE_STAGE_ROWS > WINDOW_TILE_ROWS && WINDOW_SLIDE_STAGE_ROWS * 9 + 64 <= 64 * 1024, "window_slide_value stages at most this span");
// window_slide for a (lo, hi) of window_value_bounds, whose span no offset bounds before the launch: a tile's span runs from the
// smallest lo to the largest hi of its non-empty rows (one block reduction).  A span of at most WINDOW_SLIDE_STAGE_ROWS rows is staged
// and walked in LDS as window_slide does; a longer one (narrow frames that lie far apart) is walked in global memory by the same loop.
// Every frame holds at most WINDOW_SLIDE_MAX_ROWS rows (the caller read `widest`).  The additions have window_slide's order.
hipError_t launch_window_slide_value(const LaunchCfg& cfg, int op, int kind, int out_dtype, const ColumnRef& arg, const uint32_t* lo,
                                     const uint32_t* hi, int64_t n, void* out, uint64_t* validity);

}  // namespace bhip
