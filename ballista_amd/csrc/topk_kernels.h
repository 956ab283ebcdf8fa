// topk_kernels.h — launchers of kernels_topk.hip (internal C++ interface): the threshold selection behind a limit over a sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace bhip {

// the FIRST sort key of a batch: rows are ordered by the composite (NULL rank, image), the image being the sort's own
// (sort_device.h; a NULL row's is 0, then the descending flip) and the NULL rank present only where the column has a validity bitmap
struct TopkKey {
    ColumnRef col;
    int32_t descending, nulls_first;
};
// what the host reads once the passes ran: rows strictly before the threshold T, and rows equal to it — together the candidates
struct TopkCount { uint64_t less, equal; };

// 4- and 8-byte fixed-width types and Utf8 (its first 8 bytes); Boolean and the 1- and 2-byte integers are not imaged
bool topk_key_supported(int dtype);
// the image bytes (bit b: byte b, 0 = least significant) that can carry order for the type: the host queues passes for these only
uint32_t topk_key_bytes(int dtype);
constexpr int TOPK_NULL_BYTE = 8;                    // the pick over the NULL rank, the most significant digit of the composite
size_t topk_state_bytes();
const TopkCount* topk_state_count(const void* state);

// rows one thread of the diff and histogram passes loads per step: 16 bytes' worth from a fixed-width key on a 16-byte boundary,
// else one.  The host asks once per batch and hands the answer to both launchers, which instantiate exactly that form (1 is always
// allowed, anything else only where this function gives it): what the host times under "topk_*_row" is what ran.
int topk_rows_per_load(const TopkKey& key);
// zeroes `state`, sets the rank wanted (k, 1 <= k <= n) and gathers: the image bits that differ between any two rows, the rows per NULL rank
hipError_t launch_topk_diff(const LaunchCfg& cfg, const TopkKey& key, int rows_per_load, int64_t n, int64_t k, void* state);
// histogram of image byte `byte` over the rows that match the prefix chosen so far; nothing when all images agree on the byte
hipError_t launch_topk_hist(const LaunchCfg& cfg, const TopkKey& key, int rows_per_load, int64_t n, int byte, void* state);
// the bin of byte `byte` (or of the NULL rank: TOPK_NULL_BYTE) that holds the k-th row -> prefix, mask, rows still wanted, counts
hipError_t launch_topk_pick(const LaunchCfg& cfg, int byte, void* state);
// bit i = row i is a candidate (composite <= threshold) + per-tile counts (tile = SEL_TILE rows): the inputs of launch_select_indices
hipError_t launch_topk_mark(const LaunchCfg& cfg, const TopkKey& key, int64_t n, const void* state, uint64_t* bitmap, uint32_t* tile_counts);

}  // namespace bhip
