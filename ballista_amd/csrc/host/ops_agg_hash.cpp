// ops_agg_hash.cpp — the high-cardinality path of HashAggregateExec: one device-wide hash table over the packed keys of every
// input row (kernels_hash.hip), SUM(Float64) in row order (kernels_dagg.hip).  Called by run_packed (ops_agg.cpp) when the
// register path holds too few groups or accumulators.
//
// Input that comes clustered by group key (lineitem by order key) is aggregated per RUN of equal keys; runs that turn out to be
// distinct groups need no table at all and can be emitted straight from their slots (HashAggResult::slots).  The host waits once
// for the run statistics (clustered input only) and once for the tail: group count, spill list length, scan status.
#include "../sort_kernels.h"
#include "../util_kernels.h"
#include "hash_kernels.h"
#include "plan.hpp"

namespace bhip {

HashAggResult hash_aggregate(const Exec& ex, Temp& tmp, const ScanParams& P0, const ProgramBuilder& pb, const std::vector<BatchPtr>& inputs,
                             bool nullable, ScanStatus* status, std::atomic<int>* clustered_hint, bool slot_keys) {
    const LaunchCfg cfg = ex.cfg();
    int64_t total_rows = 0;
    for (auto& b : inputs) total_rows += b->n_rows;
    // slots are 32-bit indices into a table of >= 2 x rows entries
    if (total_rows > 0x7FFFFFF0ll) fail(BHIP_ENOTIMPL, "hash aggregate over more than 2^31 input rows per partition");
    const int n_acc = P0.n_acc > 0 ? P0.n_acc : 1;
    HashAggTable T;
    memset(&T, 0, sizeof(T));
    T.n_acc = P0.n_acc;
    uint64_t* keys = tmp.get<uint64_t>(2 * (size_t)total_rows);
    T.keys128 = keys;
    MergeAccKinds kinds;
    for (int i = 0; i < VM_MAX_ACC; ++i) kinds.kind[i] = i < P0.n_acc ? P0.acc[i].kind : (uint8_t)ACC_COUNT_ROWS;
    uint64_t* tail = tmp.get<uint64_t>(2);          // [0] the group count, [1] the spill list's entry count | "lists too long" << 32: read in one piece
    {
        FillMany fm;
        static_assert(sizeof(ScanStatus) % 4 == 0, "cleared word-wise");
        fm.add(status, sizeof(ScanStatus));
        fm.add(tail, 16);
        TIMED_LAUNCH(ex, "fill_many", launch_fill_many(cfg, fm));
    }
    // SUM(Float64) accumulators are summed in row order after the scan (kernels_dagg.hip); BHIP_AGG_ATOMIC=1: atomic adds
    // (order of addition left to the scheduler: the same sums to ~1e-16 relative, not bit for bit)
    static const bool atomic_sums = env_flag("BHIP_AGG_ATOMIC");
    memset(T.fsum_of_acc, 0xFF, sizeof(T.fsum_of_acc));
    DetSum D;
    memset(&D, 0, sizeof(D));
    if (!atomic_sums && total_rows > 0) {
        for (int a = 0; a < P0.n_acc; ++a)
            if (P0.acc[a].kind == ACC_SUM_F64) { D.acc_of_fsum[T.n_fsum] = (uint8_t)a; T.fsum_of_acc[a] = (uint8_t)T.n_fsum++; }
    }
    T.total_rows = (uint64_t)total_rows;
    T.rowslot = tmp.get<uint32_t>((size_t)total_rows + 1);
    if (T.n_fsum) T.fvals = tmp.get<double>((size_t)total_rows * T.n_fsum);

    // ---- the packed key of every row --------------------------------------------------------------------------------------
    {
        // plain NULL-free integer / date key columns: a streaming pack (kernels_util.hip) instead of a launch of the expression VM
        static const bool no_fixed_pack = env_flag("BHIP_NO_FIXED_KEY_PACK");
        std::vector<ProgramBuilder::PlainKeyPart> parts;
        const bool plain = !no_fixed_pack && pb.plain_fixed_keys(parts) && parts.size() <= (size_t)FIXED_KEY_PARTS_MAX;
        uint32_t row_base = 0;
        for (auto& b : inputs) {
            bool packed = false;
            if (plain) {
                FixedKeyParts K;
                memset(&K, 0, sizeof(K));
                K.n = (int32_t)parts.size();
                packed = true;
                for (size_t p = 0; p < parts.size(); ++p) {
                    const Column& c = b->cols[(size_t)parts[p].schema_index];
                    if (c.validity || c.is_view() || !c.data) { packed = false; break; }
                    K.src[p] = c.data->ptr(); K.width[p] = (uint8_t)parts[p].width; K.pos[p] = (uint8_t)parts[p].pos;
                }
                if (packed) TIMED_LAUNCH_N(ex, "pack_fixed_keys", b->n_rows, launch_pack_fixed_keys(cfg, K, b->n_rows, keys + 2ull * row_base));
            }
            if (!packed) {
                ScanParams P = P0;
                ProgramBuilder::bind(P, pb.columns(), *b, nullable);
                TIMED_LAUNCH_N(ex, "scan_keys", b->n_rows, launch_scan_keys(cfg, P, keys + 2ull * row_base, nullptr, nullptr, status));
            }
            row_base += (uint32_t)b->n_rows;
        }
    }

    // ---- rows of a group mostly consecutive?  the table is consulted per RUN of equal keys, slots = runs (kernels_hash.hip) ------
    // Decided on the leading rows: at most half as many runs as rows.  Not with a fused predicate (a filtered-out row would
    // have to leave its run).  The operator remembers what it found.
    static const bool no_runs = env_flag("BHIP_NO_RUN_AGG");
    // clustered input: 0 = look every run up in the run table; 1 = the runs are distinct groups (first key part ascending);
    // 2 = two ascending stretches (one place where it does not ascend): the second stretch is matched against the first by binary search
    bool runs = false;
    int distinct_runs = 0;
    uint32_t* run_head = nullptr;
    uint64_t n_runs_host = 0;
    if (!no_runs && P0.pred_slot < 0 && total_rows >= 4096 && clustered_hint->load() >= 0) {
        uint32_t* flags = tmp.get<uint32_t>((size_t)total_rows + 1);
        uint32_t* before = tmp.get<uint32_t>((size_t)total_rows + 1);
        uint64_t* n_runs_dev = tmp.get<uint64_t>(3);               // [0] runs, [1] places where the first key part does not ascend, [2] the first of them
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes(total_rows));
        // the first key part's bytes in the packed key (parts are laid out from byte 0: ProgramBuilder::finish)
        const int w0 = P0.n_keyparts > 0 ? P0.keyparts[0].width : 0;
        const uint64_t first_mask = w0 >= 8 ? ~0ull : w0 > 0 ? ((1ull << (8 * w0)) - 1ull) : 0ull;
        static const bool no_distinct = env_flag("BHIP_NO_DISTINCT_RUNS");      // A/B: always the run table
        const int64_t sample = std::min<int64_t>(total_rows, 1 << 20);
        const uint64_t info0[3] = {0, 0, ~0ull};
        HIP_CHECK(hipMemcpyAsync(n_runs_dev, info0, sizeof(info0), hipMemcpyHostToDevice, ex.stream));
        TIMED_LAUNCH_N(ex, "run_heads", sample, launch_run_heads(cfg, keys, (uint32_t)sample, flags, first_mask, n_runs_dev + 1));
        HIP_CHECK(exclusive_scan_u32_u32(ex.stream, flags, sample, before, false, n_runs_dev, scan_tmp));
        struct RunInfo { uint64_t n_runs, breaks, first_break; };
        RunInfo ri = read_device(ex, reinterpret_cast<const RunInfo*>(n_runs_dev));
        runs = clustered_hint->load() == 1 || 2 * ri.n_runs <= (uint64_t)sample;
        clustered_hint->store(runs ? 1 : -1);
        if (runs) {
            if (sample < total_rows) {
                HIP_CHECK(hipMemcpyAsync(n_runs_dev, info0, sizeof(info0), hipMemcpyHostToDevice, ex.stream));
                TIMED_LAUNCH_N(ex, "run_heads", total_rows, launch_run_heads(cfg, keys, (uint32_t)total_rows, flags, first_mask, n_runs_dev + 1));
                HIP_CHECK(exclusive_scan_u32_u32(ex.stream, flags, total_rows, before, false, n_runs_dev, scan_tmp));
                // one more (short) wait: with the run count on the host every table below is sized by the runs, not by the rows, and
                // when the runs turn out distinct the run table, the slot flags, their scan and the slot compaction are not run at all
                if (ri.breaks <= 1 && !no_distinct) ri = read_device(ex, reinterpret_cast<const RunInfo*>(n_runs_dev));
                else ri.breaks = 2;
            }
            distinct_runs = (no_distinct || first_mask == 0 || ri.breaks > 1) ? 0 : ri.breaks == 0 ? 1 : 2;
            n_runs_host = ri.n_runs;
            uint32_t* head = tmp.get<uint32_t>((size_t)total_rows + 1);
            run_head = head;
            TIMED_LAUNCH_N(ex, "run_slots", total_rows, launch_run_slots(cfg, flags, before, (uint32_t)total_rows, T.rowslot, head));
            if (distinct_runs == 2) {
                // the runs from the break on: matched against the first stretch, new groups numbered behind it
                const uint32_t split_row = (uint32_t)ri.first_break;
                uint32_t* head2 = tmp.get<uint32_t>((size_t)n_runs_host + 1);
                uint32_t* match = tmp.get<uint32_t>((size_t)n_runs_host + 1);
                uint32_t* fresh = tmp.get<uint32_t>((size_t)n_runs_host + 1);
                uint32_t* fresh_before = tmp.get<uint32_t>((size_t)n_runs_host + 2);
                // (the second stretch's length is only known on the device: sized by the runs; entries past it are never read)
                HIP_CHECK(hipMemsetAsync(fresh, 0, ((size_t)n_runs_host + 1) * 4, ex.stream));
                TIMED_LAUNCH_N(ex, "run_tail_resolve", total_rows, launch_run_tail_resolve(cfg, keys, head, n_runs_dev, T.rowslot, (uint32_t)total_rows, split_row, first_mask,
                                                                                          head2, match, fresh));
                // the scan runs over all `n_runs` entries of `fresh` (zeros past the second stretch): fresh_before[t] for t < tail length,
                // and fresh_before[tail length] = the number of new groups, whatever the tail length is
                HIP_CHECK(exclusive_scan_u32_u32(ex.stream, fresh, (int64_t)n_runs_host + 1, fresh_before, false, nullptr, scan_tmp));
                TIMED_LAUNCH_N(ex, "run_tail_remap", total_rows, launch_run_tail_remap(cfg, head, n_runs_dev, (uint32_t)total_rows, split_row, match, fresh_before, T.rowslot,
                                                                                      head2, tail));
                run_head = head2;
            } else if (!distinct_runs) {
                const uint64_t tcap = table_capacity((uint64_t)total_rows);
                uint32_t* table = tmp.get<uint32_t>(tcap);
                uint32_t* min_head = tmp.get<uint32_t>(tcap);
                uint32_t* slot_of_run = tmp.get<uint32_t>((size_t)total_rows + 1);
                uint32_t* winner = tmp.get<uint32_t>((size_t)total_rows + 1);
                T.owner = tmp.get<uint32_t>((size_t)total_rows + 1);
                HIP_CHECK(hipMemsetAsync(table, 0, tcap * 4, ex.stream));
                HIP_CHECK(hipMemsetAsync(min_head, 0xFF, tcap * 4, ex.stream));
                HIP_CHECK(hipMemsetAsync(T.owner, 0, ((size_t)total_rows + 1) * 4, ex.stream));
                TIMED_LAUNCH_N(ex, "run_groups", total_rows, launch_run_groups(cfg, keys, (uint32_t)total_rows, head, n_runs_dev, table, tcap - 1, min_head, slot_of_run,
                                                                                winner, T.owner, T.rowslot));
            }
        }
    }

    uint64_t cap;
    bool table_owner = false;
    if (runs) {
        // the slot space is the space of runs: at most one per row (unused ones stay empty); exactly the runs when they are distinct
        cap = distinct_runs ? std::max<uint64_t>(n_runs_host, 1) : (uint64_t)total_rows;
        T.slots_given = 1;
        T.mask = cap - 1;
    } else {
        cap = table_capacity((uint64_t)total_rows);         // (every row could be its own group)
        T.mask = cap - 1;
        T.owner = tmp.get<uint32_t>(cap);
        table_owner = true;
    }
    T.acc = tmp.get<uint64_t>(cap * n_acc);
    T.rows = tmp.get<uint64_t>(cap);
    if (nullable) T.nvalid = tmp.get<uint64_t>(cap * n_acc);
    if (T.n_fsum) {
        D.runs = tmp.get<uint32_t>(cap);
        D.spill_head = tmp.get<uint32_t>(cap);
    }
    {
        FillMany fm;                                 // everything the scan and the ordered sums expect cleared, one launch
        if (table_owner) fm.add(T.owner, cap * 4);       // (the run paths filled theirs)
        fm.add(T.rows, cap * 8);
        if (nullable) fm.add(T.nvalid, cap * n_acc * 8);
        if (T.n_fsum) {
            fm.add(D.runs, cap * 4);
            fm.add(D.spill_head, cap * 4, 0xFFFFFFFFu);
        }
        TIMED_LAUNCH(ex, "fill_many", launch_fill_many(cfg, fm));
    }
    if (P0.n_acc > 0) TIMED_LAUNCH(ex, "hash_agg_init", launch_hash_agg_init(cfg, T, kinds));

    uint32_t row_base = 0;
    for (auto& b : inputs) {
        ScanParams P = P0;
        ProgramBuilder::bind(P, pb.columns(), *b, nullable);
        TIMED_LAUNCH_N(ex, "scan_agg_hash", b->n_rows, launch_scan_agg_hash(cfg, P, T, row_base, status));
        row_base += (uint32_t)b->n_rows;
    }
    if (T.n_fsum) {
        const size_t n_tiles = ((size_t)total_rows + 1023) / 1024, stage_n = n_tiles * 1024;
        D.rowslot = T.rowslot;
        D.fvals = T.fvals;
        D.total_rows = T.total_rows;
        D.n_fsum = T.n_fsum;
        D.n_acc = T.n_acc;
        D.seg_slot = tmp.get<uint32_t>(stage_n);
        D.seg_first = tmp.get<uint32_t>(stage_n);
        D.seg_sum = tmp.get<double>(stage_n * T.n_fsum);
        D.tile_nseg = tmp.get<uint32_t>(n_tiles);
        D.acc = T.acc;
        D.rows = T.rows;
        D.spill_key = tmp.get<uint64_t>(stage_n);
        D.spill_seg = tmp.get<uint32_t>(stage_n);
        D.spill_count = reinterpret_cast<uint32_t*>(tail + 1);
        D.spill_next = tmp.get<uint32_t>(stage_n);
        // (D.runs, D.spill_head and the spill count — the second word of `tail` — were cleared above)
        TIMED_LAUNCH_N(ex, "det_segments", total_rows, launch_det_segments(cfg, D));
        TIMED_LAUNCH_N(ex, "det_apply", total_rows, launch_det_apply(cfg, D));
        // groups with several runs: combined through their lists right here; the entry count and the "lists too long" flag are
        // read together with the group count below (ONE host wait for the whole tail of the aggregate)
        TIMED_LAUNCH_N(ex, "det_spill_lists", total_rows, launch_det_spill_lists(cfg, D));
    }
    // used slots -> dense records (slot order: deterministic for a given input); distinct runs ARE the dense records
    uint64_t* dense = nullptr;
    if (!distinct_runs) {
        uint32_t* flags = tmp.get<uint32_t>(cap);
        dense = tmp.get<uint64_t>(cap + 1);
        void* scan_tmp = tmp.get<uint8_t>(exclusive_scan_temp_bytes((int64_t)cap));
        TIMED_LAUNCH_N(ex, "hash_agg_flags", cap, launch_hash_agg_flags(cfg, T, flags));
        HIP_CHECK(exclusive_scan_u32_u64(ex.stream, flags, (int64_t)cap, dense, false, tail, scan_tmp));
    }
    struct Tail { uint64_t n_groups; uint32_t n_spill, lists_too_long; };
    const Tail tl = read_device(ex, reinterpret_cast<const Tail*>(tail));
    const uint64_t ng = distinct_runs == 1 ? n_runs_host : tl.n_groups;           // (two stretches: written by run_tail_remap)
    if (T.n_fsum && tl.lists_too_long) {
        // some group has many runs (unclustered input): the whole list ordered by (slot, first row), then added up left to right
        const uint32_t n_spill = tl.n_spill;
        BufferPtr kb = std::make_shared<Buffer>(ex.ctx, D.spill_key, (size_t)n_spill * 8), pb2 = std::make_shared<Buffer>(ex.ctx, D.spill_seg, (size_t)n_spill * 4);
        radix_sort_pairs(ex, kb, pb2, (int64_t)n_spill);
        TIMED_LAUNCH_N(ex, "det_spill_combine", n_spill, launch_det_spill_combine(cfg, D, kb->as<uint64_t>(), pb2->as<uint32_t>(), n_spill));
    }
    if (pb.can_raise()) check_scan_status(ex, status);   // (after the one wait above: immediate; fixed-width keys and no integer division raise nothing)
    HashAggResult res;
    memset(&res, 0, sizeof(res));
    res.n_groups = (int64_t)ng;
    static const bool no_slot_emit = env_flag("BHIP_NO_SLOT_EMIT");
    if (ng && distinct_runs && slot_keys && !no_slot_emit) {
        // distinct runs: slot g IS group g — the caller emits its columns straight from the slot arrays (no GroupRec table in between)
        res.slots = SlotSource{T.keys128, run_head, T.acc, nullable ? T.nvalid : nullptr, T.rows, T.n_acc, 1};
        return res;
    }
    GroupRec* table = res.table = tmp.get<GroupRec>(ng ? ng : 1);
    if (ng && distinct_runs) TIMED_LAUNCH_N(ex, "run_compact", ng, launch_run_compact(cfg, T, run_head, (uint32_t)ng, nullable, table));
    else if (ng) TIMED_LAUNCH_N(ex, "hash_agg_compact", cap, launch_hash_agg_compact(cfg, T, dense, nullable, table));
    return res;
}


}  // namespace bhip
