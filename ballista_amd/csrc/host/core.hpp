// core.hpp — host-side runtime objects: errors, the per-GPU context (caching allocator, stream
// pool, pinned staging), device buffers, columns, schemas, record batches.
//
// Reference conventions being mirrored: RecordBatch columns are Arc'd immutable buffers
// (rust/core/src/memory_stream.rs:29-92); errors are Result<_, DataFusionError> values, never
// panics (rust/core/src/execution_plans/unresolved_shuffle.rs:83-90; rust/core/src/error.rs).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ballista_hip.h"
#include "../kernels.h"

namespace bhip {

// ---- errors ---------------------------------------------------------------------------------
struct Error : std::runtime_error {
    bhip_status code;
    Error(bhip_status c, const std::string& m) : std::runtime_error(m), code(c) {}
};
// The keys do not fit the 16-byte packed key: too many key parts or too wide a layout at plan time (ProgramBuilder::add_key / finish),
// a Utf8 value longer than its share at run time (check_scan_flags).  HashAggregateExec and HashJoinExec catch it and take their
// wide-key forms; everybody else sees an ordinary BHIP_ENOTIMPL.
struct KeyWidthError : Error {
    explicit KeyWidthError(const std::string& m) : Error(BHIP_ENOTIMPL, m) {}
};
[[noreturn]] inline void fail(bhip_status c, const std::string& m) { throw Error(c, m); }
[[noreturn]] inline void fail_key_width(const std::string& m) { throw KeyWidthError(m); }
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        if (e == hipErrorOutOfMemory) fail(BHIP_EOOM, std::string(what) + ": " + hipGetErrorString(e));
        fail(BHIP_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    }
}
#define HIP_CHECK(expr) ::bhip::hip_check((expr), #expr)

void set_last_error(const std::string& m);
const char* get_last_error();

const char* dtype_name(int dt);
int dtype_width(int dt);   // bytes of a fixed-width value; 0 for Utf8 / Boolean

// ---- context ----------------------------------------------------------------------------------
class Context;

struct Block {               // one allocation of the caching allocator
    void* ptr = nullptr;
    size_t bytes = 0;
    hipStream_t last_stream = nullptr;
    hipEvent_t ready = nullptr;   // recorded on last_stream only when ANOTHER stream takes the block over (Context::alloc)
};

class Context : public std::enable_shared_from_this<Context> {
public:
    explicit Context(int device);
    ~Context();
    int device() const { return device_; }
    int cus() const { return cus_; }
    void set_device() const { HIP_CHECK(hipSetDevice(device_)); }

    // stream-aware caching allocator: a released block is reused by the same stream at once and
    // by another stream only after the release event
    void* alloc(size_t bytes, hipStream_t stream);
    void free(void* ptr, hipStream_t stream);
    void memory(uint64_t* in_use, uint64_t* peak);
    void trim();

    hipStream_t acquire_stream();
    void release_stream(hipStream_t s);

    // "everything enqueued on `stream` so far has finished", optionally with `bytes` (<= 56, a multiple of 4) of device
    // memory brought along: a one-thread kernel writes them and then a sequence number into a pinned host slot the caller
    // spins on.  A runtime wait (hipStreamSynchronize after a device-to-host copy) costs 30-40 us of wake-up latency on this
    // stack; an operator tree makes dozens of them per query.  Falls back to the runtime wait after ~2 ms of spinning.
    void wait_stream(hipStream_t stream, const void* dev_src = nullptr, void* host_dst = nullptr, size_t bytes = 0);

    // kernel timing hook (bench roofline): accumulated by the aggregate operator
    void add_kernel_time(double ms, uint64_t launches, const char* kernel = nullptr, const char* variant = nullptr);
    std::string kernel_name();
    std::string kernel_variant();   // instantiation of kernel_name() that ran ("" where the call site names none)
    // how the last lean scan + aggregate launch (timed or not) read its Utf8 keys: "fixed" (known uniform width, no offsets),
    // "offsets", or "none" (no Utf8 key); "" before the first one
    void set_lean_key_form(const char* form);
    std::string lean_key_form();
    // which loaded column each chain step of the last lean scan + aggregate launch used: "0,1,2,3,2" where the kernel formed
    // step 4's value from the registers of step 2 (an aliased instantiation of lean_spec_kernel.h), "none" where every step
    // loaded its own column (alias: 4 bits per step); "" before the first one
    void set_lean_step_alias(uint32_t alias, int n_steps);
    std::string lean_step_alias();
    // how the last limit directly over a sort ran: "topk" (threshold selection), "topk_fallback" (the selection declined every batch:
    // the plain sort, cut to k), "sort" (the full-sort route: k >= the rows there were, or BHIP_NO_TOPK); "" before the first one
    void set_sort_limit_form(const char* form);
    std::string sort_limit_form();
    // the table form of the HashJoinExec build side most recently built or probed: "narrow" (one integer key, unique: rank map /
    // CAS table), "packed" (the general table over 16-byte packed keys), "wide" (the table over row hashes that compares the key
    // columns: keys of any width — also when a probe batch forced it beside a packed table); "" before the first one
    void set_join_key_form(const char* form);
    std::string join_key_form();
    // how NestedLoopJoinExec ran its last probe batch: "compare" (the fused kernel), "general" (chunked candidates through the
    // filter), "cross" (no filter, pairs emitted directly), "exists" (an existence type without a filter); "" before the first one
    void set_nested_loop_form(const char* form);
    std::string nested_loop_form();
    // the probe kernel variant the narrow path launched for its last probe batch (kernels_join.hip launch_join_filter_probe):
    // "rank/mapbuf", "rank/flat", "rank/bits" (+perm, +resid, +rows8, +gather), "filter/map", "filter/table" (+present, +resid);
    // "" before the first one
    void set_join_probe_form(const char* form);
    std::string join_probe_form();
    void kernel_time(bool reset, double* ms, uint64_t* launches);
    bool timing_enabled() const { return timing_ > 0; }
    int timing_level() const { return timing_; }
    // per-kernel-name totals (BHIP_KERNEL_TIMING=1): event pairs queued by KernelTimer are resolved when read
    struct KernelStat { double ms = 0; uint64_t launches = 0; uint64_t bytes = 0; };    // bytes: algorithmic bytes of the timed launches
    void push_timed(hipEvent_t a, hipEvent_t b, const char* name, uint64_t bytes = 0);
    hipEvent_t timing_event();
    std::map<std::string, KernelStat> kernel_stats(bool reset);

private:
    int device_;
    int cus_ = 256;
    int timing_ = 0;
    std::mutex mu_;
    std::multimap<size_t, Block> free_blocks_;
    std::map<void*, Block> live_;
    uint64_t in_use_ = 0, peak_ = 0, cached_ = 0;
    std::vector<hipStream_t> stream_pool_;
    static constexpr size_t N_SLOTS = 1024;
    struct HostSlot { volatile uint64_t w[8]; };      // one cache line of pinned host memory: w[0] = sequence, w[1..7] = payload
    HostSlot* slots_ = nullptr;
    std::atomic<uint64_t> slot_seq_{0};
    bool spin_wait_ = true;
    double k_ms_ = 0;
    uint64_t k_launches_ = 0;
    std::string k_name_, k_variant_, k_key_form_, k_step_alias_, k_sort_limit_form_, k_join_key_form_, k_nested_loop_form_, k_join_probe_form_;
    struct PendingTimed { hipEvent_t a, b; const char* name; uint64_t bytes; };
    std::vector<PendingTimed> pending_timed_;
    std::vector<hipEvent_t> event_pool_;
    std::map<std::string, KernelStat> k_stats_;
};
using ContextPtr = std::shared_ptr<Context>;

// execution context of one task: the context + the HIP stream every kernel of the task runs on
struct Exec {
    ContextPtr ctx;
    hipStream_t stream;
    LaunchCfg cfg() const { return LaunchCfg{ctx->cus(), stream}; }
};

// times the launches enqueued on ex.stream during its lifetime under `name` (no-op unless BHIP_KERNEL_TIMING=1);
// nothing waits here: the event pair is read when the statistics are (bhip_ctx_kernel_stats)
struct KernelTimer {
    const Exec& ex;
    const char* name;
    hipEvent_t a = nullptr, b = nullptr;
    // rows: what the launch covers.  BHIP_KERNEL_TIMING=1 times launches over >= 2^18 rows only (an event pair per tiny
    // launch would stretch the small-launch tail it is there to measure); =2 times every launch
    uint64_t bytes = 0;
    KernelTimer(const Exec& e, const char* n, int64_t rows = -1, uint64_t algorithmic_bytes = 0) : ex(e), name(n), bytes(algorithmic_bytes) {
        const int level = ex.ctx->timing_level();
        if (level <= 0 || (level == 1 && rows < (1 << 18))) return;
        a = ex.ctx->timing_event();
        b = ex.ctx->timing_event();
        hipEventRecord(a, ex.stream);
    }
    void stop() {
        if (!a) return;
        hipEventRecord(b, ex.stream);
        ex.ctx->push_timed(a, b, name, bytes);
        a = b = nullptr;
    }
    ~KernelTimer() { stop(); }
};

#define TIMED_LAUNCH(ex, name, call) do { ::bhip::KernelTimer _kt((ex), (name)); HIP_CHECK(call); } while (0)
#define TIMED_LAUNCH_N(ex, name, rows, call) do { ::bhip::KernelTimer _kt((ex), (name), (int64_t)(rows)); HIP_CHECK(call); } while (0)
// ... with the launch's algorithmic bytes, for the roofline line of bench.py
#define TIMED_LAUNCH_B(ex, name, rows, bytes, call) do { ::bhip::KernelTimer _kt((ex), (name), (int64_t)(rows), (uint64_t)(bytes)); HIP_CHECK(call); } while (0)

// ---- device buffers -----------------------------------------------------------------------------
constexpr size_t BUFFER_SLACK = 16;

class Buffer {
public:
    Buffer(ContextPtr ctx, size_t bytes, hipStream_t stream);          // owned
    Buffer(ContextPtr ctx, void* borrowed, size_t bytes);              // borrowed device pointer
    // slice of `parent` (kept alive); the slicer leaves BUFFER_SLACK readable bytes behind every slice
    Buffer(ContextPtr ctx, std::shared_ptr<Buffer> parent, void* ptr, size_t bytes);
    ~Buffer();
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    void* ptr() const { return ptr_; }
    size_t bytes() const { return bytes_; }
    // owned buffers carry BUFFER_SLACK readable bytes past bytes(): kernels may over-read short strings
    bool owned() const { return owned_ || parent_ != nullptr; }
    template <class T> T* as() const { return reinterpret_cast<T*>(ptr_); }
    void set_stream(hipStream_t s) { stream_ = s; }
    // A fact about a Utf8 OFFSETS buffer, internal to the library (never part of bhip_column_desc): its first `rows` values are all
    // `w` bytes long, so row i's bytes are data[offsets[0] + i*w, +w).  0: unknown.  It is set by producers that know it by
    // construction and by the lean scan once it has read every length (ops_agg.cpp); whoever ignores it stays correct, the
    // offsets are all there.  It lives here because the buffer is what every copy of a column shares and nothing rewrites: a
    // take, a concatenation, an exchange or a slice builds new buffers, which start unknown.  Atomic: partitions that scan one
    // column at the same time may learn it at the same time.
    int32_t uniform_width(int64_t rows) const {
        const uint64_t f = uniform_.load(std::memory_order_relaxed);
        return (int64_t)(f >> 32) >= rows ? (int32_t)(f & 0x7FFFFFFFu) : 0;
    }
    void set_uniform_width(int64_t rows, int32_t w) {
        if (w < 1 || rows < 1 || rows > 0xFFFFFFFFll) return;
        const uint64_t f = ((uint64_t)rows << 32) | (uint32_t)w;
        uint64_t cur = uniform_.load(std::memory_order_relaxed);
        while ((cur >> 32) < (uint64_t)rows && !uniform_.compare_exchange_weak(cur, f, std::memory_order_relaxed)) {}
    }
private:
    std::atomic<uint64_t> uniform_{0};
    ContextPtr ctx_;
    void* ptr_;
    size_t bytes_;
    bool owned_;
    hipStream_t stream_;
    std::shared_ptr<Buffer> parent_;
};
using BufferPtr = std::shared_ptr<Buffer>;
BufferPtr make_buffer(const Exec& ex, size_t bytes);
// n uint32_t row indices: a selection, a permutation, a view's index vector
inline BufferPtr index_buffer(const Exec& ex, int64_t n) { return make_buffer(ex, (size_t)n * 4 + 8); }
inline size_t bitmap_bytes(int64_t n_bits) { return (size_t)((n_bits + 63) / 64) * 8; }
// slots of an open-addressing table over `rows` keys: the power of two >= 2 x rows, at least 1024
inline uint64_t table_capacity(uint64_t rows) { uint64_t cap = 1024; while (cap < 2 * rows) cap <<= 1; return cap; }

// scratch that lives for one operator call
struct Temp {
    const Exec& ex;
    std::vector<BufferPtr> held;
    explicit Temp(const Exec& e) : ex(e) {}
    template <class T> T* get(size_t count) {
        held.push_back(make_buffer(ex, count * sizeof(T) + 16));
        return held.back()->as<T>();
    }
};

// ---- columns / schema / batches -------------------------------------------------------------------
struct Column {
    int dtype = 0;
    int64_t length = 0;
    BufferPtr data;        // values | Utf8 bytes | Boolean bitmap
    BufferPtr offsets;     // Utf8
    BufferPtr validity;    // may be null
    int64_t data_bytes = 0;   // Utf8 value bytes
    // A VIEW (only between a HashJoinExec and the HashJoinExec that asked for it, host/ops_join.cpp): row i is row view_idx[i] of
    // *view_base, NULL where the index is 0xFFFFFFFF; data / offsets / validity are unset.  take_columns composes the indices, so a
    // payload column that passes through several joins is gathered ONCE, for the rows that survive them all.
    std::shared_ptr<const Column> view_base;
    BufferPtr view_idx;
    bool view_may_null = false;
    bool is_view() const { return (bool)view_base; }
    // Utf8: the one width of the first `rows` values where it is known (Buffer::uniform_width), else 0.
    // INVARIANT this rests on: a Column has no row offset — its row i is entry i of `offsets` — and whatever makes a column of
    // other rows (slice, take, concatenation, exchange) makes a NEW offsets Buffer.  A slicing path that shared the offsets
    // BufferPtr with a shifted start would have to carry the shift here (or drop the fact), or the fixed-width key form
    // would read the wrong bytes.
    int32_t utf8_width(int64_t rows) const { return dtype == DT_UTF8 && offsets ? offsets->uniform_width(rows) : 0; }
    // the validity bitmap as the kernels take it, nullptr where there is none (not const: as Buffer::as, it serves whoever fills the column too)
    uint64_t* validity_words() const { return validity ? validity->as<uint64_t>() : nullptr; }
    ColumnRef ref() const {
        ColumnRef r;
        r.data = data ? data->ptr() : nullptr;
        r.offsets = offsets ? offsets->as<int32_t>() : nullptr;
        r.validity = validity_words();
        r.dtype = dtype;
        r.data_bytes = (int32_t)data_bytes;
        return r;
    }
    int64_t memory_size() const;
};

// The buffers of a materialised column: THE place that knows which buffers a column of a type has and how many bytes each holds.
// Everything that moves a column across the library's edge (host import and export, the packed blocks of the exchange) walks
// this, in the order it needs, and every column an operator produces is allocated from it (alloc_column below).
enum BufferRole { BUF_VALIDITY = 0, BUF_OFFSETS = 1, BUF_DATA = 2 };
struct BufferSpec {
    bool present = false;
    bool bitmap = false;       // validity, Boolean values: the device copy is zero-padded to whole words
    size_t arrow_bytes = 0;    // what the Arrow buffer holds: (n+7)/8, (n+1)*4, the Utf8 value bytes, n*width
    size_t device_bytes = 0;   // on the device: bitmaps as whole 64-bit words (they are read as u64), everything else as in Arrow
    size_t alloc_bytes = 0;    // logical size of a buffer the library allocates: device_bytes, + 8 of slack on values and bitmaps
};
struct ColumnLayout {
    BufferSpec buf[3];         // by BufferRole
    const BufferSpec& operator[](BufferRole r) const { return buf[r]; }
};
ColumnLayout column_layout(int dtype, int64_t n_rows, int64_t data_bytes, bool has_validity);
inline ColumnLayout column_layout(const Column& c) { return column_layout(c.dtype, c.length, c.data_bytes, (bool)c.validity); }
inline const BufferPtr& column_buffer(const Column& c, BufferRole r) { return r == BUF_VALIDITY ? c.validity : r == BUF_OFFSETS ? c.offsets : c.data; }

// THE allocator of a column the library produces: dtype, length and data_bytes set, and every buffer that column_layout marks
// present allocated at its alloc_bytes — uninitialised, but for the one zero that is the offsets of a zero-row Utf8 column.
// utf8_data_bytes < 0: a Utf8 column whose value bytes are known only once its offsets are written (plan.hpp utf8_from_lengths):
// no data buffer yet, utf8_alloc_data brings it.
Column alloc_column(const Exec& ex, int dtype, int64_t n_rows, bool with_validity, int64_t utf8_data_bytes = 0);
// ... the data buffer, with room for `bytes` value bytes (BHIP_EEXEC above 2 GiB: the offsets are Int32).  `bytes` may be a bound:
// out.data_bytes stays with whoever knows the total.
void utf8_alloc_data(const Exec& ex, Column& out, int64_t bytes);
// a validity bitmap over n rows, for a column that turns out to need one after it was allocated
BufferPtr validity_buffer(const Exec& ex, int64_t n_rows);

struct Field {
    std::string name;
    int dtype;
    bool nullable;
    // LargeUtf8 at the boundary (Arrow C data, IPC files, wire schemas): 64-bit offsets there; the device column is an ordinary Utf8
    // column (int32 offsets: < 2 GiB of value bytes per batch, refused beyond).  The flag follows the column through the operators.
    bool large = false;
    // Binary at the boundary (sha224 .. sha512 produce it): the same buffers as Utf8, nothing reads them as text
    bool binary = false;
};

struct Schema {
    std::vector<Field> fields;
    int index_of(const std::string& name) const {
        for (size_t i = 0; i < fields.size(); ++i)
            if (fields[i].name == name) return (int)i;
        return -1;
    }
};
using SchemaPtr = std::shared_ptr<const Schema>;

struct Batch {
    SchemaPtr schema;
    std::vector<Column> cols;
    int64_t n_rows = 0;
    ContextPtr ctx;
    int64_t memory_size() const;
};
using BatchPtr = std::shared_ptr<const Batch>;
// a batch of n_rows rows whose columns the caller is about to fill
inline std::shared_ptr<Batch> new_batch(const ContextPtr& ctx, const SchemaPtr& schema, int64_t n_rows) {
    auto b = std::make_shared<Batch>();
    b->schema = schema;
    b->ctx = ctx;
    b->n_rows = n_rows;
    return b;
}

// host <-> device movement
BatchPtr batch_from_host(const ContextPtr& ctx, int n_cols, const bhip_column_desc* cols, int64_t n_rows, bool device_ptrs);
void column_to_host(const Batch& b, int i, void* data, int32_t* offsets, uint8_t* validity);
// text in host memory -> device batch of the projected fields (text_scan.cpp).  BHIP_TEXT_TBL: '|'-separated TPC-H text
// (kernels_tbl.hip); BHIP_TEXT_CSV: any one-byte delimiter, quoted fields, NULLs, optional header (kernels_csv.hip, csv_opts)
BatchPtr batch_from_text(const ContextPtr& ctx, int format, const void* text_host, int64_t n_bytes, int n_fields,
                         const bhip_column_desc* fields, int n_proj, const int32_t* projection, const bhip_csv_opts& csv_opts);

// pinned host blocks from a process-wide pool, pageable memory when no pinned memory is left (parquet.cpp: PinnedPool)
void* pinned_host_alloc(size_t bytes);
void pinned_host_free(void* p, size_t bytes);

// whole-batch operations (ops_basic.cpp)
// permutation: `indices` holds every input row exactly once (Utf8 value bytes are then known without a read-back)
BatchPtr take_batch(const Exec& ex, const Batch& in, const uint32_t* indices, int64_t n_out, SchemaPtr schema = nullptr,
                    bool permutation = false);
Column take_column(const Exec& ex, const Column& c, const uint32_t* indices, int64_t n_out, int64_t known_bytes = -1);
BatchPtr concat_batches(const Exec& ex, const SchemaPtr& schema, const std::vector<BatchPtr>& parts);
BatchPtr slice_head(const Exec& ex, const Batch& in, int64_t n);

// BHIP_TRACE_HOST=1: one stderr line per call, "[bhip-host] <us since the first point> <what>" — where the host's time goes between
// the launches of a task (the device side is rocprofv3's job)
void trace_point(const char* what);

// read a small device value once the task's stream has caught up (Context::wait_stream)
template <class T>
T read_device(const Exec& ex, const T* dev) {
    T host;
    if (sizeof(T) <= 56 && sizeof(T) % 4 == 0) {
        ex.ctx->wait_stream(ex.stream, dev, &host, sizeof(T));
        return host;
    }
    HIP_CHECK(hipMemcpyAsync(&host, dev, sizeof(T), hipMemcpyDeviceToHost, ex.stream));
    HIP_CHECK(hipStreamSynchronize(ex.stream));
    return host;
}
inline void stream_wait(const Exec& ex) { ex.ctx->wait_stream(ex.stream); }

}  // namespace bhip

// opaque C handles
struct bhip_ctx { bhip::ContextPtr p; std::atomic<int> rc{1}; };
struct bhip_batch { bhip::BatchPtr p; std::atomic<int> rc{1}; std::vector<std::string> names; };
