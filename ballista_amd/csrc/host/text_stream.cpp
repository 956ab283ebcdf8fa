// text_stream.cpp — CsvExec over files of any size: the scan leaf of `--format tbl` / `--format csv`
// (rust/benchmarks/tpch/src/main.rs:129-150, rust/core/src/serde/physical_plan/from_proto.rs:93-110) as a slab pipeline.
//
// A file is cut into slabs of `slab_bytes` of text, wherever those fall.  One reader thread preads slab k + 2 into a ring of
// pinned host buffers while slab k + 1 crosses PCIe on a copy stream and slab k goes through the passes of text_scan.cpp on
// the task's stream; events order the three.  A slab yields the records that END in it: what lies behind its last record end
// (the carry, `cut` of text_scan.hpp) is moved device-to-device in front of the next slab's bytes:
//
//      base          base + gap            A (fixed, 256-byte aligned)              A + n_new
//       | 0 0 ... 0 0 | carry of slab k - 1 | bytes of slab k, copied from the host ... |
//
// base = A - carry rounded up to 256, so the text the kernels see stays 256-byte aligned with its pieces at multiples of 16;
// the gap (< 256 bytes) is NUL — neither a quote nor a newline — and the first record starts behind it (TextSlab::first_record).
// A slab in which no record ends waits whole for the next one; what waits may be one slab at most, so a record has to end in
// the slab it starts in or in the next one (BHIP_ENOTIMPL otherwise) — always true of a record that fits one slab — and every
// offset stays below 4 GiB.  Room for the carry in front of A is CARRY_ROOM; a longer carry (one record of more than 1 MiB)
// takes the slow path: carry and new bytes are put together in a buffer of their own.
//
// Every host-to-device copy reads a ring buffer that lives as long as the stream; the small values the passes need are kernel
// arguments or written by kernels.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <thread>

#include "plan.hpp"
#include "text_scan.hpp"

namespace bhip {

namespace {

constexpr int64_t SLAB_DEFAULT = 64ll << 20, SLAB_MIN = TBL_CHUNK, SLAB_MAX = 2ll << 30;
constexpr int64_t CARRY_ROOM = 1ll << 20;
constexpr int RING = 3;

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// a record that does not end inside carry + slab
[[noreturn]] void fail_record_too_long(const char* what) {
    fail(BHIP_ENOTIMPL, std::string(what) + ": a record does not end within the carry (one slab at most) plus one slab: it is longer "
                        "than the slab (raise slab_bytes / BHIP_TEXT_SLAB_MB), or a quoted field is not closed");
}

void check_slab_bytes(int64_t v, const std::string& what) {
    if (v < SLAB_MIN || v > SLAB_MAX || v % TBL_CHUNK != 0)
        fail(BHIP_EINVAL, what + " = " + std::to_string(v) + " bytes: a slab is a multiple of 16 KiB between 16 KiB and 2 GiB");
}

// BHIP_TEXT_SLAB_MB (MiB, fractions allowed: 0.015625 = 16 KiB), read when the library is loaded
struct SlabEnv { bool set = false; bool number = false; double mb = 0; std::string text; };
const SlabEnv g_slab_env = [] {
    SlabEnv e;
    if (const char* v = getenv("BHIP_TEXT_SLAB_MB")) {
        e.set = true;
        e.text = v;
        char* end = nullptr;
        e.mb = strtod(v, &end);
        e.number = end != v && *end == '\0' && std::isfinite(e.mb);
    }
    return e;
}();

int64_t resolve_slab_bytes(int64_t requested) {
    if (requested != 0) {
        check_slab_bytes(requested, "slab_bytes");
        return requested;
    }
    if (!g_slab_env.set) return SLAB_DEFAULT;
    if (!g_slab_env.number || g_slab_env.mb <= 0 || g_slab_env.mb > 4096) fail(BHIP_EINVAL, "BHIP_TEXT_SLAB_MB = '" + g_slab_env.text + "' is not a slab size in MiB");
    const double bytes = g_slab_env.mb * 1048576.0;
    if (bytes != std::floor(bytes)) fail(BHIP_EINVAL, "BHIP_TEXT_SLAB_MB = '" + g_slab_env.text + "' is not a whole number of bytes");
    check_slab_bytes((int64_t)bytes, "BHIP_TEXT_SLAB_MB");
    return (int64_t)bytes;
}

struct TextScanConfig {
    int format = BHIP_TEXT_TBL;
    uint8_t delimiter = '|';
    bool has_header = false;
    int64_t slab_bytes = SLAB_DEFAULT;
    SchemaPtr file_schema;
    std::vector<uint32_t> proj;
    bool has_proj = false;
};

class TextScanStream : public RecordBatchStream {
public:
    TextScanStream(SchemaPtr schema, std::shared_ptr<const TextScanConfig> cfg, std::string file, const Exec& ex)
        : schema_(std::move(schema)), cfg_(std::move(cfg)), file_(std::move(file)), ex_(ex) {}
    ~TextScanStream() override { close(); }
    SchemaPtr schema() const override { return schema_; }

    BatchPtr next() override {
        if (done_) return nullptr;
        ex_.ctx->set_device();
        try {
            if (!open_) open();
            while (!done_)
                if (BatchPtr b = next_slab()) return b;
            return nullptr;
        } catch (...) {
            done_ = true;                   // the stream ends at its first error; the reader stops when the stream is released
            throw;
        }
    }

private:
    // ---- the reader thread's side: no device call except the allocation of its pinned buffers -----------------------------
    struct HostSlab {
        uint8_t* p = nullptr;
        int64_t n = 0, offset = 0;
        bool last = false, full = false;
        std::string error;
    };

    void reader_main() {
        (void)hipSetDevice(ex_.ctx->device());      // pinned allocations belong to this device's context
        for (int64_t k = 0;; ++k) {
            HostSlab& h = ring_[k % RING];
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return stop_ || !h.full; });
                if (stop_) return;
            }
            if (!h.p) h.p = static_cast<uint8_t*>(pinned_host_alloc((size_t)slot_bytes_));
            const int64_t off = k * slot_bytes_;
            int64_t got = 0;
            std::string error;
            if (!h.p) error = "Ballista Error: no host memory for a slab of " + file_;
            while (error.empty() && got < slot_bytes_) {
                const ssize_t r = pread(fd_, h.p + got, (size_t)(slot_bytes_ - got), (off_t)(off + got));
                if (r < 0 && errno == EINTR) continue;
                if (r < 0) { error = "Ballista Error: cannot read " + file_ + ": " + strerror(errno); break; }
                if (r == 0) break;
                got += r;
            }
            const bool last = got < slot_bytes_ || off + got >= file_bytes_;
            {
                std::lock_guard<std::mutex> g(mu_);
                h.n = got;
                h.offset = off;
                h.last = last;
                h.error = error;
                h.full = true;
            }
            cv_.notify_all();
            if (last || !error.empty()) return;
        }
    }

    // ---- the consumer's side ---------------------------------------------------------------------------------------------
    void open() {
        fd_ = ::open(file_.c_str(), O_RDONLY | O_CLOEXEC);
        if (fd_ < 0) fail(BHIP_EEXEC, "Ballista Error: cannot open " + file_);
        struct stat st;
        if (fstat(fd_, &st) != 0 || !S_ISREG(st.st_mode)) fail(BHIP_EEXEC, "Ballista Error: cannot read " + file_);
        file_bytes_ = (int64_t)st.st_size;
        std::vector<bhip_column_desc> fields(cfg_->file_schema->fields.size());
        for (size_t i = 0; i < fields.size(); ++i) {
            memset(&fields[i], 0, sizeof(fields[i]));
            fields[i].name = cfg_->file_schema->fields[i].name.c_str();
            fields[i].dtype = cfg_->file_schema->fields[i].dtype;
            fields[i].nullable = cfg_->file_schema->fields[i].nullable;
        }
        const std::vector<int32_t> proj(cfg_->proj.begin(), cfg_->proj.end());
        const int n_proj = cfg_->has_proj ? (int)proj.size() : 0;
        const int32_t* projection = cfg_->has_proj ? proj.data() : nullptr;
        spec_ = make_text_spec(cfg_->format, (int)fields.size(), fields.data(), n_proj, projection,
                               bhip_csv_opts{cfg_->delimiter, cfg_->has_header ? 1 : 0});
        // a file that fits one slab needs one buffer of its own size (+ 1: the read that tells the end) and no room for a carry
        const bool one_slab = file_bytes_ < cfg_->slab_bytes;
        slot_bytes_ = one_slab ? align_up(file_bytes_ + 1, 4096) : cfg_->slab_bytes;
        carry_room_ = one_slab ? 0 : std::min<int64_t>(cfg_->slab_bytes, CARRY_ROOM);
        HIP_CHECK(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) HIP_CHECK(hipEventCreateWithFlags(&copied_[i], hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&exec_point_, hipEventDisableTiming));
        header_pending_ = cfg_->has_header;
        open_ = true;
        reader_ = std::thread([this] { reader_main(); });
    }

    uint8_t* landing(int64_t k) {           // A of slab k's device buffer
        BufferPtr& b = dev_[k & 1];
        if (!b) b = make_buffer(ex_, (size_t)(carry_room_ + slot_bytes_ + 256 + 64));
        return reinterpret_cast<uint8_t*>(align_up((int64_t)reinterpret_cast<uintptr_t>(b->ptr()), 256)) + carry_room_;
    }

    // queue the host-to-device copy of slab k once the reader has it; wait = false: only if it is there already
    bool queue_copy(int64_t k, bool wait) {
        if (k < copies_queued_) return true;
        HostSlab& h = ring_[k % RING];
        {
            std::unique_lock<std::mutex> g(mu_);
            if (!wait && !h.full) return false;
            cv_.wait(g, [&] { return h.full; });
        }
        if (!h.error.empty()) fail(BHIP_EEXEC, h.error);
        uint8_t* a = landing(k);
        // what the task's stream still has queued on this buffer (the allocator's hand-over, the move of a carry out of it) first
        HIP_CHECK(hipEventRecord(exec_point_, ex_.stream));
        HIP_CHECK(hipStreamWaitEvent(copy_stream_, exec_point_, 0));
        if (h.n) HIP_CHECK(hipMemcpyAsync(a, h.p, (size_t)h.n, hipMemcpyHostToDevice, copy_stream_));
        HIP_CHECK(hipEventRecord(copied_[k & 1], copy_stream_));
        copies_queued_ = k + 1;
        return true;
    }

    // slab k_: the batch of the records that end in it, or null when none does (the whole slab then waits as carry)
    BatchPtr next_slab() {
        const int64_t k = k_;
        queue_copy(k, true);
        HostSlab& h = ring_[k % RING];
        const bool last = h.last;
        const int64_t n_new = h.n;
        if (!last) queue_copy(k + 1, false);                    // crosses PCIe while slab k is parsed
        HIP_CHECK(hipStreamWaitEvent(ex_.stream, copied_[k & 1], 0));

        uint8_t* a = landing(k);
        const int64_t pad = align_up(carry_, 256), gap = pad - carry_;
        TextSlab slab;
        BufferPtr joined;
        if (!long_carry_) {
            slab.text = a - pad;                                // the carry already ends at A (moved there behind slab k - 1)
            if (gap) HIP_CHECK(hipMemsetAsync(a - pad, 0, (size_t)gap, ex_.stream));
        } else {                                                // a carry that has no room in front of A
            joined = make_buffer(ex_, (size_t)(pad + n_new + 256 + 64));
            uint8_t* base = reinterpret_cast<uint8_t*>(align_up((int64_t)reinterpret_cast<uintptr_t>(joined->ptr()), 256));
            if (gap) HIP_CHECK(hipMemsetAsync(base, 0, (size_t)gap, ex_.stream));
            HIP_CHECK(hipMemcpyAsync(base + gap, long_carry_->ptr(), (size_t)carry_, hipMemcpyDeviceToDevice, ex_.stream));
            if (n_new) HIP_CHECK(hipMemcpyAsync(base + pad, a, (size_t)n_new, hipMemcpyDeviceToDevice, ex_.stream));
            slab.text = base;
        }
        const char* what = cfg_->format == BHIP_TEXT_TBL ? "tbl" : "csv";
        slab.n_bytes = pad + n_new;
        slab.first_record = gap;
        slab.last = last;
        slab.unterminated = n_new ? h.p[n_new - 1] != '\n' : carry_ > 0;        // a carry never ends with a record end
        slab.header_here = header_pending_;

        TextParsed parsed;
        try {
            if (slab.n_bytes > 0xFFFFFFF0ll) fail_record_too_long(what);       // 32-bit offsets in the kernels
            parsed = parse_text_slab(ex_, spec_, slab);
            // no record ends in the slab: all of it waits for the next one, as long as what waits is no more than one slab
            if (!parsed.batch && slab.n_bytes - parsed.cut > cfg_->slab_bytes) fail_record_too_long(what);
        } catch (const Error& e) {
            fail(e.code, file_ + ": " + e.what() + " (in the slab that starts at byte " + std::to_string(h.offset) + ")");
        }
        // the parse has waited for the copy: the reader may fill the host buffer again
        {
            std::lock_guard<std::mutex> g(mu_);
            h.full = false;
        }
        cv_.notify_all();
        if (parsed.batch) header_pending_ = false;
        if (last) {
            done_ = true;
        } else {
            const int64_t carry = slab.n_bytes - parsed.cut;
            BufferPtr moved;
            if (carry > carry_room_) {
                moved = make_buffer(ex_, (size_t)carry + 64);
                HIP_CHECK(hipMemcpyAsync(moved->ptr(), slab.text + parsed.cut, (size_t)carry, hipMemcpyDeviceToDevice, ex_.stream));
            } else if (carry) {
                HIP_CHECK(hipMemcpyAsync(landing(k + 1) - carry, slab.text + parsed.cut, (size_t)carry, hipMemcpyDeviceToDevice, ex_.stream));
            }
            long_carry_ = moved;
            carry_ = carry;
        }
        k_ = k + 1;
        return parsed.batch;
    }

    void close() noexcept {
        if (open_) {
            {
                std::lock_guard<std::mutex> g(mu_);
                stop_ = true;
            }
            cv_.notify_all();
            if (reader_.joinable()) reader_.join();
        }
        (void)hipSetDevice(ex_.ctx->device());
        if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);        // nothing may still read the ring or write the slabs
        if (open_) (void)hipStreamSynchronize(ex_.stream);
        for (auto& h : ring_)
            if (h.p) pinned_host_free(h.p, (size_t)slot_bytes_);
        for (hipEvent_t e : {copied_[0], copied_[1], exec_point_})
            if (e) (void)hipEventDestroy(e);
        if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
        if (fd_ >= 0) ::close(fd_);
        (void)hipGetLastError();
    }

    SchemaPtr schema_;
    std::shared_ptr<const TextScanConfig> cfg_;
    std::string file_;
    Exec ex_;
    TextScanSpec spec_;
    bool open_ = false, done_ = false;
    int fd_ = -1;
    int64_t file_bytes_ = 0, slot_bytes_ = 0, carry_room_ = 0;
    // reader <-> consumer
    std::mutex mu_;
    std::condition_variable cv_;
    bool stop_ = false;
    HostSlab ring_[RING];
    std::thread reader_;
    // device side
    hipStream_t copy_stream_ = nullptr;
    hipEvent_t copied_[2] = {nullptr, nullptr}, exec_point_ = nullptr;
    BufferPtr dev_[2], long_carry_;
    int64_t k_ = 0, copies_queued_ = 0, carry_ = 0;
    bool header_pending_ = false;
};

class EmptyStream : public RecordBatchStream {
public:
    explicit EmptyStream(SchemaPtr s) : schema_(std::move(s)) {}
    SchemaPtr schema() const override { return schema_; }
    BatchPtr next() override { return nullptr; }
private:
    SchemaPtr schema_;
};

class TextScanExec : public ExecutionPlan {
public:
    TextScanExec(ContextPtr ctx, std::string path, std::vector<std::string> files, std::shared_ptr<const TextScanConfig> cfg)
        : path_(std::move(path)), files_(std::move(files)), cfg_(std::move(cfg)) {
        ctx_ = std::move(ctx);
        if (!cfg_->has_proj) schema_ = cfg_->file_schema;
        else {
            auto o = std::make_shared<Schema>();
            for (uint32_t i : cfg_->proj) {
                if (i >= cfg_->file_schema->fields.size()) fail(BHIP_EINVAL, "scan projection index " + std::to_string(i) + " is out of range");
                o->fields.push_back(cfg_->file_schema->fields[i]);
            }
            schema_ = o;
        }
    }
    const char* name() const override { return "CsvExec"; }
    SchemaPtr schema() const override { return schema_; }
    Partitioning output_partitioning() const override { return Partitioning{BHIP_PART_UNKNOWN, (int)std::max<size_t>(1, files_.size()), {}}; }
    std::vector<PlanPtr> children() const override { return {}; }
    PlanPtr with_new_children(const std::vector<PlanPtr>& c) const override {
        if (!c.empty()) fail(BHIP_EINVAL, "CsvExec has no children");
        return shared_from_this();
    }
    std::string describe() const override {
        std::string s = "CsvExec: path=" + path_ + ", delimiter='" + std::string(1, (char)cfg_->delimiter) + "'";
        if (cfg_->format == BHIP_TEXT_CSV) s += std::string(", has_header=") + (cfg_->has_header ? "true" : "false");
        s += ", device scan, projection=[";
        for (size_t i = 0; i < schema_->fields.size(); ++i) s += (i ? ", " : "") + schema_->fields[i].name;
        // the reference's reader cuts batches by rows (batch_size); this one cuts by bytes of text
        return s + "], files=" + std::to_string(files_.size()) + ", one batch per slab of " + std::to_string(cfg_->slab_bytes) +
               " bytes (batch_size is not used)";
    }
    StreamPtr execute(int partition, const Exec& ex) const override {
        check_partition(*this, partition);
        if (files_.empty()) return StreamPtr(new EmptyStream(schema_));
        return StreamPtr(new TextScanStream(schema_, cfg_, files_[partition], ex));
    }
private:
    std::string path_;
    std::vector<std::string> files_;
    std::shared_ptr<const TextScanConfig> cfg_;
    SchemaPtr schema_;
};

}  // namespace

PlanPtr make_text_scan_exec(const ContextPtr& ctx, std::string path, std::vector<std::string> files, SchemaPtr file_schema,
                            std::vector<uint32_t> projection, bool has_projection, int format, uint8_t delimiter, bool has_header,
                            int64_t slab_bytes) {
    if (format != BHIP_TEXT_TBL && format != BHIP_TEXT_CSV) fail(BHIP_EINVAL, "text scan format must be BHIP_TEXT_TBL or BHIP_TEXT_CSV");
    auto cfg = std::make_shared<TextScanConfig>();
    cfg->format = format;
    cfg->delimiter = format == BHIP_TEXT_TBL ? (uint8_t)'|' : delimiter;
    cfg->has_header = format == BHIP_TEXT_CSV && has_header;
    check_csv_delimiter(cfg->delimiter);
    cfg->slab_bytes = resolve_slab_bytes(slab_bytes);
    if (!file_schema) fail(BHIP_EINVAL, "text scan without a schema");
    cfg->file_schema = std::move(file_schema);
    cfg->proj = std::move(projection);
    cfg->has_proj = has_projection;
    return std::make_shared<TextScanExec>(ctx, std::move(path), std::move(files), cfg);
}

}  // namespace bhip
