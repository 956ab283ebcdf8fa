// parquet_decode_check.cpp — the host half of ParquetExec (parquet_host.cpp) finished in plain sequential C++ and printed, under
// AddressSanitizer + UndefinedBehaviorSanitizer, no GPU.
//
// Built by `make -C ballista_amd/csrc parquet-check` from the same sanitizer objects as host_fuzz and run by
// tests/test_parquet_decode_cpu.py, which compares the whole output with pyarrow's read of the same files.  For every row group
// and supported column the program calls read_chunk_bytes + parse_chunk, then does what the device half does with a HostChunk —
// but written independently of the kernels: the run table is walked in order (no binary search, one bit at a time, no byte
// window), NULLs are re-inserted by walking the validity bits (no prefix table), dictionary values are gathered by index, pages
// are appended.  Both forms of a HostChunk are read: the staged one (STAGED_FIXED / STAGED_DICT) and, with
// BHIP_PARQUET_PER_PAGE=1 in the environment, the page list.
//
//   parquet_decode_check <file.parquet>...
//     # <file> group <g> column <name> rows <n>      then one value per line:
//     NULL | decimal integer | hex bit pattern of a float | hex bytes of a string | 0 / 1
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "parquet_host.hpp"

using namespace bhip;
using namespace bhip::pq;

namespace {

[[noreturn]] void die(const std::string& m) {
    fprintf(stderr, "parquet_decode_check: %s\n", m.c_str());
    exit(1);
}

// the indices of a run table, in order; every run must start where the one before it ended
template <class Runs>
std::vector<uint32_t> expand(const Runs& runs, const uint8_t* bytes, size_t n_bytes, int64_t n) {
    std::vector<uint32_t> out;
    for (const PqRun& r : runs) {
        if (r.out_start != out.size()) die("run table out of order");
        for (uint32_t k = 0; k < r.count; ++k) {
            uint32_t v = 0;
            if (!r.packed) v = r.value;
            else
                for (uint32_t b = 0; b < r.packed; ++b) {
                    const uint64_t bit = (uint64_t)k * r.packed + b;
                    const size_t at = (size_t)r.value + (size_t)(bit >> 3);
                    if (at >= n_bytes) die("bit-packed run past its bytes");
                    v |= (uint32_t)((bytes[at] >> (bit & 7)) & 1u) << b;
                }
            out.push_back(v);
        }
    }
    if ((int64_t)out.size() != n) die("run table holds " + std::to_string(out.size()) + " values, expected " + std::to_string(n));
    return out;
}

struct Printer {
    const PqColumn& pc;
    const HostDict& dict;
    size_t width;
    void null() const { puts("NULL"); }
    void fixed(const uint8_t* p) const {
        uint64_t raw = 0;
        memcpy(&raw, p, width);
        switch (pc.out_dtype) {
            case DT_FLOAT32: printf("%08" PRIx32 "\n", (uint32_t)raw); break;
            case DT_FLOAT64: printf("%016" PRIx64 "\n", raw); break;
            case DT_INT8: printf("%d\n", (int)(int8_t)raw); break;
            case DT_UINT8: printf("%u\n", (unsigned)(uint8_t)raw); break;
            case DT_INT16: printf("%d\n", (int)(int16_t)raw); break;
            case DT_UINT16: printf("%u\n", (unsigned)(uint16_t)raw); break;
            case DT_UINT32: printf("%" PRIu32 "\n", (uint32_t)raw); break;
            case DT_UINT64: printf("%" PRIu64 "\n", raw); break;
            default:
                if (width == 4) printf("%" PRId32 "\n", (int32_t)(uint32_t)raw);
                else printf("%" PRId64 "\n", (int64_t)raw);
        }
    }
    void bytes(const uint8_t* p, size_t n) const {
        for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
        putchar('\n');
    }
    void from_dict(uint32_t idx) const {
        if ((int64_t)idx >= dict.n) die("dictionary index " + std::to_string(idx) + " of " + std::to_string(dict.n));
        if (pc.phys == PQ_BYTE_ARRAY) bytes(dict.bytes.data() + dict.offsets[idx], (size_t)(dict.offsets[idx + 1] - dict.offsets[idx]));
        else fixed(dict.bytes.data() + width * idx);
    }
};

void print_chunk(const PqColumn& pc, const HostChunk& hc) {
    const size_t width = (pc.phys == PQ_INT32 || pc.phys == PQ_FLOAT) ? 4 : (pc.phys == PQ_INT64 || pc.phys == PQ_DOUBLE) ? 8 : 0;
    const Printer pr{pc, hc.dict, width};
    if (hc.staged == STAGED_FIXED) {
        if (hc.staged_bytes.size() != width * (size_t)hc.rows) die("staged values do not cover the chunk");
        for (int64_t i = 0; i < hc.rows; ++i) pr.fixed(hc.staged_bytes.data() + width * (size_t)i);
        return;
    }
    if (hc.staged == STAGED_DICT) {
        for (uint32_t idx : expand(hc.staged_runs, hc.staged_bytes.data(), hc.staged_bytes.size(), hc.rows)) pr.from_dict(idx);
        return;
    }
    int64_t rows = 0;
    for (const HostPage& pg : hc.pages) {
        if (pg.has_nulls && pc.repetition != 1) die("a required column with NULLs");
        std::vector<uint32_t> idx;
        if (pg.kind == PG_DICT) idx = expand(pg.runs, pg.bytes.data(), pg.bytes.size(), pg.n_valid);
        int64_t k = 0;                                       // valid values seen so far
        for (int64_t i = 0; i < pg.n; ++i) {
            const bool valid = !pg.has_nulls || ((pg.validity[(size_t)(i >> 3)] >> (i & 7)) & 1);
            if (pg.kind == PG_STRINGS) {
                const int32_t a = pg.offsets[(size_t)i], b = pg.offsets[(size_t)i + 1];
                if (a > b || (size_t)b > pg.bytes.size() || (!valid && a != b)) die("string offsets of a page");
                if (valid) pr.bytes(pg.bytes.data() + a, (size_t)(b - a));
            } else if (pg.kind == PG_BOOL) {
                const int bit = (pg.bytes[(size_t)(i >> 3)] >> (i & 7)) & 1;
                if (!valid && bit) die("a NULL Boolean row with its bit set");
                if (valid) printf("%d\n", bit);
            } else if (valid) {
                if (pg.kind == PG_DICT) pr.from_dict(idx[(size_t)k]);
                else {
                    if (width * (size_t)(k + 1) > pg.bytes.size()) die("PLAIN page shorter than its valid values");
                    pr.fixed(pg.bytes.data() + width * (size_t)k);
                }
            }
            if (valid) ++k;
            else pr.null();
        }
        if (k != pg.n_valid) die("validity bits and n_valid disagree");
        if (pg.has_nulls) {
            // what the device half indexes by word: the prefix table covers every word and ends at n_valid; no bit behind the page's rows
            if (pg.prefix.size() != (size_t)((pg.n + 63) / 64) + 1 || pg.prefix.back() != (uint32_t)pg.n_valid) die("prefix table of a page");
            for (int64_t i = pg.n; i < (int64_t)pg.validity.size() * 8; ++i)
                if ((pg.validity[(size_t)(i >> 3)] >> (i & 7)) & 1) die("validity bit behind the last row of a page");
        }
        rows += pg.n;
    }
    if (rows != hc.rows) die("pages do not add up to the chunk's rows");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: parquet_decode_check <file.parquet>...\n"); return 2; }
    try {
        for (int a = 1; a < argc; ++a) {
            const std::string path = argv[a];
            const std::string base = path.substr(path.find_last_of('/') + 1);
            const PqFile F = read_footer(path);
            for (size_t g = 0; g < F.groups.size(); ++g) {
                const PqRowGroup& grp = F.groups[g];
                if (grp.num_rows == 0) continue;
                for (size_t ci = 0; ci < F.cols.size(); ++ci) {
                    const PqColumn& pc = F.cols[ci];
                    if (!pc.dtype) continue;
                    if (ci >= grp.cols.size()) die("row group without column " + pc.name);
                    const std::vector<uint8_t> raw = read_chunk_bytes(F, grp.cols[ci], pc.name);
                    const HostChunk hc = parse_chunk(raw.data(), raw.size(), pc, grp.cols[ci], grp.num_rows);
                    if (hc.rows != grp.num_rows) die("chunk of " + pc.name + " does not hold its row group's rows");
                    printf("# %s group %zu column %s rows %" PRId64 "\n", base.c_str(), g, pc.name.c_str(), grp.num_rows);
                    print_chunk(pc, hc);
                }
            }
        }
    } catch (const Error& e) {
        die(e.what());
    }
    return 0;
}
