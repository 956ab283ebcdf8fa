// scalar_text_check.cpp — stand-alone check of ballista_amd/csrc/str_text.h and of date_part in temporal_text.h on the CPU
// (tests/test_string_fns_cpu.py builds it with -fsanitize=address,undefined and compares every line with the Python restatement,
// tests/string_fn_cases.py).
//
//   scalar_text_check <cases file>
// One case per line, fields separated by TABs:
//   substr <s> <start> [<count>]     left <s> <n>     right <s> <n>     char_length <s>     strpos <s> <sub>     starts_with <s> <prefix>
//   date_part <type>/<part> <integer>          <type> is d32, d64, s, ms, us or ns
// One answer per line: the string; the integer in decimal; true / false; "negative substring length not allowed" for a substr with
// count < 0; NULL for a date_part that does not fit Int32; UNKNOWN for a part that is none of the nine.  Every string is copied
// into a heap block of exactly its length, so that a read past either end of a value is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "str_text.h"
#include "temporal_text.h"

using namespace bhip;

struct Block {
    uint8_t* p;
    int64_t n;
    explicit Block(const std::string& s) : p(static_cast<uint8_t*>(malloc(s.size() ? s.size() : 1))), n((int64_t)s.size()) { memcpy(p, s.data(), s.size()); }
    ~Block() { free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
};

static int type_of(const std::string& u) {
    return u == "d32" ? DT_DATE32 : u == "d64" ? DT_DATE64 : u == "s" ? DT_TIMESTAMP_S : u == "ms" ? DT_TIMESTAMP_MS : u == "us" ? DT_TIMESTAMP_US
         : u == "ns" ? DT_TIMESTAMP_NS : 0;
}

static int64_t integer(const std::string& s) { return (int64_t)strtoll(s.c_str(), nullptr, 10); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: scalar_text_check <cases file>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        for (size_t a = 0;;) {
            const size_t t = line.find('\t', a);
            f.push_back(line.substr(a, t == std::string::npos ? t : t - a));
            if (t == std::string::npos) break;
            a = t + 1;
        }
        const std::string& op = f[0];
        const int range_fn = op == "substr" ? STR_SUBSTR : op == "left" ? STR_LEFT : op == "right" ? STR_RIGHT : -1;
        if (range_fn >= 0 && (f.size() == 3 || (f.size() == 4 && range_fn == STR_SUBSTR))) {
            const Block s(f[1]);
            int64_t b = 0, e = 0;
            if (!str_range(range_fn, CastPtrReader{s.p}, 0, s.n, integer(f[2]), f.size() == 4, f.size() == 4 ? integer(f[3]) : 0, b, e)) {
                puts("negative substring length not allowed");
                continue;
            }
            if (b < 0 || e < b || e > s.n) { fprintf(stderr, "range [%lld, %lld) outside the value: %s\n", (long long)b, (long long)e, line.c_str()); return 3; }
            fwrite(s.p + b, 1, (size_t)(e - b), stdout);
            putchar('\n');
        } else if (op == "char_length" && f.size() == 2) {
            const Block s(f[1]);
            printf("%lld\n", (long long)str_char_count(CastPtrReader{s.p}, 0, s.n));
        } else if ((op == "strpos" || op == "starts_with") && f.size() == 3) {
            const Block s(f[1]), sub(f[2]);
            if (op == "strpos") printf("%d\n", (int)str_strpos(CastPtrReader{s.p}, 0, s.n, CastPtrReader{sub.p}, 0, sub.n));
            else puts(str_starts_with(CastPtrReader{s.p}, 0, s.n, CastPtrReader{sub.p}, 0, sub.n) ? "true" : "false");
        } else if (op == "date_part" && f.size() == 3) {
            const size_t slash = f[1].find('/');
            const int t = type_of(f[1].substr(0, slash));
            if (slash == std::string::npos || t == 0) { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
            const std::string pname = f[1].substr(slash + 1);
            char* ptext = static_cast<char*>(malloc(pname.size() ? pname.size() : 1));
            memcpy(ptext, pname.data(), pname.size());
            const int part = date_part_name(ptext, (int64_t)pname.size());
            free(ptext);
            if (part < 0) { puts("UNKNOWN"); continue; }
            int64_t v = integer(f[2]);
            if (t == DT_DATE32) v = (int64_t)(int32_t)v;             // what a kernel loads from a Date32 column
            int32_t out = 0;
            if (temporal_part(t, part, v, out)) printf("%d\n", (int)out);
            else puts("NULL");
        } else {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
