// temporal_text_check.cpp — stand-alone check of ballista_amd/csrc/temporal_text.h on the CPU (tests/test_temporal_fns_cpu.py builds
// it with -fsanitize=address,undefined and compares every line with the Python restatement, tests/temporal_cases.py).
//
//   temporal_text_check <cases file>
// One case per line, fields separated by TABs:  P - <text>                       to_timestamp(<text>)
//                                               D <unit>/<granularity> <integer>  date_trunc(<granularity>, <integer of that unit>)
// <unit> is s, ms, us or ns.  One answer per line: the int64 in decimal; INVALID for a text outside the grammar; NULL for a floor
// that does not fit int64; UNKNOWN for a granularity that is none of the seven.  The text is copied into a heap block of exactly
// its length, so that a read past either end of a value is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "temporal_text.h"

using namespace bhip;

static int unit_of(const std::string& u) {
    return u == "s" ? DT_TIMESTAMP_S : u == "ms" ? DT_TIMESTAMP_MS : u == "us" ? DT_TIMESTAMP_US : u == "ns" ? DT_TIMESTAMP_NS : 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: temporal_text_check <cases file>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        if (t2 == std::string::npos) { fprintf(stderr, "malformed line: %s\n", line.c_str()); return 2; }
        const std::string dir = line.substr(0, t1), what = line.substr(t1 + 1, t2 - t1 - 1), arg = line.substr(t2 + 1);
        if (dir == "P") {
            uint8_t* block = static_cast<uint8_t*>(malloc(arg.size() ? arg.size() : 1));
            memcpy(block, arg.data(), arg.size());
            int64_t ns = 0;
            const bool ok = to_timestamp_parse(CastPtrReader{block}, 0, (int64_t)arg.size(), ns);
            free(block);
            if (ok) printf("%lld\n", (long long)ns);
            else puts("INVALID");
        } else if (dir == "D") {
            const size_t slash = what.find('/');
            const int unit = unit_of(what.substr(0, slash));
            if (slash == std::string::npos || unit == 0) { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
            const std::string gname = what.substr(slash + 1);
            char* gtext = static_cast<char*>(malloc(gname.size() ? gname.size() : 1));
            memcpy(gtext, gname.data(), gname.size());
            const int g = trunc_granularity(gtext, (int64_t)gname.size());
            free(gtext);
            if (g < 0) { puts("UNKNOWN"); continue; }
            int64_t out = 0;
            if (temporal_trunc(unit, g, (int64_t)strtoll(arg.c_str(), nullptr, 10), out)) printf("%lld\n", (long long)out);
            else puts("NULL");
        } else {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
