// cast_text_check.cpp — stand-alone check of ballista_amd/csrc/cast_text.h on the CPU (tests/test_cast_text_cpu.py builds it with
// -fsanitize=address,undefined and compares every line with the Python restatement of the cast table, tests/cast_text_cases.py).
//
//   cast_text_check <cases file>
// One case per line, fields separated by TABs:  P <type> <string>   CAST(<string> AS <type>)
//                                               F <type> <integer>  CAST(<integer of that type> AS Utf8)
// One answer per line: NULL, DECLINED, or the value — integers and Date32 days in decimal, Boolean as true / false, floats as the
// hex bit pattern; for F the text itself.  The string is copied into a heap block of exactly its length, so that a read past either
// end of a value is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "cast_text.h"

using namespace bhip;

static int dtype_of(const std::string& t) {
    static const struct { const char* n; int d; } names[] = {
        {"Int8", DT_INT8}, {"Int16", DT_INT16}, {"Int32", DT_INT32}, {"Int64", DT_INT64}, {"UInt8", DT_UINT8}, {"UInt16", DT_UINT16},
        {"UInt32", DT_UINT32}, {"UInt64", DT_UINT64}, {"Boolean", DT_BOOLEAN}, {"Date32", DT_DATE32}, {"Float64", DT_FLOAT64},
        {"Float32", DT_FLOAT32}};
    for (auto& e : names)
        if (t == e.n) return e.d;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: cast_text_check <cases file>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        if (t2 == std::string::npos) { fprintf(stderr, "malformed line: %s\n", line.c_str()); return 2; }
        const std::string dir = line.substr(0, t1), type = line.substr(t1 + 1, t2 - t1 - 1), arg = line.substr(t2 + 1);
        const int dt = dtype_of(type);
        if (dir == "P" && cast_parse_supported(dt)) {
            uint8_t* block = static_cast<uint8_t*>(malloc(arg.size() ? arg.size() : 1));
            memcpy(block, arg.data(), arg.size());
            uint64_t bits = 0;
            const int r = cast_parse(CastPtrReader{block}, 0, (int64_t)arg.size(), dt, bits);
            free(block);
            if (r == CAST_IS_NULL) puts("NULL");
            else if (r == CAST_DECLINED) puts("DECLINED");
            else if (dt == DT_FLOAT64) printf("0x%016llx\n", (unsigned long long)bits);
            else if (dt == DT_FLOAT32) printf("0x%08x\n", (unsigned)bits);
            else if (dt == DT_BOOLEAN) puts(bits ? "true" : "false");
            else if (dt == DT_UINT64) printf("%llu\n", (unsigned long long)bits);
            else printf("%lld\n", (long long)bits);
        } else if (dir == "F" && cast_format_supported(dt)) {
            const uint64_t v = dt == DT_UINT64 ? strtoull(arg.c_str(), nullptr, 10) : (uint64_t)strtoll(arg.c_str(), nullptr, 10);
            uint8_t* text = static_cast<uint8_t*>(malloc(CAST_TEXT_MAX));
            const int len = cast_format(dt, v, text);
            if (len < 0) puts("NULL");
            else if (len != cast_format(dt, v, nullptr) || len > cast_format_max(dt)) puts("LENGTH MISMATCH");
            else printf("%.*s\n", len, reinterpret_cast<const char*>(text));
            free(text);
        } else {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
