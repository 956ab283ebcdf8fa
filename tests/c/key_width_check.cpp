// key_width_check.cpp — "the keys do not fit the 16-byte packed key" is a TYPE (KeyWidthError, host/core.hpp), raised by exactly
// three places, and nothing else that is not implemented is one.  Under AddressSanitizer + UndefinedBehaviorSanitizer, no GPU, no
// HIP call.
//
// Built by `make -C ballista_amd/csrc key-width-check` from the same sanitizer objects as host_fuzz and run by
// tests/test_key_width_cpu.py.  Every case prints one line `ok <case>`; the first that does not hold prints why and exits with 1.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "plan.hpp"

using namespace bhip;

namespace {

enum Kind { NOTHING, KEY_WIDTH, PLAIN };

// what `f` throws: a KeyWidthError, an Error that is none, or nothing — with the code and the text it must carry
void expect(const char* name, Kind want, bhip_status code, const std::string& text, const std::function<void()>& f) {
    Kind got = NOTHING;
    bhip_status got_code = BHIP_OK;
    std::string got_text;
    try {
        f();
    } catch (const Error& e) {                              // (by reference, as every handler of the library: the type survives)
        got = dynamic_cast<const KeyWidthError*>(&e) ? KEY_WIDTH : PLAIN;
        got_code = e.code;
        got_text = e.what();
    }
    if (got != want || got_code != code || got_text != text) {
        fprintf(stderr, "key_width_check: %s: kind %d code %d \"%s\", expected kind %d code %d \"%s\"\n", name, (int)got, (int)got_code,
                got_text.c_str(), (int)want, (int)code, text.c_str());
        exit(1);
    }
    printf("ok %s\n", name);
}

Schema columns(int n, int dtype) {
    Schema s;
    for (int i = 0; i < n; ++i) s.fields.push_back(Field{"c" + std::to_string(i), dtype, false});
    return s;
}

void pack_keys(const Schema& s, int n_keys) {
    ProgramBuilder pb(s);
    for (int i = 0; i < n_keys; ++i) pb.add_key(make_column(s.fields[i].name));
    ScanParams P;
    pb.finish(P);
}

}  // namespace

int main() {
    const std::string parts = "more than 8 key columns", layout = "key columns do not fit the 16-byte packed key",
                      value = "a Utf8 key value is longer than the packed-key path supports";
    // 1. the number of key parts
    const Schema i32 = columns(9, DT_INT32);
    expect("eight_int32_keys", NOTHING, BHIP_OK, "", [&] {                      // (8 x 4 bytes: the count is fine, the layout is not)
        ProgramBuilder pb(i32);
        for (int i = 0; i < 8; ++i) pb.add_key(make_column(i32.fields[i].name));
    });
    expect("nine_int32_keys", KEY_WIDTH, BHIP_ENOTIMPL, parts, [&] { pack_keys(i32, 9); });
    // 2. the layout, at finish
    const Schema i64 = columns(3, DT_INT64);
    expect("two_int64_keys", NOTHING, BHIP_OK, "", [&] { pack_keys(i64, 2); });
    expect("three_int64_keys_before_finish", NOTHING, BHIP_OK, "", [&] {
        ProgramBuilder pb(i64);
        for (int i = 0; i < 3; ++i) pb.add_key(make_column(i64.fields[i].name));
    });
    expect("three_int64_keys", KEY_WIDTH, BHIP_ENOTIMPL, layout, [&] { pack_keys(i64, 3); });
    // 3. another plan the VM does not run: the same code, not the same type
    const Schema six = columns(6, DT_INT64);
    expect("seventeen_accumulators", PLAIN, BHIP_ENOTIMPL, "more than 16 distinct accumulators", [&] {
        ProgramBuilder pb(six);
        const int kinds[3] = {ACC_SUM_I64, ACC_MIN_I64, ACC_MAX_I64};
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 6; ++c) pb.add_acc(kinds[k], pb.compile(make_column(six.fields[c].name)));
    });
    // 4. the run-time flags
    auto flags = [](uint32_t f) {
        ScanStatus st{};
        st.flags = f;
        check_scan_flags(st);
    };
    expect("no_flag", NOTHING, BHIP_OK, "", [&] { flags(0); });
    expect("divide_by_zero", PLAIN, BHIP_EEXEC, "Arrow error: Divide by zero error", [&] { flags(SCAN_ERR_DIV_ZERO); });
    expect("key_too_long", KEY_WIDTH, BHIP_ENOTIMPL, value, [&] { flags(SCAN_ERR_KEY_TOO_LONG); });
    expect("both_flags", PLAIN, BHIP_EEXEC, "Arrow error: Divide by zero error", [&] { flags(SCAN_ERR_DIV_ZERO | SCAN_ERR_KEY_TOO_LONG); });
    return 0;
}
