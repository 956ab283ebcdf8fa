// cast_text.h — CAST between Utf8 and the fixed-width types: the value grammar, written once (DESIGN.md §3.2 has the table).
//
// Plain host / device inline functions, no HIP call: the cast kernels (kernels_cast.hip), the host-side folding of literals
// (host/expr.cpp, host/utf8_exprs.cpp) and the stand-alone check program (tests/c/cast_text_check.cpp) all run THIS code, so a
// literal, a column and the test cannot disagree.
//
// The rule is arrow's cast kernel: a value the target cannot hold is NULL, never an error; nothing is trimmed; the whole
// string must match.  One case is neither a value nor a NULL: a float string outside the exactly rounded path is DECLINED, and the
// caller fails the batch with BHIP_ENOTIMPL (never a mis-rounded value).
#pragma once
#include <stdint.h>
#include "vm_isa.h"

namespace bhip {

enum CastResult : int { CAST_VALUE = 0, CAST_IS_NULL = 1, CAST_DECLINED = 2 };

// byte source over memory the caller holds (the kernels read HBM through it: a "global reader" in the sense of text_device.h)
struct CastPtrReader {
    const uint8_t* text;
    BHIP_HD uint8_t operator()(int64_t pos) const { return text[pos]; }
};

BHIP_HD inline int64_t days_from_civil(int64_t y, unsigned m, unsigned d) {
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const unsigned yoe = (unsigned)(y - era * 400);
    const unsigned doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const unsigned doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + (int64_t)doe - 719468;
}

// the inverse (proleptic Gregorian), for any day count of a Date32
BHIP_HD inline void civil_from_days(int64_t z, int64_t& y, unsigned& m, unsigned& d) {
    z += 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const unsigned doe = (unsigned)(z - era * 146097);
    const unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const unsigned mp = (5 * doy + 2) / 153;
    d = doy - (153 * mp + 2) / 5 + 1;
    m = mp < 10 ? mp + 3 : mp - 9;
    y = (int64_t)yoe + era * 400 + (m <= 2 ? 1 : 0);
}

constexpr int64_t CAST_DATE_MIN = -719528;      // 0000-01-01
constexpr int64_t CAST_DATE_MAX = 2932896;      // 9999-12-31

BHIP_HD inline bool cast_is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
BHIP_HD inline uint8_t cast_lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32) : c; }

// the types a Utf8 value can be cast to / a value can be written as text from
BHIP_HD inline bool cast_parse_supported(int to) { return (dt_is_integer(to) && (!dt_is_temporal(to) || to == DT_DATE32)) || to == DT_BOOLEAN || dt_is_float(to); }
BHIP_HD inline bool cast_format_supported(int from) { return (dt_is_integer(from) && (!dt_is_temporal(from) || from == DT_DATE32)) || from == DT_BOOLEAN; }

// ---- Utf8 -> integer: [+-]?[0-9]+ (no '-' for an unsigned target), leading zeros and any length allowed, NULL outside the range ----
template <class Reader>
BHIP_HD inline int cast_parse_integer(const Reader& rd, int64_t pos, int64_t end, int to, uint64_t& out) {
    out = 0;
    if (pos >= end) return CAST_IS_NULL;
    bool neg = false;
    const uint8_t c0 = rd(pos);
    if (c0 == '+' || c0 == '-') {
        neg = c0 == '-';
        ++pos;
        if (neg && dt_is_unsigned(to)) return CAST_IS_NULL;
    }
    if (pos >= end) return CAST_IS_NULL;
    uint64_t mag = 0;
    bool over = false;
    for (; pos < end; ++pos) {
        const uint8_t c = rd(pos);
        if (!cast_is_digit(c)) return CAST_IS_NULL;
        const uint64_t d = (uint64_t)(c - '0');
        if (mag > (0xFFFFFFFFFFFFFFFFull - d) / 10) over = true;        // (keep walking: a later non-digit is NULL as well)
        else mag = mag * 10 + d;
    }
    if (over) return CAST_IS_NULL;
    if (to == DT_UINT64) { out = mag; return CAST_VALUE; }
    int64_t lo, hi;
    dt_int_range(to, lo, hi);
    if (neg) {
        if (mag > (uint64_t)0 - (uint64_t)lo) return CAST_IS_NULL;
        out = (uint64_t)0 - mag;
    } else {
        if (mag > (uint64_t)hi) return CAST_IS_NULL;
        out = mag;
    }
    return CAST_VALUE;
}

// ---- Utf8 -> Boolean: true t yes y on 1 / false f no n off 0, ASCII case-insensitive ----------------------------------------
template <class Reader>
BHIP_HD inline int cast_parse_boolean(const Reader& rd, int64_t pos, int64_t end, uint64_t& out) {
    out = 0;
    const int64_t len = end - pos;
    if (len < 1 || len > 5) return CAST_IS_NULL;
    uint8_t w[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < (int)len; ++k) w[k] = cast_lower(rd(pos + k));
    auto is = [&](const char* s, int n) {
        if (len != n) return false;
        for (int k = 0; k < n; ++k)
            if (w[k] != (uint8_t)s[k]) return false;
        return true;
    };
    if (is("true", 4) || is("t", 1) || is("yes", 3) || is("y", 1) || is("on", 2) || is("1", 1)) { out = 1; return CAST_VALUE; }
    if (is("false", 5) || is("f", 1) || is("no", 2) || is("n", 1) || is("off", 3) || is("0", 1)) { out = 0; return CAST_VALUE; }
    return CAST_IS_NULL;
}

// ---- Utf8 -> Date32: exactly YYYY-MM-DD, a day that exists -------------------------------------------------------------------
template <class Reader>
BHIP_HD inline int cast_parse_date32(const Reader& rd, int64_t pos, int64_t end, uint64_t& out) {
    out = 0;
    if (end - pos != 10) return CAST_IS_NULL;
    unsigned v[10];
    for (int k = 0; k < 10; ++k) {
        const uint8_t c = rd(pos + k);
        if (k == 4 || k == 7) { if (c != '-') return CAST_IS_NULL; v[k] = 0; }
        else { if (!cast_is_digit(c)) return CAST_IS_NULL; v[k] = (unsigned)(c - '0'); }
    }
    const unsigned y = v[0] * 1000 + v[1] * 100 + v[2] * 10 + v[3], m = v[5] * 10 + v[6], d = v[8] * 10 + v[9];
    if (m < 1 || m > 12 || d < 1) return CAST_IS_NULL;
    const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
    const unsigned dim = m == 2 ? (leap ? 29u : 28u) : ((m == 4 || m == 6 || m == 9 || m == 11) ? 30u : 31u);
    if (d > dim) return CAST_IS_NULL;
    out = (uint64_t)days_from_civil((int64_t)y, m, d);
    return CAST_VALUE;
}

BHIP_HD inline double cast_pow10(int k) {       // 10^k, 0 <= k <= 22: every one a double
    const double t[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                          1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return t[k];
}
BHIP_HD inline uint64_t cast_f64_bits(double d) { union { double d; uint64_t u; } x; x.d = d; return x.u; }
BHIP_HD inline double cast_bits_f64(uint64_t u) { union { double d; uint64_t u; } x; x.u = u; return x.d; }
BHIP_HD inline uint32_t cast_f32_bits(float f) { union { float f; uint32_t u; } x; x.f = f; return x.u; }
BHIP_HD inline float cast_bits_f32(uint32_t u) { union { float f; uint32_t u; } x; x.u = u; return x.f; }

// ---- Utf8 -> Float64 ----------------------------------------------------------------------------------------------------------
// [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?  or  [+-]?(inf|infinity|nan), ASCII case-insensitive.  Exact path only: with m the digit
// string (integer digits then fraction digits) stripped of leading and of z trailing zeros and e10 = exponent + z - fraction digits,
// m < 2^53 and -22 <= e10 <= 22 gives (double)m * 10^e10 or (double)m / 10^-e10: both operands are doubles, so the one operation
// rounds the true value correctly (Clinger's exact case; the build has -ffp-contract=off).  m == 0 is a signed zero.  Every other
// matching string is CAST_DECLINED.  out = the double's bits.
template <class Reader>
BHIP_HD inline int cast_parse_float64(const Reader& rd, int64_t pos, int64_t end, uint64_t& out) {
    out = 0;
    if (pos >= end) return CAST_IS_NULL;
    bool neg = false;
    const uint8_t c0 = rd(pos);
    if (c0 == '+' || c0 == '-') { neg = c0 == '-'; ++pos; }
    if (pos >= end) return CAST_IS_NULL;
    const uint64_t sign = neg ? 0x8000000000000000ull : 0ull;
    {
        const int64_t len = end - pos;
        const uint8_t f = cast_lower(rd(pos));
        if (f == 'i' || f == 'n') {
            if (len != 3 && len != 8) return CAST_IS_NULL;
            const char* word = f == 'n' ? "nan" : "infinity";
            if (f == 'n' && len != 3) return CAST_IS_NULL;
            for (int k = 0; k < (int)len; ++k)
                if (cast_lower(rd(pos + k)) != (uint8_t)word[k]) return CAST_IS_NULL;
            out = sign | (f == 'n' ? 0x7FF8000000000000ull : 0x7FF0000000000000ull);
            return CAST_VALUE;
        }
    }
    constexpr uint64_t LIMIT = 1ull << 53;
    uint64_t m = 0;                  // the significant digits so far, trailing zeros held back in `zeros`
    int64_t zeros = 0;               // zeros seen since the last non-zero digit (ignored while m == 0: leading zeros)
    bool big = false;                // m reached 2^53: not on the exact path whatever follows
    int64_t n_int = 0, n_frac = 0;
    bool in_frac = false;
    for (; pos < end; ++pos) {
        const uint8_t c = rd(pos);
        if (c == '.') {
            if (in_frac) return CAST_IS_NULL;
            in_frac = true;
            continue;
        }
        if (!cast_is_digit(c)) break;
        if (in_frac) ++n_frac; else ++n_int;
        if (c == '0') { if (m != 0) ++zeros; continue; }
        for (; zeros > 0 && !big; --zeros) { m *= 10; big = m >= LIMIT; }         // m < 2^53: m * 10 < 2^57
        zeros = 0;
        if (!big) { m = m * 10 + (uint64_t)(c - '0'); big = m >= LIMIT; }
    }
    if (n_int + n_frac == 0) return CAST_IS_NULL;
    int64_t exp10 = 0;
    if (pos < end) {
        const uint8_t c = rd(pos);
        if (c != 'e' && c != 'E') return CAST_IS_NULL;
        ++pos;
        bool eneg = false;
        if (pos < end && (rd(pos) == '+' || rd(pos) == '-')) { eneg = rd(pos) == '-'; ++pos; }
        if (pos >= end) return CAST_IS_NULL;
        for (; pos < end; ++pos) {
            const uint8_t d = rd(pos);
            if (!cast_is_digit(d)) return CAST_IS_NULL;
            if (exp10 < 1000000000ll) exp10 = exp10 * 10 + (d - '0');           // clamped: far outside [-22, 22] either way
        }
        if (eneg) exp10 = -exp10;
    }
    if (m == 0) { out = sign; return CAST_VALUE; }
    if (big) return CAST_DECLINED;
    const int64_t e10 = exp10 + zeros - n_frac;
    if (e10 < -22 || e10 > 22) return CAST_DECLINED;
    const double v = e10 >= 0 ? (double)m * cast_pow10((int)e10) : (double)m / cast_pow10((int)-e10);
    out = sign | cast_f64_bits(v);
    return CAST_VALUE;
}

// ---- Utf8 -> Float32: the Float64 result d, rounded to float --------------------------------------------------------------------
// d is within half a double-ulp of the true value t, and every midpoint of two adjacent floats is itself a double.  So when d is
// not such a midpoint, t lies strictly on d's side of every float midpoint (or d == t), and (float)d is the correctly rounded
// float of t.  Only when d IS a midpoint can t sit on either side of it: that case is declined.  (A d that is itself a float is
// the nearest float to t for the same reason.)  out = the float's bits.
template <class Reader>
BHIP_HD inline int cast_parse_float32(const Reader& rd, int64_t pos, int64_t end, uint64_t& out) {
    uint64_t bits;
    const int r = cast_parse_float64(rd, pos, end, bits);
    out = 0;
    if (r != CAST_VALUE) return r;
    const double d = cast_bits_f64(bits);
    if (d != d) { out = (bits >> 63) ? 0xFFC00000u : 0x7FC00000u; return CAST_VALUE; }
    const float f = (float)d;
    const uint32_t fb = cast_f32_bits(f);
    if ((double)f != d) {
        // |d| is within [1e-22, 9.1e37]: f is a normal float and so is its neighbour on d's side
        const double ad = d < 0 ? -d : d, af = f < 0 ? -(double)f : (double)f;
        const float g = cast_bits_f32(ad > af ? fb + 1 : fb - 1);
        if (((double)f + (double)g) * 0.5 == d) return CAST_DECLINED;
    }
    out = fb;
    return CAST_VALUE;
}

// any supported target; out: the value as the VM holds it except for floats (Float64: the double's bits, Float32: the float's bits)
template <class Reader>
BHIP_HD inline int cast_parse(const Reader& rd, int64_t pos, int64_t end, int to, uint64_t& out) {
    if (to == DT_BOOLEAN) return cast_parse_boolean(rd, pos, end, out);
    if (to == DT_DATE32) return cast_parse_date32(rd, pos, end, out);
    if (to == DT_FLOAT64) return cast_parse_float64(rd, pos, end, out);
    if (to == DT_FLOAT32) return cast_parse_float32(rd, pos, end, out);
    return cast_parse_integer(rd, pos, end, to, out);
}

// ---- fixed-width -> Utf8 ------------------------------------------------------------------------------------------------------
constexpr int CAST_TEXT_MAX = 20;       // "-9223372036854775808", "18446744073709551615"

// longest text of a value of the type
BHIP_HD inline int cast_format_max(int from) {
    switch (from) {
        case DT_BOOLEAN: return 1;
        case DT_UINT8: return 3;
        case DT_INT8: return 4;
        case DT_UINT16: return 5;
        case DT_INT16: return 6;
        case DT_UINT32: case DT_DATE32: return 10;
        case DT_INT32: return 11;
        default: return CAST_TEXT_MAX;
    }
}

BHIP_HD inline int cast_digits(uint64_t v) {
    int n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

// `v`: the value as the VM holds it (sign- or zero-extended; Boolean 0 / 1).  Writes at most CAST_TEXT_MAX bytes to buf (when it
// is not null) and returns their count, -1 for a NULL (a Date32 outside 0000-01-01 .. 9999-12-31).
//   integers: decimal digits, '-' for negatives (Rust's Display); Boolean: "1" / "0"; Date32: YYYY-MM-DD
BHIP_HD inline int cast_format(int from, uint64_t v, uint8_t* buf) {
    if (from == DT_BOOLEAN) {
        if (buf) buf[0] = v ? '1' : '0';
        return 1;
    }
    if (from == DT_DATE32) {
        const int64_t days = (int64_t)v;
        if (days < CAST_DATE_MIN || days > CAST_DATE_MAX) return -1;
        if (buf) {
            int64_t y;
            unsigned m, d;
            civil_from_days(days, y, m, d);
            const unsigned yy = (unsigned)y;
            buf[0] = (uint8_t)('0' + yy / 1000); buf[1] = (uint8_t)('0' + yy / 100 % 10); buf[2] = (uint8_t)('0' + yy / 10 % 10); buf[3] = (uint8_t)('0' + yy % 10);
            buf[4] = '-'; buf[5] = (uint8_t)('0' + m / 10); buf[6] = (uint8_t)('0' + m % 10);
            buf[7] = '-'; buf[8] = (uint8_t)('0' + d / 10); buf[9] = (uint8_t)('0' + d % 10);
        }
        return 10;
    }
    const bool neg = !dt_is_unsigned(from) && (int64_t)v < 0;
    uint64_t mag = neg ? (uint64_t)0 - v : v;
    const int nd = cast_digits(mag), len = nd + (neg ? 1 : 0);
    if (buf) {
        if (neg) buf[0] = '-';
        for (int k = len - 1; k >= (neg ? 1 : 0); --k) { buf[k] = (uint8_t)('0' + mag % 10); mag /= 10; }
    }
    return len;
}

}  // namespace bhip
