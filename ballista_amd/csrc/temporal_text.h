// temporal_text.h — to_timestamp's text grammar, date_trunc's and date_part's calendar arithmetic, written once (DESIGN.md §3.2 has
// the table).
//
// Plain host / device inline functions like cast_text.h, which this header extends (civil_from_days / days_from_civil live there):
// the kernels (kernels_cast.hip), the host's folding of literals (host/expr.cpp) and the stand-alone check program
// (tests/c/temporal_text_check.cpp) all run THIS code.
//
// Timestamps carry no zone: the arithmetic is UTC on the proleptic Gregorian calendar, and every truncation is a floor.
#pragma once
#include "cast_text.h"

namespace bhip {

enum TruncGranularity : int { TRUNC_SECOND = 0, TRUNC_MINUTE, TRUNC_HOUR, TRUNC_DAY, TRUNC_WEEK, TRUNC_MONTH, TRUNC_YEAR, TRUNC_COUNT };

// the granularity named by text[0, len): exactly one of the seven lower-case words, else -1
BHIP_HD inline int trunc_granularity(const char* text, int64_t len) {
    const char* names[TRUNC_COUNT] = {"second", "minute", "hour", "day", "week", "month", "year"};
    for (int g = 0; g < TRUNC_COUNT; ++g) {
        int64_t k = 0;
        while (k < len && names[g][k] != 0 && names[g][k] == text[k]) ++k;
        if (k == len && names[g][k] == 0) return g;
    }
    return -1;
}

// units of a Timestamp type in one second; 0 for every other type
BHIP_HD inline int64_t timestamp_units_per_second(int t) {
    switch (t) {
        case DT_TIMESTAMP_S: return 1ll;
        case DT_TIMESTAMP_MS: return 1000ll;
        case DT_TIMESTAMP_US: return 1000000ll;
        case DT_TIMESTAMP_NS: return 1000000000ll;
        default: return 0;
    }
}

constexpr int64_t TEMPORAL_I64_MIN = -9223372036854775807ll - 1;

// date_trunc of one value `v` of Timestamp type `unit`: true and the floor in `out`, false where the floor does not fit int64 in
// the unit (the result is NULL: only within a year of the int64 minimum, for nanoseconds)
BHIP_HD inline bool temporal_trunc(int unit, int g, int64_t v, int64_t& out) {
    out = 0;
    const int64_t ups = timestamp_units_per_second(unit);
    if (ups == 0 || g < 0 || g >= TRUNC_COUNT) return false;
    if (g <= TRUNC_DAY) {
        const int64_t period = ups * (g == TRUNC_SECOND ? 1ll : g == TRUNC_MINUTE ? 60ll : g == TRUNC_HOUR ? 3600ll : 86400ll);
        int64_t r = v % period;                     // C++ rounds towards zero: a negative remainder belongs to the period before
        if (r < 0) r += period;
        if (v < TEMPORAL_I64_MIN + r) return false;
        out = v - r;
        return true;
    }
    const int64_t upd = ups * 86400ll;
    int64_t days = v / upd;
    if (v % upd < 0) --days;
    if (g == TRUNC_WEEK) {
        int64_t dow = (days + 3) % 7;               // 1970-01-01 is a Thursday: Monday = 0
        if (dow < 0) dow += 7;
        days -= dow;
    } else {
        int64_t y;
        unsigned m, d;
        civil_from_days(days, y, m, d);
        days = days_from_civil(y, g == TRUNC_MONTH ? m : 1u, 1u);
    }
    // days <= v / upd, so only the lower end can be missed; INT64_MIN / upd rounds towards zero: the first day that fits
    if (days < TEMPORAL_I64_MIN / upd) return false;
    out = days * upd;
    return true;
}

// ---- date_part('part', x): one calendar field of a Date32, a Date64 or a Timestamp, as Int32 --------------------------------------
enum DatePart : int { PART_YEAR = 0, PART_QUARTER, PART_MONTH, PART_DAY, PART_DOW, PART_DOY, PART_HOUR, PART_MINUTE, PART_SECOND, PART_COUNT };

// the part named by text[0, len): exactly one of the nine lower-case words, else -1
BHIP_HD inline int date_part_name(const char* text, int64_t len) {
    const char* names[PART_COUNT] = {"year", "quarter", "month", "day", "dow", "doy", "hour", "minute", "second"};
    for (int p = 0; p < PART_COUNT; ++p) {
        int64_t k = 0;
        while (k < len && names[p][k] != 0 && names[p][k] == text[k]) ++k;
        if (k == len && names[p][k] == 0) return p;
    }
    return -1;
}

// units of a temporal type in one day; 0 for every other type.  (Date64 counts milliseconds.)
BHIP_HD inline int64_t temporal_units_per_day(int t) {
    if (t == DT_DATE32) return 1ll;
    if (t == DT_DATE64) return 86400000ll;
    return timestamp_units_per_second(t) * 86400ll;
}

// date_part of one value `v` of temporal type `t`: true and the field in `out`, false where it does not fit Int32 (the result is
// NULL: the year of a value far from 1970).  Instants before 1970 floor; dow: 0 = Sunday; doy: 1 .. 366; whole seconds.
BHIP_HD inline bool temporal_part(int t, int part, int64_t v, int32_t& out) {
    out = 0;
    const int64_t upd = temporal_units_per_day(t);
    if (upd == 0 || part < 0 || part >= PART_COUNT) return false;
    int64_t days = v / upd, rem = v % upd;          // C++ rounds towards zero: a negative remainder belongs to the day before
    if (rem < 0) { rem += upd; --days; }
    if (part >= PART_HOUR) {
        const int64_t ups = upd / 86400ll;
        const int64_t sod = ups ? rem / ups : 0;    // second of the day; a Date32 has none
        out = (int32_t)(part == PART_HOUR ? sod / 3600 : part == PART_MINUTE ? sod / 60 % 60 : sod % 60);
        return true;
    }
    if (part == PART_DOW) {
        int64_t dow = (days % 7 + 4) % 7;           // 1970-01-01 is a Thursday
        if (dow < 0) dow += 7;
        out = (int32_t)dow;
        return true;
    }
    int64_t y;
    unsigned m, d;
    civil_from_days(days, y, m, d);
    if (part == PART_YEAR) {
        if (y < -2147483648ll || y > 2147483647ll) return false;
        out = (int32_t)y;
    } else if (part == PART_QUARTER) out = (int32_t)((m - 1) / 3 + 1);
    else if (part == PART_MONTH) out = (int32_t)m;
    else if (part == PART_DAY) out = (int32_t)d;
    else out = (int32_t)(days - days_from_civil(y, 1u, 1u) + 1);
    return true;
}

// ---- to_timestamp: YYYY-MM-DD ('T' | ' ') hh:mm:ss [ '.' 1-9 digits ] [ 'Z' | 'z' | ('+' | '-') hh ':' mm ] ----------------------
// over the whole value, no blanks around it; the date must exist; without an offset the text is UTC; the instant must fit int64
// nanoseconds.  true and the nanoseconds since 1970-01-01T00:00:00Z in `out`, false for every other text.
template <class Reader>
BHIP_HD inline bool to_timestamp_parse(const Reader& rd, int64_t pos, int64_t end, int64_t& out) {
    out = 0;
    if (end - pos < 19 || end - pos > 35) return false;
    unsigned v[19];
    for (int k = 0; k < 19; ++k) {
        const uint8_t c = rd(pos + k);
        v[k] = 0;
        if (k == 4 || k == 7) { if (c != '-') return false; }
        else if (k == 10) { if (c != 'T' && c != ' ') return false; }
        else if (k == 13 || k == 16) { if (c != ':') return false; }
        else { if (!cast_is_digit(c)) return false; v[k] = (unsigned)(c - '0'); }
    }
    const unsigned y = v[0] * 1000 + v[1] * 100 + v[2] * 10 + v[3], mo = v[5] * 10 + v[6], d = v[8] * 10 + v[9];
    const unsigned hh = v[11] * 10 + v[12], mi = v[14] * 10 + v[15], ss = v[17] * 10 + v[18];
    if (mo < 1 || mo > 12 || d < 1 || hh > 23 || mi > 59 || ss > 59) return false;
    const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
    const unsigned dim = mo == 2 ? (leap ? 29u : 28u) : ((mo == 4 || mo == 6 || mo == 9 || mo == 11) ? 30u : 31u);
    if (d > dim) return false;
    pos += 19;
    int64_t frac = 0;
    if (pos < end && rd(pos) == '.') {
        ++pos;
        int nd = 0;
        for (; pos < end && cast_is_digit(rd(pos)); ++pos) {
            if (++nd > 9) return false;
            frac = frac * 10 + (rd(pos) - '0');
        }
        if (nd == 0) return false;
        for (; nd < 9; ++nd) frac *= 10;
    }
    int64_t offset = 0;                              // seconds east of UTC
    if (pos < end) {
        const uint8_t c = rd(pos);
        if (c == 'Z' || c == 'z') ++pos;
        else if (c == '+' || c == '-') {
            if (end - pos != 6) return false;
            const uint8_t h1 = rd(pos + 1), h0 = rd(pos + 2), m1 = rd(pos + 4), m0 = rd(pos + 5);
            if (!cast_is_digit(h1) || !cast_is_digit(h0) || rd(pos + 3) != ':' || !cast_is_digit(m1) || !cast_is_digit(m0)) return false;
            const int oh = (h1 - '0') * 10 + (h0 - '0'), om = (m1 - '0') * 10 + (m0 - '0');
            if (oh > 23 || om > 59) return false;
            offset = (int64_t)(oh * 3600 + om * 60);
            if (c == '-') offset = -offset;
            pos += 6;
        } else return false;
    }
    if (pos != end) return false;
    const int64_t secs = days_from_civil((int64_t)y, mo, d) * 86400ll + (int64_t)(hh * 3600u + mi * 60u + ss) - offset;
    // int64 nanoseconds: 1677-09-21T00:12:43.145224192 .. 2262-04-11T23:47:16.854775807
    if (secs > 9223372036ll || secs < -9223372037ll) return false;
    if (secs == 9223372036ll && frac > 854775807ll) return false;
    if (secs == -9223372037ll && frac < 145224192ll) return false;
    out = (int64_t)((uint64_t)secs * 1000000000ull + (uint64_t)frac);      // modulo 2^64: the checks above keep the true value in range
    return true;
}

}  // namespace bhip
