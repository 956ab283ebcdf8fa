// str_text.h — the code-point string functions substr / left / right / char_length / strpos / starts_with, written once
// (DESIGN.md §3.2 has the table).
//
// Plain host / device inline functions over a byte reader, like cast_text.h: the kernels (kernels_str.hip), the host's folding of
// literal-only calls (host/expr.cpp) and the stand-alone check program (tests/c/scalar_text_check.cpp) all run THIS code.
//
// A code point starts at every byte b with (b & 0xC0) != 0x80.  Arrow Utf8 is valid UTF-8 by contract; whatever the bytes are, no
// function here reads outside [pos, end) of the value it is given.  Positions are byte positions of the reader; counts of code
// points are int64 and may be as large as the type allows: every walk stops at the end of the value.
#pragma once
#include <stdint.h>
#include "cast_text.h"

namespace bhip {

enum StrRangeFn : int { STR_SUBSTR = 0, STR_LEFT = 1, STR_RIGHT = 2 };

constexpr int64_t STR_I64_MAX = 9223372036854775807ll;
constexpr int64_t STR_I64_MIN = -9223372036854775807ll - 1;

BHIP_HD inline bool str_is_continuation(uint8_t b) { return (b & 0xC0) == 0x80; }

// the number of code points of [pos, end)
template <class Reader>
BHIP_HD inline int64_t str_char_count(const Reader& rd, int64_t pos, int64_t end) {
    int64_t n = 0;
    for (; pos < end; ++pos) n += str_is_continuation(rd(pos)) ? 0 : 1;
    return n;
}

// the byte position `k` code points after `pos` (k >= 0), `end` when the value has fewer
template <class Reader>
BHIP_HD inline int64_t str_skip_forward(const Reader& rd, int64_t pos, int64_t end, int64_t k) {
    for (; k > 0 && pos < end; --k) {
        ++pos;
        while (pos < end && str_is_continuation(rd(pos))) ++pos;
    }
    return pos;
}

// the byte position `k` code points before `end` (k >= 0), `pos` when the value has fewer
template <class Reader>
BHIP_HD inline int64_t str_skip_backward(const Reader& rd, int64_t pos, int64_t end, int64_t k) {
    for (; k > 0 && end > pos; --k) {
        --end;
        while (end > pos && str_is_continuation(rd(end))) --end;
    }
    return end;
}

// |n| as a count of code points (the magnitude of the int64 minimum saturates: no value is that long)
BHIP_HD inline int64_t str_magnitude(int64_t n) { return n >= 0 ? n : (n == STR_I64_MIN ? STR_I64_MAX : -n); }

// substr(s, start[, count]): the code points at positions [start, start + count) intersected with [1, len], positions 1-based.
// `skip` code points are left out at the front and at most `take` kept; start + count saturates instead of overflowing.
// false for count < 0 ("negative substring length not allowed").
BHIP_HD inline bool substr_window(int64_t start, bool has_count, int64_t count, int64_t& skip, int64_t& take) {
    skip = take = 0;
    if (has_count && count < 0) return false;
    int64_t stop = STR_I64_MAX;                         // one past the last position
    if (has_count) stop = start > STR_I64_MAX - count ? STR_I64_MAX : start + count;       // (count >= 0: only the upper end can overflow)
    const int64_t first = start < 1 ? 1 : start;
    skip = first - 1;
    take = stop > first ? stop - first : 0;
    return true;
}

// the byte range [begin, stop) of the result of substr / left / right inside the value [pos, end).  `a` is start (substr) or n
// (left / right); `b` is substr's count when has_count.  false only for substr with count < 0.
template <class Reader>
BHIP_HD inline bool str_range(int fn, const Reader& rd, int64_t pos, int64_t end, int64_t a, bool has_count, int64_t b, int64_t& begin,
                              int64_t& stop) {
    begin = stop = pos;
    if (fn == STR_SUBSTR) {
        int64_t skip, take;
        if (!substr_window(a, has_count, b, skip, take)) return false;
        begin = str_skip_forward(rd, pos, end, skip);
        stop = str_skip_forward(rd, begin, end, take);
    } else if (fn == STR_LEFT) {
        stop = a >= 0 ? str_skip_forward(rd, pos, end, a) : str_skip_backward(rd, pos, end, str_magnitude(a));
    } else {
        begin = a >= 0 ? str_skip_backward(rd, pos, end, a) : str_skip_forward(rd, pos, end, str_magnitude(a));
        stop = end;
    }
    return true;
}

// starts_with(s, prefix): byte-wise; an empty prefix is a prefix of every value
template <class Reader, class SubReader>
BHIP_HD inline bool str_starts_with(const Reader& rd, int64_t pos, int64_t end, const SubReader& sub, int64_t sub_pos, int64_t sub_end) {
    const int64_t m = sub_end - sub_pos;
    if (m > end - pos) return false;
    for (int64_t k = 0; k < m; ++k)
        if (rd(pos + k) != sub(sub_pos + k)) return false;
    return true;
}

// strpos(s, sub): the 1-based code-point index of the first byte-wise occurrence of sub; 0 when there is none, 1 for an empty sub
template <class Reader, class SubReader>
BHIP_HD inline int32_t str_strpos(const Reader& rd, int64_t pos, int64_t end, const SubReader& sub, int64_t sub_pos, int64_t sub_end) {
    const int64_t m = sub_end - sub_pos;
    int64_t index = 0;                                  // code points that start in [pos, p]
    for (int64_t p = pos; p + m <= end; ++p) {
        if (p < end && !str_is_continuation(rd(p))) ++index;
        if (str_starts_with(rd, p, end, sub, sub_pos, sub_end)) return (int32_t)(index > 0 ? index : 1);
    }
    return 0;
}

}  // namespace bhip
