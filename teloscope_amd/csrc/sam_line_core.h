// sam_line_core.h — the rule of one SAM line (include/teloscan.h: "SAM text in the same resident chunk"), one source for the
// gfx950 kernels (sam.hip) and for a host test program (tests/cpp/sam_line_host.cpp, built by g++ under ASan + UBSan).  Like
// inflate_core.h, track_format_core.h and match_format_core.h: no allocation, no library calls, no local arrays.
//
// The caller has the chunk's bytes, every tab's offset in ascending order (the chunk layer's tab index) and the line's bounds
// from the line index: [ls, end) is the line's content, without its '\n' and without one '\r' that is its last byte.  It knows
// the line's kind from its first byte; header lines never come here.
#ifndef TS_SAM_LINE_CORE_H
#define TS_SAM_LINE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS_SAM_HD __host__ __device__ __forceinline__
#else
#define TS_SAM_HD inline
#endif

namespace tssam {

// the codes of include/teloscan.h (TS_SAM_*), which static_asserts in sam.cpp hold against these
enum Error { OK = 0, HEADER_AFTER_RECORD = 1, TOO_FEW_FIELDS = 2, EMPTY_SEQ = 3, BAD_LENGTHS = 4 };
constexpr uint32_t kSeqIsStar = 1u;                 // ts_sam_record.flags, bit 0

struct Line { uint32_t seq_at, seq_len, flags; };  // seq_at: relative to the line's first byte

// the first tab at or behind byte pos, as an index into tabs (n_tabs: there is none)
TS_SAM_HD uint32_t tab_lower_bound(const uint32_t *tabs, uint32_t n_tabs, uint32_t pos) {
    uint32_t lo = 0, hi = n_tabs;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tabs[mid] < pos) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// An alignment line with content [ls, end) whose first tab, if it has one, is tabs[k] (k = tab_lower_bound(tabs, n_tabs, ls)).
// Tabs 9 and 10 (counted from 1) bound SEQ, tab 10 and tab 11 or the content's end bound QUAL; a tab counts only when it lies
// before `end`, so a short line never borrows the tabs of the lines behind it.  -> OK and *out, or the first check that fails.
TS_SAM_HD Error line_rule(const unsigned char *text, uint32_t ls, uint32_t end, const uint32_t *tabs, uint32_t n_tabs, uint32_t k,
                          Line *out) {
    out->seq_at = 0u; out->seq_len = 0u; out->flags = 0u;
    // (k + 9 in 64 bits: k may be n_tabs, and n_tabs nearly 2^32)
    if ((unsigned long long)k + 9ull >= n_tabs || tabs[k + 9u] >= end) return TOO_FEW_FIELDS;
    const uint32_t t9 = tabs[k + 8u], t10 = tabs[k + 9u];
    const uint32_t t11 = (unsigned long long)k + 10ull < n_tabs && tabs[k + 10u] < end ? tabs[k + 10u] : end;
    const uint32_t seq_len = t10 - t9 - 1u, qual_len = t11 - t10 - 1u;
    out->seq_at = t9 + 1u - ls; out->seq_len = seq_len;
    if (seq_len == 0u) return EMPTY_SEQ;
    const bool seq_star = seq_len == 1u && text[t9 + 1u] == '*', qual_star = qual_len == 1u && text[t10 + 1u] == '*';
    if (seq_star) out->flags = kSeqIsStar;
    if (!seq_star && !qual_star && seq_len != qual_len) return BAD_LENGTHS;
    return OK;
}

}  // namespace tssam

#endif
