// text_out.hpp — what the host sides of the device text formatters (tracks.cpp, match_text.cpp) share: the caller's text arrays,
// the pool's blocks of one call, a segment's checks, and the way a slice of formatted text leaves the device.
#ifndef TS_TEXT_OUT_HPP
#define TS_TEXT_OUT_HPP

#include "capi_internal.hpp"
#include "../../include/teloscan.h"

#include <chrono>
#include <cstdlib>

inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// k files of text in a caller's struct (ts_track_text, ts_match_text); the line counts stay with the struct's owner.
struct TextFiles {
    char **text;
    uint64_t *len, *capacity;
    int k;
    bool grow(int f, uint64_t more) const {         // room for `more` bytes behind file f's text (an existing file: text != NULL)
        const uint64_t need = len[f] + more + 1;
        if (text[f] && need <= capacity[f]) return true;
        const uint64_t cap = std::max<uint64_t>(need, capacity[f] + capacity[f] / 2);
        char *p = (char *)std::realloc(text[f], cap);
        if (!p) return false;
        text[f] = p; capacity[f] = cap;
        return true;
    }
    // The start of a call: the struct is zero-initialised, or an earlier call's result, whose arrays are kept and filled again
    // (a route that formats chunk after chunk neither frees nor faults in ~100 MB per chunk); a file outside keep_mask is freed.
    void begin(uint32_t keep_mask) const {
        for (int f = 0; f < k; ++f) {
            if (!(keep_mask >> f & 1u) || !text[f]) { std::free(text[f]); text[f] = nullptr; capacity[f] = 0; }
            len[f] = 0;
        }
    }
    void free_all() const {
        for (int f = 0; f < k; ++f) { std::free(text[f]); text[f] = nullptr; len[f] = capacity[f] = 0; }
    }
};
inline TextFiles text_files(ts_track_text *t) { return TextFiles{t->text, t->len, t->capacity, TS_N_TRACKS}; }
inline TextFiles text_files(ts_match_text *t) { return TextFiles{t->text, t->len, t->capacity, TS_N_MATCH_FILES}; }

struct PoolReturn {                                 // device blocks of one call, back to the pool at its end
    ts_ctx *c;
    std::vector<DevBuf *> bufs;
    ~PoolReturn() { for (DevBuf *d : bufs) c->pool.give(std::move(*d)); }
};

// Segment i of a formatter's table: its name inside the names and no longer than the device's 32-bit line lengths are made for
// (64 of them are summed per wave: a name is at most 16 MiB, reported, not misprinted), its end inside 64 bits.
inline int text_check_segment(const ts_ctx *c, const char *what, size_t i, uint64_t name_off, uint64_t name_len, uint64_t names_len,
                              uint64_t abs_pos, uint64_t len) {
    const std::string who = std::string(what) + ": segment " + std::to_string(i);
    if (name_off > names_len || name_len > names_len - name_off) return c->fail(TS_ERR_INVALID_ARG, who + ": its name lies outside the names");
    if (name_len > TS_TRACK_MAX_NAME)
        return c->fail(TS_ERR_UNSUPPORTED, who + ": a name of more than 16 MiB (2^24 bytes) is not formatted on the device");
    if (abs_pos + len < abs_pos) return c->fail(TS_ERR_INVALID_ARG, who + ": abs_pos + len exceeds 64 bits");
    return TS_OK;
}

struct TextTimes { double write = 0, copy = 0; };   // ms, summed over a call's slices (write only under knobs.timing)

// A slice of text leaves the device: the files' bytes[f] bytes are placed in `block` at 256-byte offsets (the block taken again
// from the pool when it is too small), launch() runs the caller's write kernel on dev[f], and one copy per file appends the
// text to out.  Synchronous on st.
template <class Launch>
int text_slice_out(ts_ctx *c, const char *what, hipStream_t st, DevBuf &block, const TextFiles &out, const unsigned long long *bytes,
                   void **dev, TextTimes &ms, const Launch &launch) {
    auto t0 = std::chrono::steady_clock::now();
    auto padded = [](unsigned long long b) { return (b + 255u) & ~255ull; };
    uint64_t need = 0, off = 0;
    for (int f = 0; f < out.k; ++f) need += padded(bytes[f]);
    if (block.bytes < need) { c->pool.give(std::move(block)); HIP_TRY(c, c->pool.take(need, block)); }
    for (int f = 0; f < out.k; ++f) { dev[f] = (char *)block.p + off; off += padded(bytes[f]); }
    if (launch() != 0) return c->fail(TS_ERR_HIP, std::string(what) + ": write launch failed");
    if (c->knobs.timing) { HIP_TRY(c, hipStreamSynchronize(st)); ms.write += ms_since(t0); t0 = std::chrono::steady_clock::now(); }
    for (int f = 0; f < out.k; ++f) {
        if (!bytes[f]) continue;
        if (!out.grow(f, bytes[f])) return c->fail(TS_ERR_ALLOC, "out of host memory");
        HIP_TRY(c, hipMemcpyAsync(out.text[f] + out.len[f], dev[f], bytes[f], hipMemcpyDeviceToHost, st));
        out.len[f] += bytes[f];
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    ms.copy += ms_since(t0);
    return TS_OK;
}

#endif
