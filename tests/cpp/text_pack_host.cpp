// text_pack_host.cpp — the FASTA-text half of the packed upload on the host, under ASan + UBSan: ts::pack_text (pack.cpp), the
// text walks strip_copy / text_locate / strip_take and the staging workers' range cuts (text_core.h), each against a statement of
// the same thing a byte at a time.  Built by tests/test_text_pack_core_cpu.py together with pack.cpp.
//
// The statement: a byte of body text is a line end if it is '\n', or if it is '\r' and the next byte is '\n' or it is the text's
// last byte; every other byte is a base.  A base's code is (c >> 1) & 3 of the (optionally case-folded) byte, a base that is not
// A, C, G or T after folding is invalid and packs as code 0, adjacent invalid positions merge into runs.
//
// Every text and every output buffer is a heap block of EXACTLY the size the contract allows (a block per size, refilled before
// each call), so a byte read or written beyond it in either direction is a sanitizer report.
//
//   text_pack_host exhaustive MAXLEN PREFIX FULL SHARD SHARDS
//                                               every text of length <= MAXLEN over {A, n, \r, \n} (those whose number is SHARD modulo
//                                               SHARDS), behind PREFIX bases and in front of 40 more when PREFIX > 0 (the four bytes'
//                                               combinations then cross the end of a 32-byte round); up to FULL bytes with every
//                                               (start, count) pair, longer ones as check_text says
//   text_pack_host random SEED CASES            rendered random sequences (widths, line-end styles, lone CRs, blank lines, ...)
//   text_pack_host cuts SEED CASES              range_cuts
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/host.hpp"
#include "../../teloscope_amd/csrc/text_core.h"

namespace {

[[noreturn]] void fail(const char *what, const std::string &text, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
void fail(const char *what, const std::string &text, const char *fmt, ...) {
    fprintf(stderr, "FAILED %s: ", what);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fprintf(stderr, "\n  text (%zu bytes):", text.size());
    for (size_t i = 0; i < text.size() && i < 400; ++i) {
        const unsigned char c = (unsigned char)text[i];
        if (c == '\n') fprintf(stderr, "\\n"); else if (c == '\r') fprintf(stderr, "\\r"); else fputc(c, stderr);
    }
    fputc('\n', stderr);
    exit(1);
}

// ---------------------------------------------------------------------------------------------- exact-size heap blocks
struct Blocks {                                                  // one block per size, never one byte more
    std::vector<unsigned char *> by_size;
    unsigned char *get(size_t n) {
        if (n >= by_size.size()) by_size.resize(n + 1, nullptr);
        if (!by_size[n]) by_size[n] = (unsigned char *)malloc(n ? n : 1);       // (n == 0: a block nobody may touch ...
        return by_size[n] + (n ? 0 : 1);                                         // ... handed out past its end)
    }
    ~Blocks() { for (unsigned char *p : by_size) free(p); }
};
Blocks g_text, g_out;

// ---------------------------------------------------------------------------------------------- the statement
struct Ref {
    std::vector<unsigned char> base;      // the bases
    std::vector<size_t> at;               // text index of each
};

bool is_line_end(const std::string &t, size_t i) {
    return t[i] == '\n' || (t[i] == '\r' && (i + 1 == t.size() || t[i + 1] == '\n'));
}

void parse(const std::string &t, Ref &r) {
    r.base.clear(); r.at.clear();
    for (size_t i = 0; i < t.size(); ++i)
        if (!is_line_end(t, i)) { r.base.push_back((unsigned char)t[i]); r.at.push_back(i); }
}

bool valid(unsigned char c, bool fold) {
    if (fold) c &= 0xDF;
    return c == 'A' || c == 'C' || c == 'G' || c == 'T';
}
unsigned code_of(unsigned char c, bool fold) { return valid(c, fold) ? (((fold ? c & 0xDF : c) >> 1) & 3u) : 0u; }

const std::vector<unsigned char> &ref_codes(const Ref &r, size_t k, size_t n, bool fold) {
    static std::vector<unsigned char> out;
    out.assign((n + 3) / 4, 0);
    for (size_t i = 0; i < n; ++i) out[i >> 2] |= (unsigned char)(code_of(r.base[k + i], fold) << (2 * (i & 3)));
    return out;
}

const std::vector<ts::InvalidRun> &ref_runs(const Ref &r, size_t k, size_t n, bool fold, uint32_t pos0) {
    static std::vector<ts::InvalidRun> out;
    out.clear();
    for (size_t i = 0; i < n; ++i) {
        if (valid(r.base[k + i], fold)) continue;
        const uint32_t pos = pos0 + (uint32_t)i;
        if (!out.empty() && out.back().start + out.back().len == pos) ++out.back().len;
        else out.push_back({pos, 1});
    }
    return out;
}

// a cursor behind `taken` bases from base k on: behind the last base taken, at or in front of the next one
void check_cursor(const char *what, const std::string &t, const Ref &r, size_t k, size_t taken, size_t cursor, bool may_split_crlf) {
    const size_t lo = taken ? r.at[k + taken - 1] + 1 : 0;
    const size_t hi = k + taken < r.at.size() ? r.at[k + taken] : t.size();
    if (cursor < lo || cursor > hi) fail(what, t, "cursor %zu outside [%zu, %zu] after %zu bases from base %zu", cursor, lo, hi, taken, k);
    if (!may_split_crlf && cursor > 0 && cursor < t.size() && t[cursor - 1] == '\r' && t[cursor] == '\n')
        fail(what, t, "cursor %zu left between a carriage return and its line feed", cursor);
}

const char *put_text(const std::string &t) {
    char *p = (char *)g_text.get(t.size());
    if (!t.empty()) memcpy(p, t.data(), t.size());
    return p;
}

// which of the code under test this host runs: without AVX2 (pack_text: and BMI2) the scalar loops are the whole path
int have_avx2() { return __builtin_cpu_supports("avx2") ? 1 : 0; }
int have_bmi2() { return __builtin_cpu_supports("bmi2") ? 1 : 0; }

struct Tally { uint64_t cases = 0, calls = 0, cr31 = 0, run_over_end = 0, split_crlf = 0; };

// ---------------------------------------------------------------------------------------------- a: pack_text in sequence
// consecutive calls of `sizes` bases (cycled; each a multiple of 4) and an odd last call that takes the rest (asked for `over` more)
void pack_in_sequence(const std::string &t, const Ref &r, const char *text, bool fold, const std::vector<size_t> &sizes, size_t over, Tally &ty) {
    const size_t B = r.base.size();
    const uint32_t pos_base = 4000;
    static ts::PackRuns R;
    R.runs.clear(); R.open_len = 0;
    const char *cur = text, *end = text + t.size();
    size_t k = 0, call = 0;
    while (k < B || call == 0) {
        size_t n = sizes[call % sizes.size()];
        const bool last = n >= B - k;
        if (last) n = B - k + over;
        const size_t want = last ? B - k : n;
        unsigned char *dst = g_out.get((want + 3) / 4);
        memset(dst, 0xEE, (want + 3) / 4);
        const size_t got = ts::pack_text(&cur, end, n, dst, fold, pos_base + (uint32_t)k, R);
        ++ty.calls;
        if (got != want) fail("pack_text in sequence", t, "call %zu from base %zu: %zu bases taken, %zu expected (n %zu)", call, k, got, want, n);
        const std::vector<unsigned char> &codes = ref_codes(r, k, want, fold);
        if (want && memcmp(dst, codes.data(), codes.size()) != 0) fail("pack_text in sequence", t, "call %zu from base %zu, n %zu, fold %d: codes differ", call, k, n, (int)fold);
        check_cursor("pack_text in sequence", t, r, k, want, (size_t)(cur - text), false);
        if (cur > text && cur < end && cur[-1] == '\r' && cur[0] == '\n') ++ty.split_crlf;
        k += want;
        ++call;
        if (last) break;
    }
    R.finish();
    const std::vector<ts::InvalidRun> &runs = ref_runs(r, 0, B, fold, pos_base);
    if (runs.size() != R.runs.size()) fail("pack_text in sequence", t, "%zu runs, %zu expected (fold %d)", R.runs.size(), runs.size(), (int)fold);
    for (size_t i = 0; i < runs.size(); ++i)
        if (runs[i].start != R.runs[i].start || runs[i].len != R.runs[i].len)
            fail("pack_text in sequence", t, "run %zu is {%u, %u}, expected {%u, %u}", i, R.runs[i].start, R.runs[i].len, runs[i].start, runs[i].len);
}

// ---------------------------------------------------------------------------------------------- b: pack_text entered anywhere
void pack_from(const std::string &t, const Ref &r, const char *text, bool fold, size_t k, size_t n, Tally &ty) {
    const char *cur = tstext::text_locate(text, t.size(), k);
    if ((size_t)(cur - text) != r.at[k]) fail("text_locate", t, "base %zu found at %zu, lies at %zu", k, (size_t)(cur - text), r.at[k]);
    unsigned char *dst = g_out.get((n + 3) / 4);
    memset(dst, 0xEE, (n + 3) / 4);
    static ts::PackRuns R;                                        // (kept for its vector's memory)
    R.runs.clear(); R.open_len = 0;
    const uint32_t pos0 = 100 + (uint32_t)k;
    const size_t got = ts::pack_text(&cur, text + t.size(), n, dst, fold, pos0, R);
    R.finish();
    ++ty.calls;
    if (got != n) fail("pack_text entered", t, "from base %zu: %zu of %zu bases taken", k, got, n);
    const std::vector<unsigned char> &codes = ref_codes(r, k, n, fold);
    if (memcmp(dst, codes.data(), codes.size()) != 0) fail("pack_text entered", t, "from base %zu, n %zu, fold %d: codes differ", k, n, (int)fold);
    const std::vector<ts::InvalidRun> &runs = ref_runs(r, k, n, fold, pos0);
    bool same = runs.size() == R.runs.size();
    for (size_t i = 0; same && i < runs.size(); ++i) same = runs[i].start == R.runs[i].start && runs[i].len == R.runs[i].len;
    if (!same) fail("pack_text entered", t, "from base %zu, n %zu, fold %d: invalid runs differ", k, n, (int)fold);
    check_cursor("pack_text entered", t, r, k, n, (size_t)(cur - text), false);
}

// ---------------------------------------------------------------------------------------------- c: strip_take
// n may exceed what the text holds: then the rest is taken and the cursor is the text's end.  dst: exactly n bytes.
void take_from(const std::string &t, const Ref &r, const char *text, size_t k, size_t n, Tally &ty) {
    const size_t B = r.base.size(), want = n < B - k ? n : B - k;
    const char *cur = k < B ? text + r.at[k] : text + t.size();
    if (k && k < B && r.at[k] != r.at[k - 1] + 1 && (n & 1)) cur = text + r.at[k - 1] + 1;      // (also from in front of the line end before base k)
    char *dst = (char *)g_out.get(n);
    memset(dst, 0xEE, n);
    const uint64_t got = tstext::strip_take(dst, n, &cur, text + t.size());
    ++ty.calls;
    if (got != want) fail("strip_take", t, "from base %zu: %zu bases taken, %zu expected (n %zu)", k, (size_t)got, want, n);
    if (want && memcmp(dst, r.base.data() + k, want) != 0) fail("strip_take", t, "from base %zu, n %zu: bases differ", k, n);
    check_cursor("strip_take", t, r, k, want, (size_t)(cur - text), false);
    if (want < n && cur != text + t.size()) fail("strip_take", t, "from base %zu, n %zu: the text ended, the cursor is not at its end", k, n);
}

// ---------------------------------------------------------------------------------------------- d: strip_copy
void copy_from(const std::string &t, const Ref &r, const char *text, size_t k, size_t n) {
    const size_t B = r.base.size(), from = k < B ? r.at[k] : t.size();
    char *dst = (char *)g_out.get(n);
    memset(dst, 0xEE, n);
    const bool ok = tstext::strip_copy(dst, text + from, t.size() - from, n);
    if (ok != (n <= B - k)) fail("strip_copy", t, "from base %zu, %zu bases declared, %zu there: answered %d", k, n, B - k, (int)ok);
    const size_t want = n < B - k ? n : B - k;
    if (want && memcmp(dst, r.base.data() + k, want) != 0) fail("strip_copy", t, "from base %zu, n %zu: bases differ", k, n);
}

// Every check on one text.  level 2: every (k, n) pair; level 1: every n from the first base and every k to the last; level 0:
// a few n per k, and for a long text a sample of the k.
// What level 1 leaves out, the pairs (k > 0, n < what is left): in the family WITHOUT a prefix they are another text's — the
// family holds every suffix of each of its texts and none of the functions looks in front of its cursor, so base k with n bases
// of one text is the first base with n bases of another.  In the family BEHIND a prefix that does not hold and those pairs are
// simply not checked; that run is about the bytes around the end of a 32-byte round, which every n from the first base (the
// round ends inside the four bytes, calls end before, in and behind them) and every k to the end (the rounds move over them)
// do reach.
void check_text(const std::string &t, int level, std::mt19937_64 &rng, Tally &ty, bool count) {
    static Ref r;
    parse(t, r);
    const char *text = put_text(t);
    const size_t B = r.base.size();
    static const std::vector<std::vector<size_t>> schedules = {{16384}, {4}, {32, 4, 64}, {128, 36}, {100, 8, 12}, {60}};
    const size_t stride = B > 1500 ? B / 48 : 1;
    for (int fold = 0; fold < 2; ++fold) {
        if (level == 1 && fold != (int)(t.size() & 1)) continue;      // (the family holds no letter that folding changes the fate of)
        for (size_t s = 0; s < schedules.size(); ++s) {
            if (level == 1 ? s > 1 : (level == 0 && s && s != 1 + rng() % (schedules.size() - 1))) continue;
            pack_in_sequence(t, r, text, fold != 0, schedules[s], s % 3 == 2 ? 5 : 0, ty);
        }
        for (size_t k = 0; k < B; k += (stride > 1 ? 1 + rng() % (2 * stride) : 1)) {
            const size_t left = B - k;
            if (level == 2 || (level == 1 && k == 0)) { for (size_t n = 1; n <= left; ++n) pack_from(t, r, text, fold != 0, k, n, ty); continue; }
            if (level == 1) { pack_from(t, r, text, fold != 0, k, left, ty); continue; }
            const size_t ns[] = {left, 1, 31, 32, 33, 36, 1 + rng() % left};
            for (size_t n : ns) if (n <= left && ((n == left && left < 1500) || rng() % 3 == 0)) pack_from(t, r, text, fold != 0, k, n, ty);
        }
    }
    for (size_t k = 0; k <= B; k += (stride > 1 ? 1 + rng() % (2 * stride) : 1)) {
        const size_t left = B - k;
        if (level == 2 || (level == 1 && k == 0)) { for (size_t n = 0; n <= left + 2; ++n) take_from(t, r, text, k, n, ty); }
        else if (level == 1) take_from(t, r, text, k, left, ty);
        else {
            const size_t ns[] = {left, left + 3, 0, 1, 31, 32, 33, 64, 1 + rng() % (left + 1)};
            for (size_t n : ns) if (n <= left + 3 && ((n >= left && left < 1500) || rng() % 3 == 0)) take_from(t, r, text, k, n, ty);
        }
        if (k == 0 || level == 2 || rng() % 8 == 0) for (size_t n : {left, left + 1, left / 2, (size_t)0}) copy_from(t, r, text, k, n);
    }
    if (!count) return;
    ++ty.cases;
    // g: does a vector round of pack_text from the text's first byte (all bases asked for) see a carriage return in its byte 31
    // and the line feed in byte 32; and does an invalid run (no folding) go on across a line end
    size_t bases_before = 0, at = 0;
    bool cr31 = false;
    for (size_t o = 0; o + 33 <= t.size(); o += 32) {
        while (at < B && r.at[at] < o) { ++at; }
        bases_before = at;
        if (B - bases_before < 32) break;
        if (t[o + 31] == '\r' && t[o + 32] == '\n') cr31 = true;
    }
    bool over = false;
    for (size_t i = 1; i < B && !over; ++i) over = r.at[i] != r.at[i - 1] + 1 && !valid(r.base[i], false) && !valid(r.base[i - 1], false);
    ty.cr31 += cr31;
    ty.run_over_end += over;
}

// ---------------------------------------------------------------------------------------------- f: the texts
// (texts of more than `full` bytes: level 1 of check_text)
int run_exhaustive(size_t maxlen, size_t prefix, size_t full, uint64_t shard, uint64_t n_shards) {
    static const char alpha[4] = {'A', 'n', '\r', '\n'};
    std::mt19937_64 rng(1);
    Tally ty;
    std::string head, tail, t;
    for (size_t i = 0; i < prefix; ++i) head.push_back("ACGT"[i & 3]);
    if (prefix) for (size_t i = 0; i < 40; ++i) tail.push_back("TGCA"[i & 3]);
    uint64_t texts = 0;
    for (size_t len = 0; len <= maxlen; ++len) {
        const uint64_t count = 1ull << (2 * len);
        for (uint64_t v = shard; v < count; v += n_shards) {
            t = head;
            for (size_t i = 0; i < len; ++i) t.push_back(alpha[(v >> (2 * i)) & 3]);
            t += tail;
            check_text(t, len <= full ? 2 : 1, rng, ty, false);
            ++texts;
        }
    }
    printf("exhaustive avx2 %d bmi2 %d texts %llu calls %llu cursor_between_cr_and_lf_after_pack_text %llu\n", have_avx2(), have_bmi2(), (unsigned long long)texts,
           (unsigned long long)ty.calls, (unsigned long long)ty.split_crlf);
    return 0;
}

std::string render(std::mt19937_64 &rng, size_t n_bases) {
    static const size_t widths[] = {1, 2, 31, 32, 33, 60, 63, 64, 65, 70, 80};
    const std::string alpha = rng() % 2 ? "ACGT" : "ACGTacgtNnRY";
    std::string seq;
    for (size_t i = 0; i < n_bases; ++i) seq.push_back(alpha[rng() % alpha.size()]);
    if (alpha.size() > 4)                                              // N runs, wherever they fall (line ends among them)
        for (int q = 0; q < 3 && n_bases > 10; ++q) { const size_t a = rng() % (n_bases - 8), ln = 1 + rng() % 8; for (size_t i = a; i < a + ln; ++i) seq[i] = "Nn"[rng() & 1]; }
    size_t width = widths[rng() % 11];
    if (width <= 2 && n_bases > 200) width = widths[2 + rng() % 9];
    const int style = (int)(rng() % 5);                                // 0 LF, 1, 2 CRLF, 3, 4 a mix
    // the first line ends at byte 30, 31, 32 or 33 of the first 32-byte round in two cases of five; in the CRLF styles that puts the
    // carriage return or the line feed there, and lines of 62 or 30 bases + CRLF keep later ones on the same byte of their rounds
    size_t first = rng() % 5 < 2 ? 30 + rng() % 4 : width;
    if (style != 0 && rng() % 3 == 0) { first = 31; width = rng() & 1 ? 62 : 30; }
    std::string t;
    size_t in_line = 0, limit = first;
    for (size_t i = 0; i < seq.size(); ++i) {
        t.push_back(seq[i]);
        if (rng() % 97 == 0) t.push_back('\r');                       // a lone carriage return inside a line: a base (an invalid one) ...
        if (++in_line < limit || i + 1 == seq.size()) continue;
        in_line = 0; limit = width;
        const bool crlf = style == 1 || style == 2 || (style >= 3 && (rng() & 1));
        if (rng() % 29 == 0) t += "\r\r\n";                            // ... as is the first of two in front of a line feed
        else t += crlf ? "\r\n" : "\n";
        if (rng() % 23 == 0) t += crlf ? "\r\n" : "\n";               // a blank line
    }
    // (a lone '\r' pushed behind the last base would be a line end: only in the ending drawn below)
    while (!t.empty() && t.back() == '\r') t.pop_back();
    switch (rng() % 4) { case 0: t += "\r"; break; case 1: t += "\r\n"; break; case 2: t += "\n"; break; default: break; }
    return t;
}

int run_random(uint64_t seed, size_t cases) {
    std::mt19937_64 rng(seed);
    Tally ty;
    for (size_t c = 0; c < cases; ++c) {
        const size_t n = c % 50 == 49 ? 40000 + rng() % 20000 : (rng() % 4 == 0 ? rng() % 40 : 33 + rng() % 668);
        check_text(render(rng, n), n <= 60 ? 2 : 0, rng, ty, true);
    }
    printf("random avx2 %d bmi2 %d cases %llu calls %llu cr_in_byte_31_lf_in_byte_32 %llu invalid_run_across_line_end %llu cursor_between_cr_and_lf_after_pack_text %llu\n",
           have_avx2(), have_bmi2(), (unsigned long long)ty.cases, (unsigned long long)ty.calls, (unsigned long long)ty.cr31, (unsigned long long)ty.run_over_end,
           (unsigned long long)ty.split_crlf);
    return 0;
}

// ---------------------------------------------------------------------------------------------- e: the cuts
int run_cuts(uint64_t seed, size_t cases) {
    std::mt19937_64 rng(seed);
    std::vector<uint64_t> sizes;
    for (uint64_t p = 1; p <= 70; ++p) sizes.push_back(p);
    for (int b = 7; b <= 27; ++b) for (int d = -1; d <= 1; ++d) if ((1ull << b) + d <= (1ull << 27)) sizes.push_back((1ull << b) + d);
    for (uint64_t p : {4095ull, 4097ull, 8191ull, 12288ull, 16384ull * 3 + 5, (8ull << 20) + 64, (9ull << 20) + 12345}) sizes.push_back(p);
    while (sizes.size() < cases) sizes.push_back(1 + rng() % (1ull << (3 + rng() % 25)));
    uint64_t checked = 0, snapped = 0;
    for (uint64_t P : sizes) {
        for (int layout = 0; layout < 4; ++layout) {                 // 0 no pieces listed, 1 plain only, 2 text only, 3 both
            std::vector<tstext::CutPiece> pieces;
            if (layout) {
                const uint64_t typical = 1 + rng() % (1 + P / (1 + rng() % 40));
                for (uint64_t off = rng() % 64; off < P && pieces.size() < 5000;) {
                    pieces.push_back({off, layout == 2 || (layout == 3 && (rng() & 1))});
                    off += 1 + rng() % (2 * typical) + (rng() % 4 == 0 ? rng() % 65536 : 0);
                }
            }
            for (unsigned nt = 1; nt <= 8; ++nt) {
                const std::vector<uint64_t> cut = tstext::range_cuts(P, nt, pieces.data(), pieces.size());
                ++checked;
                std::string what = "P " + std::to_string(P) + " nt " + std::to_string(nt) + " layout " + std::to_string(layout);
                if (cut.size() != nt + 1 || cut[0] != 0 || cut[nt] != P) fail("range_cuts", "", "%s: the cuts do not run from 0 to P", what.c_str());
                for (unsigned t = 1; t <= nt; ++t) if (cut[t] < cut[t - 1]) fail("range_cuts", "", "%s: cut %u descends", what.c_str(), t);
                for (unsigned t = 1; t < nt; ++t) {
                    // (a cut at P leaves nothing for the workers behind it, and P need not be a multiple of anything)
                    if (cut[t] == P) continue;
                    if (cut[t] & 3u) fail("range_cuts", "", "%s: cut %u = %llu is not a multiple of 4", what.c_str(), t, (unsigned long long)cut[t]);
                    if ((cut[t] & 4095u) == 0) continue;
                    bool is_start = false;
                    for (const tstext::CutPiece &pc : pieces) if (pc.text && ((pc.off + 3) & ~3ull) == cut[t]) is_start = true;
                    if (!is_start) fail("range_cuts", "", "%s: cut %u = %llu is neither a multiple of 4096 nor a text piece's start", what.c_str(), t, (unsigned long long)cut[t]);
                    ++snapped;
                }
            }
        }
    }
    printf("cuts checked %llu cuts_at_a_text_piece %llu\n", (unsigned long long)checked, (unsigned long long)snapped);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 7 && !strcmp(argv[1], "exhaustive"))
        return run_exhaustive((size_t)atoll(argv[2]), (size_t)atoll(argv[3]), (size_t)atoll(argv[4]), (uint64_t)atoll(argv[5]), (uint64_t)atoll(argv[6]));
    if (argc == 4 && !strcmp(argv[1], "random")) return run_random((uint64_t)atoll(argv[2]), (size_t)atoll(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "cuts")) return run_cuts((uint64_t)atoll(argv[2]), (size_t)atoll(argv[3]));
    fprintf(stderr, "usage: text_pack_host exhaustive MAXLEN PREFIX FULL SHARD SHARDS | random SEED CASES | cuts SEED CASES\n");
    return 2;
}
