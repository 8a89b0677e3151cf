// text_core.h — the walks over FASTA body text of the host upload (upload_stage_core.h: the staging of a chunk; pipeline.cpp:
// region_pieces) and the staging workers' range cuts of a packed chunk, one source for the library and for a host test program
// (tests/cpp/text_pack_host.cpp, built by g++ under ASan + UBSan).  Host only: no HIP include, no allocation beyond the cuts' vector.
//
// A byte of body text is a base unless it is (part of) a line end: a line feed, or a carriage return right before one or at the
// very end of the text.  ts::pack_text (pack.cpp) reads text by the same rule.
#ifndef TS_TEXT_CORE_H
#define TS_TEXT_CORE_H

#include <immintrin.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace tstext {

// the bases of a run of FASTA body text, without its line ends ('\n', and a '\r' right before one or at the very end)
inline bool strip_copy(char *dst, const char *text, uint64_t text_len, uint64_t n_bases) {
    const char *p = text, *end = text + text_len;
    uint64_t left = n_bases;
    while (left && p < end) {
        const char *nl = (const char *)std::memchr(p, '\n', (size_t)(end - p));
        const char *stop = nl ? nl : end;
        uint64_t line = (uint64_t)(stop - p);
        if (line && stop[-1] == '\r') --line;
        const uint64_t take = std::min(line, left);
        std::memcpy(dst, p, take);
        dst += take; left -= take;
        p = nl ? nl + 1 : end;
    }
    return left == 0;
}

// The two walks over FASTA body text below — find the text position of a base, copy bases without their line ends — took a
// memchr and a memcpy per 81-byte LINE (37 M lines per 3 Gb: FASTA text in ran at half the rate of joined bases).  With AVX2 they
// go 32 bytes at a time.  A byte is a base unless it is a line feed, or a carriage return right before one (the byte behind the
// chunk is looked at for the chunk's last byte, so a chunk's count is exact by itself).  The scalar loops finish the last bytes of
// a piece and are the whole path without AVX2.
__attribute__((target("avx2")))
inline uint32_t line_end_mask32(const char *p) {               // bit i: byte i of the chunk is (part of) a line end; p[32] is readable
    const __m256i v = _mm256_loadu_si256((const __m256i *)p);
    const uint32_t lf = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, _mm256_set1_epi8('\n')));
    const uint32_t cr = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, _mm256_set1_epi8('\r')));
    const uint32_t lf_next = (lf >> 1) | (p[32] == '\n' ? 0x80000000u : 0u);     // bit i: byte i + 1 is a line feed
    return lf | (cr & lf_next);
}

// skips whole 32-byte chunks of [p, end) while base `*skip` lies behind them; returns the chunk it lies in (or the last bytes)
__attribute__((target("avx2")))
inline const char *text_locate_avx2(const char *p, const char *end, uint64_t *skip) {
    while (end - p >= 33) {
        const uint32_t bases = 32u - (uint32_t)__builtin_popcount(line_end_mask32(p));
        if (*skip < bases) break;
        *skip -= bases;
        p += 32;
    }
    return p;
}

// copies bases of [*pp, end) to dst, 32 text bytes at a time, while at least 32 more are wanted; the cursor stays at a place the
// scalar walk can go on from (never between a carriage return and its line feed).  Every 32-byte store lies within dst[0, n):
// a round runs only while 32 more bases are wanted, so dst needs no slack (the mixed block strips into the end of its buffer).
__attribute__((target("avx2")))
inline uint64_t strip_take_avx2(char *dst, uint64_t n, const char **pp, const char *end) {
    const char *p = *pp;
    uint64_t left = n;
    while (left >= 32 && end - p >= 33) {
        const uint32_t m = line_end_mask32(p);
        _mm256_storeu_si256((__m256i *)dst, _mm256_loadu_si256((const __m256i *)p));
        if (m == 0u) { dst += 32; p += 32; left -= 32; continue; }
        const uint32_t pos = (uint32_t)__builtin_ctz(m);             // the bases before the chunk's first line end are in place
        dst += pos; left -= pos;
        p += pos;
        if (*p == '\r') ++p;                                        // (followed by a line feed: that is what the mask says)
        ++p;                                                        // the line feed
    }
    *pp = p;
    return n - left;
}

// text position of base `skip` of a text piece (skip < its n_bases)
inline const char *text_locate(const char *text, uint64_t text_len, uint64_t skip) {
    const char *p = text, *end = text + text_len;
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
    if (have_avx2) p = text_locate_avx2(p, end, &skip);          // (chunks begin anywhere in a line: the walk below counts from any byte)
    while (p < end) {
        const char *nl = (const char *)std::memchr(p, '\n', (size_t)(end - p));
        const char *stop = nl ? nl : end;
        uint64_t line = (uint64_t)(stop - p);
        if (line && stop[-1] == '\r') --line;
        if (skip < line) return p + skip;
        skip -= line;
        p = nl ? nl + 1 : end;
    }
    return end;
}

// Up to n bases of FASTA body text from the cursor *pp on (line ends skipped), cursor advanced; returns the bases taken
// (fewer than n only when the text ends).
inline uint64_t strip_take(char *dst, uint64_t n, const char **pp, const char *end) {
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
    uint64_t left = n;
    if (have_avx2) { const uint64_t got = strip_take_avx2(dst, n, pp, end); dst += got; left -= got; }
    const char *p = *pp;
    while (left && p < end) {
        const char *nl = (const char *)std::memchr(p, '\n', (size_t)(end - p));
        const char *stop = nl ? nl : end;
        uint64_t line = (uint64_t)(stop - p);
        const bool cr = line && stop[-1] == '\r';
        if (cr) --line;
        const uint64_t take = std::min(line, left);
        std::memcpy(dst, p, take);
        dst += take; left -= take;
        if (take < line) { p += take; break; }             // stopped inside the line
        p = nl ? nl + 1 : end;
    }
    *pp = p;
    return n - left;
}

// The staging workers' ranges of a packed chunk of P positions (position 0: the 64-position boundary at or below the chunk's
// first base): worker t packs [cut[t], cut[t + 1]).  Equal shares that end at multiples of 4096 positions — but where FASTA text
// pieces lie in the chunk, a range begins where a piece begins (rounded up to a whole byte of codes) when one does within half a
// share of the even cut: a worker that enters a text piece in its middle has to find the text position of its first base, i.e.
// read the piece's text up to there, and the same text is read again when it is packed (text in ran memory-bound at 1.5 x the
// traffic of joined bases).  pieces: the chunk's, ascending; off: a piece's first position in the chunk.
struct CutPiece { uint64_t off; bool text; };
inline std::vector<uint64_t> range_cuts(uint64_t P, unsigned nt, const CutPiece *pieces, size_t n_pieces) {
    const uint64_t share = ((P + nt - 1) / nt + 4095) & ~4095ull;
    std::vector<uint64_t> cut(nt + 1);
    for (unsigned t = 0; t <= nt; ++t) cut[t] = std::min<uint64_t>(P, (uint64_t)t * share);
    size_t q = 0;
    for (unsigned t = 1; t < nt; ++t) {
        const uint64_t ideal = (uint64_t)t * share;
        if (ideal >= P) break;
        while (q < n_pieces && pieces[q].off < ideal) ++q;                  // first piece that begins at or behind the even cut
        uint64_t best = ideal, dist = share / 2;
        for (size_t c = (q > 0 ? q - 1 : q); c < n_pieces && c <= q; ++c) {  // the piece starts either side of it
            if (!pieces[c].text) continue;
            const uint64_t at = (pieces[c].off + 3) & ~3ull;
            const uint64_t d = at > ideal ? at - ideal : ideal - at;
            if (d < dist && at > cut[t - 1] && at < P) { best = at; dist = d; }
        }
        cut[t] = best;
    }
    for (unsigned t = 1; t <= nt; ++t) cut[t] = std::max(cut[t], cut[t - 1]);
    return cut;
}

}  // namespace tstext

#endif
