// inflate_core.h — raw deflate (RFC 1951) decoder and CRC32 arithmetic, one source for the gfx950 kernel (bgzf.hip) and for a
// host test program (tests/cpp/inflate_core_host.cpp, built by g++ under ASan + UBSan).  No allocation, no recursion, no
// library calls.  The host build is test infrastructure only: nothing in libteloscan.so inflates on the CPU.
//
// The decoder accepts exactly what zlib's inflate(Z_FINISH) on a raw stream accepts when the caller then demands
// total_in == payload_len and total_out == isize (include/teloscope_mi355x_io.hpp, inflateBgzfBlock): the final block ends in
// the payload's last byte and exactly isize bytes come out.  zlib's table rules are part of that (inftrees.c): block type 3,
// LEN != ~NLEN, HLIT > 286 or HDIST > 30, a repeat with no previous length or running past the end, no end-of-block code,
// over-subscribed sets, incomplete sets other than the single one-bit code, an unused code met in the data, symbols 286 / 287,
// distance symbols 30 / 31, a distance beyond the bytes written so far.
//
// Everything the decoder touches goes through a policy object P, which is what differs between the two builds:
//   uint32_t word(uint32_t i)       the i-th little-endian dword of the payload, zero beyond its last byte (never reads past it)
//   uint32_t lane(), nlanes()       this caller's share of the data-parallel loops (host: 0 of 1; device: lane of 64)
//   void     sync()                 orders the callers' accesses to the tables (device: the wave's LDS traffic)
//   uint32_t uni(uint32_t v)        v, known to be the same for all callers (device: read from the first lane, so that bit
//                                   buffer and control flow stay on the scalar unit)
//   void     put(uint32_t k, uint32_t e)         queue entry k of the batch (k < 64): kLiteral | byte, or length | distance << 9
//   void     flush(uint32_t n, uint32_t pos)     writes the n queued symbols' bytes at out[pos ...]; a match may read bytes of the
//                                                same batch
//   void     copy_stored(uint32_t from, uint32_t n, uint32_t pos)   out[pos .. pos + n) = payload[from .. from + n)
// The core checks every read against payload_len and every write against isize before it asks the policy for it: word() is
// asked for dwords below payload_len / 4 + 3 only, put / flush / copy_stored only for bytes below isize and for match sources
// at or above 0.  Every loop is bounded by those two numbers: a symbol costs at least one payload bit or ends the call.
#ifndef TS_INFLATE_CORE_H
#define TS_INFLATE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TS_HD __host__ __device__ __forceinline__
#else
#define TS_HD inline
#endif

namespace tsinf {

enum { kOk = 0, kBadDeflate = 1, kBadCrc = 2 };

constexpr uint32_t kLiteral = 0x80000000u;
constexpr uint32_t kBatch = 64;
constexpr int kLitFast = 10, kDistFast = 8, kCodeFast = 7;      // first-level lookup widths (bits)
enum { kCodes = 0, kLens = 1, kDists = 2 };

// One Huffman code: canonical form (count per length, symbols sorted by length then value: what decodes the rare codes longer
// than the lookup width, and finds unused codes) and a first-level lookup, entry = symbol << 4 | length, 0 = not there.
struct Tables {
    uint8_t  lens[288 + 32];            // code lengths as read: literal/length codes, then distance codes
    uint8_t  clens[20];                 // the code-length code's own lengths
    uint16_t cnt[3][16];                // by table kind (kCodes, kLens, kDists)
    uint16_t first[16], start[16], off[16];     // build scratch: first code / first sorted index / fill cursor per length
    uint16_t csym[20], lsym[288], dsym[32];
    uint16_t clut[1 << kCodeFast], llut[1 << kLitFast], dlut[1 << kDistFast];
};

// the order in which the code-length code's lengths are sent, five bits each in two words (no table in memory)
TS_HD uint32_t code_length_order(uint32_t i) {
    constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                            10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

template <class P>
struct BitReader {
    P &p;
    uint64_t buf = 0;
    uint32_t cnt = 0;               // valid bits in buf
    uint32_t next = 0;              // next payload dword to take
    uint32_t used = 0;              // bits consumed so far
    uint32_t total;                 // 8 * payload_len
    bool err = false;               // asked for bits beyond the payload
    TS_HD BitReader(P &p_, uint32_t payload_len) : p(p_), total(8u * payload_len) {}
    // at least 33 bits in buf (zeros beyond the payload: drop() is what notices the end)
    TS_HD void fill() {
        if (cnt <= 32) {
            const uint32_t w = next <= total / 32u + 1u ? p.word(next) : 0u;
            buf |= (uint64_t)w << cnt;
            cnt += 32;
            ++next;
        }
    }
    TS_HD uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }         // n <= 16
    TS_HD void drop(uint32_t n) {                                                                // n <= cnt
        if (n > total - used) { err = true; n = total - used; }
        buf >>= n; cnt -= n; used += n;
    }
    TS_HD uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }          // n <= 16, after fill()
    // continue at bit position `at` (a multiple of 8, at <= total)
    TS_HD void seek(uint32_t at) {
        used = at;
        next = at / 32u;
        const uint32_t w = next <= total / 32u + 1u ? p.word(next) : 0u;
        ++next;
        buf = (uint64_t)(w >> (at & 31u));
        cnt = 32u - (at & 31u);
    }
};

TS_HD uint32_t bit_reverse(uint32_t c, uint32_t n) {             // the low n bits of c, reversed (n in 1..15)
    uint32_t r = 0;
    for (uint32_t i = 0; i < 15; ++i) if (i < n) { r = (r << 1) | (c & 1u); c >>= 1; }
    return r;
}

// Builds one code from n lengths (n <= 288).  zlib's verdict (inftrees.c): false for an over-subscribed set, and for an
// incomplete one unless it is a single one-bit code of a literal/length or distance set; a set without any code is accepted
// (its use in the data is what fails).
template <class P>
TS_HD bool build_code(P &p, Tables *t, const uint8_t *lens, uint32_t n, int kind, uint16_t *sym, uint16_t *lut, int fast) {
    uint16_t *cnt = t->cnt[kind];
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    p.sync();
    for (uint32_t s = 0; s < n; ++s) cnt[lens[s] & 15u] = (uint16_t)(cnt[lens[s] & 15u] + 1u);
    p.sync();
    int left = 1;
    uint32_t max = 0, code = 0, idx = 0;
    bool over = false;
    for (uint32_t l = 1; l < 16; ++l) {
        const uint32_t c = p.uni(cnt[l]);
        left = left * 2 - (int)c;
        if (left < 0) over = true;
        if (over) left = 0;                                     // (keeps the doubling in range; the verdict is already fixed)
        if (c) max = l;
        t->first[l] = (uint16_t)code; t->start[l] = (uint16_t)idx; t->off[l] = (uint16_t)idx;
        code = (code + c) << 1; idx += c;
        code &= 0xffffu;
    }
    if (over) return false;
    if (max != 0 && left > 0 && (kind == kCodes || max != 1)) return false;
    p.sync();
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        if (l) { const uint32_t at = t->off[l]; sym[at] = (uint16_t)s; t->off[l] = (uint16_t)(at + 1u); }
    }
    const uint32_t size = 1u << fast;
    for (uint32_t i = p.lane(); i < size; i += p.nlanes()) lut[i] = 0;
    p.sync();
    for (uint32_t i = p.lane(); i < idx; i += p.nlanes()) {
        const uint32_t s = sym[i], l = lens[s] & 15u;
        if (l <= (uint32_t)fast) {
            const uint32_t c = (uint32_t)t->first[l] + (i - (uint32_t)t->start[l]);
            for (uint32_t j = bit_reverse(c, l); j < size; j += 1u << l) lut[j] = (uint16_t)(s << 4 | l);
        }
    }
    p.sync();
    return true;
}

// The next symbol of a code, or -1: an unused code, or the payload ended inside it (br.err).
template <class P>
TS_HD int decode_symbol(P &p, BitReader<P> &br, const uint16_t *cnt, const uint16_t *sym, const uint16_t *lut, int fast) {
    const uint32_t e = p.uni(lut[br.peek((uint32_t)fast)]);
    if (e) { br.drop(e & 15u); return br.err ? -1 : (int)(e >> 4); }
    uint32_t code = 0, first = 0, index = 0, bits = br.peek(15);
    for (uint32_t l = 1; l < 16; ++l) {
        code |= bits & 1u; bits >>= 1;
        const uint32_t c = p.uni(cnt[l]);
        if (code < first + c) {                                 // (code >= first always: the set is not over-subscribed)
            br.drop(l);
            return br.err ? -1 : (int)p.uni(sym[index + (code - first)]);
        }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return -1;
}

// payload[0, payload_len) -> isize bytes through the policy: kOk or kBadDeflate.
template <class P>
TS_HD int inflate(P &p, Tables *t, uint32_t payload_len, uint32_t isize) {
    if (payload_len > 65536u || isize > 65536u) return kBadDeflate;
    BitReader<P> br(p, payload_len);
    uint32_t pos = 0;               // bytes produced, the queued ones included
    uint32_t queued = 0, qpos = 0;  // symbols in the batch, and where its first byte goes
    for (;;) {                      // (a block costs 3 bits at least: at most 8 * payload_len / 3 + 1 rounds)
        br.fill();
        const uint32_t last = br.take(1), type = br.take(2);
        if (br.err || type == 3) return kBadDeflate;
        if (type == 0) {
            br.drop((0u - br.used) & 7u);
            br.fill();
            const uint32_t len = br.take(16);
            br.fill();
            const uint32_t nlen = br.take(16);
            if (br.err || len != (nlen ^ 0xffffu)) return kBadDeflate;
            const uint32_t from = br.used / 8u;
            if (len > payload_len - from || len > isize - pos) return kBadDeflate;
            if (queued) { p.flush(queued, qpos); queued = 0; }
            if (len) p.copy_stored(from, len, pos);
            pos += len;
            br.seek(br.used + 8u * len);
        } else {
            const uint16_t *lcnt = t->cnt[kLens], *dcnt = t->cnt[kDists];
            if (type == 1) {
                for (uint32_t s = p.lane(); s < 288u + 32u; s += p.nlanes())
                    t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
                p.sync();
                build_code(p, t, t->lens, 288, kLens, t->lsym, t->llut, kLitFast);
                build_code(p, t, t->lens + 288, 32, kDists, t->dsym, t->dlut, kDistFast);
            } else {
                const uint32_t nl = br.take(5) + 257u, nd = br.take(5) + 1u, nc = br.take(4) + 4u;
                if (br.err || nl > 286u || nd > 30u) return kBadDeflate;
                for (uint32_t i = p.lane(); i < 19u; i += p.nlanes()) t->clens[i] = 0;
                p.sync();
                for (uint32_t i = 0; i < nc; ++i) { br.fill(); t->clens[code_length_order(i)] = (uint8_t)br.take(3); }
                if (br.err) return kBadDeflate;
                p.sync();
                if (!build_code(p, t, t->clens, 19, kCodes, t->csym, t->clut, kCodeFast)) return kBadDeflate;
                uint32_t have = 0, prev = 0;
                while (have < nl + nd) {                        // (a round adds one length at least, or ends the call)
                    br.fill();
                    const int s = decode_symbol(p, br, t->cnt[kCodes], t->csym, t->clut, kCodeFast);
                    if (s < 0) return kBadDeflate;
                    if (s < 16) { t->lens[have++] = (uint8_t)s; prev = (uint32_t)s; continue; }
                    uint32_t rep, val = 0;
                    if (s == 16) { if (have == 0) return kBadDeflate; val = prev; rep = 3u + br.take(2); }
                    else if (s == 17) rep = 3u + br.take(3);
                    else rep = 11u + br.take(7);
                    if (br.err || have + rep > nl + nd) return kBadDeflate;
                    for (uint32_t i = 0; i < rep; ++i) t->lens[have + i] = (uint8_t)val;
                    have += rep; prev = val;
                }
                p.sync();
                if (p.uni(t->lens[256]) == 0) return kBadDeflate;
                if (!build_code(p, t, t->lens, nl, kLens, t->lsym, t->llut, kLitFast)) return kBadDeflate;
                if (!build_code(p, t, t->lens + nl, nd, kDists, t->dsym, t->dlut, kDistFast)) return kBadDeflate;
            }
            for (;;) {                                          // (a symbol costs one payload bit at least)
                br.fill();
                const int s = decode_symbol(p, br, lcnt, t->lsym, t->llut, kLitFast);
                if (s < 0 || s > 285) return kBadDeflate;
                if (s == 256) break;
                uint32_t e, n;
                if (s < 256) {
                    if (pos >= isize) return kBadDeflate;
                    e = kLiteral | (uint32_t)s; n = 1;
                } else {
                    const uint32_t ls = (uint32_t)s;
                    if (ls < 265u) n = ls - 254u;
                    else if (ls == 285u) n = 258u;
                    else { const uint32_t x = (ls - 261u) >> 2; n = 3u + ((4u + ((ls - 261u) & 3u)) << x) + br.take(x); }
                    br.fill();
                    const int d = decode_symbol(p, br, dcnt, t->dsym, t->dlut, kDistFast);
                    if (d < 0 || d > 29) return kBadDeflate;
                    uint32_t dist;
                    if (d < 4) dist = 1u + (uint32_t)d;
                    else { const uint32_t x = ((uint32_t)d >> 1) - 1u; dist = 1u + ((2u + ((uint32_t)d & 1u)) << x) + br.take(x); }
                    if (br.err || dist > pos || n > isize - pos) return kBadDeflate;
                    e = n | dist << 9;
                }
                if (queued == 0) qpos = pos;
                p.put(queued, e);
                pos += n;
                if (++queued == kBatch) { p.flush(queued, qpos); queued = 0; }
            }
        }
        if (last) break;
    }
    if (queued) p.flush(queued, qpos);
    if (br.err || (br.used + 7u) / 8u != payload_len || pos != isize) return kBadDeflate;
    return kOk;
}

// ---- CRC32 (the gzip polynomial, reflected): table entry, x^(8n) mod P, and the product mod P that zlib's crc32_combine uses
constexpr uint32_t kCrcPoly = 0xedb88320u;

TS_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
    return c;
}
TS_HD uint32_t crc_mul(uint32_t a, uint32_t b) {                 // a(x) * b(x) mod P, 32 shift-and-xor steps
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) {
        r ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return r;
}
TS_HD uint32_t crc_x8n(uint32_t n) {                             // x^(8n) mod P, n < 2^20
    uint32_t r = 0x80000000u, sq = 0x00800000u;                  // x^0, x^8
    for (int i = 0; i < 20; ++i) {
        if ((n >> i) & 1u) r = crc_mul(sq, r);
        sq = crc_mul(sq, sq);
    }
    return r;
}
// crc(A || B) from crc(A), crc(B) and B's length
TS_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) { return crc_mul(crc_x8n(len_b), crc_a) ^ crc_b; }

}  // namespace tsinf
#endif
