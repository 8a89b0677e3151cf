// deflate_core.h — raw deflate (RFC 1951) encoder for one block of at most 65 280 plain bytes and the CRC32 of those bytes, one
// source for the gfx950 kernel (deflate.hip) and for a host test program (tests/cpp/deflate_core_host.cpp, built by g++ under
// ASan + UBSan).  No allocation, no recursion, no library calls.  The reference's counterpart is zlib behind BgzfWriter
// (src/bgzf.cpp:227-276); nothing in libteloscan.so links zlib.
//
// What comes out: one final block, BTYPE 2 (dynamic codes built from the block's own symbol counts) or, where that is no
// shorter, BTYPE 0 (stored): payload <= n + 5 bytes.  The bytes are a function of the input alone: the host build (one lane) and
// the device (64 lanes) write the same payload.
//
// Method.  Positions are taken 64 at a time (a batch, whatever the lane count).  A position that no earlier token covers hashes
// its next four bytes and has two candidates: the highest earlier position with that hash that an EARLIER batch inserted, and the
// position as far back as the last match chosen before this batch reached (a repeat goes on at its distance whatever became of
// its bucket).  The batch's own positions go into the table only after all of its lookups, and of those that share a bucket the
// highest alone stores: the table never depends on which lane comes first.  A candidate is always behind its position and at or
// after the block's first byte; it is used when it is at most 32 768 back and at least kMinMatch bytes agree (compared a word at
// a time, never beyond the block's end); of two, the longer, and at equal length the repeat.  One wave-uniform
// pass per batch makes the greedy choice: the first match that starts at or after the end of the token before it wins, positions
// it covers are skipped.  The tokens are not kept: the same search runs twice, once to count symbols and once to write them
// (pass 2 is skipped where the block is stored), which costs a second search and no memory beside the tables below.
// Huffman lengths: symbols ranked by (count, symbol) in parallel, the tree joined from two queues by one lane, and where the
// deepest leaf is beyond the limit (15; 7 for the code-length code) the counts are halved (rounded up) and the tree rebuilt, at
// most kMaxRounds times (equal counts give a tree of depth 9 / 5).  An alphabet with fewer than two used symbols gets two one-bit
// codes, as zlib sends them ("no distance codes" included): every code set written is complete.
// In pass 2 a prefix sum over the batch's bit lengths places every token, and each token ORs its bits into the zeroed output.
//
// Everything goes through a policy object P (inflate_core.h has the same arrangement):
//   uint32_t lane(), nlanes()       this caller's share of the data-parallel loops (host: 0 of 1; device: lane of 64)
//   void     sync()                 orders the callers' accesses to the tables
//   uint32_t uni(uint32_t v)        v, known to be the same for all callers
//   uint32_t byte(uint32_t i)       plain byte i, i < n
//   uint32_t load32(uint32_t i)     the little-endian dword at plain byte i, i + 4 <= n
//   void     tab_add / tab_or (uint32_t *at, uint32_t v)    atomic on a word of the tables
//   uint32_t prefix64(uint32_t *a)  a[0, 64) -> its exclusive prefix sums in place; returns the total (called by all, uniform)
//   void     out_or(uint32_t w, uint32_t v)   payload dword w |= v (the payload is zero before the call; atomic)
//   void     out_byte(uint32_t i, uint32_t v) payload byte i = v (the stored form only)
// The core asks for plain bytes below n only and writes payload bytes below n + 5 only (dwords below (n + 8) / 4).  Every loop
// is bounded by n or by a table size; none waits for another lane.
#ifndef TS_DEFLATE_CORE_H
#define TS_DEFLATE_CORE_H

#include <stdint.h>

#include "inflate_core.h"

namespace tsdef {

constexpr uint32_t kMaxBlock = 0xff00u;         // plain bytes per block (BGZF's payload size)
constexpr uint32_t kBatch = 64;
constexpr uint32_t kHashBits = 13, kNoHash = 0xffffu;
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr uint32_t kFarShort = 4096;            // a match of kMinMatch bytes further back than this costs more than its literals
constexpr uint32_t kLitSyms = 286, kDistSyms = 30, kCodeSyms = 19;
constexpr uint32_t kMaxRounds = 20;

// The tables of one block: LDS on the device (27 KB: five waves a CU have room), plain memory on the host.
struct Work {
    uint16_t hash[1u << kHashBits];             // position + 1 of the last insertion, 0 = none
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    uint32_t extra_bits;                        // extra bits of all length and distance symbols
    uint32_t wf[288];                           // the counts a tree is built from (halved on a retry)
    uint32_t nw[576];                           // tree: node weights, leaves first
    uint16_t par[576];
    uint16_t sorted[288];
    uint8_t  dep[576];
    uint32_t nused, deep;
    uint8_t  llen[288], dlen[32], clen[20];
    uint16_t lcode[288], dcode[32], ccode[20];
    uint16_t rle[320];                          // code-length symbols of the header: symbol | extra << 5
    uint32_t nrle, nl, nd, nc, header_bits, dyn_bits;
    uint32_t mask[2];                           // the batch's positions that have a match
    uint16_t mlen[kBatch], mdist[kBatch], mhash[kBatch];
    uint32_t nbits[kBatch];
    uint32_t crc_table[256], crc_part[kBatch], crc_len[kBatch];
};

TS_HD uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32u - kHashBits); }
TS_HD uint32_t log2_floor(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }                 // v > 0

// length 3..258 -> symbol, extra bit count and value
TS_HD void length_symbol(uint32_t len, uint32_t &sym, uint32_t &nx, uint32_t &x) {
    const uint32_t l = len - 3u;
    if (len == 258u) { sym = 285u; nx = 0; x = 0; }
    else if (l < 8u) { sym = 257u + l; nx = 0; x = 0; }
    else { nx = log2_floor(l) - 2u; sym = 261u + 4u * nx + ((l >> nx) & 3u); x = l & ((1u << nx) - 1u); }
}
// distance 1..32768 -> symbol, extra bit count and value
TS_HD void distance_symbol(uint32_t dist, uint32_t &sym, uint32_t &nx, uint32_t &x) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { sym = d; nx = 0; x = 0; }
    else { nx = log2_floor(d) - 1u; sym = 2u * nx + 2u + ((d >> nx) & 1u); x = d & ((1u << nx) - 1u); }
}

// Code lengths of at most `limit` bits for the n symbols counted in freq (n <= 288): 0 for an unused symbol, and at least two
// symbols with a length.  Called by all lanes; lens is complete behind the last sync.
template <class P>
TS_HD void build_lengths(P &p, Work *w, const uint32_t *freq, uint32_t n, uint32_t limit, uint8_t *lens) {
    for (uint32_t s = p.lane(); s < n; s += p.nlanes()) { w->wf[s] = freq[s]; lens[s] = 0; }
    for (uint32_t round = 0; round < kMaxRounds; ++round) {
        if (p.lane() == 0) { w->nused = 0; w->deep = 0; }
        p.sync();
        // rank among the used symbols by (count, symbol)
        for (uint32_t s = p.lane(); s < n; s += p.nlanes()) {
            const uint32_t f = w->wf[s];
            if (f == 0) continue;
            uint32_t rank = 0;
            for (uint32_t t = 0; t < n; ++t) {
                const uint32_t g = w->wf[t];
                rank += (g != 0 && (g < f || (g == f && t < s))) ? 1u : 0u;
            }
            w->sorted[rank] = (uint16_t)s;
            p.tab_add(&w->nused, 1u);
        }
        p.sync();
        const uint32_t used = p.uni(w->nused);
        if (used < 2u) {
            if (p.lane() == 0) {
                const uint32_t s = used ? w->sorted[0] : 0u;
                lens[s] = 1;
                lens[s == 0u ? 1u : 0u] = 1;
            }
            p.sync();
            return;
        }
        if (p.lane() == 0) {
            for (uint32_t i = 0; i < used; ++i) w->nw[i] = w->wf[w->sorted[i]];
            uint32_t leaf = 0, inner = used, next = used;
            for (; next < 2u * used - 1u; ++next) {             // two queues: the leaves ascending, the joined nodes as they were made
                uint32_t sum = 0;
                for (int k = 0; k < 2; ++k) {
                    uint32_t pick;
                    if (leaf < used && (inner >= next || w->nw[leaf] <= w->nw[inner])) pick = leaf++;
                    else pick = inner++;
                    sum += w->nw[pick];
                    w->par[pick] = (uint16_t)next;
                }
                w->nw[next] = sum;
            }
            const uint32_t root = 2u * used - 2u;
            w->dep[root] = 0;
            uint32_t deep = 0;
            for (uint32_t v = root; v-- > 0u;) {
                const uint32_t d = (uint32_t)w->dep[w->par[v]] + 1u;
                w->dep[v] = (uint8_t)d;
                if (v < used) { lens[w->sorted[v]] = (uint8_t)d; if (d > deep) deep = d; }
            }
            w->deep = deep;
        }
        p.sync();
        if (p.uni(w->deep) <= limit) return;
        for (uint32_t s = p.lane(); s < n; s += p.nlanes()) { const uint32_t f = w->wf[s]; w->wf[s] = f ? (f + 1u) >> 1 : 0u; }
        p.sync();
    }
    // (not reached: counts of 1 give a tree of depth <= 9.  Equal lengths that hold every used symbol keep the set decodable.)
    for (uint32_t s = p.lane(); s < n; s += p.nlanes()) lens[s] = freq[s] ? (uint8_t)(n > 32u ? 9u : 5u) : 0u;
    p.sync();
}

// canonical codes, bit-reversed for the LSB-first stream (one lane)
TS_HD void assign_codes(const uint8_t *lens, uint32_t n, uint16_t *codes) {
    uint32_t count[16], next[16];
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++count[lens[s] & 15u];
    count[0] = 0;
    uint32_t code = 0;
    for (uint32_t l = 1; l < 16; ++l) { code = (code + count[l - 1]) << 1; next[l] = code; }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        codes[s] = l ? (uint16_t)tsinf::bit_reverse(next[l]++, l) : (uint16_t)0;
    }
}

// One lane's bit writer for the block header: whole dwords go out as they fill.
template <class P>
struct BitOut {
    P &p;
    uint64_t acc = 0;
    uint32_t cnt = 0, word = 0;
    TS_HD explicit BitOut(P &p_) : p(p_) {}
    TS_HD void put(uint32_t v, uint32_t n) {                    // n <= 16
        acc |= (uint64_t)v << cnt;
        cnt += n;
        if (cnt >= 32u) { p.out_or(word++, (uint32_t)acc); acc >>= 32; cnt -= 32u; }
    }
    TS_HD void finish() { if (cnt) p.out_or(word, (uint32_t)acc); }
};

// how many bytes at `from` and at `at` agree, `most` at the most (from < at, at + most <= n): a word at a time, then bytes
template <class P>
TS_HD uint32_t match_length(P &p, uint32_t from, uint32_t at, uint32_t most) {
    uint32_t len = 0;
    while (len + 4u <= most && p.load32(from + len) == p.load32(at + len)) len += 4u;
    while (len < most && p.byte(from + len) == p.byte(at + len)) ++len;
    return len;
}

// The tokens of batch b, decided: `starts` has the positions (bits) where a match begins, `covered` those inside a token that
// began earlier; every other position below n is a literal.  w->mlen / w->mdist hold the matches.  next: the first position no
// token covers yet (uniform, carried from batch to batch).
template <class P>
TS_HD void find_batch(P &p, Work *w, uint32_t n, uint32_t b, uint32_t &next, uint32_t &rep, uint64_t &starts, uint64_t &covered) {
    const uint32_t base = b * kBatch;
    for (uint32_t k = p.lane(); k < kBatch; k += p.nlanes()) {
        const uint32_t at = base + k;
        uint32_t len = 0, dist = 0, h = kNoHash;
        if (at + 4u <= n) {
            h = hash4(p.load32(at));
            if (at >= next) {
                const uint32_t most = n - at < kMaxMatch ? n - at : kMaxMatch;
                const uint32_t c1 = w->hash[h];                 // (c1 - 1 < base <= at: an earlier batch put it there)
                const uint32_t d1 = c1 != 0u && at - (c1 - 1u) <= kMaxDist ? at - (c1 - 1u) : 0u;
                const uint32_t d2 = rep != 0u && rep <= at && rep != d1 ? rep : 0u;
                const uint32_t l1 = d1 ? match_length(p, at - d1, at, most) : 0u;
                const uint32_t l2 = d2 ? match_length(p, at - d2, at, most) : 0u;
                if (l2 >= l1) { len = l2; dist = d2; } else { len = l1; dist = d1; }
                if (len < kMinMatch || (len == kMinMatch && dist > kFarShort)) len = 0;
            }
        }
        w->mlen[k] = (uint16_t)len;
        w->mdist[k] = (uint16_t)(dist - 1u);
        w->mhash[k] = (uint16_t)h;
        if (len) p.tab_or(&w->mask[k >> 5], 1u << (k & 31u));
    }
    p.sync();
    // the batch's positions go into the table: of those that share a bucket, the highest alone stores
    for (uint32_t k = p.lane(); k < kBatch; k += p.nlanes()) {
        const uint32_t h = w->mhash[k];
        bool mine = h != kNoHash;
        for (uint32_t j = 1; j < kBatch; ++j) if (j > k && w->mhash[j] == h) mine = false;
        if (mine) w->hash[h] = (uint16_t)(base + k + 1u);
    }
    const uint64_t have = (uint64_t)p.uni(w->mask[0]) | (uint64_t)p.uni(w->mask[1]) << 32;
    uint32_t cur = next > base ? next - base : 0u;
    starts = 0;
    covered = cur >= 64u ? ~0ull : (1ull << cur) - 1ull;
    for (uint32_t round = 0; round < kBatch && cur < kBatch; ++round) {
        const uint64_t rest = have >> cur;
        if (rest == 0ull) break;
        const uint32_t j = cur + (uint32_t)__builtin_ctzll(rest);
        const uint32_t len = p.uni(w->mlen[j]);                 // >= kMinMatch
        starts |= 1ull << j;
        rep = (uint32_t)p.uni(w->mdist[j]) + 1u;
        if (j + 1u < kBatch) covered |= (len - 1u >= kBatch - 1u - j ? ~0ull : (1ull << (len - 1u)) - 1ull) << (j + 1u);
        cur = j + len;
    }
    if (cur < kBatch) cur = kBatch;
    next = base + cur;
    p.sync();
    if (p.lane() == 0) { w->mask[0] = 0; w->mask[1] = 0; }
    p.sync();
}

template <class P>
TS_HD void reset_search(P &p, Work *w) {
    for (uint32_t i = p.lane(); i < (1u << kHashBits); i += p.nlanes()) w->hash[i] = 0;
    if (p.lane() == 0) { w->mask[0] = 0; w->mask[1] = 0; }
    p.sync();
}

// plain[0, n) -> the payload through the policy; returns its length in bytes (0: n is above kMaxBlock).
template <class P>
TS_HD uint32_t deflate(P &p, Work *w, uint32_t n) {
    if (n > kMaxBlock) return 0u;
    const uint32_t batches = (n + kBatch - 1u) / kBatch;
    bool stored = n == 0u;
    if (!stored) {
        // ---- pass 1: the symbol counts
        for (uint32_t s = p.lane(); s < 288u; s += p.nlanes()) w->lfreq[s] = s == 256u ? 1u : 0u;
        for (uint32_t s = p.lane(); s < 32u; s += p.nlanes()) { w->dfreq[s] = 0; if (s < 20u) w->cfreq[s] = 0; }
        if (p.lane() == 0) w->extra_bits = 0;
        reset_search(p, w);
        uint32_t next = 0, rep = 0;
        for (uint32_t b = 0; b < batches; ++b) {
            uint64_t starts, covered;
            find_batch(p, w, n, b, next, rep, starts, covered);
            for (uint32_t k = p.lane(); k < kBatch; k += p.nlanes()) {
                const uint32_t at = b * kBatch + k;
                if (at >= n || ((covered >> k) & 1ull)) continue;
                if ((starts >> k) & 1ull) {
                    uint32_t ls, lnx, lx, ds, dnx, dx;
                    length_symbol(w->mlen[k], ls, lnx, lx);
                    distance_symbol((uint32_t)w->mdist[k] + 1u, ds, dnx, dx);
                    p.tab_add(&w->lfreq[ls], 1u);
                    p.tab_add(&w->dfreq[ds], 1u);
                    if (lnx + dnx) p.tab_add(&w->extra_bits, lnx + dnx);
                } else p.tab_add(&w->lfreq[p.byte(at)], 1u);
            }
            p.sync();
        }
        // ---- the three codes and the header's code-length symbols
        build_lengths(p, w, w->lfreq, kLitSyms, 15u, w->llen);
        build_lengths(p, w, w->dfreq, kDistSyms, 15u, w->dlen);
        if (p.lane() == 0) {
            uint32_t nl = kLitSyms, nd = kDistSyms;
            while (nl > 257u && w->llen[nl - 1u] == 0) --nl;
            while (nd > 1u && w->dlen[nd - 1u] == 0) --nd;
            w->nl = nl; w->nd = nd;
            const uint32_t total = nl + nd;
            uint32_t m = 0;
            for (uint32_t i = 0; i < total;) {
                const uint32_t v = i < nl ? w->llen[i] : w->dlen[i - nl];
                uint32_t run = 1;
                while (i + run < total && (i + run < nl ? w->llen[i + run] : w->dlen[i + run - nl]) == v) ++run;
                i += run;
                if (v == 0u) {
                    while (run >= 11u) { const uint32_t r = run < 138u ? run : 138u; w->rle[m++] = (uint16_t)(18u | (r - 11u) << 5); run -= r; }
                    if (run >= 3u) { w->rle[m++] = (uint16_t)(17u | (run - 3u) << 5); run = 0; }
                } else {
                    w->rle[m++] = (uint16_t)v; --run;
                    while (run >= 3u) { const uint32_t r = run < 6u ? run : 6u; w->rle[m++] = (uint16_t)(16u | (r - 3u) << 5); run -= r; }
                }
                for (; run; --run) w->rle[m++] = (uint16_t)v;
            }
            w->nrle = m;
            for (uint32_t i = 0; i < m; ++i) ++w->cfreq[w->rle[i] & 31u];
        }
        p.sync();
        build_lengths(p, w, w->cfreq, kCodeSyms, 7u, w->clen);
        if (p.lane() == 0) {
            assign_codes(w->llen, kLitSyms, w->lcode);
            assign_codes(w->dlen, kDistSyms, w->dcode);
            assign_codes(w->clen, kCodeSyms, w->ccode);
            uint32_t nc = kCodeSyms;
            while (nc > 4u && w->clen[tsinf::code_length_order(nc - 1u)] == 0) --nc;
            w->nc = nc;
            uint32_t bits = 3u + 14u + 3u * nc;
            for (uint32_t i = 0; i < w->nrle; ++i) {
                const uint32_t s = w->rle[i] & 31u;
                bits += (uint32_t)w->clen[s] + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
            }
            w->header_bits = bits;
            bits += w->extra_bits;
            for (uint32_t s = 0; s < kLitSyms; ++s) bits += w->lfreq[s] * (uint32_t)w->llen[s];
            for (uint32_t s = 0; s < kDistSyms; ++s) bits += w->dfreq[s] * (uint32_t)w->dlen[s];
            w->dyn_bits = bits;
        }
        p.sync();
        stored = (p.uni(w->dyn_bits) + 7u) / 8u >= n + 5u;
    }
    if (stored) {
        if (p.lane() == 0) {
            p.out_byte(0, 1u);
            p.out_byte(1, n & 255u); p.out_byte(2, n >> 8);
            p.out_byte(3, ~n & 255u); p.out_byte(4, (~n >> 8) & 255u);
        }
        for (uint32_t i = p.lane(); i < n; i += p.nlanes()) p.out_byte(5u + i, p.byte(i));
        p.sync();
        return n + 5u;
    }
    // ---- pass 2: the header by one lane, then the same tokens again, written
    if (p.lane() == 0) {
        BitOut<P> o(p);
        o.put(5u, 3u);                                          // BFINAL = 1, BTYPE = 2
        o.put(w->nl - 257u, 5u); o.put(w->nd - 1u, 5u); o.put(w->nc - 4u, 4u);
        for (uint32_t i = 0; i < w->nc; ++i) o.put(w->clen[tsinf::code_length_order(i)], 3u);
        for (uint32_t i = 0; i < w->nrle; ++i) {
            const uint32_t s = w->rle[i] & 31u, x = (uint32_t)w->rle[i] >> 5;
            o.put(w->ccode[s], w->clen[s]);
            if (s >= 16u) o.put(x, s == 16u ? 2u : s == 17u ? 3u : 7u);
        }
        o.finish();
    }
    reset_search(p, w);
    uint32_t bitpos = p.uni(w->header_bits), next = 0, rep = 0;
    for (uint32_t b = 0; b < batches; ++b) {
        uint64_t starts, covered;
        find_batch(p, w, n, b, next, rep, starts, covered);
        for (uint32_t k = p.lane(); k < kBatch; k += p.nlanes()) {
            const uint32_t at = b * kBatch + k;
            uint32_t nb = 0;
            if (at < n && !((covered >> k) & 1ull)) {
                if ((starts >> k) & 1ull) {
                    uint32_t ls, lnx, lx, ds, dnx, dx;
                    length_symbol(w->mlen[k], ls, lnx, lx);
                    distance_symbol((uint32_t)w->mdist[k] + 1u, ds, dnx, dx);
                    nb = (uint32_t)w->llen[ls] + lnx + (uint32_t)w->dlen[ds] + dnx;
                } else nb = w->llen[p.byte(at)];
            }
            w->nbits[k] = nb;
        }
        p.sync();
        const uint32_t total = p.prefix64(w->nbits);
        for (uint32_t k = p.lane(); k < kBatch; k += p.nlanes()) {
            const uint32_t at = b * kBatch + k;
            if (at >= n || ((covered >> k) & 1ull)) continue;
            uint64_t bits;
            if ((starts >> k) & 1ull) {
                uint32_t ls, lnx, lx, ds, dnx, dx;
                length_symbol(w->mlen[k], ls, lnx, lx);
                distance_symbol((uint32_t)w->mdist[k] + 1u, ds, dnx, dx);
                uint32_t sh = w->llen[ls];
                bits = (uint64_t)w->lcode[ls] | (uint64_t)lx << sh;
                sh += lnx;
                bits |= (uint64_t)w->dcode[ds] << sh;
                sh += w->dlen[ds];
                bits |= (uint64_t)dx << sh;
            } else bits = w->lcode[p.byte(at)];
            const uint32_t bp = bitpos + w->nbits[k], sh = bp & 31u;
            const uint64_t lo = bits << sh;
            const uint32_t hi = sh ? (uint32_t)(bits >> (64u - sh)) : 0u;
            if ((uint32_t)lo) p.out_or(bp >> 5, (uint32_t)lo);
            if ((uint32_t)(lo >> 32)) p.out_or((bp >> 5) + 1u, (uint32_t)(lo >> 32));
            if (hi) p.out_or((bp >> 5) + 2u, hi);
        }
        bitpos += total;
        p.sync();
    }
    if (p.lane() == 0) {                                        // the end-of-block symbol
        const uint32_t sh = bitpos & 31u;
        const uint64_t v = (uint64_t)w->lcode[256] << sh;
        if ((uint32_t)v) p.out_or(bitpos >> 5, (uint32_t)v);
        if ((uint32_t)(v >> 32)) p.out_or((bitpos >> 5) + 1u, (uint32_t)(v >> 32));
    }
    bitpos += p.uni(w->llen[256]);
    p.sync();
    return (bitpos + 7u) / 8u;                                  // == (dyn_bits + 7) / 8
}

// CRC32 of plain[0, n): 64 consecutive slices (whole dwords but the last), joined by inflate_core.h's crc_combine.
template <class P>
TS_HD uint32_t crc32(P &p, Work *w, uint32_t n) {
    for (uint32_t i = p.lane(); i < 256u; i += p.nlanes()) w->crc_table[i] = tsinf::crc_table_entry(i);
    p.sync();
    const uint32_t slice = ((n + 63u) / 64u + 3u) & ~3u;
    const uint32_t *t = w->crc_table;
    for (uint32_t k = p.lane(); k < kBatch; k += p.nlanes()) {
        const uint32_t a = k * slice < n ? k * slice : n, e = a + slice < n ? a + slice : n;
        uint32_t c = 0xffffffffu, i = a;
        for (; i + 4u <= e; i += 4u) {
            c ^= p.load32(i);
            for (int r = 0; r < 4; ++r) c = t[c & 255u] ^ (c >> 8);
        }
        for (; i < e; ++i) c = t[(c ^ p.byte(i)) & 255u] ^ (c >> 8);
        w->crc_part[k] = c ^ 0xffffffffu;                       // (an empty slice: 0, the CRC of nothing)
        w->crc_len[k] = e - a;
    }
    p.sync();
    for (uint32_t s = 1; s < kBatch; s *= 2u) {
        for (uint32_t k = p.lane(); k < kBatch; k += p.nlanes())
            if ((k & (2u * s - 1u)) == 0u) {
                w->crc_part[k] = tsinf::crc_combine(w->crc_part[k], w->crc_part[k + s], w->crc_len[k + s]);
                w->crc_len[k] += w->crc_len[k + s];
            }
        p.sync();
    }
    return p.uni(w->crc_part[0]);
}

}  // namespace tsdef
#endif
