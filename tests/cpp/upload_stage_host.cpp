// upload_stage_host.cpp — the layer between the packing primitives and the DMA of the host upload (upload_stage_core.h), on the
// host under ASan + UBSan, and its pooled cases under TSan.  Built by tests/test_upload_stage_cpu.py together with pack.cpp.
//
// The program builds small chunks out of plain, FASTA-text and packed pieces, stages them through the functions the library's
// driver calls, and decodes what lands in the slot by unpack.hip's rule — position x at bits 2 (x & 3) of byte x >> 2, letters
// ACTG by code, 'N' over the invalid runs.  The statement it compares with, a byte at a time: a position covered by a piece
// decodes to the piece's base (case-folded when the context folds) if that is A, C, G or T, else to 'N'.
// Beyond equality: the runs ascend, are disjoint and lie inside pieces, and where codes are copied a run goes on in the one it abuts; worker t writes only the bytes [cut[t] >> 2,
// (cut[t + 1] + 3) >> 2) of the slot — it is handed a heap block of exactly those bytes — and no two workers share a byte; the
// tail zeroes the bytes behind the codes up to the slot's end, a heap block of exactly packed_bytes(P) + 8; the eight
// ts_upload_stats increments equal a count made from a position-by-position map of the chunk.
// Every source — bases, text, codes — is a heap block of exactly its size.
//
//   upload_stage_host packed SEED CASES SHARD SHARDS   chunks on the packed route, 1 to 8 workers, run one after the other
//   upload_stage_host pooled SEED CASES                the same chunks with StagePool's threads over one shared slot
//   upload_stage_host ascii SEED CASES                 the ASCII route's three forms
//   upload_stage_host extent SEED CASES                piece lists and the chunks chunk_extent makes of them, for the caller to judge
//   upload_stage_host normalise                        a call's pieces: device aside, cut at the limit, text refused
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/upload_stage_core.h"

namespace {

using tsstage::UpPiece;

[[noreturn]] void fail(const std::string &what, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void fail(const std::string &what, const char *fmt, ...) {
    fprintf(stderr, "FAILED %s: ", what.c_str());
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    exit(1);
}

// a heap block of exactly n bytes (n == 0: a block nobody may touch, handed out past its end)
struct Exact {
    unsigned char *block, *p;
    explicit Exact(size_t n, int fill = 0xEE) : block((unsigned char *)malloc(n ? n : 1)), p(block + (n ? 0 : 1)) { if (n) memset(block, fill, n); }
    ~Exact() { free(block); }
    Exact(const Exact &) = delete;
};

// ---------------------------------------------------------------------------------------------- the statement
bool is_acgt(unsigned char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
unsigned char decoded(unsigned char base, bool fold) {            // what a base of an ASCII piece reads as on the device
    const unsigned char c = fold ? base & 0xDF : base;
    return is_acgt(c) ? c : 'N';
}
unsigned code_of_letter(unsigned char c) { return (c >> 1) & 3u; }      // A 0, C 1, T 2, G 3
bool is_line_end(const std::string &t, size_t i) { return t[i] == '\n' || (t[i] == '\r' && (i + 1 == t.size() || t[i + 1] == '\n')); }

enum Format { PLAIN = 0, TEXT = 1, PACKED = 2 };

struct Chunk {                                                    // pieces of one chunk and what each position of it must decode to
    std::vector<UpPiece> pieces;
    std::vector<int> format;
    std::vector<std::vector<unsigned char>> raw;                  // ASCII pieces: the bases as they lie at the source (what they hold)
    std::vector<std::vector<unsigned char>> expect;               // per piece: the decoded letter of each base it holds
    std::deque<ts_packed_seq> seqs;
    std::deque<std::vector<ts_packed_run>> seq_runs;
    std::vector<std::unique_ptr<Exact>> heap;
    bool fold = false, short_text = false;
    uint64_t end() const { return pieces.empty() ? 0 : pieces.back().off + pieces.back().len; }
    unsigned char *keep(const void *src, size_t n) {
        heap.emplace_back(new Exact(n));
        if (n) memcpy(heap.back()->p, src, n);
        return heap.back()->p;
    }
};

std::string random_bases(std::mt19937_64 &rng, size_t n) {
    const std::string alpha = rng() % 3 ? "ACGT" : "ACGTacgtNnRY";
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back(alpha[rng() % alpha.size()]);
    for (int q = 0; q < 3 && n; ++q) {                            // N runs: at the ends (they abut the neighbours') and anywhere
        if (rng() % 2) continue;
        const size_t ln = 1 + rng() % 9, a = q == 0 ? 0 : q == 1 ? (n > ln ? n - ln : 0) : rng() % n;
        for (size_t i = a; i < a + ln && i < n; ++i) s[i] = "Nn"[rng() & 1];
    }
    return s;
}

void add_plain(Chunk &c, uint64_t off, size_t n, std::mt19937_64 &rng) {
    const std::string s = random_bases(rng, n);
    c.pieces.push_back({off, (const char *)c.keep(s.data(), n), n, 0});
    c.format.push_back(PLAIN);
    c.raw.emplace_back(s.begin(), s.end());
    c.expect.emplace_back();
    for (unsigned char b : s) c.expect.back().push_back(decoded(b, c.fold));
}

// about n bases as FASTA body text in the four line-end styles of tests/textpieces.py — LF, CRLF, a mix, and a mix with blank lines,
// CR CR LF and lone CRs inside lines (bases, invalid ones) — that begins inside a line, at a line's start, with the LF of a CRLF
// cut in two, or with a blank line, and ends in a base, LF, CRLF or CR (a line end at the very end: the CR of a CRLF cut in two).
// The piece holds what the statement reads out of its text; it declares `extra` bases more.
void add_text(Chunk &c, uint64_t off, size_t n, size_t extra, std::mt19937_64 &rng) {
    static const size_t widths[] = {1, 2, 31, 32, 33, 60, 63, 64, 65, 70, 80};
    const std::string seq = random_bases(rng, n);
    const int style = (int)(rng() % 4);
    size_t width = widths[rng() % 11];
    if (width <= 2 && n > 300) width = widths[2 + rng() % 9];
    std::string t;
    switch (rng() % 4) { case 0: t = "\n"; break; case 1: t = "\r\n"; break; default: break; }
    size_t in_line = 0, limit = 1 + rng() % width;
    for (size_t i = 0; i < seq.size(); ++i) {
        t.push_back(seq[i]);
        if (style == 3 && rng() % 97 == 0 && i + 1 < seq.size()) { t.push_back('\r'); t.push_back(seq[i]); }      // a lone CR inside a line
        if (++in_line < limit || i + 1 == seq.size()) continue;
        in_line = 0; limit = width;
        const bool crlf = style == 1 || (style >= 2 && (rng() & 1));
        if (style == 3 && rng() % 29 == 0) t += "\r\r\n";
        else t += crlf ? "\r\n" : "\n";
        if (style == 3 && rng() % 23 == 0) t += crlf ? "\r\n" : "\n";
    }
    switch (rng() % 4) { case 0: t += "\r"; break; case 1: t += "\r\n"; break; case 2: t += "\n"; break; default: break; }
    std::vector<unsigned char> bases;
    for (size_t i = 0; i < t.size(); ++i) if (!is_line_end(t, i)) bases.push_back((unsigned char)t[i]);
    if (bases.empty()) { add_plain(c, off, n ? n : 1, rng); return; }
    c.pieces.push_back({off, (const char *)c.keep(t.data(), t.size()), bases.size() + extra, t.size()});
    c.format.push_back(TEXT);
    c.expect.emplace_back();
    for (unsigned char b : bases) c.expect.back().push_back(decoded(b, c.fold));
    c.raw.push_back(std::move(bases));
    if (extra) c.short_text = true;
}

// n bases as codes [first, first + n) of a packed sequence with a few bases behind them; invalid runs inside, at both ends of the
// slice (they abut the neighbour's), across its start (when first > 0) and across its end; now and then a run given as two that
// abut, and codes other than 0 under a run (the device writes 'N' over them)
void add_packed(Chunk &c, uint64_t off, size_t n, uint64_t first, std::mt19937_64 &rng) {
    const size_t total = (size_t)first + n + rng() % 7;
    std::vector<unsigned char> letter(total);
    std::vector<bool> bad(total, false);
    for (size_t i = 0; i < total; ++i) letter[i] = "ACGT"[rng() % 4];
    auto mark = [&](size_t a, size_t ln) { for (size_t i = a; i < a + ln && i < total; ++i) bad[i] = true; };
    if (rng() % 2) mark(first, 1 + rng() % 5);
    if (rng() % 2) mark(first + n - std::min<size_t>(n, 1 + rng() % 5), 5);
    if (first && rng() % 2) mark(first - std::min<size_t>(first, 1 + rng() % 3), 2 + rng() % 4);
    if (rng() % 2) mark(first + n - 1, 2 + rng() % 3);
    for (int q = (int)(rng() % 4); q > 0; --q) mark(rng() % total, 1 + rng() % (rng() % 5 ? 9 : 40000));
    std::vector<unsigned char> codes((total + 3) / 4, 0);
    c.seq_runs.emplace_back();
    std::vector<ts_packed_run> &runs = c.seq_runs.back();
    const bool dirty = rng() % 2;
    for (size_t i = 0; i < total; ++i) {
        const unsigned code = bad[i] ? (dirty ? (unsigned)(rng() % 4) : 0u) : code_of_letter(letter[i]);
        codes[i >> 2] |= (unsigned char)(code << (2 * (i & 3)));
        if (!bad[i]) continue;
        if (!runs.empty() && runs.back().start + runs.back().len == i && rng() % 8) ++runs.back().len;
        else runs.push_back({i, 1});
    }
    c.seqs.push_back({c.keep(codes.data(), codes.size()), runs.empty() && rng() % 2 ? nullptr : (const ts_packed_run *)c.keep(runs.data(), runs.size() * sizeof(ts_packed_run)),
                      runs.size()});
    UpPiece pc{off, nullptr, n, 0};
    pc.packed = &c.seqs.back();
    pc.packed_first = first;
    c.pieces.push_back(pc);
    c.format.push_back(PACKED);
    c.raw.emplace_back();
    c.expect.emplace_back();
    for (size_t i = 0; i < n; ++i) c.expect.back().push_back(bad[first + i] ? 'N' : letter[first + i]);
}

// Chunks of 1 to 5 x 16384 + 63 positions: the first base at every interesting place within 64, pieces of one format or of all
// three (the seams of every ordered pair fall inside blocks), lengths of 1 to 9, around 4096 and 16384 and anything up to three
// blocks, gaps of 0, 1, 15 and 4097, pieces that end exactly on a multiple of 4096 or 16384 positions of the chunk.
// formats: bit per Format.  exact_P != 0: one plain or packed piece that makes a chunk of exactly that many positions.
void make_chunk(Chunk &c, std::mt19937_64 &rng, unsigned formats, bool allow_short, uint64_t exact_P = 0) {
    static const uint64_t leads[] = {0, 1, 3, 4, 15, 16, 63};
    uint64_t lead = leads[rng() % 7];
    while (exact_P && lead >= exact_P) lead = leads[rng() % 7];
    const uint64_t c0a = 64 * (rng() % 100000), c0 = c0a + lead;
    c.fold = rng() & 1;
    static const uint64_t firsts[] = {0, 0, 1, 2, 3, 4, 5, 64, 16385, 99999};
    if (exact_P) {
        if (formats & (1u << PACKED)) add_packed(c, c0, exact_P - lead, firsts[rng() % 10], rng); else add_plain(c, c0, exact_P - lead, rng);
        return;
    }
    const uint64_t maxP = 5 * 16384 + 63;
    const uint64_t target = std::max(c0 + 1, c0a + (rng() % 4 == 0 ? 1 + rng() % 200 : rng() % 3 == 0 ? maxP : 1 + rng() % maxP));
    uint64_t at = c0;
    std::vector<int> fm;
    for (int f = 0; f < 3; ++f) if (formats & (1u << f)) fm.push_back(f);
    bool short_given = false;
    while (at < target) {
        uint64_t left = target - at, n;
        switch (rng() % 8) {
        case 0: n = 1 + rng() % 9; break;
        case 1: n = 4090 + rng() % 12; break;
        case 2: n = 16380 + rng() % 8; break;
        case 3: { const uint64_t g = rng() & 1 ? 4096 : 16384; n = g - (at - c0a) % g; break; }      // ends on a cut / a block boundary
        case 4: n = 1 + rng() % 300; break;
        default: n = 1 + rng() % (3 * 16384); break;
        }
        n = std::min(n, left);
        const int f = fm[rng() % fm.size()];
        if (f == TEXT) {
            const bool make_short = allow_short && !short_given && rng() % 4 == 0;
            add_text(c, at, n, make_short ? 1 + rng() % 40 : 0, rng);
            short_given |= make_short;
            if (c.end() - c0a > maxP) {                               // (a text holds what its lines hold: over the limit, try the rest as plain bases)
                c.pieces.pop_back(); c.format.pop_back(); c.raw.pop_back(); c.expect.pop_back();
                if (make_short) { short_given = false; c.short_text = false; }
                add_plain(c, at, n, rng);
            }
        } else if (f == PACKED) add_packed(c, at, n, firsts[rng() % 10], rng);
        else add_plain(c, at, n, rng);
        static const uint64_t gaps[] = {0, 0, 0, 0, 1, 15, 4097};
        at = c.end() + gaps[rng() % 7];
    }
}

// ---------------------------------------------------------------------------------------------- the packed route
struct Tally {
    uint64_t chunks = 0, kinds[4] = {0, 0, 0, 0}, phase[4] = {0, 0, 0, 0}, short_text = 0, runs = 0, n_over_block = 0, n_over_cut = 0,
             seams[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, several_workers = 0, off_boundary = 0, ends_on_block = 0, ends_on_cut = 0, n_abutting = 0, merged = 0;
};

void check_packed(const Chunk &c, unsigned nt, tsstage::StagePool *pool, Tally &ty, const std::string &what) {
    const size_t np = c.pieces.size();
    tsstage::PackedChunk pk(c.pieces.data(), 0, np, nt);
    const uint64_t c0 = c.pieces[0].off, c0a = c0 & ~63ull, P = c.end() - c0a;
    if (pk.c0 != c0 || pk.c0a != c0a || pk.P != P) fail(what, "chunk base %llu / %llu, %llu positions", (unsigned long long)pk.c0, (unsigned long long)pk.c0a, (unsigned long long)pk.P);
    const std::vector<uint64_t> &cut = pk.cut;
    if (cut.size() != nt + 1 || cut[0] != 0 || cut[nt] != P) fail(what, "the cuts do not run from 0 to P");
    uint64_t prev_hi = 0;
    for (unsigned t = 0; t < nt; ++t) {                               // no byte of the slot belongs to two workers
        if (cut[t + 1] < cut[t]) fail(what, "cut %u descends", t + 1);
        if (cut[t + 1] == cut[t]) continue;
        if ((cut[t] >> 2) < prev_hi) fail(what, "worker %u begins in a byte of the worker before it", t);
        prev_hi = (cut[t + 1] + 3) >> 2;
    }
    // the statement, position by position: who owns it and what it decodes to (0: nobody reads it)
    std::vector<int> owner(P, -1);
    std::vector<unsigned char> want(P, 0);
    for (size_t p = 0; p < np; ++p)
        for (uint64_t b = 0; b < c.pieces[p].len; ++b) {
            const uint64_t x = c.pieces[p].off - c0a + b;
            owner[x] = (int)p;
            want[x] = b < c.expect[p].size() ? c.expect[p][b] : 0;          // (declared, not held: a short text)
        }
    // stage
    const uint64_t pbytes = tsstage::packed_bytes(P);
    Exact slot(pbytes + 8);
    bool ok = true;
    if (pool) {
        std::atomic<int> bad{0};
        pool->run(nt, [&](unsigned t) { if (!pk.pack(t, (char *)slot.p, c.fold)) bad.store(1); });
        ok = !bad.load();
    } else {
        for (unsigned t = 0; t < nt; ++t) {
            const uint64_t lo = cut[t] >> 2, hi = cut[t + 1] > cut[t] ? (cut[t + 1] + 3) >> 2 : lo;
            Exact mine(hi - lo);                                       // exactly the worker's bytes, addressed as the slot's
            ok &= pk.pack(t, (char *)((uintptr_t)mine.p - lo), c.fold);
            memcpy(slot.p + lo, mine.p, hi - lo);
        }
    }
    if (ok == c.short_text) fail(what, "short text %s", ok ? "not reported" : "reported where every text holds what it declares");
    const size_t nruns = pk.n_runs();
    Exact hr_block(nruns * sizeof(ts::InvalidRun));
    ts::InvalidRun *hr = (ts::InvalidRun *)hr_block.p;
    uint64_t add[8];
    memset(add, 0xEE, sizeof add);
    pk.finish((char *)slot.p, hr, pool != nullptr, add);
    for (uint64_t b = (P + 3) >> 2; b < pbytes + 8; ++b) if (slot.p[b]) fail(what, "padding byte %llu of %llu is not zero", (unsigned long long)b, (unsigned long long)(pbytes + 8));
    // decode
    std::vector<unsigned char> got(P);
    for (uint64_t x = 0; x < P; ++x) got[x] = "ACTG"[(slot.p[x >> 2] >> (2 * (x & 3))) & 3];
    std::vector<int32_t> run_of(P, -1);
    uint64_t prev_end = 0;
    for (size_t r = 0; r < nruns; ++r) {
        const uint64_t a = hr[r].start, z = a + hr[r].len;
        if (!hr[r].len || a < prev_end || z > P) fail(what, "run %zu {%u, %u} does not ascend behind %llu inside %llu positions", r, hr[r].start, hr[r].len, (unsigned long long)prev_end, (unsigned long long)P);
        if (a == prev_end && r) ++ty.n_abutting;
        for (uint64_t x = a; x < z; ++x) {
            if (owner[x] < 0) fail(what, "run %zu {%u, %u} covers position %llu, which no piece holds (first base at %llu)", r, hr[r].start, hr[r].len, (unsigned long long)x, (unsigned long long)(c0 - c0a));
            got[x] = 'N';
            run_of[x] = (int32_t)r;
        }
        prev_end = z;
    }
    ty.runs += nruns;
    for (uint64_t x = 0; x < P; ++x)
        if (want[x] && got[x] != want[x])
            fail(what, "position %llu (piece %d, format %d, base %llu of it) decodes to %c, expected %c", (unsigned long long)x, owner[x], c.format[owner[x]],
                 (unsigned long long)(c0a + x - c.pieces[owner[x]].off), got[x], want[x]);
    // the counters, from the map
    uint64_t kinds[4] = {0, 0, 0, 0};
    unsigned workers = 0;
    for (unsigned t = 0; t < nt; ++t) {
        if (cut[t + 1] > cut[t]) ++workers;
        for (uint64_t a = cut[t]; a < cut[t + 1]; a += 16384) {
            const uint64_t z = std::min(cut[t + 1], a + 16384);
            bool gap = false, all_packed = true, one = true;
            int first = -1;
            for (uint64_t x = a; x < z; ++x) {
                if (owner[x] < 0) { gap = true; continue; }
                if (first < 0) first = owner[x];
                if (owner[x] != first) one = false;
                if (c.format[owner[x]] != PACKED) all_packed = false;
            }
            const int kind = first >= 0 && one && !gap && c.format[first] != PACKED ? c.format[first] : first >= 0 && all_packed ? 2 : 3;
            ++kinds[kind];
            // copied codes: a run that begins where the worker's last one ends goes on in it, across a seam and across a block's start
            for (uint64_t x = std::max(a, cut[t] + 1); kind == 2 && x < z; ++x) {
                if (want[x] != 'N' || want[x - 1] != 'N') continue;
                if (run_of[x] != run_of[x - 1]) fail(what, "the invalid positions %llu and %llu lie in two runs", (unsigned long long)(x - 1), (unsigned long long)x);
                if (x == a || owner[x] != owner[x - 1]) ++ty.merged;
            }
            if (a > cut[t] && want[a] == 'N' && want[a - 1] == 'N' && owner[a] == owner[a - 1] && c.format[owner[a]] == PACKED) ++ty.n_over_block;
        }
        if (t && cut[t] < P && cut[t] > cut[t - 1] && want[cut[t]] == 'N' && want[cut[t] - 1] == 'N' && owner[cut[t]] == owner[cut[t] - 1] && c.format[owner[cut[t]]] == PACKED) ++ty.n_over_cut;
    }
    const uint64_t expect_add[8] = {1, 0, kinds[0], kinds[1], kinds[2], kinds[3], workers > 1 && pool ? 1u : 0u, c0 != c0a ? 1u : 0u};
    for (int q = 0; q < 8; ++q)
        if (add[q] != expect_add[q]) fail(what, "ts_upload_stats increment %d is %llu, the map says %llu", q, (unsigned long long)add[q], (unsigned long long)expect_add[q]);
    ++ty.chunks;
    for (int q = 0; q < 4; ++q) ty.kinds[q] += kinds[q];
    ty.several_workers += workers > 1;
    ty.off_boundary += c0 != c0a;
    ty.short_text += c.short_text;
    if (nt == 1) {
        for (size_t p = 0; p < np; ++p) {
            if (c.format[p] == PACKED) ++ty.phase[((c.pieces[p].off - c0a) ^ c.pieces[p].packed_first) & 3];
            const uint64_t e = c.pieces[p].off + c.pieces[p].len - c0a;
            ty.ends_on_block += e % 16384 == 0;
            ty.ends_on_cut += e % 4096 == 0;
            if (p && (c.pieces[p].off - c0a) / 16384 == (c.pieces[p - 1].off + c.pieces[p - 1].len - 1 - c0a) / 16384) ++ty.seams[3 * c.format[p - 1] + c.format[p]];
        }
    }
}

unsigned formats_of(uint64_t n) {                                    // plain only, text only, packed only, and all three twice as often
    static const unsigned sets[] = {1u << PLAIN, 1u << TEXT, 1u << PACKED, 7u, 7u};
    return sets[n % 5];
}

int run_packed(uint64_t seed, size_t cases, uint64_t shard, uint64_t shards, bool pooled) {
    Tally ty;
    std::unique_ptr<tsstage::StagePool> pool(pooled ? new tsstage::StagePool(8) : nullptr);
    for (size_t n = shard; n < cases; n += shards) {
        std::mt19937_64 rng(seed * 1000003ull + n);
        Chunk c;
        static const uint64_t exact[] = {1, 2, 3, 4, 5, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 5 * 16384 + 63};
        if (n < 2 * 14) {
            make_chunk(c, rng, n % 2 ? 1u << PACKED : 1u << PLAIN, false, exact[n / 2]);
        } else make_chunk(c, rng, formats_of(n), n % 3 == 0);
        for (unsigned nt = 1; nt <= 8; ++nt)
            check_packed(c, nt, pool.get(), ty, "case " + std::to_string(n) + " workers " + std::to_string(nt));
    }
    printf("%s chunks %llu plain %llu text %llu copied %llu mixed %llu phase0 %llu phase1 %llu phase2 %llu phase3 %llu short_text %llu runs %llu "
           "n_over_block %llu n_over_cut %llu merged_runs %llu abutting_runs %llu several_workers %llu off_boundary %llu ends_on_block %llu ends_on_cut %llu",
           pooled ? "pooled" : "packed", (unsigned long long)ty.chunks, (unsigned long long)ty.kinds[0], (unsigned long long)ty.kinds[1], (unsigned long long)ty.kinds[2],
           (unsigned long long)ty.kinds[3], (unsigned long long)ty.phase[0], (unsigned long long)ty.phase[1], (unsigned long long)ty.phase[2], (unsigned long long)ty.phase[3],
           (unsigned long long)ty.short_text, (unsigned long long)ty.runs, (unsigned long long)ty.n_over_block, (unsigned long long)ty.n_over_cut, (unsigned long long)ty.merged, (unsigned long long)ty.n_abutting,
           (unsigned long long)ty.several_workers, (unsigned long long)ty.off_boundary, (unsigned long long)ty.ends_on_block, (unsigned long long)ty.ends_on_cut);
    for (int q = 0; q < 9; ++q) printf(" seam%d%d %llu", q / 3, q % 3, (unsigned long long)ty.seams[q]);
    printf("\n");
    return 0;
}

// ---------------------------------------------------------------------------------------------- the ASCII route
// dst: a heap block of exactly the bytes from the chunk's first base to its last.  Covered bytes are the pieces' bases as they
// lie at the source (no folding, nothing replaced), bytes between pieces are not written.
int run_ascii(uint64_t seed, size_t cases) {
    tsstage::StagePool pool(8);
    uint64_t checked = 0, shorts = 0, forms[3] = {0, 0, 0};
    for (size_t n = 0; n < cases; ++n) {
        std::mt19937_64 rng(seed * 7919ull + n);
        Chunk c;
        const bool text = n % 2;
        make_chunk(c, rng, text ? (n % 4 == 1 ? 1u << TEXT : 3u) : 1u << PLAIN, n % 3 == 0);
        const UpPiece *pieces = c.pieces.data();
        const size_t np = c.pieces.size();
        const uint64_t c0 = pieces[0].off, size = c.end() - c0;
        uint64_t bytes = 0;
        for (const UpPiece &pc : c.pieces) bytes += pc.len;
        for (unsigned nt = 1; nt <= 8; ++nt) {
            for (int form = 0; form < 3; ++form) {
                if (form == 2 && text) continue;                           // (equal byte shares: plain pieces only)
                const std::string what = "ascii case " + std::to_string(n) + " workers " + std::to_string(nt) + " form " + std::to_string(form);
                Exact dst(size);
                std::atomic<int> bad{0};
                std::atomic<size_t> next{0};
                if (form == 0) { if (nt > 1) continue; if (!tsstage::ascii_single(pieces, 0, np, c0, (char *)dst.p)) bad.store(1); }
                else if (form == 1) pool.run(nt, [&](unsigned) { if (!tsstage::ascii_whole_pieces(pieces, np, c0, (char *)dst.p, next)) bad.store(1); });
                else pool.run(nt, [&](unsigned t) { tsstage::ascii_share(pieces, 0, np, c0, (char *)dst.p, bytes, nt, t); });
                if ((bad.load() != 0) != c.short_text) fail(what, "short text %s", bad.load() ? "reported where every text holds what it declares" : "not reported");
                std::vector<bool> covered(size, false);
                for (size_t p = 0; p < np; ++p)
                    for (uint64_t b = 0; b < pieces[p].len; ++b) {
                        const uint64_t x = pieces[p].off - c0 + b;
                        covered[x] = true;
                        if (b < c.raw[p].size() && dst.p[x] != c.raw[p][b]) fail(what, "byte %llu (piece %zu, base %llu) is %02x, expected %02x", (unsigned long long)x, p, (unsigned long long)b, dst.p[x], c.raw[p][b]);
                    }
                for (uint64_t x = 0; x < size; ++x) if (!covered[x] && dst.p[x] != 0xEE) fail(what, "byte %llu between pieces was written", (unsigned long long)x);
                ++checked; ++forms[form];
                shorts += c.short_text;
            }
        }
    }
    printf("ascii checked %llu single %llu whole_pieces %llu shares %llu short_text %llu\n", (unsigned long long)checked, (unsigned long long)forms[0],
           (unsigned long long)forms[1], (unsigned long long)forms[2], (unsigned long long)shorts);
    return 0;
}

// ---------------------------------------------------------------------------------------------- chunk extent
// one line per piece list: "limit L gap G pieces off len ... chunks end bytes ..." — the caller restates the two rules
int run_extent(uint64_t seed, size_t cases) {
    std::mt19937_64 rng(seed);
    for (size_t n = 0; n < cases; ++n) {
        const uint64_t limit = 1 + rng() % 64, gap = rng() % 9;
        std::vector<UpPiece> pieces;
        uint64_t at = rng() % 100;
        for (size_t k = 1 + rng() % 12; k > 0; --k) {
            const uint64_t len = rng() % 5 == 0 ? limit - std::min(limit - 1, rng() % 3) : 1 + rng() % (rng() % 6 == 0 ? 2 * limit : limit / 2 + 1);
            pieces.push_back({at, nullptr, len, 0});
            at += len + (rng() % 3 == 0 ? gap + rng() % 3 : rng() % (gap + 1));          // gaps at, just above and below the rule's
        }
        printf("limit %llu gap %llu pieces", (unsigned long long)limit, (unsigned long long)gap);
        for (const UpPiece &pc : pieces) printf(" %llu %llu", (unsigned long long)pc.off, (unsigned long long)pc.len);
        printf(" chunks");
        for (size_t i = 0; i < pieces.size();) {
            const tsstage::Extent e = tsstage::chunk_extent(pieces.data(), pieces.size(), i, limit, gap);
            if (e.end <= i || e.end > pieces.size()) fail("chunk_extent", "a chunk from piece %zu to %zu of %zu", i, e.end, pieces.size());
            printf(" %zu %llu", e.end, (unsigned long long)e.bytes);
            i = e.end;
        }
        printf("\n");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- a call's pieces
int run_normalise() {
    const uint64_t limit = 10;
    static const char src[64] = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACG";
    const ts_packed_seq ps{(const uint8_t *)src, nullptr, 0};
    std::vector<UpPiece> in;
    in.push_back({100, src, 25, 0});                                       // plain: 10 + 10 + 5
    UpPiece dev{130, src, 40, 0}; dev.device = true;
    in.push_back(dev);                                                     // device: aside, whole
    UpPiece pk{200, nullptr, 20, 0}; pk.packed = &ps; pk.packed_first = 3;
    in.push_back(pk);                                                      // packed: 10 + 10, an exact multiple
    in.push_back({300, src, 10, 14});                                      // text at the limit: whole
    in.push_back({400, src, 1, 0});
    tsstage::CallPieces out;
    if (tsstage::normalise_pieces(in, limit, out) != tsstage::Refused::Nothing) fail("normalise", "refused");
    struct Want { uint64_t off, len, first; const char *src; uint64_t text_len; bool packed; };
    const Want want[] = {{100, 10, 0, src, 0, false}, {110, 10, 0, src + 10, 0, false}, {120, 5, 0, src + 20, 0, false}, {200, 10, 3, nullptr, 0, true},
                         {210, 10, 13, nullptr, 0, true}, {300, 10, 0, src, 14, false}, {400, 1, 0, src, 0, false}};
    if (out.host.size() != 7) fail("normalise", "%zu host pieces, 7 expected", out.host.size());
    for (size_t i = 0; i < 7; ++i) {
        const UpPiece &g = out.host[i];
        if (g.off != want[i].off || g.len != want[i].len || g.packed_first != want[i].first || g.src != want[i].src || g.text_len != want[i].text_len ||
            (g.packed != nullptr) != want[i].packed || g.device) fail("normalise", "host piece %zu differs", i);
    }
    if (out.on_device.size() != 1 || out.on_device[0].off != 130 || out.on_device[0].len != 40 || !out.on_device[0].device) fail("normalise", "the device piece");
    if (!out.any_text || !out.any_packed || out.total_bytes != 25 + 20 + 10 + 1) fail("normalise", "flags or total %llu", (unsigned long long)out.total_bytes);
    tsstage::CallPieces plain_only;
    if (tsstage::normalise_pieces({{0, src, 30, 0}}, limit, plain_only) != tsstage::Refused::Nothing || plain_only.any_text || plain_only.any_packed || plain_only.host.size() != 3)
        fail("normalise", "plain only");
    tsstage::CallPieces refused;
    if (tsstage::normalise_pieces({{0, src, 11, 15}}, limit, refused) != tsstage::Refused::TextPieceTooLong) fail("normalise", "a text piece over the limit was taken");
    printf("normalise ok 1\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "packed")) return run_packed((uint64_t)atoll(argv[2]), (size_t)atoll(argv[3]), (uint64_t)atoll(argv[4]), (uint64_t)atoll(argv[5]), false);
    if (argc == 4 && !strcmp(argv[1], "pooled")) return run_packed((uint64_t)atoll(argv[2]), (size_t)atoll(argv[3]), 0, 1, true);
    if (argc == 4 && !strcmp(argv[1], "ascii")) return run_ascii((uint64_t)atoll(argv[2]), (size_t)atoll(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "extent")) return run_extent((uint64_t)atoll(argv[2]), (size_t)atoll(argv[3]));
    if (argc == 2 && !strcmp(argv[1], "normalise")) return run_normalise();
    fprintf(stderr, "usage: upload_stage_host packed SEED CASES SHARD SHARDS | pooled SEED CASES | ascii SEED CASES | extent SEED CASES | normalise\n");
    return 2;
}
