// upload_stage_core.h — everything about a chunk of the host upload that is decided without a device: which pieces of a call
// make a chunk, what the staging workers write into its pinned slot — 2-bit codes + invalid runs (the packed route) or the
// bytes themselves (the ASCII route) — and what the chunk adds to ts_upload_stats.  One source for the library's driver
// (pipeline.cpp: upload_pieces, which keeps the slots, the DMAs and the unpack launches) and for a host test program
// (tests/cpp/upload_stage_host.cpp, built by g++ under ASan + UBSan and under TSan).  Host only: no HIP include, no ts_ctx.
// Under it: ts::pack_bases / ts::pack_text (pack.cpp, through host.hpp) and the text walks and range cuts of text_core.h.
//
// A packed chunk: position 0 is the 64-position boundary c0a at or below the chunk's first base c0; position x lies at bits
// 2 (x & 3) of byte x >> 2 (A 0, C 1, T 2, G 3); worker t packs the positions [cut[t], cut[t + 1]) — cuts in front of the end are
// multiples of 4, so no two workers write the same byte — in blocks of 16384, each packed the cheapest way its pieces allow.
#ifndef TS_UPLOAD_STAGE_CORE_H
#define TS_UPLOAD_STAGE_CORE_H

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "host.hpp"
#include "text_core.h"

namespace tsstage {

struct UpPiece { uint64_t off; const char *src; uint64_t len; uint64_t text_len;     // off: byte offset in the input layout; len: bases;
                                                                                     // text_len != 0: src is FASTA text (line ends to skip)
                 const ts_packed_seq *packed = nullptr; uint64_t packed_first = 0;     // packed: the bases are codes [packed_first, + len) of *packed
                 bool device = false; };                                               // device: src is memory of the context's device (TS_INPUT_DEVICE)

constexpr uint64_t kChunk = 32u << 20, kMaxGap = 64u << 10;
constexpr uint64_t kChunkPacked = 4 * kChunk;              // a packed chunk fills the same 32 MB pinned slot with 128 MB of layout
constexpr uint64_t kBlock = 16384;                         // positions a worker packs at a time

// ---------------------------------------------------------------------------------------------- a call's pieces
// The pieces of one call as the chunks take them: device pieces set aside, plain and packed pieces cut at `limit` bases; a text
// piece of more than `limit` bases is refused (its text cannot be cut without walking it).
enum class Refused { Nothing, TextPieceTooLong };
struct CallPieces {
    std::vector<UpPiece> host, on_device;
    bool any_text = false, any_packed = false;
    uint64_t total_bytes = 0;                              // bases of the host pieces
};
inline Refused normalise_pieces(const std::vector<UpPiece> &in, uint64_t limit, CallPieces &out) {
    out.host.reserve(in.size());
    for (const UpPiece &pc : in) {
        if (pc.device) { out.on_device.push_back(pc); continue; }
        if (pc.text_len) {
            if (pc.len > limit) return Refused::TextPieceTooLong;
            out.host.push_back(pc);
            out.any_text = true;
        } else {
            for (uint64_t a = 0; a < pc.len; a += limit) {
                UpPiece q = pc;
                q.off = pc.off + a; q.len = std::min<uint64_t>(limit, pc.len - a);
                if (pc.packed) q.packed_first = pc.packed_first + a; else q.src = pc.src + a;
                out.host.push_back(q);
            }
            if (pc.packed) out.any_packed = true;
        }
        out.total_bytes += pc.len;
    }
    return Refused::Nothing;
}

// The chunk that begins with piece i: pieces [i, end) and their bases.  A piece joins while the span from the chunk's first base
// to the piece's end is at most chunk_limit and the piece begins at most max_gap behind the end of the one before it.
struct Extent { size_t end; uint64_t bytes; };
inline Extent chunk_extent(const UpPiece *pieces, size_t n, size_t i, uint64_t chunk_limit, uint64_t max_gap) {
    const uint64_t c0 = pieces[i].off;
    Extent e{i + 1, pieces[i].len};
    while (e.end < n && pieces[e.end].off + pieces[e.end].len - c0 <= chunk_limit &&
           pieces[e.end].off - (pieces[e.end - 1].off + pieces[e.end - 1].len) <= max_gap) { e.bytes += pieces[e.end].len; ++e.end; }
    return e;
}

// ---------------------------------------------------------------------------------------------- 2-bit codes
inline unsigned code_at(const uint8_t *codes, uint64_t i) { return (codes[i >> 2] >> (2u * (i & 3u))) & 3u; }

// n codes from index i0 of `codes` to positions [d0, d0 + n) of out, whose bits there are zero: whole bytes where source and
// destination agree on the phase within a byte (full scans: segments start on 16-byte boundaries of the layout), the ragged ends
// and every other phase a code at a time.  Bits of out outside the n positions are left as they are.
inline void copy_codes(unsigned char *out, uint64_t d0, const uint8_t *codes, uint64_t i0, uint64_t n) {
    auto put = [&](uint64_t x) { out[(d0 + x) >> 2] |= (unsigned char)(code_at(codes, i0 + x) << (2u * ((d0 + x) & 3u))); };
    uint64_t x = 0;
    if (((d0 ^ i0) & 3u) == 0u) {
        for (; x < n && ((d0 + x) & 3u); ++x) put(x);                            // up to the first whole byte
        const uint64_t whole = (n - x) >> 2;
        std::memcpy(out + ((d0 + x) >> 2), codes + ((i0 + x) >> 2), whole);
        x += whole * 4;
    }
    for (; x < n; ++x) put(x);
}

// f(ra, rz) for the invalid runs of a packed sequence that reach into its bases [i0, i0 + n), clipped to them, ascending
template <typename F>
inline void for_runs_in(const ts_packed_seq &ps, uint64_t i0, uint64_t n, F f) {
    const ts_packed_run *pr = ps.runs;
    const uint64_t nr = pr ? ps.n_runs : 0;
    size_t r = (size_t)(std::upper_bound(pr, pr + nr, i0, [](uint64_t v, const ts_packed_run &q) { return v < q.start + q.len; }) - pr);
    for (; r < nr && pr[r].start < i0 + n; ++r) {
        const uint64_t ra = std::max<uint64_t>(pr[r].start, i0), rz = std::min<uint64_t>(pr[r].start + pr[r].len, i0 + n);
        if (rz > ra) f(ra, rz);
    }
}

// ... appended to a worker's runs as chunk positions (base i0 lies at chunk position pos0); a run that begins where the last one
// ends — the open one included: it is finished first — goes on in it
inline void translate_runs(const ts_packed_seq &ps, uint64_t i0, uint64_t n, uint64_t pos0, ts::PackRuns &R) {
    for_runs_in(ps, i0, n, [&](uint64_t ra, uint64_t rz) {
        R.finish();
        const uint32_t cs = (uint32_t)(pos0 + (ra - i0));
        if (!R.runs.empty() && R.runs.back().start + R.runs.back().len == cs) R.runs.back().len += (uint32_t)(rz - ra);
        else R.runs.push_back({cs, (uint32_t)(rz - ra)});
    });
}

// ---------------------------------------------------------------------------------------------- a block of a packed chunk
// The layout range [la, lz) of a block, at most kBlock positions whose first is chunk position `a` (a multiple of 4: blocks of
// 16384 from a cut), goes to out = the slot's byte a >> 2, as exactly (lz - la + 3) / 4 bytes.  pieces[k] is the first piece of
// the chunk [.., j) that ends behind la.
struct BlockKinds { uint64_t plain = 0, text = 0, copied = 0, mixed = 0; };     // (ts_upload_stats out[2..5])
enum class BlockKind { Plain, Text, Copied, Mixed };
inline BlockKind block_kind(const UpPiece *pieces, size_t k, size_t j, uint64_t la, uint64_t lz) {
    if (k < j && !pieces[k].packed && pieces[k].off <= la && pieces[k].off + pieces[k].len >= lz)      // wholly inside one ASCII piece
        return pieces[k].text_len ? BlockKind::Text : BlockKind::Plain;
    bool any_here = false;
    for (size_t q = k; q < j && pieces[q].off < lz; ++q) {
        if (pieces[q].off + pieces[q].len <= la) continue;
        if (!pieces[q].packed) return BlockKind::Mixed;
        any_here = true;
    }
    return any_here ? BlockKind::Copied : BlockKind::Mixed;        // (nothing here: padding, spelled out like a seam)
}

// where a worker stands in the text piece it is reading: kept across its blocks, so that a piece is located in once
struct TextCursor {
    const char *cur = nullptr, *end = nullptr;
    size_t piece = (size_t)-1;
    void enter(const UpPiece &pc, size_t q, uint64_t base) {          // piece q, from its base `base` on
        if (piece == q) return;
        piece = q;
        end = pc.src + pc.text_len;
        cur = base ? tstext::text_locate(pc.src, pc.text_len, base) : pc.src;
    }
};

// wholly inside one plain piece: packed from where it lies
inline void block_plain(const UpPiece &pc, uint64_t la, uint64_t lz, unsigned char *out, bool fold, uint32_t a, ts::PackRuns &R) {
    ts::pack_bases((const unsigned char *)pc.src + (la - pc.off), lz - la, out, fold, a, R);
}

// wholly inside one FASTA text piece: packed straight from the text (ts::pack_text: 32 text bytes at a time, the line ends' slots
// taken out of the codes) — the stripped copy in between made text in half as fast as joined bases.  false: the text ended first.
inline bool block_text(const UpPiece &pc, size_t k, uint64_t la, uint64_t lz, unsigned char *out, bool fold, uint32_t a, ts::PackRuns &R,
                       TextCursor &tc) {
    tc.enter(pc, k, la - pc.off);
    return ts::pack_text(&tc.cur, tc.end, lz - la, out, fold, a, R) == lz - la;
}

// every piece the block touches arrived packed (TS_INPUT_PACKED2): their codes are copied and their invalid runs translated; the
// codes under a run stay what the front end wrote (the unpack kernel writes 'N' over them anyway), the padding is code 0
inline void block_copied(const UpPiece *pieces, size_t k, size_t j, uint64_t la, uint64_t lz, unsigned char *out, uint32_t a, ts::PackRuns &R) {
    std::memset(out, 0, (lz - la + 3) >> 2);
    for (size_t q = k; q < j && pieces[q].off < lz; ++q) {
        const UpPiece &pc = pieces[q];
        const uint64_t s0 = std::max(pc.off, la), s1 = std::min(pc.off + pc.len, lz);
        if (s1 <= s0) continue;
        const uint64_t d0 = s0 - la, i0 = pc.packed_first + (s0 - pc.off);       // block position, source base index
        copy_codes(out, d0, pc.packed->codes, i0, s1 - s0);
        translate_runs(*pc.packed, i0, s1 - s0, a + d0, R);
    }
}

// anything else — the seam between two segments, a piece's end, padding: spelled out as letters in buf ('A' in the padding between
// pieces, which nobody reads; packed pieces' codes as letters, 'N' under their runs), then packed.  false: a text ended first.
inline bool block_mixed(const UpPiece *pieces, size_t k, size_t j, uint64_t la, uint64_t lz, unsigned char *out, bool fold, uint32_t a,
                        ts::PackRuns &R, TextCursor &tc, unsigned char *buf) {
    bool ok = true;
    std::memset(buf, 'A', lz - la);
    for (size_t q = k; q < j && pieces[q].off < lz; ++q) {
        const UpPiece &pc = pieces[q];
        const uint64_t s0 = std::max(pc.off, la), s1 = std::min(pc.off + pc.len, lz);
        if (s1 <= s0) continue;
        unsigned char *at = buf + (s0 - la);
        if (pc.packed) {
            const uint64_t i0 = pc.packed_first + (s0 - pc.off);
            for (uint64_t x = 0; x < s1 - s0; ++x) at[x] = "ACTG"[code_at(pc.packed->codes, i0 + x)];
            for_runs_in(*pc.packed, i0, s1 - s0, [&](uint64_t ra, uint64_t rz) { std::memset(at + (ra - i0), 'N', rz - ra); });
        } else if (!pc.text_len) {
            std::memcpy(at, pc.src + (s0 - pc.off), s1 - s0);
        } else {
            tc.enter(pc, q, s0 - pc.off);
            if (tstext::strip_take((char *)at, s1 - s0, &tc.cur, tc.end) != s1 - s0) ok = false;
        }
    }
    ts::pack_bases(buf, lz - la, out, fold, a, R);
    return ok;
}

// A worker's range [a0, z0) of the chunk of pieces [i, j) whose position 0 is layout byte c0a, packed into dst (the slot: position
// x at byte x >> 2) block by block; the range's invalid runs to R, finished, its blocks counted in `kinds` (written once, at the
// end: the workers' entries share cache lines).  Writes the bytes [a0 >> 2, (z0 + 3) >> 2) of dst and no other.  false: a text
// piece holds fewer bases than it declares.
inline bool pack_range(const UpPiece *pieces, size_t i, size_t j, uint64_t c0a, uint64_t a0, uint64_t z0, char *dst, bool fold,
                       ts::PackRuns &R, BlockKinds &kinds) {
    if (a0 >= z0) return true;
    BlockKinds seen;
    alignas(64) unsigned char buf[kBlock];
    bool ok = true;
    size_t k = i;
    TextCursor tc;
    for (uint64_t a = a0; a < z0; a += kBlock) {
        const uint64_t z = std::min(z0, a + kBlock), la = c0a + a, lz = c0a + z;   // layout range of the block
        while (k < j && pieces[k].off + pieces[k].len <= la) ++k;
        unsigned char *out = (unsigned char *)dst + (a >> 2);
        switch (block_kind(pieces, k, j, la, lz)) {
        case BlockKind::Plain:  block_plain(pieces[k], la, lz, out, fold, (uint32_t)a, R); ++seen.plain; break;
        case BlockKind::Text:   ok &= block_text(pieces[k], k, la, lz, out, fold, (uint32_t)a, R, tc); ++seen.text; break;
        case BlockKind::Copied: block_copied(pieces, k, j, la, lz, out, (uint32_t)a, R); ++seen.copied; break;
        case BlockKind::Mixed:  ok &= block_mixed(pieces, k, j, la, lz, out, fold, (uint32_t)a, R, tc, buf); ++seen.mixed; break;
        }
    }
    R.finish();
    kinds = seen;
    return ok;
}

// ---------------------------------------------------------------------------------------------- a packed chunk
inline uint64_t packed_bytes(uint64_t P) { return (((P + 3) >> 2) + 3) & ~3ull; }      // the codes of P positions, whole dwords

// One chunk on the packed route, staged by nt workers: worker t calls pack(t, ..) — any thread, any order — and when all have
// returned, finish() makes the tail.  The slot holds packed_bytes(P) + 8 bytes (the unpack kernel reads one dword past the last code).
struct PackedChunk {
    const UpPiece *pieces;
    size_t i, j;
    uint64_t c0, c0a, P;                                   // first base, position 0 (c0 & ~63), positions incl. the lead before c0
    std::vector<uint64_t> cut;                             // the workers' ranges: equal shares that snap to where a text piece begins (range_cuts)
    std::vector<ts::PackRuns> runs;                        // one entry per worker, written by it alone
    std::vector<BlockKinds> kinds;

    PackedChunk(const UpPiece *pieces_, size_t i_, size_t j_, unsigned nt)
        : pieces(pieces_), i(i_), j(j_), c0(pieces_[i_].off), c0a(c0 & ~63ull), P(pieces_[j_ - 1].off + pieces_[j_ - 1].len - c0a), runs(nt), kinds(nt) {
        std::vector<tstext::CutPiece> cut_pieces;
        if (nt > 1u) {
            cut_pieces.reserve(j - i);
            for (size_t q = i; q < j; ++q) cut_pieces.push_back({pieces[q].off - c0a, pieces[q].text_len != 0});
        }
        cut = tstext::range_cuts(P, nt, cut_pieces.data(), cut_pieces.size());
    }
    bool pack(unsigned t, char *dst, bool fold) { return pack_range(pieces, i, j, c0a, cut[t], cut[t + 1], dst, fold, runs[t], kinds[t]); }
    size_t n_runs() const { size_t n = 0; for (const ts::PackRuns &R : runs) n += R.runs.size(); return n; }
    // The tail: the workers' runs in order to hr (room for n_runs()), the padding behind the codes zeroed — dst[(P + 3) >> 2,
    // packed_bytes(P) + 8) — and what the chunk adds to ts_upload_stats.  pooled: several workers are several threads.
    void finish(char *dst, ts::InvalidRun *hr, bool pooled, uint64_t add[8]) const {
        size_t at = 0;
        for (const ts::PackRuns &R : runs) { if (!R.runs.empty()) std::memcpy(hr + at, R.runs.data(), R.runs.size() * sizeof(ts::InvalidRun)); at += R.runs.size(); }
        std::memset(dst + ((P + 3) >> 2), 0, packed_bytes(P) - ((P + 3) >> 2) + 8);
        BlockKinds sum;
        unsigned workers = 0;
        for (size_t t = 0; t < kinds.size(); ++t) {
            sum.plain += kinds[t].plain; sum.text += kinds[t].text; sum.copied += kinds[t].copied; sum.mixed += kinds[t].mixed;
            if (cut[t + 1] > cut[t]) ++workers;
        }
        const uint64_t all[8] = {1, 0, sum.plain, sum.text, sum.copied, sum.mixed, workers > 1u && pooled ? 1u : 0u, c0 != c0a ? 1u : 0u};
        std::memcpy(add, all, sizeof all);
    }
};

// ---------------------------------------------------------------------------------------------- an ASCII chunk
// The pieces [i, j) of a chunk whose first base is layout byte c0, as they are, to dst[0, end of the last piece - c0); bytes
// between pieces are not written.  Three ways of handing out the work; false: a text piece holds fewer bases than it declares.
inline bool ascii_piece(const UpPiece &pc, uint64_t c0, char *dst) {
    if (pc.text_len) return tstext::strip_copy(dst + (pc.off - c0), pc.src, pc.text_len, pc.len);
    std::memcpy(dst + (pc.off - c0), pc.src, pc.len);
    return true;
}
inline bool ascii_single(const UpPiece *pieces, size_t i, size_t j, uint64_t c0, char *dst) {            // one worker: everything
    bool ok = true;
    for (size_t k = i; k < j; ++k) ok &= ascii_piece(pieces[k], c0, dst);
    return ok;
}
// text present: whole pieces, handed out dynamically — every worker takes pieces from `next` (begun at i) until they run out
inline bool ascii_whole_pieces(const UpPiece *pieces, size_t j, uint64_t c0, char *dst, std::atomic<size_t> &next) {
    bool ok = true;
    for (size_t k; (k = next.fetch_add(1)) < j;) ok &= ascii_piece(pieces[k], c0, dst);
    return ok;
}
// plain only: worker t of nt copies the bytes [t, t + 1) x share of the concatenated pieces (`bytes` in all)
inline void ascii_share(const UpPiece *pieces, size_t i, size_t j, uint64_t c0, char *dst, uint64_t bytes, unsigned nt, unsigned t) {
    const size_t share = (bytes + nt - 1) / nt;
    const size_t lo = (size_t)t * share, hi = std::min<size_t>(bytes, lo + share);
    size_t at = 0;
    for (size_t k = i; k < j; ++k) {
        const UpPiece &pc = pieces[k];
        const size_t a = std::max(lo, at), z = std::min<size_t>(hi, at + pc.len);
        if (z > a) std::memcpy(dst + (pc.off - c0) + (a - at), pc.src + (a - at), z - a);
        at += pc.len;
        if (at >= hi) break;
    }
}

// ---------------------------------------------------------------------------------------------- the staging threads
// They live for a whole call, not for one 32 MB chunk (a chunk is staged in ~0.6 ms: spawning and joining eight threads for each
// cost a tenth of the upload): job(t) runs on worker t, the caller is worker 0.
struct StagePool {
    std::mutex m;
    std::condition_variable cv_go, cv_done;
    std::function<void(unsigned)> job;
    uint64_t generation = 0;
    unsigned active = 0, pending = 0;
    bool quit = false;
    std::vector<std::thread> threads;
    explicit StagePool(unsigned n) {
        for (unsigned t = 1; t < n; ++t)
            threads.emplace_back([this, t] {
                uint64_t seen = 0;
                for (;;) {
                    std::function<void(unsigned)> f;
                    {
                        std::unique_lock<std::mutex> g(m);
                        cv_go.wait(g, [&] { return quit || generation != seen; });
                        if (quit) return;
                        seen = generation;
                        if (t >= active) continue;
                        f = job;
                    }
                    f(t);
                    { std::lock_guard<std::mutex> g(m); if (--pending == 0) cv_done.notify_one(); }
                }
            });
    }
    void run(unsigned n, const std::function<void(unsigned)> &f) {       // f(0 .. n-1), n <= workers
        if (n <= 1 || threads.empty()) { for (unsigned t = 0; t < n; ++t) f(t); return; }
        { std::lock_guard<std::mutex> g(m); job = f; active = n; pending = n - 1; ++generation; }
        cv_go.notify_all();
        f(0);
        std::unique_lock<std::mutex> g(m);
        cv_done.wait(g, [&] { return pending == 0; });
    }
    ~StagePool() {
        { std::lock_guard<std::mutex> g(m); quit = true; }
        cv_go.notify_all();
        for (std::thread &th : threads) th.join();
    }
};

}  // namespace tsstage

#endif
