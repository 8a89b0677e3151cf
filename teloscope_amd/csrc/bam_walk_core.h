// bam_walk_core.h — the record rule of the BAM walk and the three steps of the parallel record index (ts_bam_chunk_index) as
// templates over a byte accessor: compiled by the kernels of bgzf.hip, by bgzf.cpp (the chain) and by a stand-alone host
// program (tests/cpp/bam_index_host.cpp), like inflate_core.h and track_format_core.h.  ts_bam_walk_kernel does NOT use this
// file: it stays the independent statement of the same rule that the index is compared with.
//
// The index cuts the chunk at absolute multiples of a span size S.  Per span, CANDIDATES are offsets from which the serial
// rule survives to the span's end (candidate); the CHAIN starts at `from`, looks each span's entry up among that span's rows and
// settles a miss by the serial rule for that span alone (chain); a last pass walks every entered span again from its verified
// entry and stores the table (span_walk with an emitter).  Every record of the table comes from span_walk at an offset reached
// from `from`, so the table is the serial walk's whatever the rows say: rows decide how fast, never what.
//
// An accessor A has  uint32_t byte(uint64_t p), uint32_t le32(uint64_t p)  for p (+ 4) <= n, and  void stage(uint64_t pos, uint64_t n)
// which record_at calls before it reads the record at pos (the kernels' LDS windows; a no-op elsewhere).
#ifndef TS_BAM_WALK_CORE_H
#define TS_BAM_WALK_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSBAM_FN __host__ __device__ __forceinline__
#else
#define TSBAM_FN inline
#endif

namespace tsbam {

constexpr uint32_t kMaxBlockSize = 256u << 20;
constexpr uint32_t kHeader = 4u + 32u + 256u;          // bytes from a record's start that its checks may read
constexpr uint32_t kMinSpan = 64u, kMaxSpan = 1u << 30, kMaxCandidates = 8u;

// what ends a walk: 1 .. 4 are the TS_BAM_* error codes of include/teloscan.h
enum : uint32_t { kSpanEnd = 0, kBadBlockSize = 1, kBadLengths = 2, kFieldsExceed = 3, kNameNotNul = 4,
                  kIncomplete = 5,      // a valid block_size whose record does not end inside the chunk
                  kShort = 6,           // fewer than 4 bytes left
                  kTableFull = 7 };     // the caller's limit of records

struct Record { uint32_t block_size, seq_at, l_seq; };             // seq_at as ts_bam_record holds it: from the block_size field
struct SpanResult { uint64_t exit, records; uint32_t stop; };      // exit: where the walk stood when it stopped
struct Row { uint32_t entry, exit, records, stop; };               // a candidate: entry and exit count from the span's first byte
constexpr uint32_t kNoRow = 0xffffffffu;                           // Row::entry of a slot that holds nothing
struct Task { uint64_t entry, base; };                             // a span the chain entered: where, and its first table index

// The per-record rule, checks in the host route's order (bamSubset in include/teloscope_mi355x_io.hpp).  pos <= n.  0 = a valid,
// complete record in r.  Every read lies below n: block_size is compared in 64 bits before any field is touched.
template <class A>
TSBAM_FN uint32_t record_at(A &a, uint64_t n, uint64_t pos, Record &r) {
    if (n - pos < 4ull) return kShort;
    a.stage(pos, n);
    const uint32_t bs = a.le32(pos);
    if ((int32_t)bs < 32 || bs > kMaxBlockSize) return kBadBlockSize;
    if (n - pos < 4ull + bs) return kIncomplete;
    const uint64_t core = pos + 4ull;
    const uint32_t lname = a.byte(core + 8), ncigar = a.byte(core + 12) | a.byte(core + 13) << 8, lseq = a.le32(core + 16);
    const uint64_t seq_at = 32ull + lname + 4ull * ncigar;
    if (lname == 0u || lseq > 0x7fffffffu) return kBadLengths;
    if (seq_at + ((uint64_t)lseq + 1ull) / 2ull + lseq > (uint64_t)bs) return kFieldsExceed;
    if (a.byte(core + 32ull + lname - 1ull) != 0u) return kNameNotNul;
    r.block_size = bs; r.seq_at = 4u + (uint32_t)seq_at; r.l_seq = lseq;
    return 0u;
}

// The candidate test's prefilter, stricter than the rule: refID, pos, next refID and next pos of a record are >= -1.  A record
// that fails it is merely no candidate (its span is settled by the rule); it is never applied to a record the table takes.
template <class A>
TSBAM_FN bool plausible_first(A &a, uint64_t pos) {
    return (int32_t)a.le32(pos + 4) >= -1 && (int32_t)a.le32(pos + 8) >= -1 && (int32_t)a.le32(pos + 24) >= -1 &&
           (int32_t)a.le32(pos + 28) >= -1;
}

// The serial rule from `entry` until the walk stands at or beyond span_end, stops, or has taken `limit` records;
// emit(index, offset, record) for every record taken.
template <class A, class Emit>
TSBAM_FN SpanResult span_walk(A &a, uint64_t n, uint64_t entry, uint64_t span_end, uint64_t limit, Emit &&emit) {
    SpanResult s;
    s.exit = entry; s.records = 0; s.stop = kSpanEnd;
    while (s.exit < span_end) {
        if (s.records == limit) { s.stop = kTableFull; break; }
        Record r;
        const uint32_t code = record_at(a, n, s.exit, r);
        if (code != 0u) { s.stop = code; break; }
        emit(s.records, s.exit, r);
        ++s.records;
        s.exit += 4ull + r.block_size;
    }
    return s;
}

struct NoEmit { TSBAM_FN void operator()(uint64_t, uint64_t, const Record &) const {} };

// Is p (span_lo <= p < span_end) a candidate?  Its first record is complete, valid and plausible (read through `first`), and the
// rule survives from behind it (read through `rest`) to the span's end, to an incomplete record or to the chunk's last bytes.
template <class A1, class A2>
TSBAM_FN bool candidate(A1 &first, A2 &rest, uint64_t n, uint64_t p, uint64_t span_lo, uint64_t span_end, Row &row) {
    Record r;
    if (record_at(first, n, p, r) != 0u || !plausible_first(first, p)) return false;
    const SpanResult s = span_walk(rest, n, p + 4ull + r.block_size, span_end, ~0ull, NoEmit());
    if (s.stop >= kBadBlockSize && s.stop <= kNameNotNul) return false;
    row.entry = (uint32_t)(p - span_lo); row.exit = (uint32_t)(s.exit - span_lo); row.records = (uint32_t)(s.records + 1ull); row.stop = s.stop;
    return true;
}

// Which offsets of span k the candidate pass tests: the span that holds `from` has one known entry, `from` itself; an offset
// with fewer than 36 bytes behind it holds no complete record.  -> [lo, hi), empty where lo >= hi.
TSBAM_FN void scan_range(uint64_t n, uint64_t from, uint32_t span_log2, uint64_t k, uint64_t &lo, uint64_t &hi) {
    lo = k << span_log2;
    hi = lo + (1ull << span_log2);
    const uint64_t last = n >= 36ull ? n - 35ull : 0ull;
    if (hi > last) hi = last;
    if (k == from >> span_log2) { lo = from; if (hi > from + 1ull) hi = from + 1ull; }
}

struct ChainResult {
    uint64_t n, next, error_off;
    uint32_t error;
    bool next_in_span;                  // record `cap` lies inside the last task's span: the write pass reports its offset
    uint64_t entered, hits, settled;
};

// The chain.  rows_of(k) -> the K rows of absolute span k; settle(entry, span_end) -> SpanResult of the serial rule;
// push(Task) for every span entered, in order.
template <class Rows, class Settle, class Push>
inline ChainResult chain(uint64_t n, uint64_t from, uint64_t cap, uint32_t span_log2, uint32_t K, Rows &&rows_of, Settle &&settle, Push &&push) {
    ChainResult c;
    c.n = 0; c.next = from; c.error_off = 0; c.error = 0; c.next_in_span = false; c.entered = c.hits = c.settled = 0;
    uint64_t pos = from;
    while (c.n < cap) {
        c.next = pos;
        if (pos > n || n - pos < 4ull) break;
        const uint64_t k = pos >> span_log2, lo = k << span_log2, end = lo + (1ull << span_log2);
        ++c.entered;
        SpanResult s;
        const Row *rows = rows_of(k);
        uint32_t j = 0;
        while (j < K && rows[j].entry != (uint32_t)(pos - lo)) ++j;
        if (j < K) { ++c.hits; s.exit = lo + rows[j].exit; s.records = rows[j].records; s.stop = rows[j].stop; }
        else { ++c.settled; s = settle(pos, end); }
        Task t;
        t.entry = pos; t.base = c.n;
        push(t);
        if (s.records > cap - c.n) { c.n = cap; c.next_in_span = true; break; }
        c.n += s.records;
        c.next = pos = s.exit;
        if (c.n == cap) break;                                  // (the table is full: the record behind it is not looked at)
        if (s.stop >= kBadBlockSize && s.stop <= kNameNotNul) { c.error = s.stop; c.error_off = s.exit; break; }
        if (s.stop != kSpanEnd) break;
    }
    return c;
}

}  // namespace tsbam

#endif
