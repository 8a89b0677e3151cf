// bam_index_host.cpp — TEST INFRASTRUCTURE: the parallel record index of teloscope_amd/csrc/bam_walk_core.h run on the host, so
// that the code the kernels compile (the record rule, the candidate test, the span walk, the chain) can be held to the Python
// model of tests/bamindex.py under AddressSanitizer and UBSan.  The buffer it walks is exactly as long as the stream: a read
// beyond the stream's last byte is a sanitizer error.
// Usage: bam_index_host CASES   (tests/bamindex.py: case_file; per case five little-endian u64 — bytes, from, cap, S, K — and
//                                the bytes).  One line per case:
//   n N next X error E at O entered A hits H settled T : off,block_size,seq_at,l_seq ...
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../teloscope_amd/csrc/bam_walk_core.h"

namespace {

struct HostBytes {
    const unsigned char *p;
    uint32_t byte(uint64_t at) const { return p[at]; }
    uint32_t le32(uint64_t at) const { uint32_t v; std::memcpy(&v, p + at, 4); return v; }
    void stage(uint64_t, uint64_t) const {}
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: bam_index_host CASES\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t head[5];
    while (std::fread(head, 8, 5, f) == 5) {
        const uint64_t n = head[0], from = head[1], cap = head[2], S = head[3], K = head[4];
        if (S < tsbam::kMinSpan || S > tsbam::kMaxSpan || (S & (S - 1)) != 0 || K < 1 || K > tsbam::kMaxCandidates || from > n) {
            std::fprintf(stderr, "bad case\n");
            return 2;
        }
        std::vector<unsigned char> heap(n);                     // (exactly n bytes: the sanitizer sees the first read beyond them)
        if (n && std::fread(heap.data(), 1, n, f) != n) { std::fprintf(stderr, "short case\n"); return 2; }
        uint32_t lg = 0;
        while ((1ull << lg) < S) ++lg;
        HostBytes a{heap.data()};
        // candidates: every span from the one that holds `from`, offsets ascending, the first K kept
        const uint64_t first = from >> lg, n_spans = n ? ((n - 1) >> lg) - first + 1 : 0;
        tsbam::Row none;
        none.entry = tsbam::kNoRow; none.exit = none.records = none.stop = 0;
        std::vector<tsbam::Row> rows(static_cast<size_t>((n_spans + 1) * K), none);
        for (uint64_t s = 0; s < n_spans; ++s) {
            const uint64_t k = first + s, span_lo = k << lg, span_end = span_lo + S;
            uint64_t lo, hi;
            tsbam::scan_range(n, from, lg, k, lo, hi);
            uint32_t found = 0;
            for (uint64_t p = lo; p < hi && found < K; ++p) {
                tsbam::Row row;
                if (tsbam::candidate(a, a, n, p, span_lo, span_end, row)) rows[static_cast<size_t>(s * K + found++)] = row;
            }
        }
        std::vector<tsbam::Task> tasks;
        const tsbam::ChainResult c = tsbam::chain(
            n, from, cap, lg, static_cast<uint32_t>(K), [&](uint64_t k) { return rows.data() + static_cast<size_t>((k - first) * K); },
            [&](uint64_t entry, uint64_t span_end) { return tsbam::span_walk(a, n, entry, span_end, ~0ull, tsbam::NoEmit()); },
            [&](const tsbam::Task &t) { tasks.push_back(t); });
        // write: every entered span again from its verified entry, records below cap
        struct Rec { uint64_t off; uint32_t bs, seq_at, lseq; };
        std::vector<Rec> table(static_cast<size_t>(c.n));
        uint64_t next = c.next;
        for (const tsbam::Task &t : tasks) {
            const uint64_t span_end = ((t.entry >> lg) + 1) << lg;
            const tsbam::SpanResult s = tsbam::span_walk(a, n, t.entry, span_end, cap - t.base, [&](uint64_t i, uint64_t pos, const tsbam::Record &r) {
                table.at(static_cast<size_t>(t.base + i)) = Rec{pos, r.block_size, r.seq_at, r.l_seq};
            });
            if (s.stop == tsbam::kTableFull) next = s.exit;
        }
        std::printf("n %llu next %llu error %u at %llu entered %llu hits %llu settled %llu :", (unsigned long long)c.n, (unsigned long long)next, c.error,
                    (unsigned long long)c.error_off, (unsigned long long)c.entered, (unsigned long long)c.hits, (unsigned long long)c.settled);
        for (const Rec &r : table) std::printf(" %llu,%u,%u,%u", (unsigned long long)r.off, r.bs, r.seq_at, r.lseq);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
