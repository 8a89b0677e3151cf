// fastq_pairs_host.cpp — the host route of the read subset of interleaved paired FASTQ (include/teloscope_mi355x_reads_host.hpp:
// detail::fastqSubsetPairedWith over detail::FastqHostInput, detail::BlockReader and detail::HostReadJudge) and the names' core
// header (teloscope_amd/csrc/fastq_pair_core.h) without a device, over a stand-in judge that passes a read exactly when its bases
// contain TTAGGGTTAGGG.  What is expected comes from the caller (tests/test_fastq_pairs_reference_cpu.py, which holds the route
// against the rule's plain-Python statement): this program says that every way of reading the file — mapped, gzip through
// the block reader, every block and batch size — gives one and the same answer, and which.  The library calls of the read block
// report are stand-ins that fail: no case asks for a report.  Stand-alone, g++ under ASan + UBSan.
//
//   fastq_pairs_host subset FILE   the route on FILE and on FILE.gz (written here) with every block and batch size; all runs must
//                                  agree.  FILE.out: what was written; stdout: "ok <total> <kept>" or "error <message>", then
//                                  "runs <n>"; exit 1 and a message on the first difference between two runs
//   fastq_pairs_host names FILE    FILE is well-formed FASTQ with an even number of records: a line "1" or "0" per pair, whether
//                                  tspair::mates holds for it
#include <cstdio>
#include <fstream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/teloscope_mi355x_reads_host.hpp"

extern "C" {
int ts_scan_segments_blocks(ts_ctx *, const ts_segment_in *, size_t, ts_segment_out *, ts_segment_counts *) { return -1; }
const char *ts_last_error(const ts_ctx *) { return "no device in this program"; }
void ts_free_segments(ts_segment_out *, size_t) {}
}

using namespace teloscope_mi355x;
using namespace teloscope_mi355x::detail;

namespace {

const std::string kMotif = "TTAGGGTTAGGG";

struct Judge {
    void matchesPointers(const char *const *seqs, const uint64_t *lens, size_t n, uint8_t *pass) {
        for (size_t i = 0; i < n; ++i) pass[i] = std::string(seqs[i], lens[i]).find(kMotif) != std::string::npos;
    }
    ts_ctx *context(size_t) { return nullptr; }
};

std::string readFile(const std::string &path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open " + path);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

struct Outcome {
    std::string out, message;
    uint64_t kept = 0, total = 0;
};
std::string show(const Outcome &o) {
    return std::to_string(o.out.size()) + " bytes, kept " + std::to_string(o.kept) + " of " + std::to_string(o.total) + ", \"" + o.message + "\"";
}
// (the statistics of a run that threw are not the route's answer)
bool same(const Outcome &a, const Outcome &b) { return a.out == b.out && a.message == b.message && (!a.message.empty() || (a.kept == b.kept && a.total == b.total)); }

Outcome route(const std::string &path, size_t readsPerBatch, size_t bytesPerBatch) {
    Outcome o;
    std::ostringstream out;
    Judge judge;
    try {
        const FastqSubsetResult r = fastqSubsetPairedWith(path, out, judge, readsPerBatch, bytesPerBatch, nullptr);
        o.kept = r.kept; o.total = r.total;
    } catch (const std::exception &e) { o.message = e.what(); }
    o.out = out.str();
    return o;
}

int subset(const std::string &path) {
    const std::string text = readFile(path), gz = path + ".gz";
    {
        gzFile g = gzopen(gz.c_str(), "wb1");
        if (!g || (text.size() && gzwrite(g, text.data(), static_cast<unsigned>(text.size())) <= 0) || gzclose(g) != Z_OK) throw std::runtime_error("cannot write " + gz);
    }
    std::vector<size_t> blockSizes{text.size() + 1, std::max<size_t>(text.size(), 1), 64, 100, 211, 1000, 4096};
    const Outcome first = route(path, 1u << 20, 512u << 20);
    size_t runs = 1;
    for (size_t bytes : blockSizes)
        for (size_t reads : {size_t(1), size_t(2), size_t(3), size_t(38), size_t(1000)})
            for (const std::string &p : {path, gz}) {
                const Outcome got = route(p, reads, bytes);
                ++runs;
                if (!same(got, first)) {
                    std::printf("FAILED %s, %zu reads, %zu bytes: %s; the first run: %s\n", p.c_str(), reads, bytes, show(got).c_str(), show(first).c_str());
                    return 1;
                }
            }
    std::ofstream(path + ".out", std::ios::binary).write(first.out.data(), static_cast<std::streamsize>(first.out.size()));
    if (first.message.empty()) std::printf("ok %llu %llu\n", (unsigned long long)first.total, (unsigned long long)first.kept);
    else std::printf("error %s\n", first.message.c_str());
    std::printf("runs %zu\n", runs);
    return 0;
}

int names(const std::string &path) {
    const std::string text = readFile(path);
    std::vector<FastqRec> recs;
    if (parseFastqPiece(text.data(), text.data() + text.size(), text.data() + text.size(), recs) == nullptr || recs.size() % 2) {
        std::printf("FAILED %s is not an even number of well-formed records\n", path.c_str());
        return 1;
    }
    // (offsets into the whole text, as the kernel reads a chunk: one reader for both records, and one for each)
    const ReadBlockReport::Bytes whole{text.data()};
    for (size_t j = 0; j + 1 < recs.size(); j += 2) {
        const FastqRec &a = recs[j], &b = recs[j + 1];
        const bool m = tspair::mates(whole, static_cast<uint64_t>(a.begin - text.data()), static_cast<uint32_t>(a.seq - a.begin), whole,
                                     static_cast<uint64_t>(b.begin - text.data()), static_cast<uint32_t>(b.seq - b.begin));
        const ReadBlockReport::Bytes ra{a.begin}, rb{b.begin};
        if (m != tspair::mates(ra, 0, static_cast<uint32_t>(a.seq - a.begin), rb, 0, static_cast<uint32_t>(b.seq - b.begin))) {
            std::printf("FAILED pair %zu: the answer depends on the reader\n", j / 2);
            return 1;
        }
        std::printf("%d\n", m ? 1 : 0);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: fastq_pairs_host subset|names FILE\n"); return 2; }
    try {
        const std::string mode = argv[1];
        return mode == "subset" ? subset(argv[2]) : mode == "names" ? names(argv[2]) : 2;
    } catch (const std::exception &e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
}
