// fasta_subset_host.cpp — the host route of the FASTA read subset (include/teloscope_mi355x_reads_host.hpp: detail::fastaSubsetHost
// over detail::MappedInput, detail::BlockReader and detail::HostReadJudge) without a device, over a stand-in judge that keeps a read
// exactly when its bases contain TTAGGGTTAGGG.  What is expected comes from a plain whole-text statement of the rule of
// include/teloscan.h, written here and sharing no code with the header: the text is cut into lines at once, with no blocks, no
// carry and no batches.  The library calls of the read block report are stand-ins that fail: no case asks for a report.
// Stand-alone, g++ under ASan + UBSan.
//
//   fasta_subset_host DIR     runs every case with its files under DIR; stdout: one "ok <case> <runs>" line per case, then "ok";
//                             exit 1 and a message on the first difference
#include <cstdio>
#include <fstream>
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

std::string dir;
std::string writeFile(const std::string &name, const std::string &bytes, bool gzip = false) {
    const std::string path = dir + "/" + name;
    if (gzip) {
        gzFile g = gzopen(path.c_str(), "wb1");
        if (!g || (bytes.size() && gzwrite(g, bytes.data(), static_cast<unsigned>(bytes.size())) <= 0) || gzclose(g) != Z_OK) throw std::runtime_error("cannot write " + path);
    } else {
        std::ofstream f(path, std::ios::binary);
        f.write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
        if (!f.good()) throw std::runtime_error("cannot write " + path);
    }
    return path;
}

bool fail(const std::string &what) { std::printf("FAILED %s\n", what.c_str()); return false; }

struct Outcome {
    std::string out, message;                                   // what was written; the exception's text ("" when none)
    uint64_t kept = 0, total = 0, missing = 0;
};
bool same(const Outcome &a, const Outcome &b) { return a.out == b.out && a.message == b.message && a.kept == b.kept && a.total == b.total && a.missing == b.missing; }
std::string show(const Outcome &o) {
    return std::to_string(o.out.size()) + " bytes, kept " + std::to_string(o.kept) + " of " + std::to_string(o.total) + " (" + std::to_string(o.missing) + " without sequence), \"" + o.message + "\"";
}

// The statement (include/teloscan.h above ts_fasta_chunk_stage): a line starts at byte 0 or behind a '\n'; a line that begins
// with '>' opens a record, which runs to the next such line; its bases are the bytes of its other lines without '\n', a '\r' in
// front of one, and a '\r' that is the text's last byte; a record without bases is counted and never kept; a kept record is
// its text as it is, and a '\n' where it does not end in one.
Outcome statement(const std::string &t) {
    Outcome o;
    if (t.empty()) { o.message = "FASTA input is empty"; return o; }
    if (t[0] != '>') { o.message = "FASTA input must start with '>'"; return o; }
    std::vector<size_t> starts;                                 // of the header lines
    for (size_t p = 0; p < t.size();) {
        if (t[p] == '>') starts.push_back(p);
        const size_t nl = t.find('\n', p);
        p = nl == std::string::npos ? t.size() : nl + 1;
    }
    for (size_t k = 0; k < starts.size(); ++k) {
        const size_t b = starts[k], e = k + 1 < starts.size() ? starts[k + 1] : t.size();
        const size_t headEnd = t.find('\n', b);
        std::string bases;
        for (size_t p = headEnd == std::string::npos || headEnd >= e ? e : headEnd + 1; p < e; ++p) {
            const char c = t[p];
            if (c == '\n') continue;
            if (c == '\r' && (p + 1 == t.size() || t[p + 1] == '\n')) continue;
            bases.push_back(c);
        }
        ++o.total;
        if (bases.empty()) { ++o.missing; continue; }
        if (bases.find(kMotif) == std::string::npos) continue;
        ++o.kept;
        o.out += t.substr(b, e - b);
        if (o.out.back() != '\n') o.out.push_back('\n');
    }
    return o;
}
Outcome route(const std::string &path, size_t readsPerBatch, size_t bytesPerBatch) {
    Outcome o;
    std::ostringstream out;
    Judge judge;
    try {
        const FastaSubsetStats s = fastaSubsetHost(path, out, judge, readsPerBatch, bytesPerBatch, nullptr);
        o.kept = s.passedRecords; o.total = s.totalRecords; o.missing = s.missingSequenceRecords;
    } catch (const std::exception &e) { o.message = e.what(); }
    o.out = out.str();
    return o;
}

// record i of the generated text: telomeric or not, folded at a width that changes, with the odd shapes of the rule among them
std::string record(int i, const char *eol) {
    const bool telomeric = i % 3 != 1;
    std::string seq;
    for (int k = 0; k < (i == 23 ? 400 : 2 + i % 5); ++k) seq += telomeric ? "TTAGGG" : "ACGTCA";        // (i == 23: 2 400 bases, larger than most blocks)
    if (i % 10 == 6) seq = "TTAGGGTTAGG";                       // the motif short of a base
    if (i % 10 == 8) seq = "TTAGGG TTAGGG";                     // a space is a base: the motif is not there
    if (i % 13 == 7) seq.clear();                               // no body line at all
    const size_t width = i % 4 == 0 ? seq.size() + 1 : size_t(1 + (i * 7) % 23);
    std::string r = ">r" + std::to_string(i) + (i % 4 == 1 ? " some words\twith a tab" : "") + eol;
    for (size_t a = 0; a < seq.size(); a += width) r += seq.substr(a, width) + eol;
    if (i % 13 == 5) r += std::string(eol) + "\n";              // blank lines behind the body
    if (i % 13 == 9) r = ">blank" + std::to_string(i) + eol + eol + "\n\r\n";       // a body of blank lines only: no bases
    if (i % 17 == 11) r += std::string("T>TAGGGTTAGGG>") + eol; // a '>' inside a body line is a base
    return r;
}

bool everyBlock() {
    std::string text;
    for (int i = 0; i < 40; ++i) text += record(i, i % 11 == 4 ? "\r\n" : "\n");
    std::vector<std::pair<std::string, std::string>> texts;
    texts.emplace_back("as it is", text);
    texts.emplace_back("no final newline", text.substr(0, text.size() - 1));
    texts.emplace_back("final cr", text.substr(0, text.size() - 1) + "\r");
    texts.emplace_back("crlf throughout", [&] { std::string t; for (int i = 0; i < 40; ++i) t += record(i, "\r\n"); return t; }());
    texts.emplace_back("ends in a header", text + ">lonely");
    texts.emplace_back("ends in a kept record without newline", text + ">last\nTTAGGGTTAGGGTT");
    texts.emplace_back("ends in a kept record with a final cr", text + ">last\r\nTTAGGGTTAGGGTT\r");
    size_t runs = 0;
    for (const auto &[name, t] : texts) {
        const Outcome whole = statement(t);
        if (whole.total < 40 || whole.kept * 5 < whole.total || (whole.total - whole.kept) * 5 < whole.total || whole.missing < 3 || !whole.message.empty())
            return fail("the FASTA text itself (" + name + "): " + show(whole));
        const std::string plain = writeFile("reads.fa", t), gz = writeFile("reads.fa.gz", t, true);
        std::vector<size_t> blockSizes{t.size() + 1, t.size()};
        for (size_t bytes = 64; bytes <= t.size(); bytes += name == "as it is" ? 29 : 211) blockSizes.push_back(bytes);
        for (size_t bytes : blockSizes)
            for (size_t reads : {size_t(1), size_t(3), size_t(1000)})
                for (const std::string &path : {plain, gz}) {
                    const Outcome got = route(path, reads, bytes);
                    ++runs;
                    if (!same(got, whole)) return fail("FASTA (" + name + ") " + path + ", " + std::to_string(reads) + " reads, " + std::to_string(bytes) + " bytes: " + show(got) + "; the statement: " + show(whole));
                }
    }
    std::printf("ok fasta-every-block %zu\n", runs);
    return true;
}

bool smallTexts() {
    const std::vector<std::string> texts{
        ">a\n", ">a", ">", ">\n", ">a\r", ">a\r\n", ">a\nTTAGGGTTAGGG", ">a\nTTAGGGTTAGGG\n", ">a\nTTAGGGTTAGGG\r", ">a\nTTAGGGTTAGGG\r\n", ">a\nTTAGGG\nTTAGGG\n",
        ">a\nTTAGGG\r\nTTAGGG", ">a\nTTAGGG\rTTAGGG\n", ">a\n\n\n>b\nTTAGGGTTAGGG\n\n\n>c\n", ">a\n>b\n>c\nTTAGGGTTAGGG\n>d", ">a\nT\nT\nA\nG\nG\nG\nT\nT\nA\nG\nG\nG\n",
        ">a\r\nT\r\nT\r\nA\r\nG\r\nG\r\nG\r\nT\r\nT\r\nA\r\nG\r\nG\r\nG\r\n>b\r\n\r\n", ">a b\tc\nttagggttaggg\nTTAGGGTTAGGG>x\n",
    };
    size_t runs = 0, kept = 0;
    for (const std::string &t : texts) {
        const Outcome whole = statement(t);
        kept += whole.kept;
        for (bool gzip : {false, true}) {
            const std::string path = writeFile("small.fa", t, gzip);
            for (size_t bytes : {size_t(64), size_t(1000)})
                for (size_t reads : {size_t(1), size_t(2)}) {
                    const Outcome got = route(path, reads, bytes);
                    ++runs;
                    if (!same(got, whole)) return fail("FASTA text of " + std::to_string(t.size()) + " bytes, " + std::to_string(bytes) + " bytes per block: " + show(got) + "; the statement: " + show(whole));
                }
        }
    }
    if (kept < 8) return fail("the small FASTA texts keep too little");
    std::printf("ok fasta-small-texts %zu\n", runs);
    return true;
}

bool firstByte() {
    size_t runs = 0;
    for (bool gzip : {false, true})
        for (size_t bytes : {size_t(64), size_t(1000)}) {
            runs += 3;
            const Outcome empty = route(writeFile("empty.fa", "", gzip), 7, bytes), fastq = route(writeFile("reads.fq", "@r\nTTAGGGTTAGGG\n+\nIIIIIIIIIIII\n", gzip), 7, bytes),
                          blank = route(writeFile("blank.fa", "\n>a\nTTAGGGTTAGGG\n", gzip), 7, bytes);
            if (empty.message != "FASTA input is empty" || !empty.out.empty()) return fail("empty FASTA: " + show(empty));
            if (fastq.message != "FASTA input must start with '>'" || !fastq.out.empty()) return fail("FASTQ given as FASTA: " + show(fastq));
            if (blank.message != "FASTA input must start with '>'" || !blank.out.empty()) return fail("FASTA behind a blank line: " + show(blank));
        }
    const Outcome missing = route(dir + "/no-such-file", 7, 64);
    if (missing.message != "Stream not successful: " + dir + "/no-such-file") return fail("FASTA input that is not there: " + show(missing));
    std::printf("ok fasta-first-byte %zu\n", runs);
    return true;
}

// an output stream that fails: the route's own text
bool failingOutput() {
    const std::string path = writeFile("kept.fa", ">a\nTTAGGGTTAGGG\n");
    std::ostringstream out;
    out.setstate(std::ios::badbit);
    Judge judge;
    std::string message;
    try { fastaSubsetHost(path, out, judge, 7, 64, nullptr); } catch (const std::exception &e) { message = e.what(); }
    if (message != "failed while writing FASTA subset") return fail("a failing output stream: \"" + message + "\"");
    std::printf("ok fasta-failing-output 1\n");
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: fasta_subset_host DIR\n"); return 2; }
    dir = argv[1];
    try {
        if (!everyBlock() || !smallTexts() || !firstByte() || !failingOutput()) return 1;
    } catch (const std::exception &e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
