// read_host_routes_host.cpp — the host routes of the read subsets (include/teloscope_mi355x_reads_host.hpp) without a device:
// detail::BlockReader alone, and detail::fastqSubsetWith, detail::samSubsetHost and detail::bamSubsetHost over a stand-in judge
// that keeps a read exactly when its bases contain TTAGGGTTAGGG.  What is expected comes from a plain whole-text statement of each
// format, written here and sharing no code with the header: the text is cut into lines (or the BAM stream into records) at once,
// with no blocks, no carry and no batches.  The library calls of the read block report are stand-ins that fail: no case asks
// for a report.  Stand-alone, g++ under ASan + UBSan and, a second build, under TSan.
//
//   read_host_routes_host DIR     runs every case with its files under DIR; stdout: one "ok <case> <runs>" line per case, then
//                                 "ok"; exit 1 and a message on the first difference
#include <cstdio>
#include <cstring>
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
bool startsWith(const std::string &s, const std::string &prefix) { return s.compare(0, prefix.size(), prefix) == 0; }

struct Outcome {
    std::string out, message;                                   // what was written; the exception's text ("" when none)
    uint64_t kept = 0, total = 0, missing = 0, headers = 0;
    bool noEof = false;
};
bool same(const Outcome &a, const Outcome &b) {
    return a.out == b.out && a.message == b.message && a.kept == b.kept && a.total == b.total && a.missing == b.missing && a.headers == b.headers;
}
std::string show(const Outcome &o) {
    return std::to_string(o.out.size()) + " bytes, kept " + std::to_string(o.kept) + " of " + std::to_string(o.total) + ", \"" + o.message + "\"";
}

// the lines of a text: [b, e) without the '\n'; the last one may lack it
struct Line { size_t b, e; };
std::vector<Line> linesOf(const std::string &t) {
    std::vector<Line> v;
    for (size_t p = 0; p < t.size();) {
        const size_t nl = t.find('\n', p);
        v.push_back({p, nl == std::string::npos ? t.size() : nl});
        p = nl == std::string::npos ? t.size() : nl + 1;
    }
    return v;
}
std::string content(const std::string &t, const Line &l) {       // a line without its '\r'
    return t.substr(l.b, l.e - l.b - (l.e > l.b && t[l.e - 1] == '\r' ? 1 : 0));
}
std::string reverseComplement(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
    return r;
}

// ------------------------------------------------------------------------------------------------ BlockReader alone
struct Seen { std::vector<std::string> records; std::vector<size_t> afterBlock; std::string message; };
// length-prefixed records (two bytes, little-endian) out of a memory buffer; the fill throws at its failAt-th call (0: never);
// `eager`: the fill says `last` with the bytes that end the input, else with the empty read behind them
Seen readRecords(const std::string &buf, size_t block, size_t failAt, bool eager) {
    Seen s;
    size_t at = 0, calls = 0;
    try {
        BlockReader reader([&](char *dst, size_t cap, bool &last) -> size_t {
            if (++calls == failAt) throw std::runtime_error("fill " + std::to_string(calls));
            const size_t n = std::min(cap, buf.size() - at);
            std::memcpy(dst, buf.data() + at, n);
            at += n;
            last = eager ? at == buf.size() : n < cap;
            return n;
        }, block, 16);
        size_t left = 0;
        for (bool last = false; !last;) {
            const BlockReader::Block b = reader.next(left);
            last = b.last;
            const char *p = b.begin;
            while (b.end - p >= 2) {
                const size_t n = static_cast<unsigned char>(p[0]) | static_cast<size_t>(static_cast<unsigned char>(p[1])) << 8;
                if (static_cast<size_t>(b.end - p) < 2 + n) break;
                s.records.emplace_back(p + 2, n);
                p += 2 + n;
            }
            left = static_cast<size_t>(b.end - p);
            s.afterBlock.push_back(s.records.size());
        }
        if (left) s.message = "bytes left over";
    } catch (const std::exception &e) { s.message = e.what(); }
    return s;
}

bool blockReaderCases() {
    std::vector<std::string> recs;
    for (size_t n : {1, 300, 7, 1, 64, 2, 16, 17, 120})
        recs.push_back(std::string(n, static_cast<char>('a' + recs.size())));
    std::string buf;
    for (const std::string &r : recs) { buf.push_back(static_cast<char>(r.size() & 255)); buf.push_back(static_cast<char>(r.size() >> 8)); buf += r; }
    size_t runs = 0;
    for (int eager = 0; eager < 2; ++eager)
        for (size_t block = 8; block <= buf.size() + 1; ++block, ++runs) {
            const Seen s = readRecords(buf, block, 0, eager != 0);
            if (s.records != recs || !s.message.empty()) return fail("BlockReader, block " + std::to_string(block) + ": " + std::to_string(s.records.size()) + " records, \"" + s.message + "\"");
        }
    for (size_t block : {size_t(8), size_t(16), size_t(4000)}) {
        const Seen s = readRecords(std::string(), block, 0, block == 16);
        ++runs;
        if (!s.records.empty() || !s.message.empty() || s.afterBlock.size() != 1) return fail("BlockReader, empty input");
    }
    std::printf("ok block-reader-every-size %zu\n", runs);
    runs = 0;
    for (size_t block : {size_t(8), size_t(50), size_t(301)}) {
        const Seen clean = readRecords(buf, block, 0, false);
        for (size_t k = 1; k <= clean.afterBlock.size(); ++k, ++runs) {
            const Seen s = readRecords(buf, block, k, false);
            const size_t want = k >= 2 ? clean.afterBlock[k - 2] : 0;             // the records of the blocks before the k-th
            if (s.message != "fill " + std::to_string(k) || s.records.size() != want || !std::equal(s.records.begin(), s.records.end(), recs.begin()))
                return fail("BlockReader, fill " + std::to_string(k) + " of block " + std::to_string(block) + " throws: " + std::to_string(s.records.size()) + " records, \"" + s.message + "\"");
        }
    }
    std::printf("ok block-reader-failing-fill %zu\n", runs);
    return true;
}

// ------------------------------------------------------------------------------------------------ FASTQ
// The statement: blank lines in front of a header are skipped; then four lines whatever they hold — at the text's end fewer is a
// truncated record; the first begins with '@', the third with '+', the second and fourth are as long (a '\r' at a line's end
// not counted); a kept record is its four lines as they are and a '\n'.
Outcome fastqStatement(const std::string &t) {
    Outcome o;
    const std::vector<Line> ls = linesOf(t);
    auto failed = [&](const char *what) { o.message = "FASTQ record " + std::to_string(o.total + 1) + ": " + what; return o; };
    for (size_t i = 0; i < ls.size();) {
        if (content(t, ls[i]).empty()) { ++i; continue; }
        if (i + 4 > ls.size()) return failed("truncated FASTQ record");
        if (t[ls[i].b] != '@') return failed("expected header line starting with '@'");
        if (ls[i + 2].e == ls[i + 2].b || t[ls[i + 2].b] != '+') return failed("expected separator line starting with '+'");
        if (content(t, ls[i + 1]).size() != content(t, ls[i + 3]).size()) return failed("sequence and quality length differ");
        ++o.total;
        if (content(t, ls[i + 1]).find(kMotif) != std::string::npos) { ++o.kept; o.out += t.substr(ls[i].b, ls[i + 3].e - ls[i].b) + "\n"; }
        i += 4;
    }
    return o;
}
Outcome fastqRoute(const std::string &path, size_t readsPerBatch, size_t bytesPerBatch) {
    Outcome o;
    std::ostringstream out;
    Judge judge;
    try {
        const FastqSubsetResult r = fastqSubsetWith(path, out, judge, readsPerBatch, bytesPerBatch, nullptr);
        o.kept = r.kept; o.total = r.total;
    } catch (const std::exception &e) { o.message = e.what(); }
    o.out = out.str();
    return o;
}
std::string fastqRecord(int i, const char *eol) {
    const bool telomeric = i % 3 != 1;                          // (18 of the 40 are kept: the motif needs two repeats)
    std::string seq;
    for (int k = 0; k < (i == 23 ? 50 : 1 + i % 5); ++k) seq += telomeric ? "TTAGGG" : "ACGTCA";    // (i == 23: 300 bases; one TTAGGG alone is not kept)
    if (i % 10 == 6) seq = "TTAGGGTTAGG";                       // the motif short of a base
    const std::string name = "r" + std::to_string(i) + (i % 4 == 1 ? " some words" : "");
    return "@" + name + eol + seq + eol + (i % 4 == 2 ? "+" + name : std::string("+")) + eol + std::string(seq.size(), i % 5 == 1 ? '@' : 'I') + eol +
           (i % 13 == 5 ? "\n" : "") + (i % 17 == 9 ? "\r\n\n" : "");
}

bool fastqCases() {
    std::vector<std::string> recs;
    for (int i = 0; i < 40; ++i) recs.push_back(fastqRecord(i, i % 11 == 4 ? "\r\n" : "\n"));
    std::string text;
    for (const std::string &r : recs) text += r;
    text.pop_back();                                            // the last line without its '\n'
    const Outcome whole = fastqStatement(text);
    if (whole.total != 40 || whole.kept * 4 < 40 || (40 - whole.kept) * 4 < 40 || !whole.message.empty()) return fail("the FASTQ text itself: " + show(whole));
    const std::string plain = writeFile("reads.fastq", text), gz = writeFile("reads.fastq.gz", text, true);
    size_t runs = 0;
    std::vector<size_t> blockSizes{text.size() + 1};
    for (size_t bytes = 64; bytes <= text.size(); bytes += 29) blockSizes.push_back(bytes);        // (29 = 4 * 7 + 1: every residue mod 7)
    for (size_t bytes : blockSizes)
        for (size_t reads : {size_t(1), size_t(3), size_t(1000)})
            for (const std::string &path : {plain, gz}) {
                const Outcome got = fastqRoute(path, reads, bytes);
                ++runs;
                if (!same(got, whole)) return fail("FASTQ " + path + ", " + std::to_string(reads) + " reads, " + std::to_string(bytes) + " bytes: " + show(got) + "; the statement: " + show(whole));
            }
    std::printf("ok fastq-every-block %zu\n", runs);

    // texts that end in a failure: the message with its record number, the same on both paths and for every block size; what was
    // written is a prefix of what the statement writes ahead of the failure
    std::vector<std::string> bad;
    const size_t lastAt = text.size() - (recs.back().size() - 1);
    for (size_t cut = lastAt; cut < text.size(); ++cut) bad.push_back(text.substr(0, cut));
    for (int kind = 0; kind < 3; ++kind) {
        std::string t;
        for (size_t i = 0; i < recs.size(); ++i) {
            std::string r = recs[i];
            if (i == 17 && kind == 0) r[0] = 'X';
            if (i == 17 && kind == 1) r[r.find("\n+") + 1] = '-';
            if (i == 17 && kind == 2) r.insert(r.find('\n') + 1, "A");
            t += r;
        }
        bad.push_back(t);
    }
    runs = 0;
    size_t failures = 0;
    for (const std::string &t : bad) {
        const Outcome want = fastqStatement(t);
        failures += want.message.empty() ? 0 : 1;
        const std::string p = writeFile("bad.fastq", t), g = writeFile("bad.fastq.gz", t, true);
        for (size_t bytes : {size_t(64), size_t(97), size_t(1000), t.size() + 1})
            for (const std::string &path : {p, g}) {
                const Outcome got = fastqRoute(path, 7, bytes);
                ++runs;
                if (got.message != want.message || !startsWith(want.out, got.out) || (want.message.empty() && !same(got, want)))
                    return fail("FASTQ text of " + std::to_string(t.size()) + " bytes, " + path + ", " + std::to_string(bytes) + " bytes: " + show(got) + "; the statement: " + show(want));
            }
    }
    if (failures < recs.back().size() / 2 + 3) return fail("the FASTQ failure texts fail too rarely");
    std::printf("ok fastq-failures %zu\n", runs);

    runs = 0;
    for (bool gzip : {false, true}) {
        for (size_t bytes : {size_t(64), size_t(1000)}) {
            runs += 2;
            const Outcome empty = fastqRoute(writeFile("empty.fastq", "", gzip), 7, bytes), noAt = fastqRoute(writeFile("noat.fastq", text.substr(1), gzip), 7, bytes);
            if (empty.message != "FASTQ input is empty" || !empty.out.empty()) return fail("empty FASTQ: " + show(empty));
            if (noAt.message != "FASTQ input must start with '@'" || !noAt.out.empty()) return fail("FASTQ that does not start with '@': " + show(noAt));
        }
    }
    Outcome missing = fastqRoute(dir + "/no-such-file", 7, 64);
    if (missing.message != "Stream not successful: " + dir + "/no-such-file") return fail("FASTQ input that is not there: " + show(missing));
    std::printf("ok fastq-first-byte %zu\n", runs);
    return true;
}

// ------------------------------------------------------------------------------------------------ SAM
// The statement (include/teloscan.h above ts_sam_chunk_walk): lines that begin with '@' are the header while no other line has
// come, and an error behind one; an alignment line has eleven tab-separated fields or more; SEQ is not empty; SEQ and QUAL are as
// long unless one is "*".  A "*" SEQ is counted and never kept.  Plain out: the header lines and the kept lines as they are, a
// kept line with a '\n'.  FASTQ out: '@' QNAME, SEQ, '+', QUAL — reverse-complemented and reversed where FLAG has 0x10, '!' for
// every base where QUAL is "*".
Outcome samStatement(const std::string &t, bool fastq) {
    Outcome o;
    bool inHeader = true;
    const std::vector<Line> ls = linesOf(t);
    for (size_t i = 0; i < ls.size(); ++i) {
        auto failed = [&](const char *what) { o.message = "SAM line " + std::to_string(i + 1) + ": " + what; return o; };
        const std::string c = content(t, ls[i]);
        if (ls[i].e > ls[i].b && t[ls[i].b] == '@') {
            if (!inHeader) return failed("header line after the first alignment record");
            ++o.headers;
            if (!fastq) o.out += t.substr(ls[i].b, std::min(ls[i].e + 1, t.size()) - ls[i].b);
            continue;
        }
        inHeader = false;
        std::vector<std::string> f;
        for (size_t p = 0;;) {
            const size_t tab = c.find('\t', p);
            f.push_back(c.substr(p, tab == std::string::npos ? std::string::npos : tab - p));
            if (tab == std::string::npos) break;
            p = tab + 1;
        }
        if (f.size() < 11) return failed("fewer than 11 fields");
        const std::string &seq = f[9], &qual = f[10];
        if (seq.empty()) return failed("empty SEQ field");
        if (seq != "*" && qual != "*" && seq.size() != qual.size()) return failed("SEQ and QUAL length differ");
        ++o.total;
        if (seq == "*") { ++o.missing; continue; }
        if (seq.find(kMotif) == std::string::npos) continue;
        ++o.kept;
        if (!fastq) { o.out += t.substr(ls[i].b, ls[i].e - ls[i].b) + "\n"; continue; }
        const bool reverse = (std::stoul(f[1]) & 0x10u) != 0;
        const std::string q = qual == "*" ? std::string(seq.size(), '!') : qual;
        o.out += "@" + f[0] + "\n" + (reverse ? reverseComplement(seq) : seq) + "\n+\n" + (reverse ? std::string(q.rbegin(), q.rend()) : q) + "\n";
    }
    return o;
}
Outcome samRoute(const std::string &path, size_t readsPerBatch, size_t bytesPerBatch, bool fastq) {
    Outcome o;
    std::ostringstream out;
    Judge judge;
    const ReadFastqOutput asFastq;
    try {
        const SamSubsetStats s = samSubsetHost(path, out, judge, readsPerBatch, bytesPerBatch, nullptr, fastq ? &asFastq : nullptr);
        o.kept = s.passedRecords; o.total = s.totalRecords; o.missing = s.missingSequenceRecords; o.headers = s.headerLines;
    } catch (const std::exception &e) { o.message = e.what(); }
    o.out = out.str();
    return o;
}
std::string samLine(int i, const char *eol) {
    std::string seq;
    for (int k = 0; k < 2 + i % 4; ++k) seq += i % 3 != 1 ? "TTAGGG" : "ACGTCA";
    std::string qual;
    for (size_t k = 0; k < seq.size(); ++k) qual.push_back(static_cast<char>('#' + (k + static_cast<size_t>(i)) % 40));
    if (i % 7 == 3) { seq = "*"; qual = "*"; }
    if (i % 7 == 5) qual = "*";
    return "q" + std::to_string(i) + "\t" + (i % 2 ? "16" : "0") + "\tchr1\t" + std::to_string(100 + i) + "\t60\t*\t*\t0\t0\t" + seq + "\t" + qual + (i % 5 == 0 ? "\tNM:i:0\tXX:Z:a b" : "") + eol;
}

bool samCases() {
    std::vector<std::string> lines = {"@HD\tVN:1.6\tSO:unsorted\n", "@SQ\tSN:chr1\tLN:1000\r\n", "@CO\ta comment\n"};
    for (int i = 0; i < 20; ++i) lines.push_back(samLine(i, i % 6 == 2 ? "\r\n" : "\n"));
    std::string text;
    for (const std::string &l : lines) text += l;
    text.pop_back();                                            // the last line without its '\n'
    const std::string plain = writeFile("reads.sam", text), gz = writeFile("reads.sam.gz", text, true);
    size_t runs = 0;
    for (bool fastq : {false, true}) {
        const Outcome whole = samStatement(text, fastq);
        if (whole.total != 20 || whole.headers != 3 || whole.kept * 4 < 20 || (whole.total - whole.missing - whole.kept) * 4 < 20 || !whole.missing || !whole.message.empty())
            return fail("the SAM text itself: " + show(whole));
        // every block size for either output; the input (plain, gzip) and the batch (3 reads, all) take their six pairings in turn
        for (size_t bytes = 64; bytes <= text.size() + 1; ++bytes, ++runs) {
            const Outcome got = samRoute(bytes % 2 ? gz : plain, bytes % 3 == 0 ? 3 : 1000, bytes, fastq);
            if (!same(got, whole)) return fail("SAM, " + std::to_string(bytes) + " bytes, FASTQ out " + std::to_string(fastq) + ": " + show(got) + "; the statement: " + show(whole));
        }
    }
    std::printf("ok sam-every-block %zu\n", runs);

    // a line that fails a check: the line number, and everything ahead of the line written, whatever the block size
    runs = 0;
    for (int kind = 0; kind < 4; ++kind) {
        std::string t;
        for (size_t i = 0; i < lines.size(); ++i) {
            std::string l = lines[i];
            const size_t seqAt = i >= 3 ? l.find("\t0\t0\t") + 5 : 0;
            if (i == 19 && kind == 0) l = "@CO\tlate\n";
            if (i == 19 && kind == 1) l.erase(l.find('\t'), 2);                   // ten fields: FLAG and its tab gone ("\t0": i = 19 has FLAG 0)
            if (i == 19 && kind == 2) l.erase(seqAt, l.find('\t', seqAt) - seqAt);
            if (i == 19 && kind == 3) l.insert(seqAt, "A");
            t += l;
        }
        for (bool fastq : {false, true}) {
            const Outcome want = samStatement(t, fastq);
            if (!startsWith(want.message, "SAM line 20: ")) return fail("SAM failure " + std::to_string(kind) + " is none: " + show(want));
            const std::string p = writeFile("bad.sam", t);
            for (size_t bytes : {size_t(64), size_t(101), size_t(1000), t.size() + 1}) {
                const Outcome got = samRoute(p, bytes == 101 ? 2 : 1000, bytes, fastq);
                ++runs;
                if (got.message != want.message || got.out != want.out) return fail("SAM failure " + std::to_string(kind) + ", " + std::to_string(bytes) + " bytes: " + show(got) + "; the statement: " + show(want));
            }
        }
    }
    const Outcome empty = samRoute(writeFile("empty.sam", ""), 7, 64, false);
    if (empty.message != "SAM input is empty") return fail("empty SAM: " + show(empty));
    std::printf("ok sam-failures %zu\n", runs);
    return true;
}

// ------------------------------------------------------------------------------------------------ BAM
void put32(std::string &s, uint32_t v) { for (int i = 0; i < 4; ++i) s.push_back(static_cast<char>(v >> (8 * i))); }

struct BamRead { std::string name, seq, qual; uint16_t flag; };  // qual: raw values; empty with bases = missing (0xff)
std::string bamRecord(const BamRead &r) {
    auto code = [](char c) { return c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 4 : 8; };      // of "=ACMGRSVTWYHKDBN"
    std::string b;
    put32(b, 0); put32(b, 100);                                 // refID, pos
    b.push_back(static_cast<char>(r.name.size() + 1)); b.push_back(60); b.push_back(0); b.push_back(0);      // l_read_name, mapq, bin
    b.push_back(1); b.push_back(0);                             // n_cigar_op
    b.push_back(static_cast<char>(r.flag & 255)); b.push_back(static_cast<char>(r.flag >> 8));
    put32(b, static_cast<uint32_t>(r.seq.size()));
    put32(b, 0xffffffffu); put32(b, 0xffffffffu); put32(b, 0);  // next refID, next pos, tlen
    b += r.name; b.push_back(0);
    put32(b, static_cast<uint32_t>(r.seq.size()) << 4);         // one CIGAR op
    for (size_t i = 0; i < r.seq.size(); i += 2)
        b.push_back(static_cast<char>(code(r.seq[i]) << 4 | (i + 1 < r.seq.size() ? code(r.seq[i + 1]) : 0)));
    b += r.qual.empty() ? std::string(r.seq.size(), static_cast<char>(0xff)) : r.qual;
    b += "NMC"; b.push_back(0);                                 // a tag
    std::string rec;
    put32(rec, static_cast<uint32_t>(b.size()));
    return rec + b;
}
// BGZF members of 0xff00 payload bytes each (the last one shorter), the EOF marker behind them where asked for
std::string bgzf(const std::string &plain, bool eofMarker) {
    static const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    std::string out;
    std::vector<unsigned char> comp(70000);
    for (size_t at = 0; at < plain.size(); at += 0xff00) {
        const size_t n = std::min<size_t>(0xff00, plain.size() - at);
        z_stream zs{};
        if (deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2");
        zs.next_in = reinterpret_cast<unsigned char *>(const_cast<char *>(plain.data() + at)); zs.avail_in = static_cast<unsigned>(n);
        zs.next_out = comp.data(); zs.avail_out = static_cast<unsigned>(comp.size());
        if (deflate(&zs, Z_FINISH) != Z_STREAM_END) throw std::runtime_error("deflate");
        const size_t clen = zs.total_out, total = 18 + clen + 8;
        deflateEnd(&zs);
        out.append(reinterpret_cast<const char *>(head), 16);
        out.push_back(static_cast<char>((total - 1) & 255)); out.push_back(static_cast<char>((total - 1) >> 8));
        out.append(reinterpret_cast<const char *>(comp.data()), clen);
        put32(out, static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const unsigned char *>(plain.data() + at), static_cast<unsigned>(n))));
        put32(out, static_cast<uint32_t>(n));
    }
    static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (eofMarker) out.append(reinterpret_cast<const char *>(eof), sizeof eof);
    return out;
}
std::string gunzipFile(const std::string &path) {               // every member of the file, inflated
    gzFile g = gzopen(path.c_str(), "rb");
    if (!g) throw std::runtime_error("cannot open " + path);
    std::string s;
    std::vector<char> buf(1u << 20);
    for (int n; (n = gzread(g, buf.data(), static_cast<unsigned>(buf.size()))) > 0;) s.append(buf.data(), static_cast<size_t>(n));
    gzclose(g);
    return s;
}

// The statement: the stream is the header and then records, each a block_size and that many bytes; a read without bases is
// counted and never kept; BAM out is the header and the kept records as they are; FASTQ out is '@' name, the bases, '+', the
// quals as min(q, 93) + 33 — reverse-complemented and reversed where FLAG has 0x10, '!' for every base where the quals are 0xff.
Outcome bamStatement(const std::string &header, const std::vector<BamRead> &reads, bool fastq) {
    Outcome o;
    if (!fastq) o.out = header;
    for (const BamRead &r : reads) {
        ++o.total;
        if (r.seq.empty()) { ++o.missing; continue; }
        if (r.seq.find(kMotif) == std::string::npos) continue;
        ++o.kept;
        if (!fastq) { o.out += bamRecord(r); continue; }
        const bool reverse = (r.flag & 0x10) != 0;
        std::string q = std::string(r.seq.size(), '!');
        for (size_t i = 0; i < r.qual.size(); ++i) q[i] = static_cast<char>(std::min<int>(static_cast<unsigned char>(r.qual[i]), 93) + 33);
        o.out += "@" + r.name + "\n" + (reverse ? reverseComplement(r.seq) : r.seq) + "\n+\n" + (reverse ? std::string(q.rbegin(), q.rend()) : q) + "\n";
    }
    return o;
}
Outcome bamRoute(const std::string &path, size_t readsPerBatch, bool fastq) {
    Outcome o;
    const std::string outPath = dir + "/subset.out";
    Judge judge;
    const ReadFastqOutput asFastq;
    {
        std::ofstream out(outPath, std::ios::binary);
        try {
            const BamSubsetStats s = bamSubsetHost(path, out, judge, readsPerBatch, size_t(1) << 20, nullptr, fastq ? &asFastq : nullptr);
            o.kept = s.passedRecords; o.total = s.totalRecords; o.missing = s.missingSequenceRecords; o.noEof = s.missingEofBlock;
        } catch (const std::exception &e) { o.message = e.what(); }
    }
    if (fastq) { std::ifstream f(outPath, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); o.out = ss.str(); }
    else if (o.message.empty()) o.out = gunzipFile(outPath);
    return o;
}

bool bamCases() {
    std::string header = "BAM\1";
    const std::string text = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:5000000\n";
    put32(header, static_cast<uint32_t>(text.size())); header += text;
    put32(header, 1); put32(header, 5); header += std::string("chr1\0", 5); put32(header, 5000000);
    uint32_t rng = 12345;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    auto read = [&](int i, size_t len) {
        BamRead r;
        r.name = "read" + std::to_string(i);
        r.flag = i % 3 == 0 ? 0x10 : 0;
        for (size_t k = 0; k < len; ++k) r.seq.push_back("ACGT"[next() & 3]);
        if (i % 2 == 0 && len >= 40) r.seq.replace(len / 3, kMotif.size(), kMotif);         // (random bases hold the motif once in 16 M places)
        if (i % 5 != 4) for (size_t k = 0; k < len; ++k) r.qual.push_back(static_cast<char>(next() % 100));    // (some above 93)
        return r;
    };
    // reads of up to 20 k bases; the large one begins late in the first 1 MiB block of the stream — 16 members, 0xff00 bytes each —
    // so that what the second block leaves unconsumed, the record's first bytes, is more than the 1 MiB of headroom
    std::vector<BamRead> reads;
    std::string stream = header;
    const size_t fillBytes = 16 * 0xff00, largeAt = fillBytes - 40000;
    for (int i = 0; largeAt - stream.size() > 100; ++i) {
        const size_t room = largeAt - stream.size(), len = i % 9 == 7 ? 0 : 1 + next() % 20000;
        reads.push_back(read(i, room < 40000 ? (room - 70) * 2 / 3 : len));       // (the last one ends a little short of largeAt)
        stream += bamRecord(reads.back());
    }
    const size_t largeStart = stream.size();
    reads.push_back(read(1000, 800000));                        // 1.2 MB of record
    stream += bamRecord(reads.back());
    const size_t largeSize = stream.size() - largeStart;
    if (largeStart >= fillBytes || largeStart + largeSize <= 2 * fillBytes || 2 * fillBytes - largeStart <= (size_t(1) << 20))
        return fail("the BAM stream itself: the large record at " + std::to_string(largeStart) + ", " + std::to_string(largeSize) + " bytes");
    for (int i = 2000; stream.size() < 3000000; ++i) { reads.push_back(read(i, i % 9 == 7 ? 0 : 1 + next() % 20000)); stream += bamRecord(reads.back()); }
    size_t telomeric = 0, bases = 0;
    for (const BamRead &r : reads) { telomeric += r.seq.find(kMotif) != std::string::npos; bases += !r.seq.empty(); }
    if (telomeric * 4 < reads.size() || (bases - telomeric) * 4 < reads.size()) return fail("the BAM reads themselves");

    const std::string path = writeFile("reads.bam", bgzf(stream, true));
    size_t runs = 0;
    for (bool fastq : {false, true}) {
        const Outcome whole = bamStatement(header, reads, fastq);
        for (size_t readsPerBatch : {size_t(1), size_t(97), size_t(1) << 20}) {
            const Outcome got = bamRoute(path, readsPerBatch, fastq);
            ++runs;
            if (!same(got, whole) || got.noEof) return fail("BAM, " + std::to_string(readsPerBatch) + " reads, FASTQ out " + std::to_string(fastq) + ": " + show(got) + "; the statement: " + show(whole));
        }
    }
    std::printf("ok bam-large-record %zu\n", runs);

    const Outcome whole = bamStatement(header, reads, false);
    const Outcome noEof = bamRoute(writeFile("noeof.bam", bgzf(stream, false)), 97, false);
    if (!same(noEof, whole) || !noEof.noEof) return fail("BAM without the EOF marker: " + show(noEof));
    const size_t lastSize = bamRecord(reads.back()).size();
    const Outcome cutRecord = bamRoute(writeFile("cut.bam", bgzf(stream.substr(0, stream.size() - lastSize / 2), true)), 97, false);
    if (cutRecord.message != "truncated BAM record") return fail("BAM with half a last record: " + show(cutRecord));
    const Outcome cutSize = bamRoute(writeFile("cut.bam", bgzf(stream.substr(0, stream.size() - lastSize + 2), true)), 97, true);
    std::vector<BamRead> allButLast(reads.begin(), reads.end() - 1);
    if (cutSize.message != "truncated BAM record size" || cutSize.out != bamStatement(header, allButLast, true).out) return fail("BAM with half a last block_size: " + show(cutSize));
    const Outcome missing = bamRoute(dir + "/no-such-file", 97, false);
    if (missing.message != "cannot open BAM input '" + dir + "/no-such-file'") return fail("BAM input that is not there: " + show(missing));
    std::printf("ok bam-ends 4\n");
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: read_host_routes_host DIR\n"); return 2; }
    dir = argv[1];
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    try {
        if (!blockReaderCases() || !fastqCases() || !samCases() || !bamCases()) return 1;
    } catch (const std::exception &e) { std::printf("FAILED: %s\n", e.what()); return 1; }
    std::printf("ok\n");
    return 0;
}
