// teloscope_mi355x_reads_host.hpp — the host routes of the four read subsets, fastqSubset, bamSubset / bamSubsetFastq,
// samSubset / samSubsetFastq and fastaSubset: the defaults of the product and what every device read route is compared with.  A route opens its
// input (detail::MappedInput), reads it a block at a time with the next block filled behind it (detail::BlockReader), finds the
// records of a block by its format's rule, and hands them in batches to one judge-and-echo step (detail::HostReadJudge).  The
// route bodies are templates over the judge — anything with matchesPointers(seqs, lens, n, pass) and context(i) — so that all
// of this runs without a device: tests/cpp/read_host_routes_host.cpp.  The public functions pass a ReadTelomereFilter through.
// teloscope_mi355x_io.hpp includes this header; the device routes take BgzfWriter, BamHeaderParser, parseBgzfBlock and
// MappedInput from here.
#ifndef TELOSCOPE_MI355X_READS_HOST_HPP
#define TELOSCOPE_MI355X_READS_HOST_HPP

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <ostream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include "teloscope_mi355x.hpp"
#include "../teloscope_amd/csrc/read_block_format_core.h"
#include "../teloscope_amd/csrc/fastq_pair_core.h"
#include "../teloscope_amd/csrc/read_fastq_format_core.h"

namespace teloscope_mi355x {

// ---- what the routes share: the clock, the host threads, the input, the block reader, the judge step ----
namespace detail {
using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }    // ms

template <typename F>
inline void onThreads(size_t n, F &&f) {                        // f(i) for i in [0, n), dynamic, on up to 16 host threads
    const unsigned nt = static_cast<unsigned>(std::min<size_t>({size_t(16), n, size_t(std::max(1u, std::thread::hardware_concurrency()))}));
    if (nt <= 1) { for (size_t i = 0; i < n; ++i) f(i); return; }
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t) pool.emplace_back([&] { for (size_t i; (i = next.fetch_add(1)) < n;) f(i); });
    for (std::thread &th : pool) th.join();
}

// An input's descriptor and, for a regular file that is not empty and can be mapped, its bytes (`map` = false: a route that never
// looks at them, or that calls mapFile() once it knows it will).  `-` is stdin where the route says so; descriptor 0 is never closed from here (gzclose of a stream opened on it
// closes it, as it always did).
struct MappedInput {
    int fd = 0;
    bool owned = false;
    gzFile gz = nullptr;
    const unsigned char *data = nullptr;
    size_t size = 0;
    MappedInput(const std::string &file, bool dashIsStdin, const std::string &cannotOpen, bool map = true) {
        if (!dashIsStdin || file != "-") {
            fd = ::open(file.c_str(), O_RDONLY);
            if (fd < 0) throw std::runtime_error(cannotOpen);
            owned = true;
        }
        if (map) mapFile();
    }
    void mapFile() {
        struct stat st;
        if (!data && ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
            void *m = ::mmap(nullptr, static_cast<size_t>(st.st_size), PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) { data = static_cast<const unsigned char *>(m); size = static_cast<size_t>(st.st_size); ::madvise(m, size, MADV_SEQUENTIAL); }
        }
    }
    MappedInput(const MappedInput &) = delete;
    MappedInput &operator=(const MappedInput &) = delete;
    ~MappedInput() {
        if (data) ::munmap(const_cast<unsigned char *>(data), size);
        if (gz) gzclose(gz); else if (owned) ::close(fd);
    }
    // The descriptor, from where it stands, read through zlib (which passes bytes that are not gzip on as they are): `always`, or
    // only where the file begins with gzip's magic.  -> whether it is
    bool openZlib(bool always, const std::string &cannotOpen) {
        if (!always) {
            unsigned char magic[2] = {0, 0};
            if (!(::pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b)) return false;
        }
        gz = gzdopen(fd, "rb");
        if (!gz) throw std::runtime_error(cannotOpen);
        gzbuffer(gz, 1u << 20);
        return true;
    }
    // the next bytes of the descriptor, through zlib where it was opened so: their number, 0 at the end, < 0 on an error
    long get(char *dst, size_t n) {
        n = std::min<size_t>(n, size_t(1) << 30);
        return gz ? gzread(gz, dst, static_cast<unsigned>(n)) : static_cast<long>(::read(fd, dst, n));
    }
    // a BlockReader's fill: dst[0, cap) or up to the input's end, read in order
    size_t fill(char *dst, size_t cap, bool &last, const char *cannotRead) {
        size_t got = 0;
        while (got < cap) {
            const long n = get(dst + got, cap - got);
            if (n < 0) throw std::runtime_error(cannotRead);
            if (n == 0) { last = true; break; }
            got += static_cast<size_t>(n);
        }
        return got;
    }
    // what did not map (a pipe, stdin) read to its end
    void readToEnd(std::vector<unsigned char> &into, const char *cannotRead) const {
        for (;;) {
            const size_t at = into.size();
            into.resize(at + (8u << 20));
            const ssize_t r = ::read(fd, into.data() + at, 8u << 20);
            if (r < 0) throw std::runtime_error(cannotRead);
            into.resize(at + static_cast<size_t>(r));
            if (r == 0) break;
        }
    }
};

// An input in blocks, for a caller that consumes whole records and leaves the unfinished one at a block's end.  fill(dst, cap,
// last) brings up to cap new bytes and says whether the input ended with them.  Two buffers in turn: while the caller works on one
// block the other is filled on a thread of its own, its data `headroom` bytes into its buffer, and next(left) puts the last `left`
// bytes of the block before in front of it without moving it.  A leftover larger than the headroom (a record larger than a
// block) moves the block once, and the headroom is that large from then on.  A fill's exception is thrown by the next() that
// would hand its block out, so after the block before it has been worked on.  Everything the fill refers to outlives the reader.
class BlockReader {
public:
    struct Block { char *begin = nullptr, *end = nullptr; bool last = false; };
    using Fill = std::function<size_t(char *dst, size_t cap, bool &last)>;
    BlockReader(Fill fill, size_t blockBytes, size_t headroom) : fill_(std::move(fill)), block_(blockBytes), head_(headroom) {}
    BlockReader(const BlockReader &) = delete;
    BlockReader &operator=(const BlockReader &) = delete;

    // The next block; not called again behind the last one.
    Block next(size_t left = 0) {
        if (!ahead_.valid()) load(buf_[cur_]);                  // the first block
        else {
            ahead_.get();
            const Buf &c = buf_[cur_];
            Buf &n = buf_[cur_ ^= 1];
            if (left > n.begin) {
                const size_t have = n.end - n.begin;
                head_ = left;
                std::unique_ptr<char[]> grown(new char[head_ + block_]);
                std::memcpy(grown.get() + head_, n.data.get() + n.begin, have);
                n.data.swap(grown);
                n.cap = head_ + block_; n.begin = head_; n.end = head_ + have;
            }
            if (left) std::memcpy(n.data.get() + n.begin - left, c.data.get() + c.end - left, left);
            n.begin -= left;
        }
        Buf &b = buf_[cur_];
        if (!b.last) ahead_ = std::async(std::launch::async, [this] { load(buf_[cur_ ^ 1]); });
        return Block{b.data.get() + b.begin, b.data.get() + b.end, b.last};
    }
    // milliseconds spent in fills so far (read between a next() and the work on its block, or behind the last block)
    double msFill() const { return msFill_; }

private:
    struct Buf { std::unique_ptr<char[]> data; size_t cap = 0, begin = 0, end = 0; bool last = false; };
    void load(Buf &b) {
        const Clock::time_point t0 = Clock::now();
        if (b.cap < head_ + block_) { b.cap = head_ + block_; b.data.reset(new char[b.cap]); }
        b.last = false;
        b.begin = b.end = head_;
        b.end += fill_(b.data.get() + head_, block_, b.last);
        msFill_ += since(t0);
    }
    Fill fill_;
    const size_t block_;
    size_t head_;
    Buf buf_[2];
    int cur_ = 0;
    double msFill_ = 0;
    std::future<void> ahead_;                                   // (the last member: its destructor waits for a running fill)
};

// The library's first call in a process pays for its streams, its kernels' code, the device pool and the pinned staging (about
// 75 ms, whatever the size of the call).  The subset tools make it here, on one dummy read and a thread of its own, while their
// first block of input is still being read and parsed; joined before the first real batch.
template <typename Filter>
class FilterWarmUp {
    std::thread th;
public:
    explicit FilterWarmUp(Filter &filter) {
        th = std::thread([&filter] {
            try {
                const std::string seq(4096, 'A');
                const char *p = seq.data();
                uint64_t l = seq.size();
                uint8_t pass = 0;
                filter.matchesPointers(&p, &l, 1, &pass);
            } catch (...) {}
        });
    }
    void join() { if (th.joinable()) th.join(); }
    ~FilterWarmUp() { join(); }
    FilterWarmUp(const FilterWarmUp &) = delete;
    FilterWarmUp &operator=(const FilterWarmUp &) = delete;
};

// The read block report of the host routes (the rule: include/teloscan.h, "The read block report"; the output is this project's
// own, its columns those of the terminal loop of the reference's writeBEDFile, src/teloscope.cpp).  A route adds the reads it keeps
// of a batch, in output order; flush() scans them once more as tips-only segments at abs_pos 0 on the filter's context
// (ts_scan_segments_blocks: the blocks the filter's bit was made from), formats a line per terminal block with the core header the
// device formatter compiles, and writes them.  Without a stream nothing is kept and nothing runs.
class ReadBlockReport {
public:
    uint64_t lines = 0;
    ReadBlockReport(std::ostream *os, const char *failed) : os_(os), failed_(failed) {}
    bool on() const { return os_ != nullptr; }
    void add(const char *name, uint32_t nameLen, const char *seq, uint64_t len) { if (os_) kept_.push_back(Kept{name, nameLen, seq, len}); }
    void flush(ts_ctx *ctx) {
        if (!os_ || kept_.empty()) return;
        segs_.assign(kept_.size(), ts_segment_in{});
        outs_.assign(kept_.size(), ts_segment_out{});
        for (size_t i = 0; i < kept_.size(); ++i) { segs_[i].seq = kept_[i].seq; segs_[i].len = kept_[i].len; segs_[i].tips_only = 1; }
        if (ts_scan_segments_blocks(ctx, segs_.data(), segs_.size(), outs_.data(), nullptr) != TS_OK) throw std::runtime_error(std::string("block calling of the kept reads failed: ") + ts_last_error(ctx));
        text_.clear();
        for (size_t i = 0; i < kept_.size(); ++i)
            for (uint64_t j = 0; j < outs_[i].n_terminal_blocks; ++j) {
                const ts_block &b = outs_[i].terminal_blocks[j];
                const tsrb::Fields f{b.start, b.block_len, b.forward_count, b.reverse_count, b.canonical_count, b.non_canonical_count,
                                     static_cast<uint32_t>(kept_[i].len), static_cast<uint32_t>(static_cast<unsigned char>(b.block_label))};
                const size_t at = text_.size();
                text_.resize(at + tsrb::line_len(kept_[i].nameLen, f));
                Sink sink{&text_[at]};
                tsrb::put_line(sink, 0u, Bytes{kept_[i].name}, 0, kept_[i].nameLen, f);
                ++lines;
            }
        ts_free_segments(outs_.data(), outs_.size());
        kept_.clear();
        os_->write(text_.data(), static_cast<std::streamsize>(text_.size()));
        if (!os_->good()) throw std::runtime_error(failed_);
    }
    struct Bytes { const char *p; uint32_t byte(uint64_t i) const { return static_cast<unsigned char>(p[i]); } };

private:
    struct Kept { const char *name; uint32_t nameLen; const char *seq; uint64_t len; };
    struct Sink { char *p; void put(uint32_t at, uint32_t byte) { p[at] = static_cast<char>(byte); } };
    std::ostream *os_;
    const char *failed_;
    std::vector<Kept> kept_;
    std::vector<ts_segment_in> segs_;
    std::vector<ts_segment_out> outs_;
    std::string text_;
};

// The judge-and-echo step of the three routes, over the filter, its warm-up and the block report.  run() takes a batch of n
// records: seqOf(i, seq, len) says whether record i has bases to judge and where; the filter judges those (it is not called for
// none); keep(i, seq, len) is called for every passing one, in order — there the route appends the record's bytes and names the
// read for the report; written() follows, where the route writes what it appended; then the report's lines of the kept reads
// are called and written.  -> how many passed.  (a batch with nothing to judge ends at once: nothing was appended, so
// written() is not called either — an output stream that is already bad is then noticed at the next batch that keeps something, or
// where the route finishes, with the same text)
template <typename Filter>
class HostReadJudge {
public:
    ReadBlockReport report;
    double msFilter = 0;                                        // the warm-up's join and the filter's calls
    HostReadJudge(Filter &filter, std::ostream *blocks, const char *reportFailed) : report(blocks, reportFailed), filter_(filter), warmUp_(filter) {}
    template <typename SeqOf, typename Keep, typename Written>
    uint64_t run(size_t n, SeqOf &&seqOf, Keep &&keep, Written &&written) {
        ptr_.clear(); len_.clear(); idx_.clear();
        for (size_t i = 0; i < n; ++i) {
            const char *seq = nullptr;
            uint64_t len = 0;
            if (seqOf(i, seq, len)) { ptr_.push_back(seq); len_.push_back(len); idx_.push_back(i); }
        }
        if (ptr_.empty()) return 0;
        pass_.assign(ptr_.size(), 0);
        const Clock::time_point t0 = Clock::now();
        warmUp_.join();
        filter_.matchesPointers(ptr_.data(), len_.data(), ptr_.size(), pass_.data());
        msFilter += since(t0);
        uint64_t kept = 0;
        for (size_t k = 0; k < idx_.size(); ++k)
            if (pass_[k]) { keep(idx_[k], ptr_[k], len_[k]); ++kept; }
        written();
        report.flush(filter_.context(0));
        return kept;
    }

private:
    Filter &filter_;
    FilterWarmUp<Filter> warmUp_;
    std::vector<const char *> ptr_;
    std::vector<uint64_t> len_;
    std::vector<size_t> idx_;
    std::vector<uint8_t> pass_;
};
}  // namespace detail

// FASTQ out of the BAM and SAM subsets (the rule: include/teloscan.h, "FASTQ out of the BAM and SAM subsets"): what
// bamSubsetFastq, samSubsetFastq and their device forms write in place of the kept records' own bytes.  restoreStrand: a record
// whose FLAG has 0x10 set is written reverse-complemented, its quals reversed (TS_FASTQ_OUT_RESTORE_STRAND) — the read as the
// sequencer gave it; false writes SEQ and QUAL as stored.
struct ReadFastqOutput { bool restoreStrand = true; };

namespace detail {
inline uint32_t fastqOutFlags(const ReadFastqOutput &f) { return f.restoreStrand ? TS_FASTQ_OUT_RESTORE_STRAND : 0u; }
// a located record's text behind `text`: the host routes' formatter, every byte from the core header the device compiles
inline void appendFastqText(std::string &text, const char *bytes, const tsfq::Rec &r) {
    const size_t at = text.size(), n = static_cast<size_t>(tsfq::record_len(r));
    text.resize(at + n);
    const ReadBlockReport::Bytes b{bytes};
    // (the lines one after the other: out_byte's bytes, without its search for the line a byte lies in)
    char *p = &text[at];
    *p++ = '@';
    std::memcpy(p, bytes + r.name_off, r.name_len); p += r.name_len;
    *p++ = '\n';
    for (uint32_t j = 0; j < r.len; ++j) *p++ = static_cast<char>(tsfq::base_at(b, r, j));
    *p++ = '\n'; *p++ = '+'; *p++ = '\n';
    for (uint32_t j = 0; j < r.len; ++j) *p++ = static_cast<char>(tsfq::qual_at(b, r, j));
    *p++ = '\n';
}
}  // namespace detail

// ---------------------------------------------------------------------------------------------
// --fastq-subset (Input::readFastqSubset, src/input.cpp:737-832): echo the reads that carry a terminal
// telomere block, in input order, byte for byte.  Records are read by the 4-line rules of
// readFastqRecord (src/input.cpp:113-138: blank lines before a header are skipped, line contents are
// kept verbatim, '\r' included) from a plain or gzip file ("-" = stdin) and filtered in batches of up
// to readsPerBatch reads / basesPerBatch bases — a GPU batch, not the reference's 2048-record one.
// Malformed input throws std::runtime_error with the reference's message.
struct FastqSubsetResult { uint64_t kept = 0, total = 0, blockLines = 0; };     // blockLines: lines of the read block report, if one was asked for

namespace detail {
inline size_t logicalLineLength(const char *b, const char *e) { return (e > b && e[-1] == '\r') ? static_cast<size_t>(e - b) - 1 : static_cast<size_t>(e - b); }

struct FastqRec { const char *begin, *seq, *end; uint64_t seqLen; };           // the four lines [begin, end) without the last '\n'; seqLen: '\r' included

// The FASTQ record rule (readFastqRecord, src/input.cpp:113-138), once: what stands at p of the text [p, end), p < end, which
// is all of the input that is left when `eof` (its last line may then lack its '\n').  Record: `rec`, and `next` is where the
// record behind it starts.  Blank: a blank line in front of a header, `next` is behind it.  NeedMore: the line or record goes
// on beyond `end`.  The four failures, checked in this order, are what the reference reports.
enum class FastqStep { Record, Blank, NeedMore, Truncated, BadHeader, BadSeparator, BadLengths };
inline const char *fastqStepText(FastqStep s) {
    return s == FastqStep::Truncated ? "truncated FASTQ record" : s == FastqStep::BadHeader ? "expected header line starting with '@'"
         : s == FastqStep::BadSeparator ? "expected separator line starting with '+'" : "sequence and quality length differ";
}
inline FastqStep fastqRecordAt(const char *p, const char *end, bool eof, FastqRec &rec, const char *&next) {
    const char *b[4], *e[4];                                    // the lines [b, e): header, sequence, separator, quality
    for (int i = 0; i < 4; ++i) {
        const char *nl = p < end ? static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p))) : nullptr;
        if (p >= end || (!nl && !eof)) return i && eof ? FastqStep::Truncated : FastqStep::NeedMore;
        b[i] = p; e[i] = nl ? nl : end; p = nl ? nl + 1 : end;
        if (i == 0 && logicalLineLength(b[0], e[0]) == 0) { next = p; return FastqStep::Blank; }
    }
    if (*b[0] != '@') return FastqStep::BadHeader;
    if (e[2] == b[2] || *b[2] != '+') return FastqStep::BadSeparator;
    if (logicalLineLength(b[1], e[1]) != logicalLineLength(b[3], e[3])) return FastqStep::BadLengths;
    rec = FastqRec{b[0], b[1], e[3], static_cast<uint64_t>(e[1] - b[1])};
    next = p;
    return FastqStep::Record;
}

// Parses the records that START in [p, limit) of a complete FASTQ text ending at `end` (the last line may lack its '\n').
// Returns where it stopped — the start of the first record at or beyond `limit`, or `end` — or nullptr at the first thing that
// is not a well-formed record (the caller then re-parses sequentially to report it the way the reference does).
inline const char *parseFastqPiece(const char *p, const char *limit, const char *end, std::vector<FastqRec> &out) {
    while (p < limit) {
        FastqRec r{};
        const FastqStep step = fastqRecordAt(p, end, true, r, p);
        if (step == FastqStep::Record) out.push_back(r);
        else if (step != FastqStep::Blank) return nullptr;
    }
    return p;
}

// All records of a mapped FASTQ text, found by the host threads: the text is cut into pieces; a piece starts at the first
// line that looks like a header ('@' first, the line after next begins with '+', the next line does not begin with '@' — a
// quality line may begin with '@', but then the line after it is a header), every piece is parsed on its own, and the
// pieces are accepted only if each parse lands exactly on the next piece's start.  false = not provably well-formed this
// way: parse sequentially instead.
inline bool splitFastqRecords(const char *data, size_t size, std::vector<FastqRec> &records, size_t pieceBytes = size_t(32) << 20) {
    const char *end = data + size;
    const size_t np = std::max<size_t>(1, std::min<size_t>(256, size / std::max<size_t>(pieceBytes, 1)));
    if (np < 2) return false;
    std::vector<const char *> start(np + 1, nullptr);
    start[0] = data; start[np] = end;
    std::atomic<bool> bad{false};
    auto lineAfter = [&](const char *q) -> const char * {                    // start of the line after the one holding q
        const char *nl = static_cast<const char *>(std::memchr(q, '\n', static_cast<size_t>(end - q)));
        return nl ? nl + 1 : end;
    };
    onThreads(np - 1, [&](size_t k) {
        const size_t i = k + 1;
        const char *q = lineAfter(data + size / np * i - 1);                  // a line start at or after the cut
        int tries = 0;
        for (; q < end && tries < 64; ++tries) {
            const char *l1 = lineAfter(q), *l2 = l1 < end ? lineAfter(l1) : end;
            if (*q == '@' && l1 < end && *l1 != '@' && l2 < end && *l2 == '+') break;
            q = l1;
        }
        if (q < end && tries == 64) bad.store(true);                          // 64 lines without a header: not FASTQ-shaped
        start[i] = q < end ? q : end;                                         // (no record starts behind this cut)
    });
    if (bad.load()) return false;
    for (size_t i = 1; i <= np; ++i) if (start[i] < start[i - 1]) return false;
    std::vector<std::vector<FastqRec>> parts(np);
    onThreads(np, [&](size_t i) {
        if (start[i] == start[i + 1] || bad.load()) return;
        parts[i].reserve(static_cast<size_t>(start[i + 1] - start[i]) / 20000 + 16);
        if (parseFastqPiece(start[i], start[i + 1], end, parts[i]) != start[i + 1]) bad.store(true);
    });
    if (bad.load()) return false;
    size_t total = 0;
    for (const auto &v : parts) total += v.size();
    records.clear();
    records.reserve(total);
    for (const auto &v : parts) records.insert(records.end(), v.begin(), v.end());
    return true;
}

// What fastqSubset and fastqSubsetPaired do alike with their input and with a kept record.  The input: `-` is stdin; gzip and stdin
// go through zlib and are never mapped; a regular file that can be mapped is.  blocks() reads what is not mapped in blocks of
// ~bytesPerBatch: parse(begin, end, last) consumes whole units (records, or pairs) and answers where it stopped; the rest goes in
// front of the next block.
struct FastqHostInput {
    MappedInput in;
    bool zlib;
    explicit FastqHostInput(const std::string &inFile) : in(inFile, true, "Stream not successful: " + inFile, false) {
        zlib = in.openZlib(!in.owned, "Stream not successful: " + inFile);
        if (!zlib) in.mapFile();
    }
    template <typename Parse>
    void blocks(size_t bytesPerBatch, Parse &&parse) {
        const size_t blockBytes = std::max<size_t>(bytesPerBatch, 64);
        BlockReader reader([&](char *dst, size_t cap, bool &last) { return in.fill(dst, cap, last, "read error in FASTQ input"); }, blockBytes,
                           std::min<size_t>(blockBytes, 1u << 20));
        size_t left = 0;
        for (bool first = true;; first = false) {
            const BlockReader::Block b = reader.next(left);
            if (first && b.end == b.begin) throw std::runtime_error("FASTQ input is empty");
            if (first && *b.begin != '@') throw std::runtime_error("FASTQ input must start with '@'");
            left = static_cast<size_t>(b.end - parse(b.begin, b.end, b.last));
            if (b.last) break;
        }
    }
};
// a kept record's four lines and a '\n' behind `text`; a passing record's read to the block report
inline void fastqEcho(std::string &text, const FastqRec &r) {
    text.append(r.begin, r.end);
    text.push_back('\n');
}
inline void fastqReportRead(ReadBlockReport &report, const FastqRec &r, const char *seq, uint64_t len) {
    if (report.on())
        report.add(r.begin + 1, tsrb::fastq_name_len(ReadBlockReport::Bytes{r.begin}, 0, static_cast<uint32_t>(seq - r.begin)), seq, logicalLineLength(seq, seq + len));
}

// (the route itself, behind fastqSubset)  A regular file is mapped and parsed where the page cache holds it — the only copy of a
// sequence is the one into the pinned upload ring; gzip, stdin, a FIFO and a file that cannot be mapped are read in blocks.  Either
// way a batch's sequences are handed to the filter as pointers into the text and a kept record is echoed as the byte range of
// its four lines: no per-line copies.
template <typename Filter>
inline FastqSubsetResult fastqSubsetWith(const std::string &inFile, std::ostream &out, Filter &filter, size_t readsPerBatch, size_t bytesPerBatch,
                                         std::ostream *blocks) {
    HostReadJudge<Filter> judge(filter, blocks, "failed while writing the FASTQ subset's block report");
    FastqHostInput input(inFile);
    MappedInput &in = input.in;
    const bool zlib = input.zlib;
    FastqSubsetResult res;
    std::vector<FastqRec> batch;
    std::string text;
    // filters `batch` and echoes the kept records
    auto runBatch = [&]() {
        text.clear();
        res.kept += judge.run(batch.size(),
            [&](size_t i, const char *&seq, uint64_t &len) { seq = batch[i].seq; len = batch[i].seqLen; return true; },
            [&](size_t i, const char *seq, uint64_t len) {
                fastqEcho(text, batch[i]);
                fastqReportRead(judge.report, batch[i], seq, len);
            },
            [&]() {
                out.write(text.data(), static_cast<std::streamsize>(text.size()));
                if (!out.good()) throw std::runtime_error("failed while writing FASTQ subset");
            });
        res.total += batch.size();
        res.blockLines = judge.report.lines;
    };
    // The sequential parser: whole records out of [p, end) — a batch ends at readsPerBatch reads or bytesPerBatch record bytes —
    // filtered and the kept ones echoed; returns the end of the last whole record.
    uint64_t recordNumber = 0;
    auto parseRange = [&](const char *p, const char *const end, const bool eof) -> const char * {
        FastqStep step = FastqStep::Record;
        while (p < end && step != FastqStep::NeedMore) {
            batch.clear();
            for (size_t batchBytes = 0; p < end && batch.size() < readsPerBatch && batchBytes < bytesPerBatch;) {
                FastqRec r{};
                const char *next = p;
                step = fastqRecordAt(p, end, eof, r, next);
                if (step == FastqStep::NeedMore) break;         // the record continues in the next block
                if (step > FastqStep::NeedMore) throw std::runtime_error("FASTQ record " + std::to_string(recordNumber + 1) + ": " + fastqStepText(step));
                if (step == FastqStep::Record) { ++recordNumber; batch.push_back(r); batchBytes += static_cast<size_t>(next - p); }
                p = next;
            }
            runBatch();
        }
        return p;
    };
    if (!zlib && in.data) {
        const char *data = reinterpret_cast<const char *>(in.data);
        if (data[0] != '@') throw std::runtime_error("FASTQ input must start with '@'");
        // a large file's records are located by all host threads at once (one thread walks 3 GB of text in ~0.5 s); anything
        // that is not provably well-formed that way takes the sequential parser, which reports errors the way the reference does
        std::vector<FastqRec> all;
        if (in.size >= (size_t(64) << 20) && splitFastqRecords(data, in.size, all)) {
            for (size_t i = 0; i < all.size();) {
                batch.clear();
                for (size_t batchBytes = 0; i < all.size() && batch.size() < readsPerBatch && batchBytes < bytesPerBatch;) {
                    batchBytes += static_cast<size_t>(all[i].end - all[i].begin) + 1;
                    batch.push_back(all[i++]);
                }
                runBatch();
            }
        } else (void)parseRange(data, data + in.size, true);
        out.flush();
        return res;
    }
    input.blocks(bytesPerBatch, parseRange);                    // (a partial record: in front of the next block)
    out.flush();
    return res;
}
}  // namespace detail

inline FastqSubsetResult fastqSubset(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                     size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 512u << 20, std::ostream *blocks = nullptr) {
    return detail::fastqSubsetWith(inFile, out, filter, readsPerBatch, bytesPerBatch, blocks);
}

// ---------------------------------------------------------------------------------------------
// The read subset of interleaved paired FASTQ (the rule: include/teloscan.h, "Interleaved paired FASTQ"; the reference has no
// paired mode): records 2 j and 2 j + 1 are a pair, a pair whose mate names differ is an error, and a pair is kept, both records
// verbatim, when at least one mate passes the filter.  Input, record rule, judge and block report are fastqSubset's.  A batch is
// whole pairs, up to readsPerBatch records (rounded up to an even number) or bytesPerBatch bytes; with the block reader the
// unfinished pair goes in front of the next block.  Before an exception every whole, well-formed pair in front of the offending
// place has been judged and, if kept, written.
namespace detail {
template <typename Filter>
inline FastqSubsetResult fastqSubsetPairedWith(const std::string &inFile, std::ostream &out, Filter &filter, size_t readsPerBatch, size_t bytesPerBatch,
                                               std::ostream *blocks) {
    HostReadJudge<Filter> judge(filter, blocks, "failed while writing the FASTQ subset's block report");
    FastqHostInput input(inFile);
    readsPerBatch = std::max<size_t>(readsPerBatch + (readsPerBatch & 1u), 2);
    FastqSubsetResult res;
    std::vector<FastqRec> batch;                                // whole pairs
    std::vector<uint8_t> pass;
    std::string text;
    // judges `batch` and echoes the kept pairs
    auto runBatch = [&]() {
        text.clear();
        pass.assign(batch.size(), 0);
        uint64_t written = 0;
        judge.run(batch.size(),
            [&](size_t i, const char *&seq, uint64_t &len) { seq = batch[i].seq; len = batch[i].seqLen; return true; },
            [&](size_t i, const char *seq, uint64_t len) { pass[i] = 1; fastqReportRead(judge.report, batch[i], seq, len); },
            [&]() {
                for (size_t j = 0; j + 1 < batch.size(); j += 2)
                    if (pass[j] || pass[j + 1]) { fastqEcho(text, batch[j]); fastqEcho(text, batch[j + 1]); written += 2; }
                out.write(text.data(), static_cast<std::streamsize>(text.size()));
                if (!out.good()) throw std::runtime_error("failed while writing FASTQ subset");
            });
        res.kept += written;
        res.total += batch.size();
        res.blockLines = judge.report.lines;
        batch.clear();
    };
    auto fail = [&](const std::string &message) {               // what stands in front of the offending place first
        runBatch();
        throw std::runtime_error(message);
    };
    // Whole pairs out of [p, end); returns where the first pair that does not end inside the text begins.
    uint64_t recordNumber = 0;                                  // records of the whole pairs so far
    auto parseRange = [&](const char *p, const char *const end, const bool eof) -> const char * {
        size_t batchBytes = 0;
        for (;;) {
            FastqRec mate[2];
            const char *q = p, *pairStart = nullptr;
            int have = 0;
            bool needMore = false;
            while (have < 2 && q < end) {
                const char *next = q;
                const FastqStep step = fastqRecordAt(q, end, eof, mate[have], next);
                if (step == FastqStep::NeedMore) { needMore = true; break; }
                if (step > FastqStep::NeedMore) fail("FASTQ record " + std::to_string(recordNumber + static_cast<uint64_t>(have) + 1) + ": " + fastqStepText(step));
                if (step == FastqStep::Record && have++ == 0) pairStart = q;
                q = next;
            }
            if (have < 2) {
                if (!needMore && eof && have == 1) fail("FASTQ input ends with an unpaired record");
                if (batch.size()) runBatch();
                return have ? pairStart : q;                    // (blank lines behind the last pair are consumed)
            }
            const ReadBlockReport::Bytes a{mate[0].begin}, b{mate[1].begin};
            if (!tspair::mates(a, 0, static_cast<uint32_t>(mate[0].seq - mate[0].begin), b, 0, static_cast<uint32_t>(mate[1].seq - mate[1].begin)))
                fail("FASTQ records " + std::to_string(recordNumber + 1) + " and " + std::to_string(recordNumber + 2) + " do not have the same name");
            recordNumber += 2;
            batch.push_back(mate[0]); batch.push_back(mate[1]);
            batchBytes += static_cast<size_t>(q - p);
            p = q;
            if (batch.size() >= readsPerBatch || batchBytes >= bytesPerBatch) { runBatch(); batchBytes = 0; }
        }
    };
    if (!input.zlib && input.in.data) {
        const char *data = reinterpret_cast<const char *>(input.in.data);
        if (data[0] != '@') throw std::runtime_error("FASTQ input must start with '@'");
        (void)parseRange(data, data + input.in.size, true);
    } else input.blocks(bytesPerBatch, parseRange);
    out.flush();
    return res;
}
}  // namespace detail

inline FastqSubsetResult fastqSubsetPaired(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                           size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 512u << 20, std::ostream *blocks = nullptr) {
    return detail::fastqSubsetPairedWith(inFile, out, filter, readsPerBatch, bytesPerBatch, blocks);
}

// ---------------------------------------------------------------------------------------------
// --bam-subset (subsetBam, src/bam.cpp:188-259): copy the header and the alignment records whose read
// carries a terminal telomere block, byte for byte, into a new BAM.
//
// BGZF is a series of independent gzip members of at most 64 KB, each carrying its own size ("BC" extra subfield), so the
// input is not read as one stream: a few hundred MB of blocks are LOCATED by walking their headers (validated like
// BgzfReader::loadBlock, src/bgzf.cpp:57-196: FEXTRA set, reserved flag bits clear, exactly one BC subfield of length 2,
// block and uncompressed sizes <= 64 KB, optional file name / comment / header checksum), INFLATED by all host threads
// straight into their places of one buffer (raw inflate must use the whole payload and yield exactly ISIZE bytes, CRC32
// checked), the records in it are walked and validated, and their sequences (4-bit codes "=ACMGRSVTWYHKDBN") are decoded
// by all host threads into one arena that the GPU filters in batches of up to readsPerBatch records.  The output is
// written as BGZF blocks of <= 0xff00 payload bytes (raw deflate + the BC field + CRC32/ISIZE) closed by the EOF marker.
// (Round 2 until here read the input with zlib's gz* API on one thread: 0.14 Gbases/s on a HiFi BAM;
// profiles/r02/bam_subset_rate.txt.)
// (deflatePlainBytes / deflateMemberBytes / msDeflate: what bamSubsetDevice compressed on the device under BamOutputDeflate::Device —
// record bytes in, BGZF member bytes out, milliseconds its contexts spent in ts_bam_chunk_gather_bgzf; zero everywhere else)
struct BamSubsetStats {
    uint64_t totalRecords = 0, passedRecords = 0, missingSequenceRecords = 0; bool missingEofBlock = false;
    uint64_t deflatePlainBytes = 0, deflateMemberBytes = 0; double msDeflate = 0;
    uint64_t blockLines = 0;                    // lines of the read block report, if one was asked for
};

namespace detail {
struct BgzfBlockRef { const unsigned char *payload; uint32_t payloadLen, isize, crc; size_t outOff; };

// The BGZF block that starts at p, of which n bytes are at hand: its total size, or 0 when it is not complete within n
// bytes (more input is needed).  Throws on anything that is not a BGZF block.
inline size_t parseBgzfBlock(const unsigned char *p, size_t n, BgzfBlockRef &ref, bool &eofMarker) {
    static const unsigned char kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto u16 = [](const unsigned char *q) { return static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8); };
    auto u32 = [&](const unsigned char *q) { return u16(q) | (u16(q + 2) << 16); };
    if (n < 12) return 0;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8) throw std::runtime_error("input is not BGZF-compressed BAM (not a BAM file)");
    const unsigned flags = p[3];
    if ((flags & 0x04) == 0 || (flags & 0xe0) != 0) throw std::runtime_error("invalid BGZF gzip flags");
    const size_t xlen = u16(p + 10);
    if (n < 12 + xlen) return 0;
    bool found = false;
    size_t total = 0;
    for (size_t pos = 12; pos < 12 + xlen;) {
        if (12 + xlen - pos < 4) throw std::runtime_error("malformed BGZF extra field");
        const size_t slen = u16(p + pos + 2), end = pos + 4 + slen;
        if (end > 12 + xlen) throw std::runtime_error("malformed BGZF extra subfield");
        if (p[pos] == 'B' && p[pos + 1] == 'C') {
            if (slen != 2 || found) throw std::runtime_error("invalid BGZF BC subfield");
            total = static_cast<size_t>(u16(p + pos + 4)) + 1;
            found = true;
        }
        pos = end;
    }
    if (!found) throw std::runtime_error("BGZF block is missing the BC subfield");
    if (total > 65536 || total < 12 + xlen + 8) throw std::runtime_error("invalid BGZF block size");
    if (n < total) return 0;
    size_t at = 12 + xlen;
    const size_t footer = total - 8;
    auto skipText = [&](const char *what) {
        while (at < footer && p[at] != 0) ++at;
        if (at == footer) throw std::runtime_error(std::string("unterminated BGZF ") + what);
        ++at;
    };
    if (flags & 0x08) skipText("filename");
    if (flags & 0x10) skipText("comment");
    if (flags & 0x02) {
        if (footer - at < 2) throw std::runtime_error("truncated BGZF header checksum");
        const uLong crc = crc32(crc32(0L, Z_NULL, 0), p, static_cast<uInt>(at));
        if (static_cast<uint32_t>(crc & 0xffffu) != u16(p + at)) throw std::runtime_error("BGZF header checksum mismatch");
        at += 2;
    }
    ref.payload = p + at;
    ref.payloadLen = static_cast<uint32_t>(footer - at);
    ref.crc = u32(p + footer);
    ref.isize = u32(p + footer + 4);
    if (ref.isize > 65536) throw std::runtime_error("BGZF uncompressed block is too large");
    eofMarker = total == sizeof kEof && std::memcmp(p, kEof, sizeof kEof) == 0;
    return total;
}

inline void inflateBgzfBlock(const BgzfBlockRef &b, unsigned char *dst) {
    z_stream zs{};
    unsigned char dummy = 0;
    zs.next_in = const_cast<unsigned char *>(b.payload); zs.avail_in = b.payloadLen;
    zs.next_out = b.isize ? dst : &dummy; zs.avail_out = b.isize ? b.isize : 1;
    if (inflateInit2(&zs, -15) != Z_OK) throw std::runtime_error("could not initialize BGZF decompressor");
    const int rc = inflate(&zs, Z_FINISH);
    const bool whole = rc == Z_STREAM_END && zs.total_out == b.isize && zs.total_in == b.payloadLen;
    inflateEnd(&zs);
    if (!whole) throw std::runtime_error("invalid BGZF deflate payload");
    const uLong crc = crc32(crc32(0L, Z_NULL, 0), b.isize ? dst : Z_NULL, b.isize);
    if (static_cast<uint32_t>(crc) != b.crc) throw std::runtime_error("BGZF checksum mismatch");
}

// Uncompressed bytes of a BGZF file or stream, a few hundred MB per call, inflated by all host threads.
class BgzfParallelReader {
    int fd_;
    const unsigned char *map_ = nullptr;        // a regular file is mapped ...
    size_t mapSize_ = 0, mapPos_ = 0;
    std::vector<unsigned char> buf_;            // ... a pipe is read into a buffer (the incomplete block at its end is kept)
    bool streamEof_ = false;
    std::vector<BgzfBlockRef> blocks_;
public:
    bool sawEofMarker = false;
    explicit BgzfParallelReader(int fd) : fd_(fd) {
        struct stat st;
        if (::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
            void *m = ::mmap(nullptr, static_cast<size_t>(st.st_size), PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                map_ = static_cast<const unsigned char *>(m); mapSize_ = static_cast<size_t>(st.st_size);
                ::madvise(m, mapSize_, MADV_SEQUENTIAL);
            }
        }
    }
    ~BgzfParallelReader() { if (map_) ::munmap(const_cast<unsigned char *>(map_), mapSize_); }
    BgzfParallelReader(const BgzfParallelReader &) = delete;
    BgzfParallelReader &operator=(const BgzfParallelReader &) = delete;

    // Inflates the next whole blocks into dst[0 .. cap) (cap >= 64 KB): the number of bytes produced; `more` = false when
    // the input is exhausted.
    size_t next(unsigned char *dst, size_t cap, bool &more) {
        const unsigned char *w;
        size_t wn;
        bool atEnd;
        if (map_) { w = map_ + mapPos_; wn = mapSize_ - mapPos_; atEnd = true; }
        else {
            while (!streamEof_ && buf_.size() < cap) {             // compressed bytes: never more than the uncompressed room
                const size_t at = buf_.size();
                buf_.resize(at + (8u << 20));
                const ssize_t r = ::read(fd_, buf_.data() + at, 8u << 20);
                if (r < 0) throw std::runtime_error("cannot read BAM input");
                buf_.resize(at + static_cast<size_t>(r));
                if (r == 0) streamEof_ = true;
            }
            w = buf_.data(); wn = buf_.size(); atEnd = streamEof_;
        }
        blocks_.clear();
        size_t used = 0, produced = 0;
        while (used < wn) {
            BgzfBlockRef ref{};
            bool eofm = false;
            const size_t total = parseBgzfBlock(w + used, wn - used, ref, eofm);
            if (total == 0) {
                if (atEnd) throw std::runtime_error(wn - used < 12 ? "truncated BGZF header" : "truncated BGZF block");
                break;
            }
            if (produced + ref.isize > cap) break;
            sawEofMarker = sawEofMarker || eofm;
            ref.outOff = produced;
            produced += ref.isize;
            blocks_.push_back(ref);
            used += total;
        }
        if (!blocks_.empty()) {
            const size_t per = 32, tasks = (blocks_.size() + per - 1) / per;
            std::mutex em;
            std::exception_ptr err;
            onThreads(tasks, [&](size_t t) {
                try {
                    for (size_t i = t * per; i < std::min(blocks_.size(), (t + 1) * per); ++i) inflateBgzfBlock(blocks_[i], dst + blocks_[i].outOff);
                } catch (...) { std::lock_guard<std::mutex> g(em); if (!err) err = std::current_exception(); }
            });
            if (err) std::rethrow_exception(err);
        }
        if (map_) mapPos_ += used; else buf_.erase(buf_.begin(), buf_.begin() + static_cast<std::ptrdiff_t>(used));
        more = used > 0 && (map_ ? mapPos_ < mapSize_ : !(streamEof_ && buf_.empty()));
        return produced;
    }
};

class BgzfWriter {
    static constexpr size_t kPayload = 0xff00, kSlot = 65536, kBlocksPerFlush = 64;
    std::ostream &out;
    bool discard = false;                       // nothing is kept and nothing written: a route whose output is not BAM
    std::vector<unsigned char> pending, comp;
    std::vector<size_t> sizes;
    static size_t block(const unsigned char *data, size_t n, unsigned char *slot) {         // one BGZF block into its 64 KB slot
        z_stream zs{};
        if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2 failed");
        zs.next_in = const_cast<unsigned char *>(data); zs.avail_in = static_cast<unsigned>(n);
        zs.next_out = slot + 18; zs.avail_out = kSlot - 18 - 8;
        const int rc = deflate(&zs, Z_FINISH);
        deflateEnd(&zs);
        if (rc != Z_STREAM_END) throw std::runtime_error("BGZF block does not fit");
        const size_t clen = zs.total_out, total = 18 + clen + 8;
        static const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        std::memcpy(slot, head, 16);
        slot[16] = static_cast<unsigned char>((total - 1) & 0xff); slot[17] = static_cast<unsigned char>((total - 1) >> 8);
        const uint32_t crc = static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), data, static_cast<unsigned>(n)));
        unsigned char *tail = slot + 18 + clen;
        for (int i = 0; i < 4; ++i) { tail[i] = static_cast<unsigned char>(crc >> (8 * i)); tail[4 + i] = static_cast<unsigned char>(static_cast<uint32_t>(n) >> (8 * i)); }
        return total;
    }
    // the first `bytes` pending bytes leave as blocks of kPayload (the last one may be shorter), deflated by all host threads
    void flush(size_t bytes) {
        const size_t nb = (bytes + kPayload - 1) / kPayload;
        if (!nb) return;
        comp.resize(nb * kSlot);
        sizes.assign(nb, 0);
        std::mutex em;
        std::exception_ptr err;
        onThreads(nb, [&](size_t i) {
            try { sizes[i] = block(pending.data() + i * kPayload, std::min(kPayload, bytes - i * kPayload), comp.data() + i * kSlot); }
            catch (...) { std::lock_guard<std::mutex> g(em); if (!err) err = std::current_exception(); }
        });
        if (err) std::rethrow_exception(err);
        for (size_t i = 0; i < nb; ++i) out.write(reinterpret_cast<const char *>(comp.data() + i * kSlot), static_cast<std::streamsize>(sizes[i]));
        pending.erase(pending.begin(), pending.begin() + static_cast<std::ptrdiff_t>(bytes));
    }
public:
    explicit BgzfWriter(std::ostream &o, bool discardAll = false) : out(o), discard(discardAll) {}
    void write(const unsigned char *data, size_t n) {
        if (discard) return;
        pending.insert(pending.end(), data, data + n);
        if (pending.size() >= kBlocksPerFlush * kPayload) flush(pending.size() / kPayload * kPayload);      // whole blocks only
    }
    // what is pending becomes members now (the last one may be short)
    void flushPending() { flush(pending.size()); }
    // finished BGZF members, verbatim, behind whatever was pending (which is flushed first)
    void writeMembers(const unsigned char *members, size_t n) {
        flushPending();
        out.write(reinterpret_cast<const char *>(members), static_cast<std::streamsize>(n));
    }
    void finish() {
        if (discard) return;
        flush(pending.size());
        static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        out.write(reinterpret_cast<const char *>(eof), sizeof eof);
        out.flush();
        if (!out.good()) throw std::runtime_error("failed while writing BAM subset");
    }
};
// The BAM header in front of the records — magic, text, reference list — validated like copyBamHeader (src/bam.cpp:75-120:
// text <= 1 GiB, names 1 .. 1 MiB and NUL-terminated, no negative counts or lengths) and copied verbatim to the writer.  The
// bytes are the caller's: have(n) says whether n bytes lie at its cursor, bytes(off) points at them, and the cursor is moved
// past what was copied.  A step that lacks bytes makes parse() return false; it is called again when more bytes have come.
class BamHeaderParser {
    static constexpr uint32_t kMaxHeaderText = 1u << 30, kMaxReferenceName = 1u << 20;
    enum { Magic, Text, Refs, Records } phase = Magic;
    uint32_t ltext = 0, nref = 0, refsDone = 0;
    static uint32_t le32(const unsigned char *p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24); }
public:
    bool done() const { return phase == Records; }
    // the input has ended: what an unfinished header is called
    void requireDone() const { if (phase != Records) throw std::runtime_error(phase == Refs ? "truncated BAM reference" : "truncated BAM header"); }
    template <typename Have, typename Bytes, typename Cursor>
    bool parse(Have &&have, Bytes &&bytes, Cursor &pos, BgzfWriter &writer) {      // true when the header is complete
        for (;;) {
            if (phase == Magic) {
                if (!have(8)) return false;
                if (std::memcmp(bytes(0), "BAM\1", 4) != 0) throw std::runtime_error("input is not a BAM file");
                ltext = le32(bytes(4));
                if (ltext > kMaxHeaderText) throw std::runtime_error("invalid BAM header text length");
                phase = Text;
            } else if (phase == Text) {
                const size_t n = 8 + static_cast<size_t>(ltext) + 4;
                if (!have(n)) return false;
                nref = le32(bytes(8 + static_cast<size_t>(ltext)));
                if (nref > 0x7fffffffu) throw std::runtime_error("invalid BAM reference count");
                writer.write(bytes(0), n);
                pos += n;
                phase = Refs;
            } else if (phase == Refs) {
                if (refsDone == nref) { phase = Records; return true; }
                if (!have(4)) return false;
                const uint32_t lname = le32(bytes(0));
                if (lname == 0 || lname > kMaxReferenceName) throw std::runtime_error("invalid BAM reference name length");
                const size_t n = 4 + static_cast<size_t>(lname) + 4;
                if (!have(n)) return false;
                if (*bytes(4 + static_cast<size_t>(lname) - 1) != 0) throw std::runtime_error("BAM reference name is not NUL-terminated");
                if (le32(bytes(4 + static_cast<size_t>(lname))) > 0x7fffffffu) throw std::runtime_error("invalid BAM reference length");
                writer.write(bytes(0), n);
                pos += n;
                ++refsDone;
            } else {
                return true;
            }
        }
    }
};

// (the route itself, behind bamSubset and bamSubsetFastq: with `fastq` the kept records leave as FASTQ text, and no header, member
// or EOF marker is written)  Uncompressed bytes arrive in blocks of ~bytesPerBatch, inflated behind the block being parsed and
// filtered (BlockReader: its fill spreads the BGZF blocks over the host threads); the head of a record that continues in the
// next block is what a block leaves unconsumed.
template <typename Filter>
inline BamSubsetStats bamSubsetHost(const std::string &inFile, std::ostream &out, Filter &filter, size_t readsPerBatch, size_t bytesPerBatch,
                                    std::ostream *blocks, const ReadFastqOutput *fastq) {
    BamSubsetStats stats;
    HostReadJudge<Filter> judge(filter, blocks, "failed while writing the BAM subset's block report");
    std::string fastqText;
    MappedInput in(inFile, true, "cannot open BAM input '" + inFile + "'", false);
    BgzfParallelReader reader(in.fd);
    auto le32 = [](const unsigned char *p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24); };
    BgzfWriter writer(out, fastq != nullptr);
    BlockReader blocksIn([&](char *dst, size_t cap, bool &last) {
        bool more = false;
        const size_t n = reader.next(reinterpret_cast<unsigned char *>(dst), cap, more);
        last = !more;
        return n;
    }, std::max<size_t>(bytesPerBatch, 1u << 20), 1u << 20);

    const unsigned char *plain = nullptr;       // the bytes being parsed: [plain + pos, plain + plainSize)
    size_t plainSize = 0, pos = 0;
    // header: a step of the parse that lacks bytes returns false and is retried when the next block has been inflated
    BamHeaderParser header;
    auto have = [&](size_t n) { return plainSize - pos >= n; };
    auto bytesAt = [&](size_t off) { return plain + pos + off; };

    struct Rec { size_t rawOff, rawLen, seqAt; uint32_t seqLen; size_t seqOff; };
    std::vector<Rec> recs;
    std::unique_ptr<char[]> seqs;               // the block's decoded sequences, back to back
    size_t seqsCap = 0;
    double msDecode = 0, msRecords = 0;
    // two bases per packed byte
    static const std::array<uint16_t, 256> pairs = [] {
        std::array<uint16_t, 256> t{};
        const char *bases = "=ACMGRSVTWYHKDBN";
        for (unsigned v = 0; v < 256; ++v) {
            const unsigned char two[2] = {static_cast<unsigned char>(bases[v >> 4]), static_cast<unsigned char>(bases[v & 15])};
            uint16_t w;
            std::memcpy(&w, two, 2);
            t[v] = w;
        }
        return t;
    }();
    auto processRecords = [&]() {
        if (recs.empty()) return;
        size_t total = 0;
        for (Rec &r : recs) { r.seqOff = total; total += (static_cast<size_t>(r.seqLen) + 1) & ~size_t(1); }      // even lengths: whole pairs are stored
        if (total > seqsCap) { seqsCap = total + total / 8; seqs.reset(new char[seqsCap]); }
        // decode on all host threads: tasks of ~2 MB of bases
        std::vector<size_t> cut{0};
        for (size_t i = 0, acc = 0; i < recs.size(); ++i) { acc += recs[i].seqLen; if (acc >= (2u << 20)) { cut.push_back(i + 1); acc = 0; } }
        if (cut.back() != recs.size()) cut.push_back(recs.size());
        const Clock::time_point td = Clock::now();
        onThreads(cut.size() - 1, [&](size_t t) {
            for (size_t i = cut[t]; i < cut[t + 1]; ++i) {
                const Rec &r = recs[i];
                const unsigned char *packed = plain + r.seqAt;
                char *dst = seqs.get() + r.seqOff;
                for (size_t j = 0, n = (static_cast<size_t>(r.seqLen) + 1) / 2; j < n; ++j) std::memcpy(dst + 2 * j, &pairs[packed[j]], 2);
            }
        });
        msDecode += since(td);
        for (size_t a = 0; a < recs.size(); a += readsPerBatch) {
            const size_t z = std::min(recs.size(), a + readsPerBatch);
            stats.totalRecords += z - a;
            stats.passedRecords += judge.run(z - a,
                [&](size_t i, const char *&seq, uint64_t &len) {
                    const Rec &r = recs[a + i];
                    if (!r.seqLen) { ++stats.missingSequenceRecords; return false; }
                    seq = seqs.get() + r.seqOff; len = r.seqLen;
                    return true;
                },
                [&](size_t i, const char *seq, uint64_t len) {
                    const Rec &r = recs[a + i];
                    if (fastq) {
                        const ReadBlockReport::Bytes b{reinterpret_cast<const char *>(plain)};
                        appendFastqText(fastqText, b.p, tsfq::bam_locate(b, r.rawOff, static_cast<uint32_t>(r.rawLen - 4), static_cast<uint32_t>(r.seqAt - r.rawOff),
                                                                         r.seqLen, fastqOutFlags(*fastq)));
                    } else writer.write(plain + r.rawOff, r.rawLen);
                    if (judge.report.on()) {
                        const char *rec = reinterpret_cast<const char *>(plain + r.rawOff);
                        judge.report.add(rec + tsrb::kBamNameAt, tsrb::bam_name_len(ReadBlockReport::Bytes{rec}, 0), seq, len);
                    }
                },
                [&]() {
                    if (!fastq) return;
                    out.write(fastqText.data(), static_cast<std::streamsize>(fastqText.size()));
                    fastqText.clear();
                    if (!out.good()) throw std::runtime_error("failed while writing BAM subset");
                });
            stats.blockLines = judge.report.lines;
        }
        recs.clear();
    };

    size_t left = 0;
    for (bool last = false; !last;) {
        const BlockReader::Block b = blocksIn.next(left);       // (the unconsumed tail of the block before in front of it)
        last = b.last;
        const Clock::time_point t1 = Clock::now();
        plain = reinterpret_cast<const unsigned char *>(b.begin); plainSize = static_cast<size_t>(b.end - b.begin);
        pos = 0;
        if (header.done() || header.parse(have, bytesAt, pos, writer)) {
            while (have(4)) {
                const int32_t blockSize = static_cast<int32_t>(le32(plain + pos));
                if (blockSize < 32 || static_cast<uint32_t>(blockSize) > (256u << 20)) throw std::runtime_error("invalid BAM record block_size");   // BAM_MAX_RECORD_SIZE, src/bam.cpp:29
                if (!have(4 + static_cast<size_t>(blockSize))) break;
                const unsigned char *core = plain + pos + 4;
                const uint32_t lname = core[8], ncigar = static_cast<uint32_t>(core[12]) | (static_cast<uint32_t>(core[13]) << 8), lseq = le32(core + 16);
                const uint64_t seqAt = 32ull + lname + 4ull * ncigar;
                if (lname == 0 || lseq > 0x7fffffffu) throw std::runtime_error("invalid BAM record lengths");          // decodeSequence, src/bam.cpp:122-163
                if (seqAt + (static_cast<uint64_t>(lseq) + 1) / 2 + lseq > static_cast<uint64_t>(blockSize))
                    throw std::runtime_error("BAM record fields exceed block_size");
                if (core[32 + lname - 1] != 0) throw std::runtime_error("BAM read name is not NUL-terminated");
                recs.push_back(Rec{pos, 4 + static_cast<size_t>(blockSize), pos + 4 + static_cast<size_t>(seqAt), lseq, 0});
                pos += 4 + static_cast<size_t>(blockSize);
            }
            processRecords();                   // (record offsets point into `plain`: used before the next block is asked for)
        }
        left = plainSize - pos;
        msRecords += since(t1);
    }
    header.requireDone();
    if (left) throw std::runtime_error(left < 4 ? "truncated BAM record size" : "truncated BAM record");
    stats.missingEofBlock = !reader.sawEofMarker;
    writer.finish();
    if (fastq) { out.flush(); if (!out.good()) throw std::runtime_error("failed while writing BAM subset"); }
    if (std::getenv("TS_TIMING"))
        std::fprintf(stderr, "bamSubset: locate + inflate %.0f ms (reader thread), records (walk, decode, filter, write) %.0f ms of which decode %.0f ms, filter %.0f ms\n",
                     blocksIn.msFill(), msRecords, msDecode, judge.msFilter);
    return stats;
}
}  // namespace detail
inline BamSubsetStats bamSubset(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 256u << 20, std::ostream *blocks = nullptr) {
    return detail::bamSubsetHost(inFile, out, filter, readsPerBatch, bytesPerBatch, blocks, nullptr);
}
// --bam-subset with FASTQ out (the rule: include/teloscan.h, "FASTQ out of the BAM and SAM subsets"): bamSubset's arguments,
// statistics and exceptions, and the kept records as four FASTQ lines each in place of a BAM.  The valid records in front of a bad
// one are written first, as bamSubset writes them.
inline BamSubsetStats bamSubsetFastq(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, const ReadFastqOutput &fastq = ReadFastqOutput(),
                                     size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 256u << 20, std::ostream *blocks = nullptr) {
    return detail::bamSubsetHost(inFile, out, filter, readsPerBatch, bytesPerBatch, blocks, &fastq);
}

// ---------------------------------------------------------------------------------------------
// --sam-subset: the read filter over SAM text, the front end the reference names and does not have (docs/algorithm.md: "BAM I/O
// is isolated from scoring so a future SAM parser or optional CRAM backend can reuse the same filter").  The rule — lines, header
// lines, fields, the four checks, "*" sequences and what is written — is stated once in include/teloscan.h above
// ts_sam_chunk_walk; the host route below and the device route follow it, and their output bytes, statistics and exception texts
// are the same.
struct SamSubsetStats { uint64_t headerLines = 0, totalRecords = 0, passedRecords = 0, missingSequenceRecords = 0, blockLines = 0; };   // blockLines: of the read block report

namespace detail {
inline const char *samErrorText(int error) {
    return error == TS_SAM_HEADER_AFTER_RECORD ? "header line after the first alignment record" : error == TS_SAM_TOO_FEW_FIELDS ? "fewer than 11 fields"
         : error == TS_SAM_EMPTY_SEQ ? "empty SEQ field" : "SEQ and QUAL length differ";
}
inline std::runtime_error samLineError(uint64_t line, int error) {
    return std::runtime_error("SAM line " + std::to_string(line) + ": " + samErrorText(error));
}

// The host form of ts_sam_chunk_walk, with its meanings: text[0, size) starts at a line's first byte; the whole lines' header
// extent and record table, the carry, and the lowest line that fails a check, by a sequential pass over the lines.
struct SamWalk {
    std::vector<ts_sam_record> recs;
    uint64_t headerLines = 0, headerEnd = 0, lines = 0, next = 0, errorLine = 0, errorOff = 0;
    int error = TS_SAM_OK;
};
inline void samWalkHost(const char *text, size_t size, bool atEnd, bool inHeader, SamWalk &w) {
    w.recs.clear();
    w.headerLines = w.headerEnd = w.lines = w.next = w.errorLine = w.errorOff = 0;
    w.error = TS_SAM_OK;
    const char *p = text, *const end = text + size;
    bool header = inHeader;
    auto closeHeader = [&]() { if (header) { header = false; w.headerEnd = static_cast<uint64_t>(p - text); } };
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        if (!nl && !atEnd) break;                               // the unfinished last line: the carry
        const char *lineEnd = nl ? nl : end, *next = nl ? nl + 1 : end;
        const char *e = lineEnd > p && lineEnd[-1] == '\r' ? lineEnd - 1 : lineEnd;     // the content's end
        int bad = TS_SAM_OK;
        if (p < lineEnd && *p == '@') {
            if (header) ++w.headerLines; else bad = TS_SAM_HEADER_AFTER_RECORD;
        } else {
            closeHeader();
            const char *tab[11];
            int tabs = 0;
            for (const char *q = p; tabs < 11 && (q = static_cast<const char *>(std::memchr(q, '\t', static_cast<size_t>(e - q)))) != nullptr; ++q) tab[tabs++] = q;
            ts_sam_record r{};
            r.off = static_cast<uint64_t>(p - text); r.size = static_cast<uint32_t>(lineEnd - p);
            if (tabs < 10) bad = TS_SAM_TOO_FEW_FIELDS;
            else {
                const char *seq = tab[8] + 1, *qual = tab[9] + 1, *qualEnd = tabs > 10 ? tab[10] : e;
                const size_t seqLen = static_cast<size_t>(tab[9] - seq), qualLen = static_cast<size_t>(qualEnd - qual);
                const bool seqStar = seqLen == 1 && *seq == '*', qualStar = qualLen == 1 && *qual == '*';
                r.seq_at = static_cast<uint32_t>(seq - p); r.seq_len = static_cast<uint32_t>(seqLen); r.flags = seqStar ? 1u : 0u;
                if (seqLen == 0) bad = TS_SAM_EMPTY_SEQ;
                else if (!seqStar && !qualStar && seqLen != qualLen) bad = TS_SAM_BAD_LENGTHS;
            }
            if (bad == TS_SAM_OK) w.recs.push_back(r);
        }
        if (bad != TS_SAM_OK) {
            w.error = bad; w.errorLine = w.lines; w.errorOff = static_cast<uint64_t>(p - text);
            break;
        }
        ++w.lines;
        p = next;
    }
    w.next = static_cast<uint64_t>(p - text);
    if (header && inHeader) w.headerEnd = w.next;               // every whole line is a header line
}

// (the route itself, behind samSubset and samSubsetFastq: with `fastq` the kept records leave as FASTQ text and no header line is
// written)  The next block is read while this one is judged, as in the FASTQ and BAM routes: an exception thrown here, a
// "SAM line N: ..." among them, reaches the caller when the fill in flight has ended — up to a block from a slow pipe.
template <typename Filter>
inline SamSubsetStats samSubsetHost(const std::string &inFile, std::ostream &out, Filter &filter, size_t readsPerBatch, size_t bytesPerBatch,
                                    std::ostream *blocks, const ReadFastqOutput *fastq) {
    HostReadJudge<Filter> judge(filter, blocks, "failed while writing the SAM subset's block report");
    MappedInput in(inFile, true, "Stream not successful: " + inFile, false);
    in.openZlib(true, "Stream not successful: " + inFile);
    const size_t blockBytes = std::max<size_t>(bytesPerBatch, 64);
    BlockReader reader([&](char *dst, size_t cap, bool &last) { return in.fill(dst, cap, last, "read error in SAM input"); }, blockBytes,
                       std::min<size_t>(blockBytes, 1u << 20));
    readsPerBatch = std::max<size_t>(readsPerBatch, 1);

    SamSubsetStats stats;
    std::string text;
    auto write = [&](const char *p, size_t n) {
        out.write(p, static_cast<std::streamsize>(n));
        if (!out.good()) throw std::runtime_error("failed while writing SAM subset");
    };
    bool inHeader = true;
    uint64_t lines = 0;
    SamWalk walk;
    size_t left = 0;
    for (bool first = true, last = false; !last; first = false) {
        const BlockReader::Block b = reader.next(left);         // (the unfinished line of the block before in front of it)
        last = b.last;
        if (first && b.end == b.begin) throw std::runtime_error("SAM input is empty");
        samWalkHost(b.begin, static_cast<size_t>(b.end - b.begin), last, inHeader, walk);
        if (!fastq) write(b.begin, static_cast<size_t>(walk.headerEnd));
        stats.headerLines += walk.headerLines; stats.totalRecords += walk.recs.size();
        if (walk.headerLines < walk.lines || walk.error != TS_SAM_OK) inHeader = false;
        // the block's records in batches (they point into the block), the kept lines echoed
        for (size_t a = 0; a < walk.recs.size(); a += readsPerBatch) {
            text.clear();
            stats.passedRecords += judge.run(std::min(readsPerBatch, walk.recs.size() - a),
                [&](size_t i, const char *&seq, uint64_t &len) {
                    const ts_sam_record &r = walk.recs[a + i];
                    if (r.flags & 1u) { ++stats.missingSequenceRecords; return false; }      // (SEQ is "*": never kept)
                    seq = b.begin + r.off + r.seq_at; len = r.seq_len;
                    return true;
                },
                [&](size_t i, const char *seq, uint64_t len) {
                    const ts_sam_record &r = walk.recs[a + i];
                    if (fastq) appendFastqText(text, b.begin, tsfq::sam_locate(ReadBlockReport::Bytes{b.begin}, r.off, r.seq_at, r.seq_len, r.size, fastqOutFlags(*fastq)));
                    else {
                        text.append(b.begin + r.off, r.size);
                        text.push_back('\n');
                    }
                    if (judge.report.on()) judge.report.add(b.begin + r.off, tsrb::sam_name_len(ReadBlockReport::Bytes{b.begin + r.off}, 0, r.seq_at), seq, len);
                },
                [&]() { write(text.data(), text.size()); });
            stats.blockLines = judge.report.lines;
        }
        if (walk.error != TS_SAM_OK) { out.flush(); throw samLineError(lines + walk.errorLine + 1, walk.error); }
        lines += walk.lines;
        left = static_cast<size_t>(b.end - b.begin) - static_cast<size_t>(walk.next);
    }
    out.flush();
    return stats;
}
}  // namespace detail
// The host route: lines and fields are found on the host, a block of input at a time, and the sequences are judged in batches of
// up to readsPerBatch through the filter, as fastqSubset does.  Input may be plain or gzip (both through zlib, which passes plain
// bytes on as they are); `-` is stdin.
inline SamSubsetStats samSubset(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 256u << 20, std::ostream *blocks = nullptr) {
    return detail::samSubsetHost(inFile, out, filter, readsPerBatch, bytesPerBatch, blocks, nullptr);
}
// --sam-subset with FASTQ out (the rule: include/teloscan.h, "FASTQ out of the BAM and SAM subsets"): samSubset's arguments,
// statistics and exceptions, and the kept records as four FASTQ lines each; header lines are counted and not written.
inline SamSubsetStats samSubsetFastq(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, const ReadFastqOutput &fastq = ReadFastqOutput(),
                                     size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 256u << 20, std::ostream *blocks = nullptr) {
    return detail::samSubsetHost(inFile, out, filter, readsPerBatch, bytesPerBatch, blocks, &fastq);
}

// ---------------------------------------------------------------------------------------------
// The FASTA read subset: the read filter over reads that come as FASTA text (corrected reads, seqtk seq -A, samtools fasta,
// unitigs and contigs), which the reference has no mode for.  The rule — framing, the two input errors, records without bases,
// what is written, the block report's name — is stated once in include/teloscan.h above ts_fasta_chunk_stage; the host route
// below and the device route (fastaSubsetDevice) follow it, and their output bytes, statistics and exception texts are the same.
struct FastaSubsetStats { uint64_t totalRecords = 0, passedRecords = 0, missingSequenceRecords = 0, blockLines = 0; };   // blockLines: of the read block report

namespace detail {
// The host form of ts_fasta_chunk_walk, with its meanings and without its 32-bit limits: text[0, size) starts at a line's first
// byte; the complete records in order and the carry (`next`: the unfinished record's '>'; without a header line the unfinished
// last line).  Bytes in front of the first header line belong to no record.
struct FastaReadRecord { uint64_t off, textLen, bodyAt, nBases, nameLen; };     // ts_fasta_record's fields; nameLen: the header line behind '>', without its end
struct FastaReadWalk {
    std::vector<FastaReadRecord> recs;
    uint64_t next = 0;
};
inline void fastaWalkHost(const char *text, size_t size, bool atEnd, FastaReadWalk &w) {
    w.recs.clear();
    const char *p = text, *const end = text + size;
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        if (!nl && !atEnd) break;                               // the unfinished last line
        const char *lineEnd = nl ? nl : end, *next = nl ? nl + 1 : end;
        // (a '\r' in front of the '\n'; without one the line ends the input, and the '\r' is its very last byte)
        const char *e = lineEnd > p && lineEnd[-1] == '\r' ? lineEnd - 1 : lineEnd;
        if (*p == '>') {
            if (!w.recs.empty()) w.recs.back().textLen = static_cast<uint64_t>(p - text) - w.recs.back().off;
            w.recs.push_back(FastaReadRecord{static_cast<uint64_t>(p - text), 0, static_cast<uint64_t>(next - p), 0, static_cast<uint64_t>(e - p) - 1});
        } else if (!w.recs.empty()) {
            w.recs.back().nBases += static_cast<uint64_t>(e - p);
        }
        p = next;
    }
    w.next = atEnd ? size : static_cast<uint64_t>(p - text);
    if (w.recs.empty()) return;
    if (atEnd) { w.recs.back().textLen = size - w.recs.back().off; return; }
    w.next = w.recs.back().off;                                 // the last record is open: the next block may continue it
    w.recs.pop_back();
}
// a complete record's bases to dst (room for nBases): its body lines without '\n' and the '\r' the walk left out
inline char *fastaReadBases(const char *p, const char *end, char *dst) {
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        const char *stop = nl ? nl : end;
        const size_t n = static_cast<size_t>((stop > p && stop[-1] == '\r' ? stop - 1 : stop) - p);
        std::memcpy(dst, p, n);
        dst += n;
        p = nl ? nl + 1 : end;
    }
    return dst;
}

// (the route itself)  Shaped like samSubsetHost: a block at a time with the next one read behind it, the block's last record
// carried unless the input ends with it, a block without a complete record grown; per sub-batch the records' bases are joined
// into one buffer, judged, and the kept records echoed as they were read.
template <typename Filter>
inline FastaSubsetStats fastaSubsetHost(const std::string &inFile, std::ostream &out, Filter &filter, size_t readsPerBatch, size_t bytesPerBatch,
                                        std::ostream *blocks) {
    HostReadJudge<Filter> judge(filter, blocks, "failed while writing the FASTA subset's block report");
    MappedInput in(inFile, true, "Stream not successful: " + inFile, false);
    in.openZlib(true, "Stream not successful: " + inFile);
    const size_t blockBytes = std::max<size_t>(bytesPerBatch, 64);
    BlockReader reader([&](char *dst, size_t cap, bool &last) { return in.fill(dst, cap, last, "read error in FASTA input"); }, blockBytes,
                       std::min<size_t>(blockBytes, 1u << 20));
    readsPerBatch = std::max<size_t>(readsPerBatch, 1);

    FastaSubsetStats stats;
    std::string text, bases;
    std::vector<size_t> at;                                     // where each record's bases begin in `bases`
    auto write = [&](const char *p, size_t n) {
        out.write(p, static_cast<std::streamsize>(n));
        if (!out.good()) throw std::runtime_error("failed while writing FASTA subset");
    };
    FastaReadWalk walk;
    size_t left = 0;
    for (bool first = true, last = false; !last;) {
        const BlockReader::Block b = reader.next(left);         // (the unfinished record of the block before in front of it)
        last = b.last;
        const size_t size = static_cast<size_t>(b.end - b.begin);
        if (first && size) {
            if (*b.begin != '>') throw std::runtime_error("FASTA input must start with '>'");
            first = false;
        }
        if (first && last) throw std::runtime_error("FASTA input is empty");
        fastaWalkHost(b.begin, size, last, walk);
        stats.totalRecords += walk.recs.size();
        for (size_t a = 0; a < walk.recs.size(); a += readsPerBatch) {
            const size_t n = std::min(readsPerBatch, walk.recs.size() - a);
            // the sub-batch's bases, one read behind the other
            at.assign(n + 1, 0);
            for (size_t i = 0; i < n; ++i) at[i + 1] = at[i] + static_cast<size_t>(walk.recs[a + i].nBases);
            bases.resize(at[n]);
            for (size_t i = 0; i < n; ++i) {
                const FastaReadRecord &r = walk.recs[a + i];
                if (r.nBases) fastaReadBases(b.begin + r.off + r.bodyAt, b.begin + r.off + r.textLen, &bases[at[i]]);
            }
            text.clear();
            stats.passedRecords += judge.run(n,
                [&](size_t i, const char *&seq, uint64_t &len) {
                    if (walk.recs[a + i].nBases == 0) { ++stats.missingSequenceRecords; return false; }     // (no bases: never kept)
                    seq = bases.data() + at[i]; len = walk.recs[a + i].nBases;
                    return true;
                },
                [&](size_t i, const char *seq, uint64_t len) {
                    const FastaReadRecord &r = walk.recs[a + i];
                    text.append(b.begin + r.off, static_cast<size_t>(r.textLen));
                    if (text.back() != '\n') text.push_back('\n');              // (only the input's last record can lack it)
                    if (judge.report.on())
                        judge.report.add(b.begin + r.off + 1, tsrb::fasta_name_len(ReadBlockReport::Bytes{b.begin + r.off}, 0, static_cast<uint32_t>(r.nameLen)), seq, len);
                },
                [&]() { write(text.data(), text.size()); });
            stats.blockLines = judge.report.lines;
        }
        left = size - static_cast<size_t>(walk.next);
    }
    out.flush();
    return stats;
}
}  // namespace detail
// The host route: records are framed on the host, a block of input at a time, their body lines joined and judged in batches of up
// to readsPerBatch through the filter.  Input may be plain or gzip (both through zlib); `-` is stdin.
inline FastaSubsetStats fastaSubset(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                    size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 256u << 20, std::ostream *blocks = nullptr) {
    return detail::fastaSubsetHost(inFile, out, filter, readsPerBatch, bytesPerBatch, blocks);
}

}  // namespace teloscope_mi355x

#endif
