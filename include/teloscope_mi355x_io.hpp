// teloscope_mi355x_io.hpp — the callers and writers either side of the scan path (SURVEY §8 row f2,
// and the part of f3 the writers need), host-side C++17 above teloscope_mi355x.hpp:
//
//   splitPath / walkPaths   what Teloscope::walkPath does per path (src/input.cpp:942-1041): cut a
//                           record into '+' segments and N-gaps, scan, concatenate, label — but with
//                           ONE batched scanSegments call for every segment of every path, which is
//                           what a GPU back end needs;
//   writeBEDFiles           the eleven output files of handleBEDFile / writeBEDFile
//                           (src/teloscope.cpp:661-957; formats in docs/outputs.md) and the console
//                           path report;
//   printSummary            the assembly summary (src/teloscope.cpp:959-1055), to console and report.
//
// Once the scan takes milliseconds, formatting 6-15 M lines x 5 files is the end-to-end bottleneck, so
// lines are formatted by a pool of host threads into per-task buffers (std::to_chars: integers, and
// floats exactly as operator<<(float) prints them — "%g" with 6 significant digits) and written in
// path order.  Output is byte-identical for any thread count.
#ifndef TELOSCOPE_MI355X_IO_HPP
#define TELOSCOPE_MI355X_IO_HPP

#include <algorithm>
#include <array>
#include <atomic>
#include <charconv>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iostream>
#include <ostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include "teloscope_mi355x.hpp"
#include "teloscope_mi355x_filter.hpp"
#include "teloscope_mi355x_gzip.hpp"
#include "teloscope_mi355x_ring.hpp"
#include "teloscope_mi355x_reads_host.hpp"

namespace teloscope_mi355x {

struct GapInfo {                               // include/teloscope.h:97-100
    uint64_t start = 0;
    uint32_t length = 0;
};

struct PathData {                              // include/teloscope.h:151-163
    unsigned int seqPos = 0;
    std::string header;
    std::vector<GapInfo> gapInfos;
    uint64_t pathSize = 0;
    std::vector<WindowData> windows;
    std::vector<TelomereBlock> terminalBlocks;
    std::vector<TelomereBlock> interstitialBlocks;
    std::vector<MatchInfo> canonicalMatches;
    std::vector<MatchInfo> nonCanonicalMatches;
    std::string terminalLabel;
    ScaffoldType scaffoldType = ScaffoldType::NONE;
    // not in the reference: canonicalMatches.size() as the report prints it, also when the match
    // vectors were never brought to the host (walkPaths without -m counts on the device)
    uint64_t canonicalMatchCount = 0;
    // ... and windows.size() when the windows stayed on the device and came back as text (walkRecordViews with a TrackText):
    // `windows` is empty then
    uint64_t windowCount = 0;
    uint64_t nWindows() const { return windows.empty() ? windowCount : windows.size(); }
};

struct FastaRecord {
    std::string header;                        // first word after '>'
    std::string sequence;
};

// FASTA, plain or gzip-compressed (zlib reads both through the same calls; link with -lz).  The header
// is the first word after '>', line ends and '\r' are dropped, as gfalibs does.  The FASTQ/BAM front
// ends are rows f3/f4.
namespace detail {
// the body lines of one record, [p, end), joined into `seq` without their line ends
inline void joinFastaLines(const char *p, const char *end, std::string &seq) {
    seq.reserve(static_cast<size_t>(end - p));
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        const char *stop = nl ? nl : end;
        if (stop > p) seq.append(p, stop[-1] == '\r' ? stop - 1 : stop);
        p = nl ? nl + 1 : end;
    }
    seq.shrink_to_fit();
}
inline std::string fastaHeaderWord(const char *b, const char *e) {
    if (e > b && e[-1] == '\r') --e;
    const char *w = b;
    while (w < e && *w != ' ' && *w != '\t') ++w;
    return std::string(b, w);
}
}  // namespace detail

inline std::vector<FastaRecord> readFasta(const std::string &file) {
    // A regular uncompressed file is mapped: one pass finds the records ('>' at a line start), then the lines of
    // every record are joined by a pool of threads, largest record first.  Anything else goes through zlib below.
    {
        const int fd = ::open(file.c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error("cannot open " + file);
        struct Close { int fd; ~Close() { ::close(fd); } } closer{fd};
        struct stat sb;
        unsigned char magic[2] = {0, 0};
        const bool gz = ::pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        if (!gz && ::fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
            const size_t size = static_cast<size_t>(sb.st_size);
            void *map = ::mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (map != MAP_FAILED) {
                struct Unmap { void *p; size_t n; ~Unmap() { ::munmap(p, n); } } unmap{map, size};
                const char *data = static_cast<const char *>(map), *end = data + size;
                struct Span { const char *head, *body, *stop; };
                std::vector<Span> spans;
                for (const char *p = data; p < end;) {
                    const char *gt = static_cast<const char *>(std::memchr(p, '>', static_cast<size_t>(end - p)));
                    if (!gt) break;
                    p = gt + 1;
                    if (gt != data && gt[-1] != '\n') continue;            // a '>' inside a line
                    if (!spans.empty()) spans.back().stop = gt;
                    const char *nl = static_cast<const char *>(std::memchr(gt, '\n', static_cast<size_t>(end - gt)));
                    spans.push_back(Span{gt + 1, nl ? nl + 1 : end, end});
                    if (!nl) break;
                    p = nl + 1;
                }
                std::vector<FastaRecord> recs(spans.size());
                std::vector<size_t> order(spans.size());
                for (size_t i = 0; i < order.size(); ++i) order[i] = i;
                std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return spans[a].stop - spans[a].body > spans[b].stop - spans[b].body; });
                std::atomic<size_t> next{0};
                auto worker = [&]() {
                    for (size_t k; (k = next.fetch_add(1)) < order.size();) {
                        const Span &sp = spans[order[k]];
                        const char *he = sp.body > sp.head && sp.body[-1] == '\n' ? sp.body - 1 : sp.body;
                        recs[order[k]].header = detail::fastaHeaderWord(sp.head, he);
                        detail::joinFastaLines(sp.body, sp.stop, recs[order[k]].sequence);
                    }
                };
                const unsigned nthr = static_cast<unsigned>(std::min<size_t>(std::min<size_t>(16, spans.size()), std::max(1u, std::thread::hardware_concurrency())));
                if (nthr <= 1) worker();
                else {
                    std::vector<std::thread> pool;
                    for (unsigned t = 0; t < nthr; ++t) pool.emplace_back(worker);
                    for (std::thread &th : pool) th.join();
                }
                return recs;
            }
        }
    }
    gzFile in = gzopen(file.c_str(), "rb");
    if (!in) throw std::runtime_error("cannot open " + file);
    gzbuffer(in, 1u << 20);
    std::vector<FastaRecord> recs;
    std::vector<char> buf(1u << 22);
    bool in_header = false, at_line_start = true;
    std::string header_line;
    for (;;) {
        const int n = gzread(in, buf.data(), static_cast<unsigned>(buf.size()));
        if (n < 0) { gzclose(in); throw std::runtime_error("read error in " + file); }
        if (n == 0) break;
        const char *p = buf.data(), *end = p + n;
        while (p < end) {
            if (in_header) {                                    // collect the header line
                const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
                header_line.append(p, nl ? nl : end);
                if (!nl) break;
                if (!header_line.empty() && header_line.back() == '\r') header_line.pop_back();
                FastaRecord r;
                const size_t e = header_line.find_first_of(" \t");
                r.header = header_line.substr(0, e);
                recs.push_back(std::move(r));
                header_line.clear();
                in_header = false; at_line_start = true;
                p = nl + 1;
            } else if (at_line_start && *p == '>') {
                in_header = true;
                ++p;
            } else {                                            // sequence bytes up to the end of the line
                const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
                const char *stop = nl ? nl : end;
                if (!recs.empty() && stop > p) {
                    std::string &seq = recs.back().sequence;
                    const size_t before = seq.size();
                    seq.append(p, stop);
                    if (seq.size() > before && seq.back() == '\r') seq.pop_back();
                }
                at_line_start = nl != nullptr;
                p = nl ? nl + 1 : end;
            }
        }
    }
    gzclose(in);
    return recs;
}

// A record as the path model sees it: every run of N/n (X/x) is one gap, what lies between is a '+'
// segment.  Segments are views into the record (no copy; the library folds case itself, which is what
// unmaskSequence does before every reference scanSegment call).  Pinned by testFiles/expected/*_gaps.bed.
struct PathComponents {
    std::vector<std::pair<uint64_t, uint64_t>> segments;       // (absPos = offset in the record, length)
    std::vector<GapInfo> gaps;
};

namespace detail {
// first position in [i, n) whose "is a gap letter" (N n X x) state equals `want`; n if none.  Eight bytes at
// a time: with the case bit set, a gap letter is 'n' or 'x', and (v ^ pattern) has a zero byte exactly there.
inline size_t scanGapState(const char *s, size_t i, size_t n, bool want) {
    auto isGap = [](char c) { return c == 'N' || c == 'n' || c == 'X' || c == 'x'; };
    const uint64_t ones = 0x0101010101010101ull, highs = 0x8080808080808080ull;
    const uint64_t low7 = 0x7F7F7F7F7F7F7F7Full;
    auto zeroBytes = [&](uint64_t v) { return ~(((v & low7) + low7) | v | low7); };            // 0x80 in every zero byte, exactly
    while (i < n && (reinterpret_cast<uintptr_t>(s + i) & 7u)) { if (isGap(s[i]) == want) return i; ++i; }
    for (; i + 8 <= n; i += 8) {
        uint64_t v;
        std::memcpy(&v, s + i, 8);
        v |= 0x2020202020202020ull;
        const uint64_t hit = zeroBytes(v ^ (ones * 'n')) | zeroBytes(v ^ (ones * 'x'));
        // want = true: stop at a word that holds a gap letter; want = false: at one that holds anything else
        if (want ? hit != 0 : hit != highs) break;
    }
    while (i < n && isGap(s[i]) != want) ++i;
    return i;
}
}  // namespace detail

inline PathComponents splitPath(const char *s, size_t n) {
    PathComponents pc;
    size_t i = 0;
    while (i < n) {
        const bool gap = s[i] == 'N' || s[i] == 'n' || s[i] == 'X' || s[i] == 'x';
        const size_t j = detail::scanGapState(s, i + 1, n, !gap);   // the run ends where the state flips
        if (gap) pc.gaps.push_back(GapInfo{i, static_cast<uint32_t>(j - i)});
        else pc.segments.emplace_back(i, j - i);
        i = j;
    }
    return pc;
}
inline PathComponents splitPath(const std::string &seq) { return splitPath(seq.data(), seq.size()); }

// A record as walkPaths sees it: header + bases, wherever they live (a FastaRecord's std::string, or a buffer the
// streaming reader filled).
struct RecordView {
    const std::string *header;
    const char *data;                          // the bases, or nullptr when `pieces` is set
    size_t size;                               // bases
    const ts_text_piece *pieces = nullptr;     // FASTA body text in the file (line ends included), in order
    size_t nPieces = 0;
    const TextLines *lines = nullptr;          // per piece, optional
    const char *device = nullptr;              // the bases in device memory (joined there: scanFastaToFilesDevice); `data` is then
                                               // an optional host copy (-m), and the components must come precomputed
};

namespace detail {
// text position of base `skip` of a run of FASTA body text (line ends are not bases)
inline const char *textLocate(const char *text, uint64_t textLen, uint64_t skip) {
    const char *p = text, *end = text + textLen;
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        const char *stop = nl ? nl : end;
        uint64_t line = static_cast<uint64_t>(stop - p);
        if (line && stop[-1] == '\r') --line;
        if (skip < line) return p + skip;
        skip -= line;
        p = nl ? nl + 1 : end;
    }
    return end;
}

// splitPath over FASTA body text [p, end) that starts at a line start: runs in BASE coordinates (line ends are
// skipped, a run goes on across them); *nBases = the bases of the text; firstIsGap / lastIsGap as splitPaths needs them;
// *lines (optional) = how the lines lie, if they are regular (TextLines)
inline PathComponents splitPathText(const char *p, const char *end, uint64_t *nBases, bool *firstIsGap, bool *lastIsGap,
                                    TextLines *lines = nullptr) {
    PathComponents pc;
    auto isGap = [](char c) { return c == 'N' || c == 'n' || c == 'X' || c == 'x'; };
    uint64_t base = 0, runStart = 0;
    bool have = false, runGap = false;
    *firstIsGap = *lastIsGap = false;
    auto close = [&](uint64_t at) {
        if (!have || at == runStart) return;
        if (runGap) pc.gaps.push_back(GapInfo{runStart, static_cast<uint32_t>(at - runStart)});
        else pc.segments.emplace_back(runStart, at - runStart);
    };
    // line structure: `first` bases on the first line, `width` on every line between the first and the last, the last
    // at most `width`, every line end `eol` bytes
    uint64_t nLines = 0, first = 0, width = 0, eol = 0, prevLen = 0, prevEol = 0;
    bool regular = true;
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        const char *stop = nl ? nl : end;
        size_t n = static_cast<size_t>(stop - p);
        const bool cr = n && stop[-1] == '\r';
        if (cr) --n;
        const uint64_t thisEol = (nl ? 1u : 0u) + (cr ? 1u : 0u);
        if (nLines == 0) { first = n; eol = thisEol; }
        else {
            if (prevEol != eol) regular = false;
            if (nLines == 1) width = n;
            else if (prevLen != width) regular = false;                     // the previous line turned out to be a middle one
        }
        prevLen = n; prevEol = thisEol; ++nLines;
        size_t i = 0;
        while (i < n) {
            const bool gap = isGap(p[i]);
            if (!have) { have = true; runGap = gap; runStart = base; *firstIsGap = gap; }
            else if (gap != runGap) { close(base + i); runGap = gap; runStart = base + i; }
            i = scanGapState(p, i + 1, n, !gap);                            // the run goes on to where the state flips (or the line ends)
        }
        if (n) *lastIsGap = isGap(p[n - 1]);
        base += n;
        p = nl ? nl + 1 : end;
    }
    close(base);
    *nBases = base;
    if (lines) {
        *lines = TextLines{};
        if (nLines >= 3 && prevLen > width) regular = false;
        if (nLines == 1) width = first;
        if (width == 0) width = 1;
        if (eol == 0) eol = 1;
        if (regular && nLines >= 1 && first < (1u << 31) && width < (1u << 31))
            *lines = TextLines{static_cast<uint32_t>(first), static_cast<uint32_t>(width), static_cast<uint32_t>(eol)};
    }
    return pc;
}

// appends the runs of a piece (already in record coordinates) to the record's components; when the piece continues
// a record and its first run is of the kind the previous piece ended with, the two are one run
inline void appendPieceRuns(PathComponents &out, const PathComponents &pc, bool continues, bool prevLastIsGap, bool firstIsGap) {
    size_t si = 0, gi = 0;
    if (continues && prevLastIsGap == firstIsGap) {
        if (firstIsGap) { out.gaps.back().length += pc.gaps[0].length; gi = 1; }
        else { out.segments.back().second += pc.segments[0].second; si = 1; }
    }
    out.segments.insert(out.segments.end(), pc.segments.begin() + static_cast<long>(si), pc.segments.end());
    out.gaps.insert(out.gaps.end(), pc.gaps.begin() + static_cast<long>(gi), pc.gaps.end());
}
}  // namespace detail

// splitPath for every record of a group, on the host threads: records are cut into pieces (16 MB) that are scanned
// independently — one 250 Mb chromosome keeps all threads busy — and a run that crosses a cut is put together again.
inline std::vector<PathComponents> splitPaths(const std::vector<RecordView> &records, size_t pieceBytes = size_t(16) << 20) {
    std::vector<PathComponents> comps(records.size());
    struct Piece { size_t rec, a, z; PathComponents pc; bool firstIsGap, lastIsGap; };
    std::vector<Piece> pieces;
    pieceBytes = std::max<size_t>(pieceBytes, 1);
    for (size_t r = 0; r < records.size(); ++r)
        for (size_t a = 0; a < records[r].size; a += pieceBytes) pieces.push_back(Piece{r, a, std::min(records[r].size, a + pieceBytes), {}, false, false});
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < pieces.size();) {
            Piece &p = pieces[i];
            p.pc = splitPath(records[p.rec].data + p.a, p.z - p.a);
            for (auto &sg : p.pc.segments) sg.first += p.a;
            for (GapInfo &g : p.pc.gaps) g.start += p.a;
            auto isGap = [](char c) { return c == 'N' || c == 'n' || c == 'X' || c == 'x'; };
            p.firstIsGap = isGap(records[p.rec].data[p.a]);
            p.lastIsGap = isGap(records[p.rec].data[p.z - 1]);
        }
    };
    const unsigned nt = static_cast<unsigned>(std::min<size_t>({size_t(16), pieces.size(), size_t(std::max(1u, std::thread::hardware_concurrency()))}));
    if (nt <= 1) worker();
    else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; ++t) pool.emplace_back(worker);
        for (std::thread &th : pool) th.join();
    }
    for (size_t i = 0; i < pieces.size(); ++i) {
        Piece &p = pieces[i];
        detail::appendPieceRuns(comps[p.rec], p.pc, p.a != 0, p.a != 0 && pieces[i - 1].lastIsGap, p.firstIsGap);
    }
    return comps;
}

// walkPath for every record, with one batched scan (result order = record order; seqPos = seqPosBase + index, or
// (*seqPositions)[index] when given: the records' indices in the whole input, which a record filter leaves with gaps).
// context: the context the one batched scan runs on (Teloscope::context(i)).  -1, the default: host records go over all of the
// object's contexts (scanSegmentsWriterView) when it has several, and records with a device form, whose address belongs to one
// context, are scanned on the first.  A caller that produced the bases on context i passes i.
// trackText: when given — and the scan runs on one context — the windows stay on the device: *trackText receives the lines of the
// five window tracks of these records in order (Teloscope::scanSegmentsTrackText), every path's `windows` stays empty and its
// windowCount says how many there were; under -m it receives the lines of the two match files as well
// (Teloscope::scanSegmentsText), the paths' match vectors stay empty and canonicalMatchCount comes from the counts: no match
// record and no base is read on the host.  Otherwise it is left empty and everything is as without it.
inline std::vector<PathData> walkRecordViews(Teloscope &teloscope, const std::vector<RecordView> &records, size_t seqPosBase = 0,
                                             const std::vector<PathComponents> *precomputed = nullptr,
                                             const std::vector<size_t> *seqPositions = nullptr, TrackText *trackText = nullptr,
                                             int context = -1) {
    const UserInputTeloscope &ui = teloscope.input();
    bool deviceForm = false;
    for (const RecordView &rv : records) deviceForm = deviceForm || rv.device != nullptr;
    const bool multi = teloscope.deviceCount() > 1 && context < 0 && !deviceForm;    // all contexts: host segments only
    const size_t on = context < 0 ? 0 : static_cast<size_t>(context);
    // (the streaming reader finds the N-runs while the freshly joined bases are still in cache)
    const std::vector<PathComponents> split = precomputed ? std::vector<PathComponents>() : splitPaths(records);
    const std::vector<PathComponents> &comps = precomputed ? *precomputed : split;
    std::vector<Teloscope::Segment> batch;
    const bool textRoute = trackText && !multi;
    if (trackText && !textRoute) trackText->clear();            // (the text route's call replaces the text and reuses its arrays)
    std::vector<const char *> batchNames;                        // (text route: every segment's record name)
    // text records that N-runs cut into several segments: every segment gets its own piece list (reserved up front, so
    // the lists do not move while the batch points into them)
    auto oneSegment = [&](size_t pi) {
        return comps[pi].segments.size() == 1 && comps[pi].segments[0].first == 0 && comps[pi].segments[0].second == records[pi].size;
    };
    size_t nSub = 0;
    for (size_t pi = 0; pi < records.size(); ++pi)
        if (records[pi].pieces && !oneSegment(pi)) nSub += comps[pi].segments.size();
    std::vector<std::vector<ts_text_piece>> subPieces;
    std::vector<std::vector<TextLines>> subLines;
    subPieces.reserve(nSub);
    subLines.reserve(nSub);
    for (size_t pi = 0; pi < records.size(); ++pi) {
        const RecordView &rv = records[pi];
        if (!rv.pieces) {
            for (const auto &sg : comps[pi].segments) {
                batch.emplace_back(rv.data ? rv.data + sg.first : nullptr, static_cast<size_t>(sg.second), sg.first, ui.ultraFastMode);
                if (rv.device) batch.back().device = rv.device + sg.first;
                if (textRoute) batchNames.push_back(rv.header->c_str());
            }
            continue;
        }
        if (oneSegment(pi)) {
            batch.emplace_back(rv.pieces, rv.nPieces, rv.size, 0, ui.ultraFastMode, rv.lines);   // its pieces as they are
            if (textRoute) batchNames.push_back(rv.header->c_str());
            continue;
        }
        // a segment = bases [a, a + n) of the record: the text pieces that hold them, the first one entered at base a
        uint64_t cum = 0;
        size_t k = 0;
        for (const auto &sg : comps[pi].segments) {
            while (k < rv.nPieces && cum + rv.pieces[k].n_bases <= sg.first) cum += rv.pieces[k++].n_bases;
            subPieces.emplace_back();
            subLines.emplace_back();
            std::vector<ts_text_piece> &sp = subPieces.back();
            std::vector<TextLines> &sl = subLines.back();
            uint64_t at = sg.first, left = sg.second, c2 = cum;
            for (size_t q = k; left && q < rv.nPieces; ++q) {
                ts_text_piece t = rv.pieces[q];
                TextLines L = rv.lines ? rv.lines[q] : TextLines{};
                const uint64_t skip = at - c2;
                if (skip) {
                    const char *from = detail::textLocate(t.text, t.text_len, skip);
                    t.text_len -= static_cast<uint64_t>(from - t.text); t.text = from; t.n_bases -= skip;
                    if (L.width) {                                                 // entered mid-line: what is left of that line comes first
                        const char *nl = static_cast<const char *>(std::memchr(from, '\n', static_cast<size_t>(t.text_len)));
                        uint64_t rest = static_cast<uint64_t>((nl ? nl : from + t.text_len) - from);
                        if (rest && from[rest - 1] == '\r') --rest;
                        L.first = static_cast<uint32_t>(rest);
                    }
                }
                const uint64_t n = std::min<uint64_t>(t.n_bases, left);
                t.n_bases = n;                                                     // (of the last piece only what is needed)
                sp.push_back(t);
                sl.push_back(L);
                at += n; left -= n; c2 += rv.pieces[q].n_bases;
            }
            batch.emplace_back(sp.data(), sp.size(), static_cast<size_t>(sg.second), sg.first, ui.ultraFastMode, sl.data());
            if (textRoute) batchNames.push_back(rv.header->c_str());
        }
    }
    // without -m nothing downstream reads a match record: blocks and counts come from the device
    std::vector<ts_segment_counts> counts;
    // (with -m: only the two match vectors the writers read are materialised; block calling has happened on the device)
    // (several devices: the batch is cut into one shard per device, and what comes back is the writers' view either way)
    std::vector<SegmentData> scanned = textRoute ? (ui.outMatches ? teloscope.scanSegmentsText(batch, batchNames, counts, *trackText, on)
                                                                  : teloscope.scanSegmentsTrackText(batch, batchNames, counts, *trackText, on))
                                     : multi ? teloscope.scanSegmentsWriterView(batch, counts)
                                     : ui.outMatches ? teloscope.scanSegments(batch, true, on)
                                                     : teloscope.scanSegmentsNoMatches(batch, counts, on);
    const bool haveCounts = multi || !ui.outMatches || textRoute;

    std::vector<PathData> paths(records.size());
    size_t si = 0;
    for (size_t pi = 0; pi < records.size(); ++pi) {
        PathData &pd = paths[pi];
        pd.seqPos = static_cast<unsigned int>(seqPositions ? (*seqPositions)[pi] : seqPosBase + pi);
        pd.header = *records[pi].header;
        pd.pathSize = records[pi].size;
        pd.gapInfos = comps[pi].gaps;
        const size_t nseg = comps[pi].segments.size();
        if (nseg == 1) {                                        // the common case: the record is one segment — no copies
            SegmentData &sd = scanned[si];
            pd.canonicalMatchCount = haveCounts ? counts[si].n_canonical : sd.canonicalMatches.size();
            if (textRoute) pd.windowCount = counts[si].n_windows;
            pd.windows = std::move(sd.windows);
            pd.terminalBlocks = std::move(sd.terminalBlocks);
            pd.interstitialBlocks = std::move(sd.interstitialBlocks);
            pd.canonicalMatches = std::move(sd.canonicalMatches);
            pd.nonCanonicalMatches = std::move(sd.nonCanonicalMatches);
            ++si;
        } else {
            for (size_t k = 0; k < nseg; ++k, ++si) {
                SegmentData &sd = scanned[si];
                auto append = [](auto &dst, auto &src) {
                    dst.insert(dst.end(), std::make_move_iterator(src.begin()), std::make_move_iterator(src.end()));
                };
                append(pd.windows, sd.windows);
                append(pd.terminalBlocks, sd.terminalBlocks);
                append(pd.interstitialBlocks, sd.interstitialBlocks);
                pd.canonicalMatchCount += haveCounts ? counts[si].n_canonical : sd.canonicalMatches.size();
                if (textRoute) pd.windowCount += counts[si].n_windows;
                append(pd.canonicalMatches, sd.canonicalMatches);
                append(pd.nonCanonicalMatches, sd.nonCanonicalMatches);
            }
        }
        teloscope.labelTerminalBlocks(pd.terminalBlocks, static_cast<uint16_t>(pd.gapInfos.size()), pd.terminalLabel,
                                      pd.scaffoldType, pd.pathSize, ui.terminalLimit);
    }
    return paths;
}

inline std::vector<PathData> walkPaths(Teloscope &teloscope, const std::vector<FastaRecord> &records) {
    std::vector<RecordView> views(records.size());
    for (size_t i = 0; i < records.size(); ++i) views[i] = RecordView{&records[i].header, records[i].sequence.data(), records[i].sequence.size(), nullptr, 0, nullptr};
    return walkRecordViews(teloscope, views, 0);
}

namespace detail {
// a bounded queue between the stages of scanFastaToFiles (the dynamic parallel-for, onThreads: teloscope_mi355x_reads_host.hpp)
template <typename T>
class BoundedQueue {
public:
    explicit BoundedQueue(size_t cap) : cap_(cap) {}
    void push(T v) {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return q_.size() < cap_ || closed_; });
        q_.push_back(std::move(v));
        cv_.notify_all();
    }
    void close() { { std::lock_guard<std::mutex> g(m_); closed_ = true; } cv_.notify_all(); }
    bool pop(T &out) {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        cv_.notify_all();
        return true;
    }
private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<T> q_;
    size_t cap_;
    bool closed_ = false;
};
}  // namespace detail

// ---- what the four device routes share: the input's bytes into a device chunk, and the judge step of the two read subsets ----
namespace detail {

inline std::runtime_error deviceError(ts_ctx *ctx, const char *what) {      // "<what>: <the library's last error>"
    const char *why = ts_last_error(ctx);
    return std::runtime_error(std::string(what) + ": " + (why ? why : "?"));
}

// The BGZF member at p (its total size), or 0: what is there does not parse as a whole BGZF member
inline size_t bgzfMemberOrNone(const unsigned char *p, size_t n, BgzfBlockRef &ref) {
    bool eofm = false;
    try { return parseBgzfBlock(p, n, ref, eofm); } catch (const std::runtime_error &) { return 0; }
}

// The members of one inflate call, from data[at] on, for a fill that has `produced` of its `want` new bytes already: `used`
// compressed bytes give `made` bytes at dstBase + produced (descs: src_off from data + at).  The first member of a fill is taken
// whatever its size; a later one that would pass `want` ends the fill (full); one that would pass compCap ends this call only;
// what does not parse as a member ends both (foreign).  BgzfParallelReader::next's rule; no device call, no exception.
struct BgzfPick { size_t used = 0; uint64_t made = 0; bool foreign = false, full = false; };
inline BgzfPick pickBgzfMembers(const unsigned char *data, size_t size, size_t at, uint64_t dstBase, uint64_t produced, uint64_t want,
                                uint64_t compCap, std::vector<ts_bgzf_block> &descs) {
    BgzfPick pick;
    descs.clear();
    while (at + pick.used < size) {
        BgzfBlockRef ref{};
        const size_t total = bgzfMemberOrNone(data + at + pick.used, size - at - pick.used, ref);
        if (total == 0) { pick.foreign = true; break; }
        if (produced + pick.made > 0 && produced + pick.made + ref.isize > want) { pick.full = true; break; }
        if (!descs.empty() && pick.used + total > compCap) break;
        ts_bgzf_block d{};
        d.src_off = static_cast<uint64_t>(ref.payload - (data + at)); d.payload_len = ref.payloadLen; d.isize = ref.isize; d.crc = ref.crc;
        d.dst_off = dstBase + produced + pick.made;
        descs.push_back(d);
        pick.made += ref.isize;
        pick.used += total;
    }
    return pick;
}

// the members of the chunk's last inflate, into its contents or its staging region, judged: a payload that is no deflate stream
// or fails its CRC is the host routes' exception
inline void membersVerdict(ts_ctx *ctx, ts_chunk *chunk) {
    ts_bgzf_status bad{};
    if (ts_bam_chunk_status(chunk, &bad) != TS_OK) throw deviceError(ctx, "BGZF inflate failed");
    if (bad.code == TS_BGZF_BAD_DEFLATE) throw std::runtime_error("invalid BGZF deflate payload");
    if (bad.code != TS_BGZF_OK) throw std::runtime_error("BGZF checksum mismatch");
}

// `used` compressed bytes at src with their members' descriptors: uploaded, inflated and checksummed on the device behind the
// chunk's bytes from carryFrom on
inline void inflateMembers(ts_ctx *ctx, ts_chunk *chunk, const unsigned char *src, size_t used, const std::vector<ts_bgzf_block> &descs, uint64_t carryFrom) {
    if (ts_bam_chunk_inflate(chunk, src, used, descs.data(), descs.size(), carryFrom, nullptr) != TS_OK) throw deviceError(ctx, "BGZF inflate failed");
    membersVerdict(ctx, chunk);
}

// ts_gzip (include/teloscan.h) as the device GzipReader decodes with
struct TsGzipDevice : GzipDevice {
    ts_ctx *ctx;
    ts_gzip *gz;
    TsGzipDevice(ts_ctx *ctx_, uint32_t spanBytes) : ctx(ctx_), gz(ts_gzip_create(ctx_, spanBytes)) {
        if (!gz) throw deviceError(ctx, "cannot make the gzip decoder");
    }
    TsGzipDevice(const TsGzipDevice &) = delete;
    TsGzipDevice &operator=(const TsGzipDevice &) = delete;
    ~TsGzipDevice() override { ts_gzip_destroy(gz); }
    GzipWindowResult decode(const unsigned char *window, size_t n, unsigned startBit, int historyMode, const unsigned char *history, size_t historyLen) override {
        ts_gzip_result r{};
        if (ts_gzip_decode(gz, window, n, startBit, historyMode, history, historyLen, &r) != TS_OK) throw deviceError(ctx, "gzip decode failed");
        GzipWindowResult w;
        w.endBit = r.end_bit; w.plainBytes = r.plain_bytes; w.crc = r.crc32; w.status = r.status;
        return w;
    }
    void noteFallback() override { ts_gzip_note_fallback(gz, 1); }
    void history(std::vector<unsigned char> &out) override {
        out.resize(32768);
        uint64_t len = 0;
        if (ts_gzip_history(gz, out.data(), &len) != TS_OK) throw deviceError(ctx, "cannot read the gzip history");
        out.resize(static_cast<size_t>(len));
    }
};

// a ChunkFeed::Options default from the environment: the number, or `fallback` where the variable is unset or no number
inline size_t envSize(const char *name, size_t fallback) {
    const char *e = std::getenv(name);
    if (!e || !*e) return fallback;
    char *end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    return end && *end == 0 ? static_cast<size_t>(v) : fallback;
}

// Bytes of a text input -> new bytes in a device chunk, for fastqSubsetDevice, scanFastaToFilesDevice and annotateGfaDevice.
// The text comes from one of four sources —
//   Plain   a plain regular file: mapped, and copied to the device as it lies (ts_chunk_upload);
//   Bgzf    a BGZF regular file (bgzip output): the members are located on the host (parseBgzfBlock reads no payload byte) and
//           inflated and checksummed on the device (ts_bam_chunk_inflate, as bamSubsetDevice does), in as many calls per fill
//           as the compressed buffer asks for; from the first member that does not parse as BGZF on, the rest of the input is
//           a Stream.  Behind BGZF members anything that is not gzip ends the input: zlib ignores what trails a gzip stream;
//   Gzip    a mapped regular file that begins with a plain gzip member, or such members behind BGZF members, of
//           Options::gzipMinBytes or more: the deflate stream is decoded on the device a window at a time (ts_gzip_decode),
//           member headers and trailers are the host's, and zlib continues wherever the device's verified chain of blocks
//           stops short (GzipReader, teloscope_mi355x_gzip.hpp); its data errors and failed trailer checks are cannotRead,
//           as gzread's are for a Stream;
//   Stream  anything else (small plain gzip, stdin, a FIFO, a file that cannot be mapped): read in blocks, each block
//           uploaded; through zlib where gzip starts there (or always: Options), else read(2) —
// and a fill is read(want), which says how many bytes come (a Stream is read here), then put(chunk, carryFrom), which brings
// them behind the chunk's bytes from carryFrom on; fill() is the two in one.
class ChunkFeed {
public:
    enum Source { Plain, Bgzf, Stream, Gzip };
    struct Options {
        std::string cannotOpen, cannotRead;                     // the route's exception texts
        bool dashIsStdin = false;                               // `-` is stdin, always read through zlib (as fastqSubset does)
        bool zlibAlways = false;                                // a Stream goes through zlib whatever it begins with
        const char *growFailed = "cannot grow the device chunk", *uploadFailed = "upload of the text failed";
        std::function<std::runtime_error(const char *)> noRoom; // the exception of a failed growth or upload; unset: deviceError
        // told about every run of new bytes: where they lie on the host, or (host == nullptr) their offset in the chunk
        std::function<void(const char *host, uint64_t chunkAt, uint64_t len)> sink;
        // plain gzip on the device; the defaults are the environment's, read when the options are made
        bool gzipDevice = envSize("TS_GZIP_DEVICE", kGzipDeviceDefault) != 0;       // 0: zlib reads plain gzip, as a Stream
        size_t gzipSpan = envSize("TS_GZIP_SPAN", 32768);                           // compressed bytes per span (a wave each)
        size_t gzipMinBytes = envSize("TS_GZIP_MIN_BYTES", size_t(1) << 20);        // fewer compressed bytes: zlib
        size_t gzipWindow = envSize("TS_GZIP_WINDOW", size_t(8) << 20);             // compressed bytes per device call
    };
    static constexpr size_t kGzipDeviceDefault = 0;

    ChunkFeed(ts_ctx *ctx, const std::string &file, Options options)
        : ctx_(ctx), opt_(std::move(options)), in_(file, opt_.dashIsStdin, opt_.cannotOpen) {
        if (in_.data) {
            BgzfBlockRef ref{};
            if (in_.size >= 2 && in_.data[0] == 0x1f && in_.data[1] == 0x8b) source_ = bgzfMemberOrNone(in_.data, in_.size, ref) ? Bgzf : Stream;
            else source_ = Plain;
        }
        deviceInflate_ = source_ == Bgzf;
        if (source_ == Stream && in_.data && gzipWanted(0)) { source_ = Gzip; openGzip(0); }
    }

    Source source() const { return source_; }
    bool deviceInflate() const { return deviceInflate_; }       // the input began as BGZF
    // the compressed buffer of a chunk filled with chunkBytes at a time, which the fills then keep to: an inflate call takes
    // members of the mapped file, never more compressed bytes than the file has
    uint64_t compCap(size_t chunkBytes) {
        return compCap_ = source_ == Bgzf ? std::min<uint64_t>(chunkBytes + (1u << 20), std::max<size_t>(in_.size, 64)) : 64;
    }
    // a fill of BGZF members may exceed what it was asked for by one member: the chunk stays below the walk's limit all the same
    uint64_t chunkLimit(uint64_t limit) const { return deviceInflate_ && limit > (1u << 17) ? limit - 65536 : limit; }

    // The next fill: up to `want` bytes (BGZF: whole members, the first whatever its size).  -> how many put() brings: exact for
    // Plain and Stream, a bound guessed from the compressed size for Bgzf (the chunk grows).  A Stream's block is read here,
    // into `keep` where the caller wants to own it (it grows as it fills and is cut to what came).
    uint64_t read(size_t want, std::vector<char> *keep = nullptr) {
        want_ = want;
        if (source_ == Plain) return std::min<uint64_t>(want, in_.size - at_);
        if (source_ == Bgzf) return std::min<uint64_t>(want, 8 * static_cast<uint64_t>(in_.size - at_) + 65536);
        if (source_ == Gzip) return std::min<uint64_t>(want, (pendLen_ - pendOff_) + 8 * gzipReader_->bytesLeft() + 65536);
        if (!streamOpen_) openStream(0);
        std::vector<char> &b = keep ? *keep : block_;
        const size_t start = keep ? std::min<size_t>(want, size_t(4) << 20) : want;
        if (b.size() < start) b.resize(start);
        got_ = 0;
        while (!streamDone_ && got_ < want) {
            if (got_ == b.size()) b.resize(std::min(want, 2 * b.size()));
            const size_t room = std::min<size_t>(std::min(b.size(), want) - got_, size_t(1) << 30);
            const long n = in_.get(b.data() + got_, room);
            if (n < 0) throw std::runtime_error(opt_.cannotRead);
            if (n == 0) { streamDone_ = true; break; }
            got_ += static_cast<size_t>(n);
        }
        if (keep) { b.resize(got_); b.shrink_to_fit(); }
        blockData_ = b.data();
        return got_;
    }

    // What read() announced, behind the chunk's bytes from carryFrom on (those in front are dropped).  -> the input is at its end
    bool put(ts_chunk *chunk, uint64_t carryFrom) {
        auto noRoom = [&](const char *what) { return opt_.noRoom ? opt_.noRoom(what) : deviceError(ctx_, what); };
        if (source_ == Bgzf) {
            // the first call drops the consumed bytes, the later ones keep what is there
            const uint64_t carry = ts_bam_chunk_size(chunk) - carryFrom;
            uint64_t produced = 0;
            BgzfPick pick;
            do {
                pick = pickBgzfMembers(in_.data, in_.size, at_, carry, produced, want_, compCap_, descs_);
                if (ts_chunk_reserve(chunk, carry + produced + pick.made) != TS_OK) throw noRoom(opt_.growFailed);
                inflateMembers(ctx_, chunk, in_.data + at_, pick.used, descs_, carryFrom);
                if (pick.made && opt_.sink) opt_.sink(nullptr, carry + produced, pick.made);
                at_ += pick.used;
                produced += pick.made;
                carryFrom = 0;
            } while (!pick.foreign && !pick.full && at_ < in_.size);
            if (!pick.foreign) return at_ >= in_.size;
            if (gzipWanted(at_)) { source_ = Gzip; openGzip(at_); return !gzipLoad(); }
            source_ = Stream;
            openStream(at_);
            return streamDone_;
        }
        if (source_ == Gzip) {
            uint64_t got = 0;
            bool first = true;
            while (gzipLoad() && got < want_) {
                const uint64_t n = std::min<uint64_t>(want_ - got, pendLen_ - pendOff_), cf = first ? carryFrom : 0;
                const uint64_t at = ts_bam_chunk_size(chunk) - cf;
                if (pendKind_ == GzipReader::OnDevice) {
                    uint64_t moved = 0;
                    if (ts_gzip_take(gzipDevice_->gz, chunk, cf, n, &moved) != TS_OK || moved != n) throw noRoom(opt_.growFailed);
                } else if (ts_chunk_upload(chunk, pendHost_ + pendOff_, n, cf, nullptr) != TS_OK) throw noRoom(opt_.uploadFailed);
                if (opt_.sink) opt_.sink(nullptr, at, n);
                pendOff_ += n; got += n;
                first = false;
            }
            if (first && ts_chunk_upload(chunk, nullptr, 0, carryFrom, nullptr) != TS_OK) throw noRoom(opt_.uploadFailed);    // (the carry alone)
            return !gzipLoad();
        }
        if (source_ == Plain) {
            const size_t n = std::min(want_, in_.size - at_);
            if (ts_chunk_upload(chunk, in_.data + at_, n, carryFrom, nullptr) != TS_OK) throw noRoom(opt_.uploadFailed);
            if (n && opt_.sink) opt_.sink(reinterpret_cast<const char *>(in_.data + at_), 0, n);
            at_ += n;
            return at_ >= in_.size;
        }
        if (ts_chunk_upload(chunk, blockData_, got_, carryFrom, nullptr) != TS_OK) throw noRoom(opt_.uploadFailed);
        if (got_ && opt_.sink) opt_.sink(blockData_, 0, got_);
        return streamDone_;
    }

    bool fill(ts_chunk *chunk, uint64_t carryFrom, size_t want) { read(want); return put(chunk, carryFrom); }

    // The same fill in two halves for a route that deals its chunks to several contexts (detail::ChunkRing): take() is the
    // reader's, one call at a time in chunk order, and touches no device; stage() brings what was taken into the staging region
    // of a chunk of any context (ts_chunk_stage_upload, ts_chunk_stage_inflate) and may run for several fills at once.  The
    // Gzip source is bound to the context it was made on: such a feed is made with Options::gzipDevice off, and plain gzip is a
    // Stream.  Options::sink is not told about these fills.
    struct Fill {
        const char *host = nullptr;                             // Plain and Stream: the bytes (a Stream's lie in `block`)
        uint64_t n = 0;                                         // new bytes in all
        std::vector<char> block;
        struct Call { size_t at = 0, used = 0; std::vector<ts_bgzf_block> descs; };
        std::vector<Call> calls;                                // Bgzf: the members of each inflate call, dst_off from the fill's start
        bool atEnd = false;                                     // the input is at its end
    };
    void take(size_t want, Fill &f) {
        f.host = nullptr; f.n = 0; f.calls.clear(); f.atEnd = false;
        if (source_ == Gzip) throw std::logic_error("ChunkFeed::take: the Gzip source serves one context");
        if (source_ == Bgzf) {
            BgzfPick pick;
            do {
                f.calls.emplace_back();
                Fill::Call &c = f.calls.back();
                pick = pickBgzfMembers(in_.data, in_.size, at_, 0, f.n, want, compCap_, c.descs);
                c.at = at_; c.used = pick.used;
                at_ += pick.used;
                f.n += pick.made;
            } while (!pick.foreign && !pick.full && at_ < in_.size);
            if (!pick.foreign) { f.atEnd = at_ >= in_.size; return; }
            source_ = Stream;
            openStream(at_);
            f.atEnd = streamDone_;
            return;
        }
        if (source_ == Plain) {
            f.n = std::min<uint64_t>(want, in_.size - at_);
            f.host = reinterpret_cast<const char *>(in_.data + at_);
            at_ += static_cast<size_t>(f.n);
            f.atEnd = at_ >= in_.size;
            return;
        }
        f.n = read(want, &f.block);
        f.host = f.block.data();
        f.atEnd = streamDone_;
    }
    // (noRoom: the exception of a failed upload in place of Options::noRoom's, for a route whose message names the context)
    void stage(ts_ctx *ctx, ts_chunk *chunk, const Fill &f, const std::function<std::runtime_error(const char *)> *noRoom = nullptr) const {
        for (const Fill::Call &c : f.calls) {
            if (ts_chunk_stage_inflate(chunk, in_.data + c.at, c.used, c.descs.data(), c.descs.size(), nullptr) != TS_OK) throw deviceError(ctx, "BGZF inflate failed");
            membersVerdict(ctx, chunk);
        }
        if (f.calls.empty() && ts_chunk_stage_upload(chunk, f.host, f.n, nullptr) != TS_OK)
            throw noRoom ? (*noRoom)(opt_.uploadFailed) : opt_.noRoom ? opt_.noRoom(opt_.uploadFailed) : deviceError(ctx, opt_.uploadFailed);
    }

private:
    // plain gzip from `from` on goes to the device: asked for, a device to ask, a member there, and enough of it
    bool gzipWanted(size_t from) const {
        return opt_.gzipDevice && ctx_ && in_.data && in_.size - from >= std::max<size_t>(opt_.gzipMinBytes, 2) &&
               in_.data[from] == 0x1f && in_.data[from + 1] == 0x8b;
    }
    void openGzip(size_t from) {
        const size_t span = std::min<size_t>(std::max<size_t>(opt_.gzipSpan / 1024 * 1024, 1024), size_t(1) << 20);
        gzipDevice_.reset(new TsGzipDevice(ctx_, static_cast<uint32_t>(span)));
        GzipReader::Tuning tuning;
        // (the device holds 2 bytes per symbol of every span's room — 16 symbols per compressed byte, 512 Ki at least: 1 GiB here)
        const size_t spansMost = (size_t(1) << 30) / (2 * std::max<size_t>(16 * span, size_t(512) << 10));
        tuning.windowBytes = std::min<size_t>(std::max<size_t>(opt_.gzipWindow, span), std::min<size_t>(size_t(1) << 28, spansMost * span));
        tuning.minBytes = opt_.gzipMinBytes;
        gzipReader_.reset(new GzipReader(in_.data, in_.size, from, gzipDevice_.get(), tuning));
    }
    // a piece with bytes left is at hand -> true; false: the gzip input is at its end.  zlib's verdicts become the route's
    bool gzipLoad() {
        while (pendOff_ >= pendLen_) {
            pendOff_ = pendLen_ = 0;
            try { pendKind_ = gzipReader_->next(pendLen_, pendHost_); }
            catch (const GzipError &) { throw std::runtime_error(opt_.cannotRead); }
            if (pendKind_ == GzipReader::None) return false;
        }
        return true;
    }

    // the descriptor from `from` on; behind BGZF members (from > 0) only gzip is read
    void openStream(size_t from) {
        streamOpen_ = true;
        bool gz = !in_.owned || opt_.zlibAlways;
        if (from > 0) {
            if (in_.size - from < 2 || in_.data[from] != 0x1f || in_.data[from + 1] != 0x8b) { streamDone_ = true; return; }
            if (::lseek(in_.fd, static_cast<off_t>(from), SEEK_SET) == static_cast<off_t>(-1)) throw std::runtime_error(opt_.cannotRead);
            gz = true;
        }
        in_.openZlib(gz, opt_.cannotOpen);                     // (not always: where gzip begins the file)
    }

    ts_ctx *ctx_;
    Options opt_;
    MappedInput in_;
    Source source_ = Stream;
    bool deviceInflate_ = false, streamOpen_ = false, streamDone_ = false;
    uint64_t compCap_ = 64;
    size_t at_ = 0, want_ = 0, got_ = 0;                        // next byte of the mapped file; the pending fill
    const char *blockData_ = nullptr;                               // the Stream block read() filled
    std::vector<char> block_;
    std::vector<ts_bgzf_block> descs_;
    std::unique_ptr<TsGzipDevice> gzipDevice_;                      // the Gzip source: the device's decoder, the reader above it
    std::unique_ptr<GzipReader> gzipReader_;
    GzipReader::Kind pendKind_ = GzipReader::None;                  // the piece being handed out: where it lies, how far it has gone
    const char *pendHost_ = nullptr;
    uint64_t pendLen_ = 0, pendOff_ = 0;
};

// The judge step of bamSubsetDevice and fastqSubsetDevice: reads with bases, already picked out of a chunk's table (`lens`, one
// per read), staged into a tips-only batch's input buffer by stage(batch), judged by the scan and the predicate the host routes
// use (ts_batch_scan + ts_batch_read_pass, with the regrow-and-rescan of an overflowed batch: include/teloscan.h), the passing
// records' bytes gathered by gather(dPass, dst, cap, &bytes, &nPassed) into `kept`.
struct ReadJudge {
    double msStage = 0, msFilter = 0, msGather = 0, msBlocks = 0;
    std::vector<unsigned char> kept;
    uint64_t bytes = 0, nPassed = 0;                            // of the last run: kept[0, bytes) are the passing records
    // The read block report (include/teloscan.h), where a route was given a stream for it: blockLines(batch, dst, cap, &bytes,
    // &lines) is the route's ts_*_chunk_block_lines call.  Between filter and gather the judged batch's blocks are called
    // (ts_batch_call_read_blocks) and the lines of the kept reads formatted and downloaded: blockText[0, blockBytes), nBlockLines
    // of them.  Empty: no call, no kernel, no allocation.
    std::function<int(ts_batch *, unsigned char *, uint64_t, uint64_t *, uint64_t *)> blockLines;
    std::vector<unsigned char> blockText;
    uint64_t blockBytes = 0, nBlockLines = 0;
    // A step between filter and gather for a route that keeps records by more than their own pass byte (fastqSubsetPairedDevice:
    // a pair is kept when either mate passes): passRoom more bytes are asked of the chunk's pass buffer behind the reads' own, and
    // passStep(dPass) answers the pass bytes the gather reads (nothing: it failed).  Empty: no call, no kernel, no allocation.
    std::function<void *(void *)> passStep;
    uint64_t passRoom = 0;

    // room(dPass): the bytes `kept` must hold before gather is called (0: as it is), for a gather whose refused call is not cheap
    template <typename Stage, typename Gather, typename Room>
    void run(ts_ctx *ctx, ts_chunk *chunk, const std::vector<uint64_t> &lens, const char *stageFailed, Stage &&stage, Gather &&gather, Room &&room) {
        struct BatchPtr { ts_batch *p; ~BatchPtr() { ts_batch_destroy(p); } } batch{ts_batch_create(ctx, lens.data(), nullptr, lens.size(), 1, 0)};
        if (!batch.p) throw deviceError(ctx, "cannot plan the read batch");
        Clock::time_point t0 = Clock::now();
        if (stage(batch.p) != TS_OK) throw deviceError(ctx, stageFailed);
        void *dPass = ts_bam_chunk_pass_buffer(chunk, lens.size() + passRoom);
        if (!dPass) throw deviceError(ctx, "cannot allocate the pass bytes");
        msStage += since(t0); t0 = Clock::now();
        if (ts_batch_scan(batch.p, nullptr, nullptr) != TS_OK || ts_batch_read_pass(batch.p, dPass, nullptr) != TS_OK) throw deviceError(ctx, "read filter failed");
        int overflowed = 0;
        if (ts_batch_read_pass_status(batch.p, &overflowed) != TS_OK) throw deviceError(ctx, "read filter failed");
        if (overflowed) {                                       // regrow + rescan, then judge again
            if (ts_batch_sync(batch.p) != TS_OK || ts_batch_read_pass(batch.p, dPass, nullptr) != TS_OK ||
                ts_batch_read_pass_status(batch.p, &overflowed) != TS_OK || overflowed) throw deviceError(ctx, "read filter failed");
        }
        msFilter += since(t0); t0 = Clock::now();
        blockBytes = nBlockLines = 0;
        if (blockLines) {
            if (ts_batch_call_read_blocks(batch.p, nullptr) != TS_OK || ts_batch_read_pass_status(batch.p, &overflowed) != TS_OK || overflowed)
                throw deviceError(ctx, "block calling of the kept reads failed");
            if (blockText.size() < (1u << 16)) blockText.resize(1u << 16);
            int rc = blockLines(batch.p, blockText.data(), blockText.size(), &blockBytes, &nBlockLines);
            if (rc == TS_ERR_INVALID_ARG && blockBytes > blockText.size()) {
                blockText.resize(static_cast<size_t>(blockBytes));
                rc = blockLines(batch.p, blockText.data(), blockText.size(), &blockBytes, &nBlockLines);
            }
            if (rc != TS_OK) throw deviceError(ctx, "formatting the block report failed");
            msBlocks += since(t0); t0 = Clock::now();
        }
        if (passStep && !(dPass = passStep(dPass))) throw deviceError(ctx, "the pass bytes of the records failed");
        bytes = nPassed = 0;
        if (kept.size() < (1u << 20)) kept.resize(1u << 20);
        const uint64_t want = room(dPass);
        if (want > kept.size()) kept.resize(static_cast<size_t>(want));
        int rc = gather(dPass, kept.data(), kept.size(), &bytes, &nPassed);
        if (rc == TS_ERR_INVALID_ARG && bytes > kept.size()) {
            kept.resize(static_cast<size_t>(bytes));
            rc = gather(dPass, kept.data(), kept.size(), &bytes, &nPassed);
        }
        if (rc != TS_OK) throw deviceError(ctx, "gather of the passing records failed");
        msGather += since(t0);
    }
};

}  // namespace detail

// ---- the three device read routes, bamSubsetDevice, fastqSubsetDevice and samSubsetDevice: one set of chunk steps each, for a
// filter of any number of contexts ----
// A route's steps (detail::BamChunkSteps, detail::FastqChunkSteps, detail::SamChunkSteps) have two ways to bring a chunk's bytes
// in; everything behind the fill (framing, judging, emitting, the exception texts, the figures) exists once and serves both.
// What the formats do alike exists once under the three (detail::ReadChunkSteps, and detail::TextChunkSteps for the two of text).
//   In place  the new bytes go straight behind the unfinished record in the context's own chunk, and the chunk is framed, judged
//             and emitted on the caller's thread, each sub-batch's passing bytes straight from the judge to the output: no
//             staging region, no commit, no carry between chunks, no thread.  A filter of one context takes its whole input so;
//             on several contexts the BAM route takes its chunks so on context 0 until the header is behind it.
//   Dealt     detail::ChunkRing (teloscope_mi355x_ring.hpp) deals chunk k to context k mod N (ordinals may repeat), a thread per
//             context: the new bytes are staged beside the chunk while the chunks before it are still being framed, frame()
//             carries the unfinished record over and commits the staged bytes behind it, and judge() keeps the passing bytes
//             until emit() has its turn.
// The result, the statistics, the exceptions and the output bytes, those written before a failure included, do not depend on the
// number of contexts (tests/test_gpu_read_routes_multi.py).

// `walk` of bamSubsetDevice chooses how a chunk's records are framed: Serial is ts_bam_chunk_walk, one wave that follows the
// records one after the other; Index is ts_bam_chunk_index, which finds record chains in all spans of the chunk at once and links
// them.  Both give the same table, so the output bytes do not depend on it; the TS_TIMING lines name the one that ran.  Index is
// the default: its walk stage measured 6.8 ms against 98.4 ms on a HiFi BAM and 11 ms against 1 112 ms on a BAM of 150-base reads
// (profiles/bam/bam_index_rate.txt).
enum class BamRecordWalk { Serial, Index };
// `deflate` of bamSubsetDevice chooses who compresses the passing records.  Host: detail::BgzfWriter, zlib level 6 on the host
// threads inside the writer's turn, as bamSubset does (the default; nothing about it changes).  Device: every sub-batch's passing
// records are gathered, cut into payloads of 65 280 bytes, deflated and framed on the device (ts_bam_chunk_gather_bgzf) and come
// back as finished members, which the writer appends verbatim; the header still goes through zlib, into members of its own.  The
// output is then a valid BGZF file that inflates to exactly what Host's inflates to; its compressed bytes are the device
// encoder's, and do not depend on the number of contexts (they do on readsPerBatch and bytesPerBatch, which cut the sub-batches).
enum class BamOutputDeflate { Host, Device };
// One context's share of a device read route: chunks it took, reads with bases it judged, uncompressed bytes it received, and the
// milliseconds its thread spent in the source (reading, upload, inflate and CRC), waiting for the chunk before its own to be
// framed (dealt chunks only: the serial section as this context sees it), placing the carry and committing the staged bytes
// behind it (dealt chunks only), framing records (index or walk), and in ReadJudge's stage, filter and gather.
struct ReadRouteDeviceStats {
    uint64_t chunks = 0, recordsJudged = 0, bytesReceived = 0;
    double msSource = 0, msCarryWait = 0, msCommit = 0, msWalk = 0, msStage = 0, msFilter = 0, msGather = 0;
    double msBlocks = 0;                                        // in ReadJudge's block report step (0 without a `blocks` stream)
    // BamOutputDeflate::Device only: milliseconds in ts_bam_chunk_gather_bgzf (part of msGather: gather, deflate kernels, the
    // members' download), record bytes that went into it and member bytes that came out
    double msDeflate = 0;
    uint64_t deflatePlainBytes = 0, deflateMemberBytes = 0;
};

namespace detail {

// What a context of a read route owns: its chunk (contents and, once a chunk is dealt to it, a staging region), its judge and
// pass buffer, the passing records of the dealt chunk it is working on, and its figures.
struct ChunkWorker {
    ts_ctx *ctx = nullptr;
    ts_chunk *chunk = nullptr;
    ReadJudge judged;
    std::vector<uint64_t> lens;
    std::vector<unsigned char> out;                             // a dealt chunk's passing records, in input order
    std::vector<size_t> cuts;                                   // where each sub-batch's records end in `out`: the writer's pieces
    uint64_t withBases = 0, passed = 0;                         // the chunk's records that had bases, and its passing ones, however it came in
    std::vector<unsigned char> blockOut;                        // a dealt chunk's lines of the read block report, in input order
    uint64_t blockLines = 0;                                    // the chunk's report lines, however it came in
    ReadRouteDeviceStats st;
    ChunkWorker() = default;
    ChunkWorker(const ChunkWorker &) = delete;
    ChunkWorker &operator=(const ChunkWorker &) = delete;
    ~ChunkWorker() { ts_bam_chunk_destroy(chunk); }
    void fresh() { out.clear(); cuts.clear(); withBases = passed = 0; blockOut.clear(); blockLines = 0; }
    // a dealt chunk's sub-batch waits here for the chunk's turn to emit
    void keep() {
        out.insert(out.end(), judged.kept.begin(), judged.kept.begin() + static_cast<std::ptrdiff_t>(judged.bytes));
        cuts.push_back(out.size());
        blockOut.insert(blockOut.end(), judged.blockText.begin(), judged.blockText.begin() + static_cast<std::ptrdiff_t>(judged.blockBytes));
    }
    // report lines to the route's `blocks` stream (nothing without one)
    static void writeBlocks(std::ostream *os, const unsigned char *p, size_t n) {
        if (!os || !n) return;
        os->write(reinterpret_cast<const char *>(p), static_cast<std::streamsize>(n));
        if (!os->good()) throw std::runtime_error("failed while writing the block report");
    }
    // the kept pieces in the order and sizes an in-place chunk writes them (of which it keeps none)
    template <typename Write>
    void pieces(Write &&write) const {
        size_t from = 0;
        for (size_t to : cuts) { write(out.data() + from, to - from); from = to; }
    }
};

// A dealt chunk comes together: the unfinished record of the chunk framed before goes to the front of `to`, the staged bytes
// behind it.  `from` is another context's chunk (ts_chunk_carry_over: on one GPU, between peers, or through the host), `to`
// itself (the chunk's own tail moves to its front), or nothing (the first chunk of the input).
template <typename To, typename From>
inline void ringCommit(To &to, const From *from, uint64_t carryFrom) {
    const Clock::time_point t0 = Clock::now();
    if (from == &to) { if (ts_chunk_upload(to.chunk, nullptr, 0, carryFrom, nullptr) != TS_OK) throw deviceError(to.ctx, "cannot carry a record into the next device chunk"); }
    else if (from && ts_chunk_carry_over(to.chunk, from->chunk, carryFrom, nullptr) != TS_OK) throw deviceError(to.ctx, "cannot carry a record into the next device chunk");
    if (ts_chunk_commit(to.chunk, nullptr) != TS_OK) throw deviceError(to.ctx, "cannot grow the device chunk");
    to.st.msCommit += since(t0);
}

// A route's figures, to perDevice and, under TS_TIMING, to stderr: a line per context and the write line, each beginning with
// `route`.  `ring` is the ring that dealt the chunks, or nothing (every chunk came in place: no context waited for another).
template <typename Worker, typename Ring>
inline void routeFigures(const char *route, const std::vector<std::unique_ptr<Worker>> &workers, const Ring *ring, double msWrite,
                         std::vector<ReadRouteDeviceStats> *perDevice) {
    if (perDevice) perDevice->clear();
    for (size_t w = 0; w < workers.size(); ++w) {
        ReadRouteDeviceStats s = workers[w]->st;
        s.msStage = workers[w]->judged.msStage; s.msFilter = workers[w]->judged.msFilter; s.msGather = workers[w]->judged.msGather;
        s.msBlocks = workers[w]->judged.msBlocks;
        if (ring) s.msCarryWait = ring->frameWaitMs(w);
        if (perDevice) perDevice->push_back(s);
        if (std::getenv("TS_TIMING")) {
            char deflate[160] = "";                             // (a route that deflated on the device says so behind the gather)
            if (s.deflatePlainBytes)
                std::snprintf(deflate, sizeof deflate, ", of which device deflate %.0f ms (%llu record bytes -> %llu member bytes)", s.msDeflate,
                              (unsigned long long)s.deflatePlainBytes, (unsigned long long)s.deflateMemberBytes);
            char report[64] = "";                               // (a route that wrote the block report says what it cost)
            if (workers[w]->judged.blockLines) std::snprintf(report, sizeof report, ", block report %.0f ms", s.msBlocks);
            std::fprintf(stderr, "%s: context %zu of %zu: %llu chunks, %llu reads judged, %llu bytes; source %.0f ms, carry wait %.1f ms, carry + commit %.1f ms, "
                         "walk %.1f ms, stage %.0f ms, filter %.0f ms, gather %.0f ms%s%s\n", route, w, workers.size(), (unsigned long long)s.chunks,
                         (unsigned long long)s.recordsJudged, (unsigned long long)s.bytesReceived, s.msSource, s.msCarryWait, s.msCommit, s.msWalk, s.msStage,
                         s.msFilter, s.msGather, deflate, report);
        }
    }
    if (std::getenv("TS_TIMING")) std::fprintf(stderr, "%s: write %.0f ms\n", route, msWrite);
}

// ... of a record route: the chunk's record table as the walk left it, and the records of the sub-batch under way that have bases
template <typename Rec>
struct RecordWorker : ChunkWorker {
    std::vector<Rec> recs, withSeq;
    uint64_t n = 0;                                             // records of the chunk
};

// What the steps of the three device read routes share: the sub-batch judge loop and the head of emit().  Route (FastqChunkSteps,
// SamChunkSteps, BamChunkSteps) derives from it and says what its format does differently:
//   static uint64_t bases(const Rec &)      the record's bases; 0: it has none, is not judged and never kept
//   static constexpr const char *stageFailed
//   int stageReads(Worker &, ts_batch *)    the sequences of k.withSeq into the batch's input buffer
//   int gatherKept(Worker &, void *dPass, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *nPassed)
//   int blockLines(Worker &, ts_batch *, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *lines)
//   void write(const unsigned char *, size_t)       passing bytes to the route's output
// and gatherRoom(Worker &, void *dPass) where its gather needs one (ReadJudge::run).
template <typename Route, typename Worker>
class ReadChunkSteps {
public:
    double msWrite = 0;
    std::vector<std::unique_ptr<Worker>> workers;

protected:
    ReadChunkSteps(std::ostream *blocks, size_t readsPerBatch) : blocks_(blocks), readsPerBatch_(std::max<size_t>(readsPerBatch, 1)) {}
    Route &route() { return static_cast<Route &>(*this); }
    uint64_t gatherRoom(Worker &, void *) { return 0; }
    // a sub-batch begins with n records at rec; its record i was placed among the reads to judge, or has no bases (a route that
    // needs to know: FastqPairChunkSteps)
    template <typename Rec> void subBatch(Worker &, const Rec *, size_t) {}
    void placed(Worker &, size_t, bool) {}
    // Records [from, to) of the chunk's table in sub-batches of readsPerBatch, in input order.  A dealt chunk keeps a sub-batch's
    // passing bytes until its turn to emit; an in-place chunk has the turn, and they go from the judge straight to the output.
    void judgeRecords(Worker &k, size_t from, size_t to, bool dealt) {
        Route &r = route();
        for (size_t a = from; a < to; a += readsPerBatch_) {
            const auto *rec = k.recs.data() + a;
            const size_t n = std::min<size_t>(readsPerBatch_, to - a);
            k.withSeq.clear(); k.lens.clear();
            r.subBatch(k, rec, n);
            for (size_t i = 0; i < n; ++i) {
                const uint64_t bases = Route::bases(rec[i]);
                if (bases) { k.withSeq.push_back(rec[i]); k.lens.push_back(bases); }
                r.placed(k, i, bases != 0);
            }
            if (k.withSeq.empty()) continue;                    // (a read without bases is never kept)
            k.withBases += k.withSeq.size();
            k.st.recordsJudged += k.withSeq.size();
            if (blocks_ && !k.judged.blockLines)
                k.judged.blockLines = [&r, &k](ts_batch *batch, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *lines) {
                    return r.blockLines(k, batch, dst, cap, bytes, lines);
                };
            k.judged.run(k.ctx, k.chunk, k.lens, Route::stageFailed, [&](ts_batch *batch) { return r.stageReads(k, batch); },
                         [&](void *dPass, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *nPassed) { return r.gatherKept(k, dPass, dst, cap, bytes, nPassed); },
                         [&](void *dPass) { return r.gatherRoom(k, dPass); });
            k.passed += k.judged.nPassed;
            k.blockLines += k.judged.nBlockLines;
            if (dealt) k.keep();
            else { r.write(k.judged.kept.data(), static_cast<size_t>(k.judged.bytes)); ChunkWorker::writeBlocks(blocks_, k.judged.blockText.data(), static_cast<size_t>(k.judged.blockBytes)); }
        }
    }
    // the head of a chunk's turn to write: what it kept (nothing, where it came in place)
    void emitKept(const Worker &k) {
        k.pieces([&](const unsigned char *p, size_t n) { route().write(p, n); });
        ChunkWorker::writeBlocks(blocks_, k.blockOut.data(), k.blockOut.size());
    }

    std::ostream *blocks_;                                      // the read block report's stream, or nothing
    size_t readsPerBatch_;
};

// The steps of the two text routes, fastqSubsetDevice and samSubsetDevice, up to the format's framing: a chunk of chunkBytes per
// context, fed by one ChunkFeed.  Route adds frameChunk(Worker &, atEnd) (-> every record up to the chunk's end is valid; where
// the chunk's unfinished record begins goes to prevNext_), emit(w, chunk) and, where it judges with more than the loop,
// judgeChunk.  A chunk that holds no whole record (a record larger than it) passes all of its contents on: in place the next
// fill takes as much again, so the chunk doubles; a dealt chunk takes chunkBytes more.
template <typename Route, typename Worker>
class TextChunkSteps : public ReadChunkSteps<Route, Worker> {
public:
    // The whole input as in-place chunks of context 0, on the caller's thread: any source of the feed, ChunkFeed::Gzip included
    void runInPlace() {
        Worker &k = *this->workers[0];
        for (bool atEnd = false; !atEnd;) {
            const uint64_t carry = ts_bam_chunk_size(k.chunk) - prevNext_;
            // a chunk that held no whole record takes as much again
            const size_t want = static_cast<size_t>(std::max<uint64_t>(chunkBytes_, prevNext_ == 0 ? carry : 0));
            const Clock::time_point t0 = Clock::now();
            atEnd = feed_.fill(k.chunk, prevNext_, want);
            k.st.msSource += since(t0);
            ++k.st.chunks; k.st.bytesReceived += ts_bam_chunk_size(k.chunk) - carry;
            frameNext(k, atEnd);
            this->route().judgeChunk(k, false);
            this->route().emit(0, 0);
        }
    }

    // the ring's steps: a dealt chunk
    void begin(size_t w) { ts_bind_thread_to_device(this->workers[w]->ctx); }
    RingTake take(size_t w, uint64_t) {
        Worker &k = *this->workers[w];
        const Clock::time_point t0 = Clock::now();
        feed_.take(chunkBytes_, k.fill);
        k.st.msSource += since(t0);
        return k.fill.atEnd ? RingTake::Last : RingTake::More;
    }
    void stage(size_t w, uint64_t) {
        Worker &k = *this->workers[w];
        const Clock::time_point t0 = Clock::now();
        feed_.stage(k.ctx, k.chunk, k.fill);
        k.st.msSource += since(t0);
        ++k.st.chunks; k.st.bytesReceived += k.fill.n;
    }
    bool frame(size_t w, uint64_t) {                            // the serial section: carry, commit, the format's framing
        Worker &k = *this->workers[w];
        ringCommit(k, prev_, prevNext_);
        return frameNext(k, k.fill.atEnd);
    }
    void judge(size_t w, uint64_t) { this->route().judgeChunk(*this->workers[w], true); }

    void judgeChunk(Worker &k, bool dealt) { k.fresh(); this->judgeRecords(k, 0, static_cast<size_t>(k.n), dealt); }
    void write(const unsigned char *p, size_t n) {
        const Clock::time_point t0 = Clock::now();
        out_.write(reinterpret_cast<const char *>(p), static_cast<std::streamsize>(n));
        if (!out_.good()) throw std::runtime_error(writeFailed_);
        this->msWrite += since(t0);
    }

protected:
    TextChunkSteps(ReadTelomereFilter &filter, ChunkFeed &feed, std::ostream &out, size_t readsPerBatch, size_t chunkBytes, std::ostream *blocks, const char *writeFailed)
        : ReadChunkSteps<Route, Worker>(blocks, readsPerBatch), feed_(feed), out_(out), chunkBytes_(chunkBytes), writeFailed_(writeFailed) {
        const uint64_t compCap = feed.compCap(chunkBytes);
        for (size_t w = 0; w < filter.deviceCount(); ++w) {
            this->workers.emplace_back(new Worker());
            Worker &k = *this->workers.back();
            k.ctx = filter.context(w);
            k.chunk = ts_bam_chunk_create(k.ctx, compCap, chunkBytes);
            if (!k.chunk) throw deviceError(k.ctx, "cannot make the device chunk");
            k.recs.resize(std::min<size_t>(size_t(1) << 20, chunkBytes / 64 + 16));
        }
    }
    // The records of a chunk that has its bytes; the framing's state moves on to it
    bool frameNext(Worker &k, bool atEnd) {
        prev_ = &k; prevNext_ = 0;
        return this->route().frameChunk(k, atEnd);
    }

    ChunkFeed &feed_;
    std::ostream &out_;
    size_t chunkBytes_;
    const char *writeFailed_;
    // the framing's state: the chunk framed last and where its unfinished record begins; nothing framed yet held a byte
    const ChunkWorker *prev_ = nullptr;
    uint64_t prevNext_ = 0;
    bool first_ = true;
};

// fastqSubsetDevice's stages: TextChunkSteps with the FASTQ framing.  The first chunk must begin with '@'; ts_fastq_chunk_walk
// frames and validates the records, and the bytes behind the last whole one go in front of the next chunk.  A record that is not
// valid ends the framing; its chunk's valid records are still judged and written before emit() throws.
struct FastqWorker : RecordWorker<ts_fastq_record> {
    ChunkFeed::Fill fill;                                       // a dealt chunk's new bytes
    int error = TS_FASTQ_OK;
};
// (Route: FastqChunkSteps itself, or FastqPairChunkSteps, which frames pairs over the same steps)
template <typename Route, typename WorkerT = FastqWorker>
class FastqChunkStepsOf : public TextChunkSteps<Route, WorkerT> {
public:
    using Worker = WorkerT;
    FastqSubsetResult result;

    FastqChunkStepsOf(ReadTelomereFilter &filter, ChunkFeed &feed, std::ostream &out, size_t readsPerBatch, size_t chunkBytes, std::ostream *blocks = nullptr)
        : TextChunkSteps<Route, WorkerT>(filter, feed, out, readsPerBatch, chunkBytes, blocks, "failed while writing FASTQ subset") {}

    // the chunk's turn to write: what it kept, its totals, and the record that is not valid
    void emit(size_t w, uint64_t) {
        Worker &k = *this->workers[w];
        this->emitKept(k);
        result.kept += k.passed; result.total += k.n; result.blockLines += k.blockLines;
        if (k.error != TS_FASTQ_OK) throw recordError(k.error, result.total + 1);
    }
    static std::runtime_error recordError(int error, uint64_t number) {
        const char *msg = error == TS_FASTQ_TRUNCATED ? "truncated FASTQ record" : error == TS_FASTQ_BAD_HEADER ? "expected header line starting with '@'"
                        : error == TS_FASTQ_BAD_SEPARATOR ? "expected separator line starting with '+'" : "sequence and quality length differ";
        return std::runtime_error("FASTQ record " + std::to_string(number) + ": " + msg);
    }

    // the format's part of the shared steps
    static uint64_t bases(const ts_fastq_record &r) { return r.seq_len > r.seq_cr ? r.seq_len - r.seq_cr : 0; }
    static constexpr const char *stageFailed = "staging the sequences failed";
    int stageReads(Worker &k, ts_batch *batch) { return ts_fastq_chunk_stage(k.chunk, k.withSeq.data(), k.withSeq.size(), batch, nullptr); }
    int gatherKept(Worker &k, void *dPass, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *nPassed) {
        return ts_fastq_chunk_gather(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, dst, cap, bytes, nPassed, nullptr);
    }
    int blockLines(Worker &k, ts_batch *batch, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *lines) {
        return ts_fastq_chunk_block_lines(k.chunk, k.withSeq.data(), k.withSeq.size(), batch, dst, cap, bytes, lines, nullptr);
    }
    bool frameChunk(Worker &k, bool atEnd) {
        k.n = 0; k.error = TS_FASTQ_OK;
        if (this->first_) {
            if (ts_bam_chunk_size(k.chunk) == 0) {
                if (atEnd) throw std::runtime_error("FASTQ input is empty");
                return true;
            }
            unsigned char c = 0;
            if (ts_bam_chunk_read(k.chunk, 0, 1, &c) != TS_OK) throw deviceError(k.ctx, "cannot read the chunk");
            if (c != '@') throw std::runtime_error("FASTQ input must start with '@'");
            this->first_ = false;
        }
        uint64_t errorRecord = 0, errorOff = 0;
        const Clock::time_point t0 = Clock::now();
        int rc = ts_fastq_chunk_walk(k.chunk, atEnd ? 1 : 0, k.recs.data(), k.recs.size(), &k.n, &this->prevNext_, &k.error, &errorRecord, &errorOff);
        if (rc == TS_ERR_INVALID_ARG && k.n > k.recs.size()) {
            k.recs.resize(static_cast<size_t>(k.n));
            rc = ts_fastq_chunk_walk(k.chunk, atEnd ? 1 : 0, k.recs.data(), k.recs.size(), &k.n, &this->prevNext_, &k.error, &errorRecord, &errorOff);
        }
        if (rc != TS_OK) throw deviceError(k.ctx, "FASTQ walk failed");
        k.st.msWalk += since(t0);
        return k.error == TS_FASTQ_OK;
    }
};
class FastqChunkSteps : public FastqChunkStepsOf<FastqChunkSteps> {
public:
    using FastqChunkStepsOf::FastqChunkStepsOf;
};

// fastqSubsetPairedDevice's stages (the rule: include/teloscan.h, "Interleaved paired FASTQ"): FastqChunkSteps with pairs.  The
// framing hands on whole pairs only: a chunk that is not the input's last gives up the first mate at its end, so that the next
// chunk begins at an even record; ts_fastq_chunk_mates compares the names of its pairs, and the lowest pair that is not well
// formed ends the framing.  A sub-batch is whole pairs; between filter and gather ts_fastq_chunk_pair_pass gives both mates the
// pair's verdict, and the gather runs over all of the sub-batch's records.
struct FastqPairWorker : FastqWorker {
    std::vector<uint32_t> readOf;                               // of the sub-batch under way: a record's place in withSeq, or ~0
    const ts_fastq_record *sub = nullptr;                       // the sub-batch's records, with and without bases
    size_t subN = 0;
    bool mismatch = false, unpaired = false;                    // the pair behind the chunk's records is not well formed; the input ends with a first mate
    uint64_t dropped = 0;                                       // valid records in front of a record that is not: a first mate, never written
};
class FastqPairChunkSteps : public FastqChunkStepsOf<FastqPairChunkSteps, FastqPairWorker> {
public:
    using Base = FastqChunkStepsOf<FastqPairChunkSteps, FastqPairWorker>;
    FastqPairChunkSteps(ReadTelomereFilter &filter, ChunkFeed &feed, std::ostream &out, size_t readsPerBatch, size_t chunkBytes, std::ostream *blocks = nullptr)
        : Base(filter, feed, out, std::max<size_t>(readsPerBatch + (readsPerBatch & 1u), 2), chunkBytes, blocks) {}

    void emit(size_t w, uint64_t) {
        Worker &k = *workers[w];
        emitKept(k);
        result.kept += k.passed; result.total += k.n; result.blockLines += k.blockLines;
        if (k.mismatch)
            throw std::runtime_error("FASTQ records " + std::to_string(result.total + 1) + " and " + std::to_string(result.total + 2) + " do not have the same name");
        if (k.error != TS_FASTQ_OK) throw recordError(k.error, result.total + k.dropped + 1);
        if (k.unpaired) throw std::runtime_error("FASTQ input ends with an unpaired record");
    }

    bool frameChunk(Worker &k, bool atEnd) {
        k.mismatch = k.unpaired = false; k.dropped = 0;
        Base::frameChunk(k, atEnd);
        if (k.n & 1u) {
            k.n -= 1;
            if (k.error != TS_FASTQ_OK) k.dropped = 1;          // (the record error stands, with its true number)
            else if (atEnd) k.unpaired = true;                  // (raised at emit, behind the chunk's whole pairs)
            else prevNext_ = k.n ? k.recs[k.n].off : 0;         // (no whole pair: the chunk passes all of its contents on, and grows)
        }
        uint64_t bad = UINT64_MAX;
        const Clock::time_point t0 = Clock::now();
        if (ts_fastq_chunk_mates(k.chunk, k.recs.data(), static_cast<size_t>(k.n), &bad) != TS_OK) throw deviceError(k.ctx, "FASTQ mate names failed");
        k.st.msWalk += since(t0);
        if (bad != UINT64_MAX) {
            k.n = 2 * bad; k.error = TS_FASTQ_OK; k.dropped = 0; k.unpaired = false; k.mismatch = true;
            return false;
        }
        return k.error == TS_FASTQ_OK && !k.unpaired;
    }

    // the sub-batch's records and where each lies among its reads; the step that pairs the pass bytes
    void subBatch(Worker &k, const ts_fastq_record *rec, size_t n) {
        k.sub = rec; k.subN = n;
        k.readOf.assign(n, 0xffffffffu);
        k.judged.passRoom = n + 16;
        if (!k.judged.passStep)
            k.judged.passStep = [&k](void *dPass) -> void * {
                void *dPair = static_cast<unsigned char *>(dPass) + ((k.lens.size() + 15) & ~size_t(15));
                return ts_fastq_chunk_pair_pass(k.chunk, k.subN, k.readOf.data(), dPass, dPair, nullptr) == TS_OK ? dPair : nullptr;
            };
    }
    void placed(Worker &k, size_t i, bool staged) { if (staged) k.readOf[i] = static_cast<uint32_t>(k.withSeq.size() - 1); }
    int gatherKept(Worker &k, void *dPass, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *nPassed) {
        return ts_fastq_chunk_gather(k.chunk, k.sub, k.subN, dPass, dst, cap, bytes, nPassed, nullptr);
    }
};

// The driver of the two text routes, behind fastqSubsetDevice and samSubsetDeviceRun: the feed with the route's exception texts
// (`format` is the name they give the input), Steps over it with `more` behind the common arguments, the chunks dealt by the ring
// on several contexts or taken in place on one, and the figures under `route`.
template <typename Steps, typename... More>
inline auto textSubsetDeviceRun(const char *format, const std::string &route, const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                size_t readsPerBatch, size_t chunkBytes, std::vector<ReadRouteDeviceStats> *perDevice, std::ostream *blocks, More... more) {
    const bool dealt = filter.deviceCount() > 1;
    const std::string uploadFailed = std::string("upload of the ") + format + " text failed";
    ChunkFeed::Options options;
    options.cannotOpen = "Stream not successful: " + inFile;
    options.cannotRead = std::string("read error in ") + format + " input";
    options.dashIsStdin = true;
    options.uploadFailed = uploadFailed.c_str();
    if (dealt) options.gzipDevice = false;                      // (bound to one context: plain gzip is read through zlib)
    ChunkFeed feed(filter.context(0), inFile, options);
    Steps steps(filter, feed, out, readsPerBatch, std::max<size_t>(chunkBytes, 64), blocks, more...);
    std::unique_ptr<ChunkRing<Steps>> ring;
    if (dealt) {
        ring.reset(new ChunkRing<Steps>(filter.deviceCount(), 0, steps));
        ring->run();
    } else {
        steps.runInPlace();
    }
    out.flush();
    routeFigures((feed.deviceInflate() ? route + " (upload + inflate + CRC)" : route).c_str(), steps.workers, ring.get(), steps.msWrite, perDevice);
    return steps.result;
}

// bamSubsetDevice's stages.  A chunk holds as many BGZF members as inflate to chunkBytes (pick), whichever way it comes in, so
// the tables, and what is written before a record that is not valid, do not depend on the number of contexts.  The header is
// parsed on the host from the leading bytes of context 0's in-place chunks.
struct BamWorker : RecordWorker<ts_bam_record> {                // (recs: one walk's table behind the other)
    std::vector<ts_bgzf_block> descs;                           // the chunk's members: where they lie, how much they give
    size_t at = 0, used = 0;
    uint64_t produced = 0;
    std::vector<size_t> tables;                                 // where each table ends in recs
    const char *error = nullptr;                                // the record the framing stopped at is not valid
};
class BamChunkSteps : public ReadChunkSteps<BamChunkSteps, BamWorker> {
public:
    using Worker = BamWorker;
    BamSubsetStats stats;

    BamChunkSteps(ReadTelomereFilter &filter, const unsigned char *data, size_t size, std::ostream &out, size_t readsPerBatch, size_t chunkBytes, BamRecordWalk walk,
                  BamOutputDeflate deflate = BamOutputDeflate::Host, std::ostream *blocks = nullptr, const ReadFastqOutput *fastq = nullptr)
        : ReadChunkSteps(blocks, readsPerBatch), data_(data), size_(size), writer_(out, fastq != nullptr), text_(out), fastq_(fastq != nullptr),
          fastqFlags_(fastq ? fastqOutFlags(*fastq) : 0u), chunkBytes_(chunkBytes),
          table_(std::min<size_t>(size_t(1) << 20, chunkBytes / 36 + 2)), walk_(walk), deflate_(deflate),
          plainCap_((256ull << 20) + 4 + chunkBytes), compCap_(chunkBytes + (1u << 20)) {
        for (size_t w = 0; w < filter.deviceCount(); ++w) {
            workers.emplace_back(new Worker());
            Worker &k = *workers.back();
            k.ctx = filter.context(w);
            // (a chunk holds the unconsumed tail of the one before, at most a record: 4 bytes + 256 MiB, and the new members'
            // output.  Context 0's holds a header of any size the route accepts; the others grow when a carry asks for it)
            k.chunk = ts_bam_chunk_create(k.ctx, compCap_, w == 0 ? plainCap_ : chunkBytes + (1u << 20));
            if (!k.chunk) throw deviceError(k.ctx, "cannot make the device chunk");
            k.recs.resize(table_);
        }
    }

    // In-place chunks of context 0, on the caller's thread: the whole input where the filter has one context, else the chunks up
    // to the one that completes the header, its records included.  -> the first chunk for a ring to deal (0: the input has ended)
    uint64_t runInPlace() {
        Worker &k = *workers[0];
        const bool alone = workers.size() == 1;
        uint64_t pos = 0;                                       // the chunk's first byte not consumed yet
        std::vector<unsigned char> head;                        // host copy of the chunk's leading bytes (until the header is done)
        auto have = [&](uint64_t n) {                           // n more bytes from pos on, and on the host
            if (held_ - pos < n) return false;
            if (head.size() < pos + n) {
                const uint64_t from = head.size(), to = std::min<uint64_t>(held_, std::max<uint64_t>(pos + n, from + (1u << 20)));
                head.resize(static_cast<size_t>(to));
                if (ts_bam_chunk_read(k.chunk, from, to - from, head.data() + from) != TS_OK) throw deviceError(k.ctx, "cannot read the BAM header from the device");
            }
            return true;
        };
        auto bytesAt = [&](uint64_t off) { return head.data() + pos + off; };
        while (more_ && (alone || !header_.done())) {
            const uint64_t carry = held_ - pos;
            pick(k, carry);
            if (carry + k.produced > plainCap_) throw std::runtime_error("BAM header is too large for the device route");
            const Clock::time_point t0 = Clock::now();
            inflateMembers(k.ctx, k.chunk, data_ + k.at, k.used, k.descs, pos);
            k.st.msSource += since(t0);
            ++k.st.chunks; k.st.bytesReceived += k.produced;
            held_ = carry + k.produced; pos = 0;
            head.clear();
            if (header_.done() || header_.parse(have, bytesAt, pos, writer_)) {
                head.clear(); head.shrink_to_fit();
                walkRecords(k, pos);
                judgeChunk(k, false);
                emit(0, 0);
                pos = prevNext_;
            } else {
                prev_ = &k; prevNext_ = pos;
            }
        }
        return more_ ? k.st.chunks : 0;
    }

    // the ring's steps: a dealt chunk
    void begin(size_t w) { ts_bind_thread_to_device(workers[w]->ctx); }
    RingTake take(size_t w, uint64_t) {
        if (!more_) return RingTake::None;
        pick(*workers[w], 0);
        return more_ ? RingTake::More : RingTake::Last;
    }
    void stage(size_t w, uint64_t) {
        Worker &k = *workers[w];
        const Clock::time_point t0 = Clock::now();
        if (ts_chunk_stage_inflate(k.chunk, data_ + k.at, k.used, k.descs.data(), k.descs.size(), nullptr) != TS_OK) throw deviceError(k.ctx, "BGZF inflate failed");
        membersVerdict(k.ctx, k.chunk);
        k.st.msSource += since(t0);
        ++k.st.chunks; k.st.bytesReceived += k.produced;
    }
    bool frame(size_t w, uint64_t) {                            // the serial section: carry, commit, the record walk
        Worker &k = *workers[w];
        ringCommit(k, prev_, prevNext_);
        held_ = ts_bam_chunk_size(k.chunk);
        walkRecords(k, 0);
        return !k.error;
    }
    void judge(size_t w, uint64_t) { judgeChunk(*workers[w], true); }
    // the chunk's turn to write: what it kept, its totals, and the record that is not valid
    void emit(size_t w, uint64_t) {
        Worker &k = *workers[w];
        emitKept(k);
        stats.blockLines += k.blockLines;
        stats.totalRecords += k.n;
        stats.missingSequenceRecords += k.n - k.withBases;
        stats.passedRecords += k.passed;
        if (k.error) throw std::runtime_error(k.error);
    }
    // the input has ended: what is left of it is no header and no record
    void finish() {
        header_.requireDone();
        if (held_ != prevNext_) throw std::runtime_error(held_ - prevNext_ < 4 ? "truncated BAM record size" : "truncated BAM record");
        stats.missingEofBlock = !sawEofMarker_;
        writer_.finish();
        if (fastq_) { text_.flush(); if (!text_.good()) throw std::runtime_error("failed while writing BAM subset"); }
    }

    // The chunk's records in sub-batches, in input order.  A sub-batch never spans two tables of the walk, for any number of
    // contexts: each table is cut into sub-batches of readsPerBatch on its own.  Under BamOutputDeflate::Device the passing bytes
    // are finished BGZF members (ts_bam_chunk_gather_bgzf, payloads of 0xff00): a dealt chunk's compression runs here, on every
    // context at once, and emit() only writes.
    void judgeChunk(Worker &k, bool dealt) {
        k.fresh();
        size_t from = 0;
        for (size_t end : k.tables) { judgeRecords(k, from, end, dealt); from = end; }
    }

    // the format's part of the shared steps
    static uint64_t bases(const ts_bam_record &r) { return r.l_seq; }
    static constexpr const char *stageFailed = "SEQ decode failed";
    int stageReads(Worker &k, ts_batch *batch) { return ts_bam_chunk_decode(k.chunk, k.withSeq.data(), k.withSeq.size(), batch, nullptr); }
    int gatherKept(Worker &k, void *dPass, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *nPassed) {
        if (fastq_) return ts_bam_chunk_gather_fastq(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, fastqFlags_, dst, cap, bytes, nPassed, nullptr);
        if (deflate_ == BamOutputDeflate::Host) return ts_bam_chunk_gather(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, dst, cap, bytes, nPassed, nullptr);
        const Clock::time_point t0 = Clock::now();
        uint64_t plainBytes = 0;
        const int rc = ts_bam_chunk_gather_bgzf(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, 0xff00u, dst, cap, bytes, nPassed, &plainBytes, nullptr);
        k.st.msDeflate += since(t0);
        if (rc == TS_OK) { k.st.deflatePlainBytes += plainBytes; k.st.deflateMemberBytes += *bytes; }
        return rc;
    }
    // (a refused ts_bam_chunk_gather_bgzf has deflated already: the plain gather's plan, which a call without room stops at, says
    // how many record bytes pass, and a member adds 31 bytes at the most)
    uint64_t gatherRoom(Worker &k, void *dPass) {
        if (fastq_ || deflate_ == BamOutputDeflate::Host) return 0;
        uint64_t plain = 0, passed = 0;
        const int rc = ts_bam_chunk_gather(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, nullptr, 0, &plain, &passed, nullptr);
        if (rc != TS_OK && !(rc == TS_ERR_INVALID_ARG && plain > 0)) throw deviceError(k.ctx, "gather of the passing records failed");
        return plain + 31u * ((plain + 0xff00u - 1) / 0xff00u);
    }
    int blockLines(Worker &k, ts_batch *batch, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *lines) {
        return ts_bam_chunk_block_lines(k.chunk, k.withSeq.data(), k.withSeq.size(), batch, dst, cap, bytes, lines, nullptr);
    }
    // a sub-batch's passing records to the writer: plain bytes for zlib, or (Device) finished members
    void write(const unsigned char *p, size_t n) {
        const Clock::time_point t0 = Clock::now();
        if (fastq_) {                                           // FASTQ text: as it is
            text_.write(reinterpret_cast<const char *>(p), static_cast<std::streamsize>(n));
            if (!text_.good()) throw std::runtime_error("failed while writing BAM subset");
        } else if (deflate_ == BamOutputDeflate::Host) writer_.write(p, n);
        else if (n) writer_.writeMembers(p, n);
        msWrite += since(t0);
    }

private:
    // The members of the next chunk, their output from dstBase on (BgzfParallelReader::next's rule).  Not pickBgzfMembers: here a
    // member that does not parse is an error, not a change of source, a chunk never takes a member past chunkBytes, and there is
    // one inflate call per chunk.  The reader's: one call at a time, no device call.
    void pick(Worker &k, uint64_t dstBase) {
        k.descs.clear();
        k.at = at_; k.used = 0; k.produced = 0;
        while (at_ + k.used < size_) {
            BgzfBlockRef ref{};
            bool eofm = false;
            const size_t total = parseBgzfBlock(data_ + at_ + k.used, size_ - at_ - k.used, ref, eofm);
            if (total == 0) throw std::runtime_error(size_ - at_ - k.used < 12 ? "truncated BGZF header" : "truncated BGZF block");
            if (k.produced + ref.isize > chunkBytes_ || k.used + total > compCap_) break;
            sawEofMarker_ = sawEofMarker_ || eofm;
            ts_bgzf_block d{};
            d.src_off = static_cast<uint64_t>(ref.payload - (data_ + at_)); d.payload_len = ref.payloadLen; d.isize = ref.isize; d.crc = ref.crc;
            d.dst_off = dstBase + k.produced;
            k.descs.push_back(d);
            k.produced += ref.isize;
            k.used += total;
        }
        at_ += k.used;
        more_ = k.used > 0 && at_ < size_;
    }
    // The chunk's records from `from` on into k.recs, a table of table_ records at a time; the framing's state moves on to this
    // chunk.  Where a table's walk meets a record that is not valid, the table is dropped and the framing ends: the tables before
    // it are judged and written, then emit() throws.
    void walkRecords(Worker &k, uint64_t from) {
        const Clock::time_point t0 = Clock::now();
        k.n = 0; k.tables.clear(); k.error = nullptr;
        uint64_t pos = from;
        for (;;) {
            if (k.recs.size() < k.n + table_) k.recs.resize(static_cast<size_t>(k.n) + table_);
            uint64_t n = 0, next = 0, errorOff = 0;
            int error = 0;
            if ((walk_ == BamRecordWalk::Index ? ts_bam_chunk_index : ts_bam_chunk_walk)(k.chunk, pos, k.recs.data() + k.n, table_, &n, &next, &error, &errorOff) != TS_OK)
                throw deviceError(k.ctx, "record walk failed");
            if (error != TS_BAM_OK) {
                k.error = error == TS_BAM_BAD_BLOCK_SIZE ? "invalid BAM record block_size" : error == TS_BAM_BAD_LENGTHS ? "invalid BAM record lengths"
                        : error == TS_BAM_FIELDS_EXCEED ? "BAM record fields exceed block_size" : "BAM read name is not NUL-terminated";
                break;
            }
            k.n += n;
            k.tables.push_back(static_cast<size_t>(k.n));
            pos = next;
            if (n < table_) break;                              // (a full table: more records may follow in this chunk)
        }
        k.st.msWalk += since(t0);
        prev_ = &k; prevNext_ = pos;
    }
    const unsigned char *data_;
    size_t size_;
    BgzfWriter writer_;
    std::ostream &text_;                                        // the output itself, for FASTQ text (writer_ then keeps nothing)
    bool fastq_;
    uint32_t fastqFlags_;
    BamHeaderParser header_;
    size_t chunkBytes_, table_;
    BamRecordWalk walk_;
    BamOutputDeflate deflate_;
    uint64_t plainCap_, compCap_;
    // the reader's state: the next member, whether one may follow, the EOF marker seen
    size_t at_ = 0;
    bool more_ = true, sawEofMarker_ = false;
    // the framing's state: the chunk framed last, its size and where its unfinished record begins
    const ChunkWorker *prev_ = nullptr;
    uint64_t prevNext_ = 0, held_ = 0;
};

}  // namespace detail

// The device route of --bam-subset (same arguments, statistics, exceptions and output bytes as bamSubset, which stays the
// default): the compressed BGZF members cross PCIe and the uncompressed BAM stream exists in HBM only.  The input is
// detail::MappedInput's (a pipe and stdin are read to their end).  Per chunk of ~bytesPerBatch uncompressed bytes: the members
// are located on the host (parseBgzfBlock reads no payload byte), inflated and checksummed on the device
// (detail::inflateMembers, ts_chunk_stage_inflate), the records walked and validated there (ts_bam_chunk_walk or
// ts_bam_chunk_index, see BamRecordWalk: the table comes back), SEQ decoded into a tips-only batch's input buffer
// (ts_bam_chunk_decode), judged and the passing records' bytes gathered (detail::ReadJudge with ts_bam_chunk_gather).
// The BAM header is parsed on the host from the chunk's leading bytes.  The stages are detail::BamChunkSteps for every filter: a
// filter of one context takes every chunk in place, on the caller's thread and with no staging region; a filter of several
// contexts does so on context 0 until the header is behind it, and from the next chunk on the ring deals the chunks to all of
// them.  perDevice, where given, receives one entry per context.  `deflate` (BamOutputDeflate, above) moves the output's
// compression to the device as well; Host is the default and leaves every byte as it was.
// What a maintainer of the reference would call from runBamSubsetMode (src/bam.cpp:262-316) in place of subsetBam.
namespace detail {
// (the route itself, behind bamSubsetDevice's two forms below)
inline BamSubsetStats bamSubsetDeviceRun(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, size_t readsPerBatch,
                                         size_t bytesPerBatch, BamRecordWalk walk, std::vector<ReadRouteDeviceStats> *perDevice,
                                         BamOutputDeflate deflate, std::ostream *blocks, const ReadFastqOutput *fastq = nullptr) {
    // the compressed input: a regular file is mapped, a pipe is read to its end
    detail::MappedInput in(inFile, true, "cannot open BAM input '" + inFile + "'");
    std::vector<unsigned char> piped;
    if (!in.data) in.readToEnd(piped, "cannot read BAM input");
    detail::BamChunkSteps steps(filter, in.data ? in.data : piped.data(), in.data ? in.size : piped.size(), out, readsPerBatch,
                                std::max<size_t>(bytesPerBatch, 1u << 20), walk, deflate, blocks, fastq);
    std::unique_ptr<detail::ChunkRing<detail::BamChunkSteps>> ring;
    if (const uint64_t firstChunk = steps.runInPlace()) {
        ring.reset(new detail::ChunkRing<detail::BamChunkSteps>(filter.deviceCount(), firstChunk, steps));
        ring->run();
    }
    steps.finish();
    detail::routeFigures(walk == BamRecordWalk::Index ? "bamSubsetDevice (index)" : "bamSubsetDevice (serial)", steps.workers, ring.get(), steps.msWrite, perDevice);
    for (const auto &k : steps.workers) {
        steps.stats.deflatePlainBytes += k->st.deflatePlainBytes; steps.stats.deflateMemberBytes += k->st.deflateMemberBytes;
        steps.stats.msDeflate += k->st.msDeflate;
    }
    return steps.stats;
}
}  // namespace detail
inline BamSubsetStats bamSubsetDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                      size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 256u << 20,
                                      BamRecordWalk walk = BamRecordWalk::Index, std::vector<ReadRouteDeviceStats> *perDevice = nullptr) {
    return detail::bamSubsetDeviceRun(inFile, out, filter, readsPerBatch, bytesPerBatch, walk, perDevice, BamOutputDeflate::Host, nullptr);
}
// ... and with the trailing `deflate` given (an overload, so that the form above stays exactly what it was)
inline BamSubsetStats bamSubsetDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, size_t readsPerBatch,
                                      size_t bytesPerBatch, BamRecordWalk walk, std::vector<ReadRouteDeviceStats> *perDevice,
                                      BamOutputDeflate deflate, std::ostream *blocks = nullptr) {
    return detail::bamSubsetDeviceRun(inFile, out, filter, readsPerBatch, bytesPerBatch, walk, perDevice, deflate, blocks);
}
// The device route of --bam-subset with FASTQ out (same arguments, statistics, exceptions and output bytes as bamSubsetFastq):
// bamSubsetDevice's chunk steps on every context of the filter, with ts_bam_chunk_gather_fastq as detail::ReadJudge's gather — the
// kept records' text is formatted where the chunk lies and only the text comes back.  The bytes do not depend on the number of
// contexts, readsPerBatch, bytesPerBatch or the walk.  The TS_TIMING lines are bamSubsetDevice's.
inline BamSubsetStats bamSubsetFastqDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                           const ReadFastqOutput &fastq = ReadFastqOutput(), size_t readsPerBatch = 1u << 20,
                                           size_t bytesPerBatch = 256u << 20, BamRecordWalk walk = BamRecordWalk::Index,
                                           std::vector<ReadRouteDeviceStats> *perDevice = nullptr, std::ostream *blocks = nullptr) {
    return detail::bamSubsetDeviceRun(inFile, out, filter, readsPerBatch, bytesPerBatch, walk, perDevice, BamOutputDeflate::Host, blocks, &fastq);
}

// The device route of --fastq-subset (same arguments, result, exceptions and, for well-formed input, output bytes as
// fastqSubset, which stays the default): the FASTQ text exists in HBM one chunk of ~bytesPerBatch bytes at a time and the host
// reads none of it.  The text gets there through detail::ChunkFeed (a plain file, BGZF members inflated on the device, or a
// stream through zlib or read(2); `-` is stdin, always through zlib), and behind the source the stages are the same: lines
// indexed and records framed and validated (ts_fastq_chunk_walk: the table comes back), sequences staged into a tips-only
// batch's input buffer (ts_fastq_chunk_stage), judged and the passing records' bytes gathered (detail::ReadJudge with
// ts_fastq_chunk_gather).  The bytes behind the last whole record stay in the chunk for the next fill; a record larger than a
// chunk makes the chunk grow.  The stages are detail::FastqChunkSteps for every filter: a filter of one context takes every chunk
// in place, on the caller's thread and with no staging region; on a filter of several contexts the ring deals the chunks to all
// of them, and there plain gzip is read through zlib, because the opt-in device gzip source (ChunkFeed::Gzip) is bound to one
// context.  perDevice, where given, receives one entry per context.
// What a maintainer of the reference would call from Input::readFastqSubset (src/input.cpp:737-832) in place of its loop.
// (two forms, as for bamSubsetDevice: the one without `blocks` stays exactly what it was; the one with it writes the read block report)
inline FastqSubsetResult fastqSubsetDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, size_t readsPerBatch,
                                           size_t bytesPerBatch, std::vector<ReadRouteDeviceStats> *perDevice, std::ostream *blocks);
inline FastqSubsetResult fastqSubsetDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                           size_t readsPerBatch = 1u << 20, size_t bytesPerBatch = 256u << 20,
                                           std::vector<ReadRouteDeviceStats> *perDevice = nullptr) {
    return fastqSubsetDevice(inFile, out, filter, readsPerBatch, bytesPerBatch, perDevice, nullptr);
}
inline FastqSubsetResult fastqSubsetDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, size_t readsPerBatch,
                                           size_t bytesPerBatch, std::vector<ReadRouteDeviceStats> *perDevice, std::ostream *blocks) {
    return detail::textSubsetDeviceRun<detail::FastqChunkSteps>("FASTQ", "fastqSubsetDevice", inFile, out, filter, readsPerBatch, bytesPerBatch, perDevice, blocks);
}

// fastqSubsetPaired on the device: fastqSubsetDevice's route, arguments and sources, over interleaved pairs (the rule:
// include/teloscan.h, "Interleaved paired FASTQ").  A chunk hands on whole pairs, their names are compared where the chunk holds
// them (ts_fastq_chunk_mates), every record with bases is judged as fastqSubsetDevice judges it, and both records of a pair are
// gathered when either passes (ts_fastq_chunk_pair_pass).  readsPerBatch is rounded up to an even number.  Output, statistics,
// block report and exceptions are fastqSubsetPaired's, on any number of contexts.
inline FastqSubsetResult fastqSubsetPairedDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, size_t readsPerBatch = 1u << 20,
                                                 size_t bytesPerBatch = size_t(256) << 20, std::vector<ReadRouteDeviceStats> *perDevice = nullptr,
                                                 std::ostream *blocks = nullptr) {
    return detail::textSubsetDeviceRun<detail::FastqPairChunkSteps>("FASTQ", "fastqSubsetPairedDevice", inFile, out, filter, readsPerBatch, bytesPerBatch, perDevice, blocks);
}

namespace detail {

// samSubsetDevice's stages: TextChunkSteps with the SAM framing.  ts_sam_chunk_walk frames the chunk's lines — the header lines in
// front of it while the input's header goes on, then the records — and the unfinished last line goes in front of the next chunk.  A
// line that fails a check ends the framing; its chunk's header lines and valid records are still written before emit() throws.
// Whether the input is still in its header, and how many lines lie behind, is the framing's state: it moves on in the serial
// section only.
struct SamWorker : RecordWorker<ts_sam_record> {
    ChunkFeed::Fill fill;                                       // a dealt chunk's new bytes
    std::vector<char> header;                                   // the chunk's header lines as read, until they are written
    uint64_t headerLines = 0;
    int error = TS_SAM_OK;
    uint64_t errorLine = 0;                                     // of the whole input, counted from 1
};
class SamChunkSteps : public TextChunkSteps<SamChunkSteps, SamWorker> {
public:
    using Worker = SamWorker;
    SamSubsetStats result;

    SamChunkSteps(ReadTelomereFilter &filter, ChunkFeed &feed, std::ostream &out, size_t readsPerBatch, size_t chunkBytes, std::ostream *blocks = nullptr,
                  const ReadFastqOutput *fastq = nullptr)
        : TextChunkSteps(filter, feed, out, readsPerBatch, chunkBytes, blocks, "failed while writing SAM subset"), fastq_(fastq != nullptr),
          fastqFlags_(fastq ? fastqOutFlags(*fastq) : 0u) {}

    // an in-place chunk has the turn to write: its header lines, then the passing bytes, go straight to the output
    void judgeChunk(Worker &k, bool dealt) {
        if (!dealt) writeHeader(k);
        TextChunkSteps::judgeChunk(k, dealt);
    }
    // the chunk's turn to write: its header lines and what it kept (nothing, where it came in place), its totals, and the line
    // that is not valid
    void emit(size_t w, uint64_t) {
        Worker &k = *workers[w];
        writeHeader(k);
        emitKept(k);
        result.blockLines += k.blockLines;
        result.headerLines += k.headerLines; result.totalRecords += k.n; result.passedRecords += k.passed; result.missingSequenceRecords += k.n - k.withBases;
        if (k.error != TS_SAM_OK) { out_.flush(); throw samLineError(k.errorLine, k.error); }
    }

    // the format's part of the shared steps
    static uint64_t bases(const ts_sam_record &r) { return (r.flags & 1u) ? 0 : r.seq_len; }      // (SEQ is "*": never kept)
    static constexpr const char *stageFailed = "staging the sequences failed";
    int stageReads(Worker &k, ts_batch *batch) { return ts_sam_chunk_stage(k.chunk, k.withSeq.data(), k.withSeq.size(), batch, nullptr); }
    int gatherKept(Worker &k, void *dPass, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *nPassed) {
        if (fastq_) return ts_sam_chunk_gather_fastq(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, fastqFlags_, dst, cap, bytes, nPassed, nullptr);
        return ts_sam_chunk_gather(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, dst, cap, bytes, nPassed, nullptr);
    }
    int blockLines(Worker &k, ts_batch *batch, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *lines) {
        return ts_sam_chunk_block_lines(k.chunk, k.withSeq.data(), k.withSeq.size(), batch, dst, cap, bytes, lines, nullptr);
    }
    bool frameChunk(Worker &k, bool atEnd) {
        k.n = k.headerLines = 0; k.error = TS_SAM_OK; k.header.clear();
        if (first_) {
            if (ts_bam_chunk_size(k.chunk) == 0) {
                if (atEnd) throw std::runtime_error("SAM input is empty");
                return true;
            }
            first_ = false;
        }
        uint64_t headerEnd = 0, nLines = 0, errorLine = 0, errorOff = 0;
        const Clock::time_point t0 = Clock::now();
        auto walk = [&]() {
            return ts_sam_chunk_walk(k.chunk, atEnd ? 1 : 0, inHeader_ ? 1 : 0, k.recs.data(), k.recs.size(), &k.n, &k.headerLines, &headerEnd, &nLines,
                                     &prevNext_, &k.error, &errorLine, &errorOff);
        };
        int rc = walk();
        if (rc == TS_ERR_INVALID_ARG && k.n > k.recs.size()) {
            k.recs.resize(static_cast<size_t>(k.n));
            rc = walk();
        }
        if (rc != TS_OK) throw deviceError(k.ctx, "SAM walk failed");
        if (headerEnd && !fastq_) {                             // (FASTQ out writes no header line)
            k.header.resize(static_cast<size_t>(headerEnd));
            if (ts_bam_chunk_read(k.chunk, 0, headerEnd, k.header.data()) != TS_OK) throw deviceError(k.ctx, "cannot read the chunk");
        }
        k.st.msWalk += since(t0);
        k.errorLine = lines_ + errorLine + 1;
        lines_ += nLines;
        if (k.headerLines < nLines || k.error != TS_SAM_OK) inHeader_ = false;
        return k.error == TS_SAM_OK;
    }

private:
    void writeHeader(Worker &k) {
        if (k.header.empty()) return;
        write(reinterpret_cast<const unsigned char *>(k.header.data()), k.header.size());
        k.header.clear();
    }

    bool fastq_;                                                // the kept records leave as FASTQ text (ts_sam_chunk_gather_fastq)
    uint32_t fastqFlags_;
    // more of the framing's state: the input is still in its header; whole lines behind
    bool inHeader_ = true;
    uint64_t lines_ = 0;
};

// (the route itself, behind samSubsetDevice and samSubsetFastqDevice)
inline SamSubsetStats samSubsetDeviceRun(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter, size_t readsPerBatch, size_t chunkBytes,
                                         std::vector<ReadRouteDeviceStats> *perDevice, std::ostream *blocks, const ReadFastqOutput *fastq) {
    return textSubsetDeviceRun<SamChunkSteps>("SAM", "samSubsetDevice", inFile, out, filter, readsPerBatch, chunkBytes, perDevice, blocks, fastq);
}
}  // namespace detail
// The device route of --sam-subset (same arguments, result, exceptions and output bytes as samSubset): the SAM text exists in HBM
// one chunk of ~chunkBytes bytes at a time and the host reads none of it but the header lines, which it writes.  The text gets
// there through detail::ChunkFeed (a plain file, BGZF members inflated on the device, a stream through zlib or read(2), plain gzip
// on the device under TS_GZIP_DEVICE=1; `-` is stdin, always through zlib); behind the source the lines and tabs are indexed and the
// lines cut and checked (ts_sam_chunk_walk: the table comes back), the sequences staged into a tips-only batch's input buffer
// (ts_sam_chunk_stage), judged and the passing lines gathered (detail::ReadJudge with ts_sam_chunk_gather).  A filter of one
// context takes every chunk in place; on a filter of several contexts the ring deals the chunks to all of them, and there plain
// gzip is read through zlib, as for fastqSubsetDevice.  perDevice, where given, receives one entry per context.
inline SamSubsetStats samSubsetDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                      size_t readsPerBatch = 1u << 20, size_t chunkBytes = 256u << 20,
                                      std::vector<ReadRouteDeviceStats> *perDevice = nullptr, std::ostream *blocks = nullptr) {
    return detail::samSubsetDeviceRun(inFile, out, filter, readsPerBatch, chunkBytes, perDevice, blocks, nullptr);
}
// The device route of --sam-subset with FASTQ out (same arguments, statistics, exceptions and output bytes as samSubsetFastq):
// samSubsetDevice's chunk steps on every context of the filter, with ts_sam_chunk_gather_fastq as detail::ReadJudge's gather; the
// header lines are counted and stay on the device.  The bytes do not depend on the number of contexts, readsPerBatch or chunkBytes.
// The TS_TIMING lines are samSubsetDevice's.
inline SamSubsetStats samSubsetFastqDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                           const ReadFastqOutput &fastq = ReadFastqOutput(), size_t readsPerBatch = 1u << 20, size_t chunkBytes = 256u << 20,
                                           std::vector<ReadRouteDeviceStats> *perDevice = nullptr, std::ostream *blocks = nullptr) {
    return detail::samSubsetDeviceRun(inFile, out, filter, readsPerBatch, chunkBytes, perDevice, blocks, &fastq);
}

inline const char *scaffoldTypeToString(ScaffoldType t) {       // src/tools.cpp
    static const char *names[] = {"t2t", "gapped_t2t", "misassembly", "gapped_misassembly", "incomplete",
                                  "gapped_incomplete", "none", "gapped_none", "discordant", "gapped_discordant"};
    return names[static_cast<int>(t)];
}

// Totals that writeBEDFile accumulates and printSummary reports.
struct AssemblySummary {
    uint32_t totalPaths = 0, totalNWindows = 0, totalITS = 0, totalCanMatches = 0, totalTelomeres = 0, totalGaps = 0;
    uint32_t byType[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t scaffoldN50 = 0, contigN50 = 0;
    float teloMean = 0.0f, teloMedian = 0.0f, teloMin = 0.0f, teloMax = 0.0f;
    // assembly record filters (src/teloscope.cpp:1007-1012): the two counts are printed only when filtering was on
    bool filterActive = false;
    uint64_t filterInputCount = 0, filterSelectedCount = 0;
};

namespace detail {

// the text operator<< produces, appended to a string without a stream
inline void put(std::string &s, uint64_t v) {
    char b[24];
    s.append(b, std::to_chars(b, b + sizeof b, v).ptr);
}
inline void put(std::string &s, float v) {                      // default ostream float: %g, precision 6
    // The float columns of the window files take few distinct values (ratios of small integers, entropy rounded to
    // three decimals), and shortest-round-trip formatting is the costly part of a line: every thread remembers the
    // text of the values it has formatted (4096-entry direct-mapped table keyed by the float's bits).
    struct Memo { uint32_t key; uint8_t len; char text[19]; };
    thread_local std::vector<Memo> memo;
    if (memo.empty()) { memo.resize(4096); for (Memo &m : memo) { m.key = 0; m.len = 0; } }
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    Memo &m = memo[(bits * 2654435761u) >> 20];
    if (m.len == 0 || m.key != bits) {
        char b[48];
        const size_t n = static_cast<size_t>(std::to_chars(b, b + sizeof b, v, std::chars_format::general, 6).ptr - b);
        if (n > sizeof m.text) { s.append(b, n); return; }
        m.key = bits; m.len = static_cast<uint8_t>(n);
        std::memcpy(m.text, b, n);
    }
    s.append(m.text, m.len);
}
inline void put(std::string &s, const std::string &v) { s += v; }
inline void put(std::string &s, const char *v) { s += v; }
inline void put(std::string &s, char v) { s += v; }

template <typename... A>
inline void line(std::string &s, const A &...a) { (put(s, a), ...); }

inline uint64_t computeN50(std::vector<uint64_t> v) {           // include/teloscope.h:224-235
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end(), [](uint64_t a, uint64_t b) { return a > b; });
    uint64_t total = 0, cum = 0;
    for (uint64_t l : v) total += l;
    for (uint64_t l : v) { cum += l; if (cum * 2 >= total) return l; }
    return v.back();
}

enum File { DENSITY, CANON_RATIO, STRAND_RATIO, GC, ENTROPY, CAN_MATCH, NONCAN_MATCH, TERMINAL, ITS, GAPS, REPORT, CONSOLE, NFILES };

struct Task {                                  // a path's blocks/gaps/matches/report row, or a run of its windows
    uint32_t path;
    bool windows;
    size_t w0, w1;
};

}  // namespace detail

// handleBEDFile + writeBEDFile: writes <outBase>_*.bed / .bedgraph / _report.tsv and the console path
// report; fills the totals printSummary needs.  Incremental: paths are added in seqPos order, all at once
// (writeBEDFiles) or group by group while later records are still being read and scanned (scanFastaToFiles).
class BedWriter {
    std::string outBase;
    const UserInputTeloscope &ui;
    std::ostream &console;
    bool manualCuration;
    unsigned threads;
    bool on[detail::NFILES];
    std::ofstream files[detail::NFILES];
    std::vector<float> telomereLengths;
    std::vector<uint64_t> scaffoldLens, contigLens;
    AssemblySummary sum;

    void format(const PathData &pd, const detail::Task &t, std::array<std::string, detail::NFILES> &o) const {
        using namespace detail;
        const std::string &h = pd.header;
        if (t.windows) {
            // the five window files share "header \t start \t end \t" per window: it is formatted once, and every file's
            // buffer is sized up front (30 M lines for a 3 Gb assembly: string growth and per-field appends were half the cost)
            const size_t nwin = t.w1 - t.w0, per = h.size() + 48;
            for (int f : {DENSITY, CANON_RATIO, STRAND_RATIO})
                if (ui.outWinRepeats) o[f].reserve(o[f].size() + nwin * per);
            if (ui.outEntropy) o[ENTROPY].reserve(o[ENTROPY].size() + nwin * per);
            if (ui.outGC) o[GC].reserve(o[GC].size() + nwin * per);
            std::string prefix;
            prefix.reserve(per);
            auto emit = [&](std::string &dst, float v) {
                dst.append(prefix);
                put(dst, v);
                dst.push_back('\n');
            };
            for (size_t i = t.w0; i < t.w1; ++i) {
                const WindowData &w = pd.windows[i];
                const uint64_t end = w.windowStart + w.currentWindowSize;
                prefix.assign(h);
                prefix.push_back('\t');
                put(prefix, w.windowStart);
                prefix.push_back('\t');
                put(prefix, end);
                prefix.push_back('\t');
                if (ui.outWinRepeats) {
                    const uint32_t covered = w.fwdCovered + w.revCovered;
                    const float density = static_cast<float>(covered) / w.currentWindowSize;
                    const float canon = covered > 0 ? static_cast<float>(w.canonicalCovered) / (w.canonicalCovered + w.nonCanonicalCovered) : -1.0f;
                    const float strand = covered > 0 ? static_cast<float>(w.fwdCovered) / (w.fwdCovered + w.revCovered) : -1.0f;
                    emit(o[DENSITY], density);
                    emit(o[CANON_RATIO], canon);
                    emit(o[STRAND_RATIO], strand);
                }
                if (ui.outEntropy) emit(o[ENTROPY], w.shannonEntropy);
                if (ui.outGC) emit(o[GC], w.gcContent);
            }
            return;
        }
        for (const TelomereBlock &b : pd.terminalBlocks) {
            const uint64_t end = b.start + b.blockLen;
            const bool scaffoldTerminal = b.start < ui.terminalLimit || end > pd.pathSize - ui.terminalLimit;
            if (scaffoldTerminal || manualCuration)
                line(o[TERMINAL], h, '\t', b.start, '\t', end, '\t', uint64_t(b.blockLen), '\t', b.blockLabel, '\t',
                     uint64_t(b.forwardCount), '\t', uint64_t(b.reverseCount), '\t', uint64_t(b.canonicalCount), '\t',
                     uint64_t(b.nonCanonicalCount), '\t', pd.pathSize, '\t', scaffoldTerminal ? "scaffold" : "contig", '\n');
        }
        if (ui.outITS)
            for (const TelomereBlock &b : pd.interstitialBlocks)
                line(o[ITS], h, '\t', b.start, '\t', b.start + b.blockLen, '\t', uint64_t(b.blockLen), '\t', b.blockLabel, '\t',
                     uint64_t(b.forwardCount), '\t', uint64_t(b.reverseCount), '\t', uint64_t(b.canonicalCount), '\t',
                     uint64_t(b.nonCanonicalCount), '\t', pd.pathSize, '\n');
        for (const GapInfo &g : pd.gapInfos) line(o[GAPS], h, '\t', g.start, '\t', g.start + g.length, '\n');
        if (ui.outMatches) {
            for (const MatchInfo &m : pd.canonicalMatches)
                line(o[CAN_MATCH], h, '\t', m.position, '\t', m.position + m.matchSize, '\t', m.matchSeq, '\n');
            for (const MatchInfo &m : pd.nonCanonicalMatches)
                line(o[NONCAN_MATCH], h, '\t', m.position, '\t', m.position + m.matchSize, '\t', m.matchSeq, '\n');
        }
        uint64_t longest = 0;
        std::string labels;
        for (const TelomereBlock &b : pd.terminalBlocks)
            if (b.isLongest) { ++longest; labels += b.blockLabel; }
        std::string row;
        line(row, uint64_t(pd.seqPos) + 1, '\t', h, '\t', longest, '\t', labels.empty() ? std::string("none") : labels, '\t',
             uint64_t(static_cast<uint16_t>(pd.gapInfos.size())), '\t', scaffoldTypeToString(pd.scaffoldType), '\t', pd.terminalLabel);
        if (!ui.ultraFastMode)
            line(row, '\t', uint64_t(pd.interstitialBlocks.size()), '\t', pd.canonicalMatchCount, '\t',
                 pd.nWindows());
        row += '\n';
        o[REPORT] += row;
        o[CONSOLE] += row;
    }

public:
    BedWriter(const std::string &outBase_, const UserInputTeloscope &ui_, std::ostream &console_, bool manualCuration_ = false,
              unsigned threads_ = 0)
        : outBase(outBase_), ui(ui_), console(console_), manualCuration(manualCuration_), threads(threads_) {
        using namespace detail;
        static const char *suffix[NFILES] = {"_window_repeat_density.bedgraph", "_window_canonical_ratio.bedgraph",
                                             "_window_strand_ratio.bedgraph", "_window_gc.bedgraph", "_window_entropy.bedgraph",
                                             "_canonical_matches.bed", "_noncanonical_matches.bed", "_terminal_telomeres.bed",
                                             "_interstitial_telomeres.bed", "_gaps.bed", "_report.tsv", ""};
        const bool want[NFILES] = {ui.outWinRepeats, ui.outWinRepeats, ui.outWinRepeats, ui.outGC, ui.outEntropy, ui.outMatches,
                                   ui.outMatches, true, ui.outITS, true, true, false};
        for (int f = 0; f < NFILES; ++f) {
            on[f] = want[f];
            if (!on[f]) continue;
            files[f].open(outBase + suffix[f], std::ios::binary);
            if (!files[f]) throw std::runtime_error("Could not open '" + outBase + suffix[f] + "' for writing.");
        }
        if (ui.outWinRepeats) {
            files[DENSITY] << "track type=bedGraph name=\"Repeat Density\" description=\"Total repeat density per window\"\n";
            files[CANON_RATIO] << "track type=bedGraph name=\"Canonical Ratio\" description=\"Canonical fraction of repeat density per window\"\n";
            files[STRAND_RATIO] << "track type=bedGraph name=\"Strand Ratio\" description=\"Forward-strand fraction of repeat density per window\"\n";
        }
        if (ui.outEntropy) files[ENTROPY] << "track type=bedGraph name=\"Shannon Entropy\" description=\"Shannon entropy per window\"\n";
        if (ui.outGC) files[GC] << "track type=bedGraph name=\"GC Content\" description=\"GC content per window\"\n";
        console << "\n+++ Path Summary Report +++\n";
        const char *cols = ui.ultraFastMode ? "pos\theader\ttelomeres\tlabels\tgaps\ttype\tgranular\n"
                                            : "pos\theader\ttelomeres\tlabels\tgaps\ttype\tgranular\tits\tcanonical\twindows\n";
        console << cols;
        files[REPORT] << cols;
        if (threads == 0) threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    }

    // formats and writes these paths (which follow, in seqPos order, the ones added before).  text: the lines of these paths'
    // windows as the device formatted them (walkRecordViews with a TrackText; the paths' `windows` are empty then): each track's
    // bytes go to its file as they are, large ones on a thread per file as the host-formatted ones do.  Without text — null —
    // this is add(paths) as it always was.
    void add(const std::vector<PathData> &paths, const TrackText *text = nullptr) {
        using namespace detail;
        std::vector<std::thread> textWriters;
        struct JoinText { std::vector<std::thread> &t; ~JoinText() { for (std::thread &th : t) if (th.joinable()) th.join(); } } joinText{textWriters};
        if (text) {
            static_assert(DENSITY == 0 && CANON_RATIO == 1 && STRAND_RATIO == 2 && GC == 3 && ENTROPY == 4, "track order is File order");
            for (int f = DENSITY; f <= ENTROPY; ++f) {
                if (!on[f] || !text->size(f)) continue;
                auto put = [this, text, f] { files[f].write(text->data(f), static_cast<std::streamsize>(text->size(f))); };
                if (text->size(f) >= (size_t(1) << 20) && threads > 1) textWriters.emplace_back(put);
                else put();
            }
            // ... and the match lines, when the device formatted them too (the paths' match vectors are empty then)
            static_assert(NONCAN_MATCH == CAN_MATCH + 1, "match file order is File order");
            for (int k = 0; k < TS_N_MATCH_FILES; ++k) {
                const int f = CAN_MATCH + k;
                if (!on[f] || !text->matchSize(k)) continue;
                auto put = [this, text, f, k] { files[f].write(text->matchData(k), static_cast<std::streamsize>(text->matchSize(k))); };
                if (text->matchSize(k) >= (size_t(1) << 20) && threads > 1) textWriters.emplace_back(put);
                else put();
            }
        }
        // work list in output order: per path its row/blocks/gaps/matches, then its windows in runs
        constexpr size_t kRun = 1u << 16;
        std::vector<Task> tasks;
        for (uint32_t p = 0; p < paths.size(); ++p) {
            tasks.push_back(Task{p, false, 0, 0});
            for (size_t w = 0; w < paths[p].windows.size(); w += kRun)
                tasks.push_back(Task{p, true, w, std::min(paths[p].windows.size(), w + kRun)});
        }
        // batches of tasks are formatted in parallel and written in order
        const size_t batch = static_cast<size_t>(threads) * 4;
        std::vector<std::array<std::string, NFILES>> outs(batch);
        for (size_t b0 = 0; b0 < tasks.size(); b0 += batch) {
            const size_t nb = std::min(batch, tasks.size() - b0);
            for (size_t i = 0; i < nb; ++i)
                for (std::string &s : outs[i]) s.clear();
            std::atomic<size_t> next{0};
            auto worker = [&]() {
                for (size_t i; (i = next.fetch_add(1)) < nb;) format(paths[tasks[b0 + i].path], tasks[b0 + i], outs[i]);
            };
            const unsigned nt = static_cast<unsigned>(std::min<size_t>(threads, nb));
            if (nt <= 1) {
                worker();
            } else {
                std::vector<std::thread> pool;
                for (unsigned i = 0; i < nt; ++i) pool.emplace_back(worker);
                for (std::thread &th : pool) th.join();
            }
            // The files are independent of each other: a file's pieces go out in task order, different files side by side — the
            // five window tracks carry nearly all the bytes (2.6 GB per 3 Gb), and one thread copying them into the page cache
            // file after file was the write stage's bound (round 5: 12 GB/s).  Small shares are written here.
            auto write_file = [&](int f) {
                for (size_t i = 0; i < nb; ++i)
                    if (!outs[i][f].empty()) files[f].write(outs[i][f].data(), static_cast<std::streamsize>(outs[i][f].size()));
            };
            std::vector<std::thread> writers;
            for (int f = 0; f < NFILES; ++f) {
                if (f == CONSOLE || !on[f]) continue;
                size_t bytes = 0;
                for (size_t i = 0; i < nb; ++i) bytes += outs[i][f].size();
                if (bytes >= (size_t(1) << 20) && threads > 1) writers.emplace_back(write_file, f);
                else if (bytes) write_file(f);
            }
            for (size_t i = 0; i < nb; ++i) console << outs[i][CONSOLE];
            for (std::thread &th : writers) th.join();
        }
        // totals (what writeBEDFile accumulates while writing) and summary counts (computeSummaryCounts)
        sum.totalPaths += static_cast<uint32_t>(paths.size());
        for (const PathData &pd : paths) {
            for (const TelomereBlock &b : pd.terminalBlocks)
                if (b.isLongest) { ++sum.totalTelomeres; telomereLengths.push_back(static_cast<float>(b.blockLen)); }
            sum.totalGaps += static_cast<uint16_t>(pd.gapInfos.size());
            if (!ui.ultraFastMode) {
                sum.totalNWindows += static_cast<uint32_t>(pd.nWindows());
                sum.totalITS += static_cast<uint32_t>(pd.interstitialBlocks.size());
                sum.totalCanMatches += static_cast<uint32_t>(pd.canonicalMatchCount);
            }
            sum.byType[static_cast<int>(pd.scaffoldType)]++;
            scaffoldLens.push_back(pd.pathSize);
            std::vector<GapInfo> gaps = pd.gapInfos;
            std::sort(gaps.begin(), gaps.end(), [](const GapInfo &a, const GapInfo &b) { return a.start < b.start; });
            uint64_t prevEnd = 0;
            for (const GapInfo &g : gaps) {
                if (g.start > prevEnd) contigLens.push_back(g.start - prevEnd);
                prevEnd = g.start + g.length;
            }
            if (pd.pathSize > prevEnd) contigLens.push_back(pd.pathSize - prevEnd);
        }
    }

    // closes the files and returns the totals printSummary reports
    AssemblySummary finish() {
        using namespace detail;
        // (flushed and closed side by side: eleven closes one after the other were 57 ms behind a 3 Gb assembly's last group)
        {
            std::atomic<bool> bad{false};
            std::vector<std::thread> closers;
            for (int f = 0; f < NFILES; ++f)
                if (on[f]) closers.emplace_back([this, f, &bad] {
                    files[f].flush();
                    if (!files[f].good()) bad.store(true);
                    files[f].close();
                });
            const auto tc0 = std::chrono::steady_clock::now();
            for (std::thread &th : closers) th.join();
            if (std::getenv("TS_MIRROR_TRACE"))
                std::fprintf(stderr, "trace closes %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count());
            if (bad.load()) throw std::runtime_error("failed while writing the output files of " + outBase);
        }
        sum.scaffoldN50 = computeN50(scaffoldLens);
        sum.contigN50 = computeN50(contigLens);
        if (!telomereLengths.empty()) {                              // getStats, src/tools.cpp:23-51
            std::vector<float> &v = telomereLengths;
            float total = 0.0f;
            sum.teloMin = sum.teloMax = v[0];
            for (float x : v) { sum.teloMin = std::min(sum.teloMin, x); sum.teloMax = std::max(sum.teloMax, x); total += x; }
            sum.teloMean = total / v.size();
            std::sort(v.begin(), v.end());
            const size_t mid = v.size() / 2;
            sum.teloMedian = v.size() % 2 ? v[mid] : (v[mid] + v[mid - 1]) / 2;
        }
        return sum;
    }
};

// `paths` must be in seqPos order (walkPaths' order).
inline void writeBEDFiles(const std::string &outBase, const std::vector<PathData> &paths, const UserInputTeloscope &ui,
                          std::ostream &console, AssemblySummary &sum, bool manualCuration = false, unsigned threads = 0) {
    BedWriter w(outBase, ui, console, manualCuration, threads);
    w.add(paths);
    sum = w.finish();
}

// printSummary: the same text to the console and (appended) to <outBase>_report.tsv when given.
inline void printSummary(std::ostream &console, const AssemblySummary &s, bool ultraFastMode, const std::string &reportFile = "") {
    using detail::line;
    std::string t;
    line(t, "\n+++ Assembly Summary Report +++\n", "Total paths:\t", uint64_t(s.totalPaths), '\n');
    if (s.filterActive)
        line(t, "Filter input paths:\t", s.filterInputCount, '\n', "Filter selected paths:\t", s.filterSelectedCount, '\n');
    line(t, "Total gaps:\t", uint64_t(s.totalGaps), '\n',
         "Scaffold N50:\t", s.scaffoldN50, '\n', "Contig N50:\t", s.contigN50, '\n', "Total telomeres:\t", uint64_t(s.totalTelomeres), '\n');
    if (!ultraFastMode)
        line(t, "Total ITS blocks:\t", uint64_t(s.totalITS), '\n', "Total canonical matches:\t", uint64_t(s.totalCanMatches), '\n',
             "Total windows analyzed:\t", uint64_t(s.totalNWindows), '\n');
    line(t, "\n+++ Telomere Statistics +++\n");
    if (s.totalTelomeres > 0)
        line(t, "Mean length:\t", s.teloMean, '\n', "Median length:\t", s.teloMedian, '\n', "Min length:\t", s.teloMin, '\n',
             "Max length:\t", s.teloMax, '\n');
    else
        line(t, "No telomeres found for statistics.\n");
    const uint32_t *c = s.byType;
    line(t, "\n+++ Chromosome Telomere Counts+++\n", "Two telomeres:\t", uint64_t(c[0] + c[1] + c[2] + c[3]), '\n',
         "One telomere:\t", uint64_t(c[4] + c[5]), '\n', "Zero telomeres:\t", uint64_t(c[6] + c[7]), '\n');
    line(t, "\n+++ Chromosome Telomere/Gap Completeness+++\n", "T2T:\t", uint64_t(c[0]), '\n', "Gapped T2T:\t", uint64_t(c[1]), '\n',
         "Misassembled:\t", uint64_t(c[2]), '\n', "Gapped misassembled:\t", uint64_t(c[3]), '\n', "Incomplete:\t", uint64_t(c[4]), '\n',
         "Gapped incomplete:\t", uint64_t(c[5]), '\n', "No telomeres:\t", uint64_t(c[6]), '\n', "Gapped no telomeres:\t", uint64_t(c[7]), '\n',
         "Discordant:\t", uint64_t(c[8]), '\n', "Gapped discordant:\t", uint64_t(c[9]), '\n');
    console << t;
    if (!reportFile.empty()) {
        std::ofstream f(reportFile, std::ios::binary | std::ios::app);
        if (!f) throw std::runtime_error("Could not open '" + reportFile + "' for writing.");
        f << t;
    }
}

// ---------------------------------------------------------------------------------------------
// FASTA text in, all output files out, as ONE pipeline (rows f2 + f3 together).  The reference loads the whole
// genome, runs one job per path, sorts and then writes (Input::read, src/input.cpp:575-734); with the scan in
// milliseconds that order leaves three whole-genome phases — parse, scan, format — one after the other on the
// host.  Here records flow in groups of ~256 MB through three stages that overlap:
//
//   read    a mapped file's records are located by one parallel pass over the text; a group's body lines are
//           joined into one buffer per record by all host threads (two passes: count, copy — no zero-fill, no
//           per-line allocation)                                                    [reader thread + pool]
//   scan    splitPath + ONE batched scan of the group's segments + labelTerminalBlocks (walkRecordViews)
//   write   BedWriter::add formats the group's lines on the host threads and appends them to the files
//
// Groups are consecutive runs of records, so everything leaves in seqPos order: the files and the console text
// are byte-identical to readFasta + walkPaths + writeBEDFiles (tests/test_writers.py runs both).
namespace detail {

// bases of [p, end) without the line ends ('\n', and a '\r' right before it or at the very end); [p, end) starts
// at a line start.  Eight bytes at a time: line ends are counted, not searched for.
inline size_t countFastaBases(const char *p, const char *end) {
    const size_t len = static_cast<size_t>(end - p);
    const uint64_t ones = 0x0101010101010101ull, low7 = 0x7F7F7F7F7F7F7F7Full;
    auto zeroBytes = [&](uint64_t v) { return ~(((v & low7) + low7) | v | low7); };            // 0x80 in every zero byte, exactly
    size_t nl = 0, cr = 0, i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t v;
        std::memcpy(&v, p + i, 8);
        nl += static_cast<size_t>(__builtin_popcountll(zeroBytes(v ^ (ones * 0x0A))));
        cr += static_cast<size_t>(__builtin_popcountll(zeroBytes(v ^ (ones * 0x0D))));
    }
    for (; i < len; ++i) { nl += p[i] == '\n'; cr += p[i] == '\r'; }
    if (cr == 0) return len - nl;
    // carriage returns: only those that end a line are dropped (rare input: count them the careful way)
    size_t n = 0;
    while (p < end) {
        const char *q = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        const char *stop = q ? q : end;
        if (stop > p) n += static_cast<size_t>((stop[-1] == '\r' ? stop - 1 : stop) - p);
        p = q ? q + 1 : end;
    }
    return n;
}
inline char *copyFastaBases(const char *p, const char *end, char *dst) {
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        const char *stop = nl ? nl : end;
        if (stop > p) {
            const size_t n = static_cast<size_t>((stop[-1] == '\r' ? stop - 1 : stop) - p);
            std::memcpy(dst, p, n);
            dst += n;
        }
        p = nl ? nl + 1 : end;
    }
    return dst;
}

struct RawRecord {                                              // a record of a streamed group
    std::string header;
    std::unique_ptr<char[]> data;                               // joined bases (new char[]: not zero-filled) — or,
    std::vector<ts_text_piece> pieces;                          // text mode: the record's body text where the file is mapped
    std::vector<TextLines> lines;                               //            and how each piece's lines lie (for matchSeq)
    size_t size = 0;                                            // bases
};

struct FastaGroup {
    size_t firstRecord = 0;
    std::vector<size_t> seqPos;                                 // per record: its index in the whole input
    std::vector<RawRecord> records;
    std::vector<PathComponents> comps;                          // of `records`, found while their bases were copied
    std::shared_ptr<void> mapping;                              // text mode: the records' pieces point into the mapped file
    std::vector<FastaRecord> owned;                             // gzip / stdin input: records read the plain way
};

}  // namespace detail

// Groups of consecutive records of a FASTA file, each with its records' lines joined.
//
// Assembly record filters: the reader is made with strict = true (the filtered loader's rules, src/input.cpp:285-361, are
// checked while the records are located; a SequenceFilterError names the first offence), its primaryIds() go through
// SequenceSelector::select, and keep(sel.keep) before the first next() leaves the dropped records out of every group: they are
// never joined, split or handed to the library, and group sizes count kept bytes only.  Each group carries its records' input
// indices (FastaGroup::seqPos).  A strict reader of input that cannot be mapped (gzip, a FIFO) decompresses it into memory
// first and then works as on a mapped file.
class FastaGroupReader {
    struct Span { const char *head, *body, *stop; };
    int fd = -1;
    void *map = nullptr;
    size_t mapSize = 0;
    std::shared_ptr<void> mapping;                              // unmaps when the reader AND every group that points into it are gone
    const char *text = nullptr;                                 // the records' text: the mapped file, or (strict) the decompressed input
    size_t textSize = 0;
    std::vector<Span> spans;
    size_t nextSpan = 0;
    size_t groupBytes, pieceBytes;
    bool textPieces;                                            // records as text pieces (line ends skipped by the library's staging)
    std::vector<FastaRecord> all;                               // not a mapped plain file: everything was read up front
    bool mapped = false;
    bool strict = false;
    std::vector<std::string> ids;                               // primary IDs (strict: found while checking)
    std::vector<char> kept;                                     // empty = every record
    uint64_t nKept = 0;

    size_t records() const { return mapped ? spans.size() : all.size(); }
    bool isKept(size_t i) const { return kept.empty() || kept[i]; }
    static std::string idOf(const Span &sp) {                   // the header up to its first whitespace
        const char *e = sp.body > sp.head && sp.body[-1] == '\n' ? sp.body - 1 : sp.body, *w = sp.head;
        while (w < e && !std::strchr(" \t\r\n\f\v", *w)) ++w;
        return std::string(sp.head, w);
    }

    // the filtered loader's rules over the located records, in the order the reference meets them while reading line by line
    void checkStrict(const char *data, const char *first) {
        if (!spans.empty() ? spans[0].head - 1 > first : first < data + textSize)
            throw SequenceFilterError("Assembly record filters require FASTA input or a recognized GFA file.");
        auto hasBases = [](const Span &sp) {
            for (const char *p = sp.body; p < sp.stop; ++p)
                if (*p != '\n' && *p != '\r') return true;
            return false;
        };
        std::unordered_set<std::string> seen;
        ids.resize(spans.size());
        for (size_t i = 0; i < spans.size(); ++i) {
            if (i && !hasBases(spans[i - 1])) throw SequenceFilterError("FASTA record '" + ids[i - 1] + "' has no sequence.");
            ids[i] = idOf(spans[i]);
            if (ids[i].empty()) throw SequenceFilterError("FASTA input contains an empty primary sequence ID.");
            if (!seen.insert(ids[i]).second) throw SequenceFilterError("Input contains duplicate primary sequence ID: '" + ids[i] + "'.");
        }
        if (spans.empty()) throw SequenceFilterError("Assembly input is empty.");
        if (!hasBases(spans.back())) throw SequenceFilterError("FASTA record '" + ids.back() + "' has no sequence.");
    }

public:
    // pieceBytes: text bytes a host thread handles at a time (a record's lines are counted / joined by pieces, in parallel).
    // textPieces: do not join the lines at all — a record is the list of its text pieces in the mapped file, with their
    // base counts and N-runs (one pass over the text); the library strips the line ends while it stages the upload
    // (TS_INPUT_TEXT_PIECES).  Only for a mapped plain file; gzip / stdin input is joined by zlib's reader anyway.
    // strict: assembly record filters are on (see above).
    explicit FastaGroupReader(const std::string &file, size_t groupBytes_ = size_t(256) << 20, size_t pieceBytes_ = size_t(4) << 20,
                              bool textPieces_ = false, bool strict_ = false)
        : groupBytes(std::max<size_t>(groupBytes_, 1)), pieceBytes(std::min<size_t>(std::max<size_t>(pieceBytes_, 1), size_t(16) << 20)),
          textPieces(textPieces_), strict(strict_) {
        fd = ::open(file.c_str(), O_RDONLY);
        if (fd < 0) {
            if (strict) throw SequenceFilterError("Could not open assembly input '" + file + "'.");
            throw std::runtime_error("cannot open " + file);
        }
        struct stat sb;
        unsigned char magic[2] = {0, 0};
        const bool gz = ::pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        if (!gz && ::fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
            mapSize = static_cast<size_t>(sb.st_size);
            map = ::mmap(nullptr, mapSize, PROT_READ, MAP_PRIVATE, fd, 0);
            if (map == MAP_FAILED) map = nullptr;
        }
        if (map) {
            const size_t n = mapSize;
            mapping = std::shared_ptr<void>(map, [n](void *p) { ::munmap(p, n); });
            (void)::madvise(map, mapSize, MADV_SEQUENTIAL);
            text = static_cast<const char *>(map);
            textSize = mapSize;
        } else {
            ::close(fd); fd = -1;
            if (!strict) {                                       // gzip (zlib is one serial stream anyway), FIFOs, empty files
                all = readFasta(file);
                return;
            }
            auto buf = std::make_shared<std::string>();          // plain and gzip alike, through zlib
            gzFile in = gzopen(file.c_str(), "rb");
            if (!in) throw SequenceFilterError("Could not open assembly input '" + file + "'.");
            gzbuffer(in, 1u << 20);
            size_t used = 0;
            for (;;) {
                if (buf->size() - used < (size_t(1) << 20)) buf->resize(std::max<size_t>(buf->size() * 2, size_t(4) << 20));
                const int r = gzread(in, &(*buf)[used], static_cast<unsigned>(std::min<size_t>(buf->size() - used, size_t(1) << 30)));
                if (r < 0) { gzclose(in); throw SequenceFilterError("Could not read assembly input '" + file + "'."); }
                if (r == 0) break;
                used += static_cast<size_t>(r);
            }
            gzclose(in);
            buf->resize(used);
            text = buf->data();
            textSize = used;
            mapping = buf;
        }
        mapped = true;
        const char *data = text, *end = data + textSize;
        // strict: a UTF-8 byte order mark before the first line is not part of it
        const char *first = data + (strict && textSize >= 3 && std::memcmp(data, "\xef\xbb\xbf", 3) == 0 ? 3 : 0);
        // record starts = '>' at a line start; found by slices of the text in parallel, then put in order
        const size_t nslice = std::max<size_t>(1, std::min<size_t>(64, textSize >> 24));
        std::vector<std::vector<const char *>> found(nslice);
        detail::onThreads(nslice, [&](size_t k) {
            const char *lo = data + textSize / nslice * k, *hi = k + 1 == nslice ? end : data + textSize / nslice * (k + 1);
            for (const char *p = lo; p < hi;) {
                const char *gt = static_cast<const char *>(std::memchr(p, '>', static_cast<size_t>(hi - p)));
                if (!gt) break;
                if (gt == first || (gt > data && gt[-1] == '\n')) found[k].push_back(gt);
                p = gt + 1;
            }
        });
        std::vector<const char *> starts;
        for (const auto &v : found) starts.insert(starts.end(), v.begin(), v.end());
        for (size_t i = 0; i < starts.size(); ++i) {
            const char *gt = starts[i];
            const char *lim = i + 1 < starts.size() ? starts[i + 1] : end;
            const char *nl = static_cast<const char *>(std::memchr(gt, '\n', static_cast<size_t>(lim - gt)));
            spans.push_back(Span{gt + 1, nl ? nl + 1 : lim, lim});
        }
        if (strict) checkStrict(data, first);
    }
    ~FastaGroupReader() {
        if (map && !mapping) ::munmap(map, mapSize);
        if (fd >= 0) ::close(fd);
    }
    FastaGroupReader(const FastaGroupReader &) = delete;
    FastaGroupReader &operator=(const FastaGroupReader &) = delete;

    // the records' primary IDs (header up to the first whitespace), in input order: the names a SequenceSelector selects from
    const std::vector<std::string> &primaryIds() {
        if (ids.size() != records())
            for (size_t i = ids.size(); i < records(); ++i) ids.push_back(mapped ? idOf(spans[i]) : sequenceFilterId(all[i].header));
        return ids;
    }
    // keep[i] = record i goes on to the scan; before the first next()
    void keep(std::vector<char> flags) {
        if (flags.size() != records()) throw std::runtime_error("FastaGroupReader::keep: one flag per record expected");
        if (nextSpan) throw std::runtime_error("FastaGroupReader::keep: records were read already");
        kept = std::move(flags);
        nKept = static_cast<uint64_t>(std::count_if(kept.begin(), kept.end(), [](char c) { return c != 0; }));
    }
    uint64_t inputRecords() const { return records(); }
    uint64_t keptRecords() const { return kept.empty() ? records() : nKept; }
    bool isStrict() const { return strict; }
    // text pieces or joined lines (scanFastaToFiles decides once the library says what it takes); before the first next()
    void setTextPieces(bool on) { textPieces = on; }

    // the next group (false at the end of the file)
    bool next(detail::FastaGroup &g) {
        g = detail::FastaGroup{};
        // the group's records: the next kept ones, as many as fit in groupBytes (at least one)
        const size_t n = records();
        while (nextSpan < n && !isKept(nextSpan)) ++nextSpan;
        if (nextSpan >= n) return false;
        g.firstRecord = nextSpan;
        size_t bytes = 0;
        for (; nextSpan < n; ++nextSpan) {
            if (!isKept(nextSpan)) continue;
            const size_t b = mapped ? static_cast<size_t>(spans[nextSpan].stop - spans[nextSpan].body) : all[nextSpan].sequence.size();
            if (!g.seqPos.empty() && bytes + b > groupBytes) break;
            bytes += b;
            g.seqPos.push_back(nextSpan);
        }
        if (!mapped) {
            for (size_t i : g.seqPos) g.owned.push_back(std::move(all[i]));
            return true;
        }
        const size_t nrec = g.seqPos.size();
        g.records.resize(nrec);
        // pieces of ~4 MB of text, cut at line starts; pass 1 counts every piece's bases, pass 2 copies them to
        // their place in the record's buffer
        struct Piece { size_t rec; const char *a, *z; size_t bases, at; PathComponents pc; bool firstIsGap, lastIsGap; TextLines lines; };
        std::vector<Piece> pieces;
        const size_t kPiece = pieceBytes;
        for (size_t r = 0; r < nrec; ++r) {
            const Span &sp = spans[g.seqPos[r]];
            const char *he = sp.body > sp.head && sp.body[-1] == '\n' ? sp.body - 1 : sp.body;
            g.records[r].header = strict ? ids[g.seqPos[r]] : detail::fastaHeaderWord(sp.head, he);
            for (const char *a = sp.body; a < sp.stop;) {
                const char *z = sp.stop - a > static_cast<ptrdiff_t>(kPiece) ? a + kPiece : sp.stop;
                if (z < sp.stop) {
                    const char *nl = static_cast<const char *>(std::memchr(z, '\n', static_cast<size_t>(sp.stop - z)));
                    z = nl ? nl + 1 : sp.stop;
                }
                pieces.push_back(Piece{r, a, z, 0, 0, {}, false, false, TextLines{}});
                a = z;
            }
        }
        if (textPieces) {
            g.mapping = mapping;
            // ONE pass over the text: every piece's base count and N-runs; nothing is copied
            detail::onThreads(pieces.size(), [&](size_t i) {
                Piece &p = pieces[i];
                uint64_t nb = 0;
                p.pc = detail::splitPathText(p.a, p.z, &nb, &p.firstIsGap, &p.lastIsGap, &p.lines);
                p.bases = static_cast<size_t>(nb);
            });
            for (size_t i = 0; i < pieces.size(); ++i) {
                Piece &p = pieces[i];
                p.at = g.records[p.rec].size;
                g.records[p.rec].size += p.bases;
                for (auto &sg : p.pc.segments) sg.first += p.at;
                for (GapInfo &gp : p.pc.gaps) gp.start += p.at;
                if (p.bases) {
                    g.records[p.rec].pieces.push_back(ts_text_piece{p.a, static_cast<uint64_t>(p.z - p.a), static_cast<uint64_t>(p.bases)});
                    g.records[p.rec].lines.push_back(p.lines);
                }
            }
        } else {
        detail::onThreads(pieces.size(), [&](size_t i) { pieces[i].bases = detail::countFastaBases(pieces[i].a, pieces[i].z); });
        for (size_t i = 0; i < pieces.size(); ++i) {
            pieces[i].at = g.records[pieces[i].rec].size;
            g.records[pieces[i].rec].size += pieces[i].bases;
        }
        for (detail::RawRecord &rr : g.records) rr.data.reset(new char[rr.size + 1]);
        detail::onThreads(pieces.size(), [&](size_t i) {
            Piece &p = pieces[i];
            char *dst = g.records[p.rec].data.get() + p.at;
            (void)detail::copyFastaBases(p.a, p.z, dst);
            if (!p.bases) return;
            // N-runs of the piece, while its bases are still in this core's cache (in record coordinates)
            p.pc = splitPath(dst, p.bases);
            for (auto &sg : p.pc.segments) sg.first += p.at;
            for (GapInfo &gp : p.pc.gaps) gp.start += p.at;
            auto isGap = [](char c) { return c == 'N' || c == 'n' || c == 'X' || c == 'x'; };
            p.firstIsGap = isGap(dst[0]);
            p.lastIsGap = isGap(dst[p.bases - 1]);
        });
        }
        g.comps.resize(nrec);
        std::vector<int> prevLast(nrec, -1);                      // -1: no bases of the record yet
        for (const Piece &p : pieces) {
            if (!p.bases) continue;
            detail::appendPieceRuns(g.comps[p.rec], p.pc, prevLast[p.rec] >= 0, prevLast[p.rec] == 1, p.firstIsGap);
            prevLast[p.rec] = p.lastIsGap ? 1 : 0;
        }
        return true;
    }
};

// library_bases: the bases of the segments handed to the library (N-runs are not; neither are records a filter dropped)
// bases_read_back: joined bases the device routes copied back to the host (ts_fasta_chunk_bases: -m without deviceTracks)
struct ScanFastaTimes { double read_ms = 0, scan_ms = 0, write_ms = 0, wall_ms = 0; uint64_t bases = 0, windows = 0, library_bases = 0; size_t groups = 0;
                        uint64_t bases_read_back = 0; };

// FASTA file -> the eleven output files + console path report; returns the totals for printSummary.
// groupReader: a FastaGroupReader of fastaFile the caller made (and, with assembly record filters, selected from with keep())
// before any output file exists or any device call is made; nullptr = one made here.  Its groupBytes / pieceBytes are its own.
inline AssemblySummary scanFastaToFiles(Teloscope &teloscope, const std::string &fastaFile, const std::string &outBase,
                                        std::ostream &console, bool manualCuration = false,
                                        size_t groupBytes = size_t(256) << 20, ScanFastaTimes *times = nullptr,
                                        size_t pieceBytes = size_t(4) << 20, int textPieces = -1,
                                        FastaGroupReader *groupReader = nullptr) {
    // textPieces: -1 = whenever the library takes text input for this parameter set (the tiled kernel's), 0 / 1 = forced
    using Clock = std::chrono::steady_clock;
    auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t_begin = Clock::now();
    struct Scanned { detail::FastaGroup group; std::vector<PathData> paths; };
    detail::BoundedQueue<detail::FastaGroup> toScan(2);
    detail::BoundedQueue<Scanned> toWrite(2);
    std::exception_ptr readError, scanError;
    ScanFastaTimes T;
    const bool trace = std::getenv("TS_MIRROR_TRACE") != nullptr;      // per-group stage intervals on stderr (ms since the call began)

    std::thread reader([&] {
        try {
            const bool text = textPieces < 0 ? teloscope.takesTextPieces() : textPieces != 0;
            std::unique_ptr<FastaGroupReader> own;
            if (groupReader) groupReader->setTextPieces(text);
            else own.reset(new FastaGroupReader(fastaFile, groupBytes, pieceBytes, text));
            FastaGroupReader &rd = groupReader ? *groupReader : *own;
            detail::FastaGroup g;
            for (;;) {
                const auto t0 = Clock::now();
                if (!rd.next(g)) break;
                T.read_ms += ms(t0, Clock::now());
                toScan.push(std::move(g));
            }
        } catch (...) { readError = std::current_exception(); }
        toScan.close();
    });
    std::thread scanner([&] {
        try {
            detail::FastaGroup g;
            // The library's first call in a process pays for its streams, its kernels' code, the device pool and the pinned staging
            // (81-115 ms against 12-15 ms for a later group of 256 MB): made here, on a dummy record, while the reader is still
            // parsing its first group.
            {
                const auto tw = Clock::now();
                const std::string hdr = "warm-up", seq(size_t(1) << 20, 'A');
                std::vector<RecordView> one{RecordView{&hdr, seq.data(), seq.size(), nullptr, 0, nullptr}};
                try { (void)walkRecordViews(teloscope, one, 0, nullptr); } catch (...) {}
                if (trace) std::fprintf(stderr, "trace warm  %7.1f .. %7.1f\n", ms(t_begin, tw), ms(t_begin, Clock::now()));
            }
            while (toScan.pop(g)) {
                const auto t0 = Clock::now();
                std::vector<RecordView> views;
                for (const detail::RawRecord &r : g.records)
                    views.push_back(r.pieces.empty() && r.size ? RecordView{&r.header, r.data.get(), r.size, nullptr, 0, nullptr}
                                                               : RecordView{&r.header, nullptr, r.size, r.pieces.data(), r.pieces.size(), r.lines.data()});
                for (const FastaRecord &r : g.owned) views.push_back(RecordView{&r.header, r.sequence.data(), r.sequence.size(), nullptr, 0, nullptr});
                if (!g.owned.empty()) g.comps = splitPaths(views);
                for (const PathComponents &pc : g.comps)
                    for (const auto &sg : pc.segments) T.library_bases += sg.second;
                Scanned s;
                s.paths = walkRecordViews(teloscope, views, g.firstRecord, &g.comps, g.seqPos.empty() ? nullptr : &g.seqPos);
                s.group = std::move(g);                           // (-m: matchSeq was copied out of the bases already)
                T.scan_ms += ms(t0, Clock::now());
                if (trace) std::fprintf(stderr, "trace scan  %7.1f .. %7.1f\n", ms(t_begin, t0), ms(t_begin, Clock::now()));
                toWrite.push(std::move(s));
            }
        } catch (...) {
            scanError = std::current_exception();
            detail::FastaGroup drop;
            while (toScan.pop(drop)) {}
        }
        toWrite.close();
    });
    AssemblySummary sum;
    std::exception_ptr writeError;
    try {
        BedWriter writer(outBase, teloscope.input(), console, manualCuration);
        Scanned s;
        while (toWrite.pop(s)) {
            const auto t0 = Clock::now();
            writer.add(s.paths);
            for (const PathData &pd : s.paths) { T.bases += pd.pathSize; T.windows += pd.windows.size(); }
            ++T.groups;
            T.write_ms += ms(t0, Clock::now());
            if (trace) std::fprintf(stderr, "trace write %7.1f .. %7.1f\n", ms(t_begin, t0), ms(t_begin, Clock::now()));
        }
        const auto tf = Clock::now();
        sum = writer.finish();
        const UserInputTeloscope &ui = teloscope.input();          // (what the caller's selection set, as Input::read does)
        sum.filterActive = ui.sequenceFilterActive;
        sum.filterInputCount = ui.filterInputCount;
        sum.filterSelectedCount = ui.filterSelectedCount;
        if (trace) std::fprintf(stderr, "trace finish %7.1f .. %7.1f\n", ms(t_begin, tf), ms(t_begin, Clock::now()));
    } catch (...) {
        writeError = std::current_exception();
        Scanned drop;
        while (toWrite.pop(drop)) {}
    }
    reader.join();
    scanner.join();
    if (readError) std::rethrow_exception(readError);
    if (scanError) std::rethrow_exception(scanError);
    if (writeError) std::rethrow_exception(writeError);
    T.wall_ms = ms(t_begin, Clock::now());
    if (times) *times = T;
    return sum;
}

namespace detail {

// The device FASTA route's chunk sizes: chunkLimit clamped to what the walk takes (4 GiB - 2) and to what the feed leaves of
// it; -> the bytes a fill asks for.
inline size_t clampFastaChunk(const ChunkFeed &feed, size_t chunkBytesArg, uint64_t &chunkLimit) {
    chunkLimit = feed.chunkLimit(std::max<uint64_t>(std::min<uint64_t>(chunkLimit, 0xfffffffeull), 64));
    return static_cast<size_t>(std::min<uint64_t>(std::max<size_t>(chunkBytesArg, 64), chunkLimit));
}

// ts_fasta_chunk_walk over a chunk: n records in recs, their names in names (both grown, once, to what the walk asks for), the
// first byte behind the last complete record in next.
inline void walkFastaChunk(ts_ctx *ctx, ts_chunk *chunk, bool atEnd, std::vector<ts_fasta_record> &recs, std::vector<char> &names,
                           uint64_t &n, uint64_t &next) {
    for (bool grown = false;; grown = true) {
        uint64_t nameBytes = 0;
        const int rc = ts_fasta_chunk_walk(chunk, atEnd ? 1 : 0, recs.data(), recs.size(), &n, &next, names.data(), names.size(), &nameBytes);
        if (rc == TS_OK) return;
        if (grown || rc != TS_ERR_INVALID_ARG || (n <= recs.size() && nameBytes <= names.size())) throw deviceError(ctx, "FASTA walk failed");
        if (n > recs.size()) recs.resize(static_cast<size_t>(n));
        if (nameBytes > names.size()) names.resize(static_cast<size_t>(nameBytes));
    }
}

// What both bodies of scanFastaToFilesDevice do with the records of a walked chunk, and their common end: the stage times, the
// output files (made by open(), not before: a refusal in front of it leaves no file behind) and the summary.
class FastaChunkStage {
    using Clock = std::chrono::steady_clock;
    static double since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
    const Clock::time_point tBegin_ = Clock::now();
    Teloscope &teloscope_;
    // deviceTracks: the five window tracks are formatted on the device where the window records lie and come back as text
    // (opt-in: whether 13 x the records' bytes over PCIe beats the host's formatting threads depends on the box; README has the
    // measurement).  With -m the lines of the two match files are formatted there as well (ts_scan_segments_text), from the match
    // records and the joined bases where they lie: no base is read back and no match record downloaded.
    const bool useTrackText_;
    std::unique_ptr<BedWriter> writer_;
    ScanFastaTimes T_;
public:
    // What the judging of a chunk's records needs and leaves, one per context that judges (judge() fills it, any number of them
    // at once; emit() hands it to the writer, one at a time in chunk order): the host view of the bases, the runs, the window and
    // match text, the paths, and the chunk's share of the figures.
    struct Judged {
        TrackText trackText;
        std::vector<char> hostBases;
        std::vector<ts_fasta_run> runs = std::vector<ts_fasta_run>(4096);
        std::vector<uint64_t> offsets;
        std::vector<PathData> paths;
        uint64_t libraryBases = 0, basesReadBack = 0;
        double msJoin = 0, msScan = 0;
    };
private:
    Judged own_;                                                // add()'s
public:
    double msUpload = 0, msIndex = 0, msJoin = 0, msScan = 0, msWrite = 0;      // (the first two: the caller's stages)
    FastaChunkStage(Teloscope &teloscope, bool deviceTracks) : teloscope_(teloscope), useTrackText_(deviceTracks) {}
    void open(const std::string &outBase, std::ostream &console, bool manualCuration) {
        writer_.reset(new BedWriter(outBase, teloscope_.input(), console, manualCuration));
    }

    // Records recs[0, n) of the chunk: joined, their runs read (and their bases, where matchSeq needs them), scanned as device
    // segments, written.  header(i): record i's header, a string that outlives the call; seqPos: null = firstRecord, + 1, ...
    template <class Header>
    void add(ts_chunk *chunk, const ts_fasta_record *recs, size_t n, bool atEnd, const Header &header, size_t firstRecord,
             const std::vector<size_t> *seqPos) {
        judge(own_, 0, chunk, recs, n, atEnd, header, firstRecord, seqPos);
        emit(own_);
    }

    // add() up to the writer, on context `context` of the Teloscope, which is the chunk's: everything lands in `j`, and nothing
    // of the stage itself is written, so that several contexts may judge a chunk each at the same time.
    template <class Header>
    void judge(Judged &j, size_t context, ts_chunk *chunk, const ts_fasta_record *recs, size_t n, bool atEnd, const Header &header,
               size_t firstRecord, const std::vector<size_t> *seqPos) const {
        const UserInputTeloscope &ui = teloscope_.input();
        auto fail = [&](const char *what) { return deviceError(teloscope_.context(context), what); };
        auto t0 = Clock::now();
        const void *dBases = nullptr;
        uint64_t total = 0, nRuns = 0;
        j.libraryBases = j.basesReadBack = 0;
        j.offsets.resize(n);
        if (ts_fasta_chunk_join(chunk, recs, n, atEnd ? 1 : 0, &dBases, j.offsets.data(), &total, &nRuns, nullptr) != TS_OK) throw fail("FASTA join failed");
        if (nRuns > j.runs.size()) j.runs.resize(static_cast<size_t>(nRuns));
        if (ts_fasta_chunk_runs(chunk, j.runs.data(), j.runs.size(), &nRuns) != TS_OK) throw fail("reading the runs failed");
        const bool hostView = ui.outMatches && !ui.ultraFastMode && !useTrackText_;
        if (hostView) {                                         // matchSeq is cut out of the bases: one copy per chunk
            j.hostBases.resize(static_cast<size_t>(total) + 1);
            if (ts_fasta_chunk_bases(chunk, 0, total, j.hostBases.data()) != TS_OK) throw fail("reading the joined bases failed");
            j.basesReadBack = total;
        }
        j.msJoin = since(t0);
        std::vector<PathComponents> comps(n);
        std::vector<RecordView> views(n);
        for (uint64_t r = 0; r < nRuns; ++r) {
            const ts_fasta_run &run = j.runs[static_cast<size_t>(r)];
            if (run.record >= n) throw std::runtime_error("FASTA runs: a run of a record that was not joined");
            if (run.is_gap) comps[run.record].gaps.push_back(GapInfo{run.start, run.len});
            else { comps[run.record].segments.emplace_back(run.start, run.len); j.libraryBases += run.len; }
        }
        for (size_t i = 0; i < n; ++i)
            views[i] = RecordView{header(i), hostView ? j.hostBases.data() + j.offsets[i] : nullptr, recs[i].n_bases, nullptr, 0, nullptr,
                                  static_cast<const char *>(dBases) + j.offsets[i]};
        t0 = Clock::now();
        j.paths = walkRecordViews(teloscope_, views, firstRecord, &comps, seqPos, useTrackText_ ? &j.trackText : nullptr, static_cast<int>(context));
        j.msScan = since(t0);
    }
    // ... and the writer's part, in the order of the input: the judged paths written, the deterministic counters moved on
    void emit(Judged &j) {
        const auto t0 = Clock::now();
        writer_->add(j.paths, useTrackText_ ? &j.trackText : nullptr);
        for (const PathData &pd : j.paths) { T_.bases += pd.pathSize; T_.windows += pd.nWindows(); }
        T_.library_bases += j.libraryBases; T_.bases_read_back += j.basesReadBack;
        msJoin += j.msJoin; msScan += j.msScan;
        ++T_.groups;
        j.paths.clear();
        msWrite += since(t0);
    }

    // The files finished, the TS_TIMING line, *times; the summary with the filter facts the caller knows.
    AssemblySummary finish(bool filterActive, uint64_t filterInputCount, uint64_t filterSelectedCount, bool filtered, const ChunkFeed &feed,
                           ScanFastaTimes *times) {
        const auto tf = Clock::now();
        AssemblySummary sum = writer_->finish();
        sum.filterActive = filterActive; sum.filterInputCount = filterInputCount; sum.filterSelectedCount = filterSelectedCount;
        msWrite += since(tf);
        if (std::getenv("TS_TIMING"))
            std::fprintf(stderr, "scanFastaToFilesDevice%s: upload%s %.0f ms, index%s %.0f ms, join %.0f ms, scan %.0f ms, write %.0f ms\n",
                         filtered ? " (filtered)" : "", feed.deviceInflate() ? " + inflate + CRC" : "", msUpload, filtered ? " + check" : "",
                         msIndex, msJoin, msScan, msWrite);
        T_.read_ms = msUpload + msIndex + msJoin; T_.scan_ms = msScan; T_.write_ms = msWrite; T_.wall_ms = since(tBegin_);
        if (times) *times = T_;
        return sum;
    }
};

// scanFastaToFilesDevice with an active selector (its comment says what happens; the caller has checked the device count).
inline AssemblySummary scanFastaToFilesDeviceFiltered(Teloscope &teloscope, const std::string &fastaFile, const std::string &outBase,
                                                      std::ostream &console, bool manualCuration, size_t chunkBytesArg,
                                                      ScanFastaTimes *times, uint64_t chunkLimit, bool deviceTracks,
                                                      const SequenceSelector &selector, std::ostream &log, uint64_t residentLimit) {
    using Clock = std::chrono::steady_clock;
    auto since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    ts_ctx *ctx = teloscope.context();
    auto fail = [&](const char *what) { return deviceError(ctx, what); };
    FastaChunkStage stage(teloscope, deviceTracks);
    double &msUpload = stage.msUpload, &msIndex = stage.msIndex;

    struct ChunkFree { void operator()(ts_chunk *c) const { ts_bam_chunk_destroy(c); } };
    std::vector<std::unique_ptr<ts_chunk, ChunkFree>> chunks;   // every one stays until its kept records are written
    uint64_t resident = 0;
    const std::string hostRoute = "with assembly record filters the whole text stays in device memory until the selection is known; "
                                  "use scanFastaToFiles, the host route";
    auto noRoom = [&](const char *what) -> std::runtime_error {
        const char *why = ts_last_error(ctx);
        return std::runtime_error(std::string("scanFastaToFilesDevice: ") + what + " with " + std::to_string(resident) +
                                  " bytes of the assembly's text resident (" + (why ? why : "?") +
                                  "): the text does not fit the device's free memory; " + hostRoute);
    };
    ChunkFeed::Options options;
    options.cannotOpen = "Could not open assembly input '" + fastaFile + "'.";      // (the filtered host loader's words)
    options.cannotRead = "Could not read assembly input '" + fastaFile + "'.";
    options.growFailed = "cannot grow a device chunk";
    options.uploadFailed = "upload of the FASTA text failed";
    options.noRoom = noRoom;
    ChunkFeed feed(ctx, fastaFile, options);
    const size_t chunkBytes = clampFastaChunk(feed, chunkBytesArg, chunkLimit);
    const uint64_t compCap = feed.compCap(chunkBytes);
    auto makeChunk = [&](uint64_t cap) {
        ts_chunk *made = ts_bam_chunk_create(ctx, compCap, std::max<uint64_t>(cap, 64));
        if (!made) throw noRoom("cannot make a device chunk");
        chunks.emplace_back(made);
        return made;
    };
    auto checkResident = [&]() {
        if (residentLimit && resident > residentLimit)
            throw std::runtime_error("scanFastaToFilesDevice: " + std::to_string(resident) + " bytes of the assembly's text are resident and " +
                                     std::to_string(residentLimit) + " may be: the text does not fit the device's free memory; " + hostRoute);
    };

    // ---- phase 1: every chunk fed, walked, checked and kept; tables, IDs and the strict facts on the host
    struct Held { size_t slot; bool atEnd; size_t first; std::vector<ts_fasta_record> recs; };   // first: its first record's input index
    std::vector<Held> heldChunks;
    std::vector<std::string> ids;                               // primary IDs of all records, in input order
    std::vector<char> hasSequence;
    std::vector<ts_fasta_record> recs(4096);
    std::vector<char> names(size_t(1) << 16);
    std::vector<unsigned char> has;
    bool frontBytes = false, sawRecord = false;                 // bytes that belong to no record in front of the first one

    // the first bytes on their own: a UTF-8 byte order mark is not part of the first line, and is not carried on
    Clock::time_point t0 = Clock::now();
    ts_chunk *prev = nullptr, *cur = nullptr;
    uint64_t prevNext = 0, held = 0;
    bool atEnd = false, grow = false;
    {
        const uint64_t room = feed.read(64);
        prev = makeChunk(room);
        atEnd = feed.put(prev, 0);
        const uint64_t n = ts_bam_chunk_size(prev);
        unsigned char mark[3] = {0, 0, 0};
        if (n >= 3 && ts_bam_chunk_read(prev, 0, 3, mark) != TS_OK) throw fail("cannot read the chunk");
        prevNext = mark[0] == 0xef && mark[1] == 0xbb && mark[2] == 0xbf ? 3 : 0;
        resident += n;
        checkResident();
    }
    msUpload += since(t0);
    for (bool firstFill = true; firstFill || !atEnd; firstFill = false) {
        t0 = Clock::now();
        const uint64_t carry = grow ? held : ts_bam_chunk_size(prev) - prevNext;
        if (carry >= chunkLimit)
            throw std::runtime_error("a FASTA record of '" + fastaFile + "' has more than " + std::to_string(chunkLimit) +
                                     " bytes of text and does not fit a device chunk; use scanFastaToFiles, the host route");
        // a chunk that held no whole record takes as much again, up to what a chunk may hold
        const size_t want = static_cast<size_t>(std::min<uint64_t>(std::max<uint64_t>(chunkBytes, grow ? carry : 0), chunkLimit - carry));
        const uint64_t room = atEnd ? 0 : feed.read(want);
        if (!grow) {
            cur = makeChunk(carry + room);
            if (carry && ts_chunk_carry_over(cur, prev, prevNext, nullptr) != TS_OK) throw noRoom("cannot carry a record into the next device chunk");
        }
        if (!atEnd) atEnd = feed.put(cur, 0);
        msUpload += since(t0);
        resident += ts_bam_chunk_size(cur) - (grow ? held : 0);
        held = ts_bam_chunk_size(cur);
        checkResident();
        if (held == 0) continue;

        t0 = Clock::now();
        uint64_t n = 0, next = 0;
        walkFastaChunk(ctx, cur, atEnd, recs, names, n, next);
        if (!atEnd && n == 0 && next == 0) { grow = true; msIndex += since(t0); continue; }    // one unfinished record: the chunk takes more
        grow = false;
        has.resize(static_cast<size_t>(n));
        if (n && ts_fasta_chunk_strict(cur, recs.data(), static_cast<size_t>(n), has.data(), nullptr) != TS_OK) throw fail("FASTA strict check failed");
        msIndex += since(t0);
        if (!sawRecord && (n ? recs[0].off != 0 : next != 0)) frontBytes = true;
        sawRecord = sawRecord || n != 0;
        Held h{chunks.size() - 1, atEnd, ids.size(), std::vector<ts_fasta_record>(recs.begin(), recs.begin() + static_cast<ptrdiff_t>(n))};
        for (size_t i = 0; i < n; ++i) {
            ids.push_back(sequenceFilterId(std::string(names.data() + recs[i].name_at, recs[i].name_len)));
            hasSequence.push_back(static_cast<char>(has[i]));
        }
        heldChunks.push_back(std::move(h));
        prev = cur; prevNext = next;
    }

    // ---- between the phases: the filtered loader's rules in its order (FastaGroupReader::checkStrict), then the selection
    if (frontBytes) throw SequenceFilterError("Assembly record filters require FASTA input or a recognized GFA file.");
    {
        std::unordered_set<std::string> seen;
        for (size_t i = 0; i < ids.size(); ++i) {
            if (i && !hasSequence[i - 1]) throw SequenceFilterError("FASTA record '" + ids[i - 1] + "' has no sequence.");
            if (ids[i].empty()) throw SequenceFilterError("FASTA input contains an empty primary sequence ID.");
            if (!seen.insert(ids[i]).second) throw SequenceFilterError("Input contains duplicate primary sequence ID: '" + ids[i] + "'.");
        }
        if (ids.empty()) throw SequenceFilterError("Assembly input is empty.");
        if (!hasSequence.back()) throw SequenceFilterError("FASTA record '" + ids.back() + "' has no sequence.");
    }
    const SequenceSelection sel = selector.select(ids, "paths");
    log << selectionMessage(sel) << "\n";

    // ---- phase 2: the kept records of every chunk joined, scanned and written; the others are never read again
    stage.open(outBase, console, manualCuration);
    for (Held &h : heldChunks) {
        std::vector<ts_fasta_record> kept;
        std::vector<size_t> seqPos;
        for (size_t i = 0; i < h.recs.size(); ++i)
            if (sel.keep[h.first + i]) { kept.push_back(h.recs[i]); seqPos.push_back(h.first + i); }
        if (!kept.empty())
            stage.add(chunks[h.slot].get(), kept.data(), kept.size(), h.atEnd, [&](size_t i) { return &ids[seqPos[i]]; }, 0, &seqPos);
        chunks[h.slot].reset();                                 // (its text and its joined bases are done with)
    }
    // (the filter facts are this selection's: the context existed before it was known)
    return stage.finish(true, sel.inputCount, sel.selectedCount, true, feed, times);
}

}  // namespace detail

// One context's share of an assembly device route (scanFastaToFilesDevice; annotateGfaDevice in teloscope_mi355x_gfa.hpp): the
// HIP ordinal it was made on, chunks it took, records framed in them (FASTA records; GFA segments), bases it scanned (of the
// segments handed to the library), uncompressed bytes it received, and the milliseconds its thread spent filling a chunk in
// place (one context: upload or inflate straight behind the carry), staging a dealt chunk's bytes (several contexts), waiting
// for the chunk before its own to be framed (dealt chunks only: the serial section as this context sees it), placing the carry
// and committing the staged bytes behind it (dealt chunks only), indexing (the walk, and the GFA check), joining and scanning.
struct AssemblyRouteDeviceStats {
    int device = -1;
    uint64_t chunks = 0, records = 0, basesScanned = 0, bytesReceived = 0;
    double msFill = 0, msStage = 0, msFrameWait = 0, msCommit = 0, msIndex = 0, msJoin = 0, msScan = 0;
};

namespace detail {

// A route's per-context figures, to perDevice and, under TS_TIMING, to stderr: one line per context, each beginning with `route`.
// `ring` is the ring that dealt the chunks, or nothing (every chunk came in place: no context waited for another).
template <typename Worker, typename Ring>
inline void assemblyRouteFigures(const char *route, const std::vector<std::unique_ptr<Worker>> &workers, const Ring *ring,
                                 std::vector<AssemblyRouteDeviceStats> *perDevice) {
    if (perDevice) perDevice->clear();
    for (size_t w = 0; w < workers.size(); ++w) {
        AssemblyRouteDeviceStats s = workers[w]->st;
        if (ring) s.msFrameWait = ring->frameWaitMs(w);
        if (perDevice) perDevice->push_back(s);
        if (std::getenv("TS_TIMING"))
            std::fprintf(stderr, "%s: context %zu of %zu (device %d): %llu chunks, %llu records, %llu bases scanned, %llu bytes; fill %.0f ms, stage %.0f ms, "
                         "frame wait %.1f ms, carry + commit %.1f ms, index %.1f ms, join %.0f ms, scan %.0f ms\n", route, w, workers.size(), s.device,
                         (unsigned long long)s.chunks, (unsigned long long)s.records, (unsigned long long)s.basesScanned, (unsigned long long)s.bytesReceived,
                         s.msFill, s.msStage, s.msFrameWait, s.msCommit, s.msIndex, s.msJoin, s.msScan);
    }
}

// scanFastaToFilesDevice's stages (the unfiltered form), for a Teloscope of any number of contexts; the two ways a chunk's bytes
// come in are the read routes' (above): in place on one context, dealt by detail::ChunkRing on several.  Everything behind the
// fill exists once: ts_fasta_chunk_walk frames the records, the bytes behind the last complete one go in front of the next chunk,
// FastaChunkStage::judge joins and scans on the chunk's own context, FastaChunkStage::emit writes in chunk order.  A chunk that
// holds nothing but one unfinished record passes all of its contents on, and the next fill brings chunkBytes more, in place (up
// to chunkLimit) and dealt alike: the reader of dealt chunks runs ahead of the framing and cannot know that a chunk will grow, so
// growth by a fixed step is the one rule both can follow, and with it the chunks hold the same bytes, and BedWriter gets the
// same groups, for every number of contexts (ScanFastaTimes::groups and bases_read_back do not depend on it).  One exception:
// with a carry of more than chunkLimit - chunkBytes bytes the fill in place stops at chunkLimit, where a dealt chunk brings its
// chunkBytes regardless, so behind a record that comes that close to the limit the cuts, and with them `groups`, may differ; the
// files do not.  The price of the fixed step: a record of r chunks is walked r times (r <= chunkLimit / chunkBytes, 16 at the
// defaults), where growth by doubling walked it log r times.  Either way a
// record that is not complete within chunkLimit bytes of text is refused by name, with the same words.
class FastaChunkSteps {
public:
    struct Worker {
        size_t index = 0;
        ts_ctx *ctx = nullptr;
        ts_chunk *chunk = nullptr;
        ChunkFeed::Fill fill;                                   // a dealt chunk's new bytes
        std::vector<ts_fasta_record> recs = std::vector<ts_fasta_record>(4096);
        std::vector<char> names = std::vector<char>(size_t(1) << 16);
        std::vector<std::string> headers;
        uint64_t n = 0;                                         // complete records of the chunk
        size_t firstRecord = 0;                                 // the first one's index in the input: the report's `pos` column
        bool atEnd = false;
        FastaChunkStage::Judged judged;
        AssemblyRouteDeviceStats st;
        Worker() = default;
        Worker(const Worker &) = delete;
        Worker &operator=(const Worker &) = delete;
        ~Worker() { ts_bam_chunk_destroy(chunk); }
    };
    std::vector<std::unique_ptr<Worker>> workers;

    FastaChunkSteps(Teloscope &teloscope, ChunkFeed &feed, FastaChunkStage &stage, size_t chunkBytes, uint64_t chunkLimit)
        : feed_(feed), stage_(stage), chunkBytes_(chunkBytes), chunkLimit_(chunkLimit) {
        const uint64_t compCap = feed.compCap(chunkBytes);
        for (size_t w = 0; w < teloscope.deviceCount(); ++w) {
            workers.emplace_back(new Worker());
            Worker &k = *workers.back();
            k.index = w;
            k.ctx = teloscope.context(w);
            k.st.device = teloscope.deviceOrdinal(w);
            k.chunk = ts_bam_chunk_create(k.ctx, compCap, chunkBytes);
            if (!k.chunk) throw deviceError(k.ctx, "cannot make the device chunk");
        }
    }

    // The whole input as in-place chunks of context 0, on the caller's thread: any source of the feed, ChunkFeed::Gzip included
    void runInPlace() {
        Worker &k = *workers[0];
        uint64_t held = 0, pos = 0;                             // bytes in the chunk; the first one not consumed yet
        for (bool atEnd = false; !atEnd;) {
            const uint64_t carry = held - pos;
            // a chunk that held no whole record (a record larger than it) takes chunkBytes more, up to what a chunk may hold
            if (pos == 0 && carry >= chunkLimit_) throw doesNotFit(k, 0, held);
            const size_t want = static_cast<size_t>(std::min<uint64_t>(chunkBytes_, chunkLimit_ - carry));
            const Clock::time_point t0 = Clock::now();
            atEnd = feed_.fill(k.chunk, pos, want);
            k.st.msFill += since(t0);
            held = ts_bam_chunk_size(k.chunk); pos = 0;
            ++k.st.chunks; k.st.bytesReceived += held - carry;
            k.atEnd = atEnd;
            if (held == 0) continue;
            pos = walk(k);
            if (k.n == 0) continue;
            judge(0, 0);
            emit(0, 0);
        }
    }

    // the ring's steps: a dealt chunk
    void begin(size_t w) { ts_bind_thread_to_device(workers[w]->ctx); }
    RingTake take(size_t w, uint64_t) {
        Worker &k = *workers[w];
        feed_.take(chunkBytes_, k.fill);                        // (a Stream is read here: the reader's time, in nobody's figures)
        return k.fill.atEnd ? RingTake::Last : RingTake::More;
    }
    void stage(size_t w, uint64_t) {
        Worker &k = *workers[w];
        const Clock::time_point t0 = Clock::now();
        feed_.stage(k.ctx, k.chunk, k.fill);
        k.st.msStage += since(t0);
        ++k.st.chunks; k.st.bytesReceived += k.fill.n;
    }
    // the serial section: the unfinished record of the chunk before in front, the staged bytes behind it, the records framed
    bool frame(size_t w, uint64_t) {
        Worker &k = *workers[w];
        const uint64_t carry = prevSize_ - prevNext_;
        // (refused before the carry is copied, so that a copy of that size cannot fail first; the name is read where it lies)
        if (prev_ && carry >= chunkLimit_) throw doesNotFit(*prev_, prevNext_, carry);
        ringCommit(k, prev_, prevNext_);
        k.atEnd = k.fill.atEnd;
        k.n = 0;
        prev_ = &k; prevNext_ = 0; prevSize_ = ts_bam_chunk_size(k.chunk);
        if (prevSize_ == 0) return true;
        prevNext_ = walk(k);
        // (a chunk filled in place never holds chunkLimit bytes or more of one record: the same records are refused here)
        for (uint64_t i = 0; i < k.n; ++i)
            if (k.recs[i].text_len > chunkLimit_ || (k.recs[i].text_len == chunkLimit_ && !(k.atEnd && i + 1 == k.n)))
                throw doesNotFit(k, k.recs[i].off, k.recs[i].text_len);
        return true;
    }
    void judge(size_t w, uint64_t) {
        Worker &k = *workers[w];
        if (k.n == 0) return;
        const size_t n = static_cast<size_t>(k.n);
        k.headers.resize(n);
        stage_.judge(k.judged, w, k.chunk, k.recs.data(), n, k.atEnd, [&](size_t i) {
            k.headers[i] = fastaHeaderWord(k.names.data() + k.recs[i].name_at, k.names.data() + k.recs[i].name_at + k.recs[i].name_len);
            return &k.headers[i];
        }, k.firstRecord, nullptr);
        k.st.msJoin += k.judged.msJoin; k.st.msScan += k.judged.msScan;
        k.st.basesScanned += k.judged.libraryBases;
    }
    void emit(size_t w, uint64_t) {
        Worker &k = *workers[w];
        if (k.n) stage_.emit(k.judged);
    }

private:
    // The records of a chunk that has its bytes; the running record count moves on.  -> the first byte behind the last complete one
    uint64_t walk(Worker &k) {
        const Clock::time_point t0 = Clock::now();
        uint64_t next = 0;
        walkFastaChunk(k.ctx, k.chunk, k.atEnd, k.recs, k.names, k.n, next);
        const double ms = since(t0);
        k.st.msIndex += ms; stage_.msIndex += ms;
        k.firstRecord = recordsDone_;
        recordsDone_ += static_cast<size_t>(k.n);
        k.st.records += k.n;
        return next;
    }
    // the refusal of the record (or of the line in front of the first record) that begins at `off` of k's chunk, `len` bytes of it there
    std::runtime_error doesNotFit(const Worker &k, uint64_t off, uint64_t len) const {
        char head[257] = {0};
        const uint64_t hn = std::min<uint64_t>(len, 256);
        if (hn && ts_bam_chunk_read(k.chunk, off, hn, head) != TS_OK) return deviceError(k.ctx, "cannot read the chunk");
        const char *nl = static_cast<const char *>(std::memchr(head, '\n', static_cast<size_t>(hn)));
        const std::string name = head[0] == '>' ? fastaHeaderWord(head + 1, nl ? nl : head + hn) : std::string();
        return std::runtime_error(head[0] == '>' ? "FASTA record '" + name + "' does not fit a device chunk (" + std::to_string(chunkLimit_) + " bytes of text); use the host route"
                                                 : "a line of more than " + std::to_string(chunkLimit_) + " bytes in front of the first FASTA record does not fit a device chunk");
    }

    ChunkFeed &feed_;
    FastaChunkStage &stage_;
    size_t chunkBytes_;
    uint64_t chunkLimit_;
    // the framing's state: the chunk framed last, its size and where its unfinished record begins; the records framed so far
    const Worker *prev_ = nullptr;
    uint64_t prevNext_ = 0, prevSize_ = 0;
    size_t recordsDone_ = 0;
};

}  // namespace detail

// The device route of the assembly scan (same files, console report and AssemblySummary as scanFastaToFiles, which stays the
// default): the FASTA text exists in HBM one chunk of ~chunkBytes bytes at a time, and without -m the host reads none of it.
// The text gets there through detail::ChunkFeed (a plain file, BGZF members inflated on the device, or a stream through zlib
// or read(2)), and per chunk: lines indexed, records framed, names gathered (ts_fasta_chunk_walk); body lines joined into contiguous bases and
// the N-runs found (ts_fasta_chunk_join, ts_fasta_chunk_runs); PathComponents built from the runs, a few entries per record;
// every segment handed to the scan as a device segment through walkRecordViews, so that blocks, counts and windows come back
// exactly as for the host route; BedWriter fed.  With -m and without deviceTracks the joined bases are read back once per chunk
// (matchSeq needs them).
// The bytes behind the last complete record stay in the chunk for the next fill; a record larger than a chunk makes it grow.
// deviceTracks (off by default): the window tracks' lines — and with -m the two match files' — are formatted on the device too
// (ts_scan_segments_tracks, ts_scan_segments_text) and BedWriter writes them as they come; no base reaches the host then under
// any flag set; see below.
// Assembly record filters (selector given and active; otherwise nothing here changes): two phases.  Phase 1 feeds, walks and
// checks every chunk (ts_fasta_chunk_strict: which bodies hold a byte that is no line end) and KEEPS it resident, an unfinished
// record moving on device to device (ts_chunk_carry_over); tables and names stay on the host, a leading UTF-8 byte order mark
// is dropped, and no join, no scan and no output file exists yet.  Then the host applies FastaGroupReader::checkStrict's rules in
// its order, cuts the IDs as sequenceFilterId does, selects, and reports the selection on `log`.  Phase 2 joins, scans and
// writes the kept records chunk by chunk (seqPos = their input indices); an unselected record is never joined or scanned, and
// the summary's filter counts are this selection's.  The whole text must fit the device's free memory: one that does not (or
// exceeds residentLimit, a test hook like chunkLimit: 0 = no limit of its own) is refused before any output exists.
// Several contexts (a Teloscope made over a device list with DeviceRoutes::EveryContext — without it such an object is refused as
// before, "runs on one device"; the unfiltered form): detail::ChunkRing deals chunk k to context k mod N,
// a thread per context.  The new bytes are staged beside the chunk (ts_chunk_stage_upload, ts_chunk_stage_inflate) while the
// chunks before it are framed; in the serial section the unfinished record of chunk k - 1 moves in front (ts_chunk_carry_over,
// across contexts), the staged bytes are committed behind it and the records are framed, which gives the chunk its first record
// number; join, runs, the host view of the bases and the scan then run on the chunk's own context, any number of chunks at once,
// and BedWriter takes the chunks in order.  The stages are detail::FastaChunkSteps for every count: one context fills every
// chunk in place, on the caller's thread and with no staging region, exactly as before.  Files, console report, summary, the
// deterministic fields of ScanFastaTimes and the exceptions do not depend on the number of contexts
// (tests/test_gpu_assembly_routes_multi.py); plain gzip goes through zlib there, because the opt-in device gzip source
// (ChunkFeed::Gzip) is bound to one context.  perDevice, where given, receives one entry per context; TS_TIMING=1 prints a line
// per context beside the line of totals.
// Limits: the FILTERED form runs on ONE device (its two phases keep the whole text resident on it: a Teloscope over several
// throws, before any output file exists); a record
// whose text does not fit a chunk of chunkLimit bytes (4 GiB - 2, what the walk takes) is refused by name, never cut; on one
// context the stages run one after the other.  chunkLimit is a test hook (the refusal cannot be reached otherwise without 4 GiB of text):
// callers leave it alone.  What a maintainer of the reference would call in place of its FASTA load and per-path jobs
// (src/input.cpp:655-733).
inline AssemblySummary scanFastaToFilesDevice(Teloscope &teloscope, const std::string &fastaFile, const std::string &outBase,
                                              std::ostream &console, bool manualCuration = false,
                                              size_t chunkBytesArg = size_t(256) << 20, ScanFastaTimes *times = nullptr,
                                              uint64_t chunkLimit = 0xfffffffeull, bool deviceTracks = false,
                                              const SequenceSelector *selector = nullptr, std::ostream &log = std::cerr,
                                              uint64_t residentLimit = 0, std::vector<AssemblyRouteDeviceStats> *perDevice = nullptr) {
    const bool dealt = teloscope.deviceCount() > 1;
    if (dealt && !teloscope.deviceRoutesUseEveryContext())
        throw std::runtime_error("scanFastaToFilesDevice runs on one device: this Teloscope was made over " + std::to_string(teloscope.deviceCount()) +
                                 " (the joined bases lie in one device's memory); one made with DeviceRoutes::EveryContext has the route "
                                 "deal its chunks to all of them");
    if (selector && selector->active()) {
        if (dealt)
            throw std::runtime_error("scanFastaToFilesDevice with assembly record filters runs on one device: this Teloscope was made over " +
                                     std::to_string(teloscope.deviceCount()) + " (the filtered device route keeps the whole text in one device's memory "
                                     "until the selection is known; without a selector the route uses every context)");
        if (perDevice) perDevice->clear();
        return detail::scanFastaToFilesDeviceFiltered(teloscope, fastaFile, outBase, console, manualCuration, chunkBytesArg, times, chunkLimit,
                                                      deviceTracks, *selector, log, residentLimit);
    }
    detail::FastaChunkStage stage(teloscope, deviceTracks);
    detail::ChunkFeed::Options options;
    options.cannotOpen = "cannot open " + fastaFile;
    options.cannotRead = "read error in " + fastaFile;
    options.uploadFailed = "upload of the FASTA text failed";
    if (dealt) options.gzipDevice = false;                      // (bound to one context: plain gzip is read through zlib)
    detail::ChunkFeed feed(teloscope.context(0), fastaFile, options);
    const size_t chunkBytes = detail::clampFastaChunk(feed, chunkBytesArg, chunkLimit);
    detail::FastaChunkSteps steps(teloscope, feed, stage, chunkBytes, chunkLimit);

    stage.open(outBase, console, manualCuration);
    std::unique_ptr<detail::ChunkRing<detail::FastaChunkSteps>> ring;
    if (dealt) {
        ring.reset(new detail::ChunkRing<detail::FastaChunkSteps>(teloscope.deviceCount(), 0, steps));
        ring->run();
    } else {
        steps.runInPlace();
    }
    for (const auto &k : steps.workers) stage.msUpload += k->st.msFill + k->st.msStage + k->st.msCommit;
    const UserInputTeloscope &ui = teloscope.input();
    const AssemblySummary sum = stage.finish(ui.sequenceFilterActive, ui.filterInputCount, ui.filterSelectedCount, false, feed, times);
    detail::assemblyRouteFigures("scanFastaToFilesDevice", steps.workers, ring.get(), perDevice);
    return sum;
}

namespace detail {

// fastaSubsetDevice's stages: TextChunkSteps with the assembly route's framing (ts_fasta_chunk_walk) and the read routes' judge.
// The first chunk must begin with '>'; the chunk's last record is unfinished unless the input ends with it, and goes in front of
// the next chunk.  There is no record that is not valid.  The stage reads a '\r' at the chunk's end by the walk's at_end, so a
// worker remembers it.
struct FastaReadWorker : RecordWorker<ts_fasta_record> {
    ChunkFeed::Fill fill;                                       // a dealt chunk's new bytes
    std::vector<char> names;                                    // the walk's header lines: the call's room for them, not read here
    bool atEnd = false;
};
class FastaReadChunkSteps : public TextChunkSteps<FastaReadChunkSteps, FastaReadWorker> {
public:
    using Worker = FastaReadWorker;
    FastaSubsetStats result;

    FastaReadChunkSteps(ReadTelomereFilter &filter, ChunkFeed &feed, std::ostream &out, size_t readsPerBatch, size_t chunkBytes, std::ostream *blocks = nullptr)
        : TextChunkSteps(filter, feed, out, readsPerBatch, chunkBytes, blocks, "failed while writing FASTA subset") {}

    // the chunk's turn to write: what it kept (nothing, where it came in place) and its totals
    void emit(size_t w, uint64_t) {
        Worker &k = *workers[w];
        emitKept(k);
        result.blockLines += k.blockLines;
        result.totalRecords += k.n; result.passedRecords += k.passed; result.missingSequenceRecords += k.n - k.withBases;
    }

    // the format's part of the shared steps
    static uint64_t bases(const ts_fasta_record &r) { return r.n_bases; }          // (none: never kept)
    static constexpr const char *stageFailed = "staging the sequences failed";
    int stageReads(Worker &k, ts_batch *batch) { return ts_fasta_chunk_stage(k.chunk, k.withSeq.data(), k.withSeq.size(), k.atEnd ? 1 : 0, batch, nullptr); }
    int gatherKept(Worker &k, void *dPass, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *nPassed) {
        return ts_fasta_chunk_gather(k.chunk, k.withSeq.data(), k.withSeq.size(), dPass, dst, cap, bytes, nPassed, nullptr);
    }
    int blockLines(Worker &k, ts_batch *batch, unsigned char *dst, uint64_t cap, uint64_t *bytes, uint64_t *lines) {
        return ts_fasta_chunk_block_lines(k.chunk, k.withSeq.data(), k.withSeq.size(), batch, dst, cap, bytes, lines, nullptr);
    }
    bool frameChunk(Worker &k, bool atEnd) {
        k.n = 0; k.atEnd = atEnd;
        const uint64_t size = ts_bam_chunk_size(k.chunk);
        if (first_) {
            if (size == 0) {
                if (atEnd) throw std::runtime_error("FASTA input is empty");
                return true;
            }
            unsigned char c = 0;
            if (ts_bam_chunk_read(k.chunk, 0, 1, &c) != TS_OK) throw deviceError(k.ctx, "cannot read the chunk");
            if (c != '>') throw std::runtime_error("FASTA input must start with '>'");
            first_ = false;
        }
        // (ts_fasta_record counts a record's text and bases in 32 bits, and the walk takes a chunk below 4 GiB: a chunk reaches
        // that size only by growing around one record)
        if (size >= 0xffffffffull)
            throw std::runtime_error("fastaSubsetDevice: a record of 4 GiB or more of FASTA text does not fit the device route; the host route (fastaSubset) takes it");
        const Clock::time_point t0 = Clock::now();
        if (k.names.empty()) k.names.resize(static_cast<size_t>(size / 16 + 64));  // (reads: names are a few percent of the text; the walk says when it needs more)
        walkFastaChunk(k.ctx, k.chunk, atEnd, k.recs, k.names, k.n, prevNext_);
        k.st.msWalk += since(t0);
        return true;
    }
};
}  // namespace detail
// The device route of the FASTA read subset (same arguments, result, exceptions and output bytes as fastaSubset): the FASTA text
// exists in HBM one chunk of ~chunkBytes bytes at a time and the host reads none of it but its first byte.  The text gets there
// through detail::ChunkFeed as for fastqSubsetDevice (a plain file, BGZF members inflated on the device, a stream through zlib or
// read(2), plain gzip on the device under TS_GZIP_DEVICE=1; `-` is stdin); behind the source the records are framed as the
// assembly route frames them (ts_fasta_chunk_walk: the table comes back), their body lines joined straight into a tips-only
// batch's input buffer (ts_fasta_chunk_stage), judged, and the passing records gathered as they were read (detail::ReadJudge with
// ts_fasta_chunk_gather).  A record larger than a chunk makes the chunk grow; one of 4 GiB or more is refused by naming the host
// route.  A filter of one context takes every chunk in place; on several the ring deals the chunks to all of them.  perDevice,
// where given, receives one entry per context.
inline FastaSubsetStats fastaSubsetDevice(const std::string &inFile, std::ostream &out, ReadTelomereFilter &filter,
                                          size_t readsPerBatch = 1u << 20, size_t chunkBytes = 256u << 20, std::ostream *blocks = nullptr,
                                          std::vector<ReadRouteDeviceStats> *perDevice = nullptr) {
    return detail::textSubsetDeviceRun<detail::FastaReadChunkSteps>("FASTA", "fastaSubsetDevice", inFile, out, filter, readsPerBatch,
                                                                    std::min<size_t>(chunkBytes, size_t(1) << 31), perDevice, blocks);
}

}  // namespace teloscope_mi355x

#endif
