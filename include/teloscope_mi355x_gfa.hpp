// teloscope_mi355x_gfa.hpp — the reference's fourth input mode: a GFA assembly graph annotated with telomere caps for
// BandageNG (README "Annotate a graph for BandageNG"; src/input.cpp:625-716, walkSegment / walkSegmentForPath :835-939).
//
//   GfaGraph g = readGfa("asm.gfa");                           // plain or gzip; .gfa, .gfa.gz, .gfa2, .gfa2.gz
//   std::vector<GfaEnd> jobs = gfaTerminalJobs(g);             // the terminal ends the reference queues a job for
//   GfaEnds e = gfaScanEnds(teloscope, g, jobs);               // ONE Teloscope::terminalEnds call, each segment once
//   writeAnnotatedGfa(g, jobs, e.ends, "out/asm.gfa.telo.annotated.gfa", "out/asm.gfa.telo.annotated.colors.csv");
//
// or annotateGfa(teloscope, file, outDir) for all four.  The device reduces a segment to {longest terminal block at its start
// side, at its end side} (ts_terminal_ends): 8 bytes per segment, whatever the number of blocks.
//
// annotateGfaDevice(teloscope, file, outDir) is the device route of the same (not the default; on every context of a
// Teloscope made with DeviceRoutes::EveryContext): the text lies in device memory,
// lines and tabs are indexed there (ts_gfa_chunk_walk) and the segments are scanned where they lie; see its comment below.
//
// Input lines are written back verbatim (line ends as read) with two exceptions: the header says VN:Z:1.2 (added when the input
// has none, replacing a VN:Z:2.0), and a GFA 2 segment `S name len seq [tags]` loses its length field.  Other GFA 2 records are
// refused.  GFA 1.1 W lines are copied through and are not read as paths.
//
// Assembly record filters (include/teloscope_mi355x_filter.hpp) select paths, or the segments of a pathless graph:
//
//   validateFilteredGfa(file);                                  // GFA 1 with P paths or none; throws SequenceFilterError
//   GfaGraph g = readGfa(file);
//   SequenceSelection sel = selectGfa(g, selector);             // candidates: path names, or segment names without paths
//   ... Teloscope t(ui); annotateGfa(t, g, &sel, outDir);       // ends of selected paths / selected segments only
//
// or annotateGfa(teloscope, file, outDir, selector) for all of it (annotateGfaDevice(teloscope, file, outDir, selector) on the
// device route: the same checks over the text in device memory).  Every input line, unselected P lines included, is written back.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "teloscope_mi355x_filter.hpp"
#include "teloscope_mi355x_io.hpp"

namespace teloscope_mi355x {

struct GfaSegment {
    std::string name;
    const char *seq = nullptr;        // the sequence field where it lies in GfaGraph::data (nullptr: '*')
    uint64_t len = 0;
};

struct GfaPath {                      // a P line: its components as written (name, orientation)
    std::string name;
    std::vector<std::pair<std::string, char>> comps;
};

struct GfaEdit { size_t off, len; std::string text; };   // input bytes [off, off + len) written as `text`

struct GfaGraph {
    std::string file, baseName;       // baseName: the output files' stem (userInput.inSequenceName)
    std::string data;                 // the whole input, decompressed
    int version = 1;                  // 2 when the header says VN:Z:2.x
    bool hasVersion = false;          // some H line carries VN:Z
    std::vector<GfaSegment> segments; // S records in input order
    std::unordered_map<std::string, uint32_t> index;
    std::vector<GfaPath> paths;
    std::vector<GfaEdit> edits;       // ascending offsets, disjoint
};

// One terminal end the reference queues a scan job for (src/input.cpp:637-674)
struct GfaEnd {
    uint32_t seg;
    char orient;                      // path orientation ('+' for a pathless graph)
    bool isFirst;                     // path mode: the path's first (true) or last segment
    bool pathAware;                   // walkSegmentForPath (true) or walkSegment
};

struct GfaEnds {
    std::vector<std::pair<uint32_t, uint32_t>> ends;    // per graph segment: {start side, end side}, 0 = none / not scanned
    size_t scanned = 0, noSeq = 0;                       // distinct segments scanned; ends whose segment has no sequence
};

struct GfaAnnotateStats {
    size_t segments = 0, ends = 0, scanned = 0, noSeq = 0, nodes = 0;
    double parseMs = 0, scanMs = 0, writeMs = 0;
};

namespace detail {

inline std::string gfaReadAll(const std::string &file) {
    gzFile in = gzopen(file.c_str(), "rb");                     // (zlib reads plain files through the same calls)
    if (!in) throw std::runtime_error("Could not open assembly input '" + file + "'.");
    gzbuffer(in, 1u << 20);
    std::string data;
    size_t used = 0;
    for (;;) {
        if (data.size() - used < (size_t(16) << 20)) data.resize(std::max<size_t>(data.size() * 2, size_t(32) << 20));
        const int n = gzread(in, &data[used], static_cast<unsigned>(std::min<size_t>(data.size() - used, size_t(1) << 30)));
        if (n < 0) { gzclose(in); throw std::runtime_error("Could not read assembly input '" + file + "'."); }
        if (n == 0) break;
        used += static_cast<size_t>(n);
    }
    gzclose(in);
    data.resize(used);
    return data;
}

struct GfaField { size_t off, len; };

// the tab-separated fields of the line [b, e) ('\r' before the line feed already cut), offsets relative to `base`
inline void gfaFields(const char *base, const char *b, const char *e, std::vector<GfaField> &f, size_t maxFields) {
    f.clear();
    const char *p = b;
    while (f.size() + 1 < maxFields) {
        const char *t = static_cast<const char *>(std::memchr(p, '\t', static_cast<size_t>(e - p)));
        if (!t) break;
        f.push_back({static_cast<size_t>(p - base), static_cast<size_t>(t - p)});
        p = t + 1;
    }
    f.push_back({static_cast<size_t>(p - base), static_cast<size_t>(e - p)});
}

// a P line's name and components from its fields (three or four of them)
inline GfaPath gfaCutPath(const char *base, const std::vector<GfaField> &f) {
    GfaPath p;
    p.name.assign(base + f[1].off, f[1].len);
    const char *c = base + f[2].off, *ce = c + f[2].len;
    while (c < ce) {
        const char *d = c;
        while (d < ce && *d != ',' && *d != ';') ++d;
        if (d - c >= 2) p.comps.emplace_back(std::string(c, static_cast<size_t>(d - c - 1)), d[-1]);
        c = d + 1;
    }
    return p;
}

// what a chunk of lines holds (parsed side by side, joined in input order)
struct GfaChunk {
    struct S { size_t line, lineEnd, f1, f1len, f2, f2len, f3, f3len; bool has3; };   // offsets into data
    std::vector<S> segs;
    std::vector<GfaPath> paths;
    std::vector<std::pair<size_t, size_t>> headers;   // H lines carrying VN:Z: line start, content end
    std::vector<std::string> versions;
    std::string foreign;                                // first record type other than H / S / '#' (for a GFA 2 input)
};

}  // namespace detail

// Reads a GFA 1.x or 2.0 graph (plain or gzip).  Throws on an unreadable file, a GFA 2 record other than H / S, or a
// segment named twice.
inline GfaGraph readGfa(const std::string &file) {
    GfaGraph g;
    g.file = file;
    const size_t slash = file.find_last_of('/');
    g.baseName = slash == std::string::npos ? file : file.substr(slash + 1);
    g.data = detail::gfaReadAll(file);
    const char *const base = g.data.data();
    const size_t n = g.data.size();
    // chunks of ~16 MB cut at line starts, parsed on the host threads
    std::vector<size_t> cuts{0};
    for (size_t at = size_t(16) << 20; at < n;) {
        const char *nl = static_cast<const char *>(std::memchr(base + at, '\n', n - at));
        if (!nl) break;
        const size_t c = static_cast<size_t>(nl - base) + 1;
        if (c >= n) break;
        cuts.push_back(c);
        at = c + (size_t(16) << 20);
    }
    cuts.push_back(n);
    std::vector<detail::GfaChunk> chunks(cuts.size() - 1);
    detail::onThreads(chunks.size(), [&](size_t ci) {
        detail::GfaChunk &ch = chunks[ci];
        std::vector<detail::GfaField> f;
        for (size_t ls = cuts[ci]; ls < cuts[ci + 1];) {
            const char *nl = static_cast<const char *>(std::memchr(base + ls, '\n', cuts[ci + 1] - ls));
            const size_t next = nl ? static_cast<size_t>(nl - base) + 1 : cuts[ci + 1];
            size_t le = nl ? static_cast<size_t>(nl - base) : cuts[ci + 1];
            if (le > ls && base[le - 1] == '\r') --le;
            const char *b = base + ls, *e = base + le;
            if (e > b) {
                const char type = *b;
                const bool single = e - b == 1 || b[1] == '\t';
                if (type == 'S' && single) {
                    detail::gfaFields(base, b, e, f, 5);
                    if (f.size() >= 3)
                        ch.segs.push_back({ls, le, f[1].off, f[1].len, f[2].off, f[2].len, f.size() >= 4 ? f[3].off : 0,
                                           f.size() >= 4 ? f[3].len : 0, f.size() >= 4});
                } else if (type == 'P' && single) {
                    detail::gfaFields(base, b, e, f, 4);
                    if (f.size() >= 3) ch.paths.push_back(detail::gfaCutPath(base, f));
                } else if (type == 'H' && single) {
                    detail::gfaFields(base, b, e, f, size_t(-1));
                    for (size_t i = 1; i < f.size(); ++i)
                        if (f[i].len >= 5 && std::memcmp(base + f[i].off, "VN:Z:", 5) == 0) {
                            ch.headers.emplace_back(ls, le);
                            ch.versions.emplace_back(base + f[i].off + 5, f[i].len - 5);
                        }
                }
                if (ch.foreign.empty() && !(single && (type == 'H' || type == 'S')) && type != '#') {
                    const char *t = static_cast<const char *>(std::memchr(b, '\t', static_cast<size_t>(e - b)));
                    ch.foreign.assign(b, t ? t : e);
                }
            }
            ls = next;
        }
    });
    for (const detail::GfaChunk &ch : chunks)
        for (const std::string &v : ch.versions) { g.hasVersion = true; g.version = (!v.empty() && v[0] == '2') ? 2 : 1; }
    size_t nseg = 0;
    for (const detail::GfaChunk &ch : chunks) nseg += ch.segs.size();
    g.segments.reserve(nseg);
    g.index.reserve(nseg);
    for (detail::GfaChunk &ch : chunks) {
        if (g.version == 2 && !ch.foreign.empty())
            throw std::runtime_error("GFA 2 record type '" + ch.foreign + "' in '" + file +
                                     "' is not supported: only H and S records of a GFA 2 graph are read.");
        for (const auto &h : ch.headers) {
            const std::string line(base + h.first, h.second - h.first);
            if (line.find("VN:Z:2") != std::string::npos) g.edits.push_back({h.first, h.second - h.first, "H\tVN:Z:1.2"});
        }
        for (const detail::GfaChunk::S &s : ch.segs) {
            GfaSegment seg;
            seg.name.assign(base + s.f1, s.f1len);
            size_t so = s.f2, sl = s.f2len;
            if (g.version == 2 && s.has3) {                          // S name len seq [tags]: the length goes
                so = s.f3; sl = s.f3len;
                g.edits.push_back({s.f2, s.f3 - s.f2, std::string()});
            }
            if (!(sl == 1 && base[so] == '*')) { seg.seq = base + so; seg.len = sl; }
            if (!g.index.emplace(seg.name, static_cast<uint32_t>(g.segments.size())).second)
                throw std::runtime_error("segment '" + seg.name + "' is defined twice in '" + file + "'.");
            g.segments.push_back(std::move(seg));
        }
        for (GfaPath &p : ch.paths) g.paths.push_back(std::move(p));
    }
    std::sort(g.edits.begin(), g.edits.end(), [](const GfaEdit &a, const GfaEdit &b) { return a.off < b.off; });
    return g;
}

// The ends the reference scans (src/input.cpp:637-674).  With P lines: per path, the first and the last component that
// names an S record with orientation '+' / '-', as unique (segment, orientation, isFirst) ends in that order.  Without:
// every segment, '+'.  keep (a selection, selectGfa): per path — or per segment of a pathless graph — whether it takes part.
inline std::vector<GfaEnd> gfaTerminalJobs(const GfaGraph &g, const std::vector<char> *keep = nullptr) {
    std::vector<GfaEnd> jobs;
    if (!g.paths.empty()) {
        std::set<std::tuple<uint32_t, char, bool>> ends;
        for (size_t pi = 0; pi < g.paths.size(); ++pi) {
            if (keep && !(*keep)[pi]) continue;
            const GfaPath &p = g.paths[pi];
            std::vector<std::pair<uint32_t, char>> comps;
            for (const auto &c : p.comps) {
                if (c.second != '+' && c.second != '-') continue;
                const auto it = g.index.find(c.first);
                if (it != g.index.end()) comps.emplace_back(it->second, c.second);
            }
            if (comps.empty()) continue;
            ends.emplace(comps.front().first, comps.front().second, true);
            ends.emplace(comps.back().first, comps.back().second, false);
        }
        for (const auto &e : ends) jobs.push_back({std::get<0>(e), std::get<1>(e), std::get<2>(e), true});
    } else {
        jobs.reserve(g.segments.size());
        for (uint32_t i = 0; i < g.segments.size(); ++i)
            if (!keep || (*keep)[i]) jobs.push_back({i, '+', false, false});
    }
    return jobs;
}

// The distinct segments with a sequence that the ends use, in one Teloscope::terminalEnds call (each segment once, scanned
// where it lies in the input buffer; the library folds case as unmaskSequence does).  Warns on `log` about ends whose
// segment has no sequence, in the reference's words.
// onDevice: every GfaSegment::seq is an address in device memory (annotateGfaDevice), scanned from there: the first context's, or
// — segContext given, one entry per graph segment — that of context segContext[i] of the Teloscope.  The wanted segments are then
// grouped by their context and ONE terminalEnds call per context that owns any runs, a thread per context, each on its own
// device and bound to the CPUs of its NUMA node (ts_bind_thread_to_device), as the ring's threads are; the results go back in
// segment order.  scannedBases and scanMs, where given, receive per context the bases it scanned and the milliseconds its own
// call took (0 for a context that owns none of the wanted segments).
inline GfaEnds gfaScanEnds(Teloscope &teloscope, const GfaGraph &g, const std::vector<GfaEnd> &jobs, std::ostream &log = std::cerr,
                           bool onDevice = false, const std::vector<uint32_t> *segContext = nullptr,
                           std::vector<uint64_t> *scannedBases = nullptr, std::vector<double> *scanMs = nullptr) {
    GfaEnds r;
    r.ends.assign(g.segments.size(), {0u, 0u});
    std::vector<char> want(g.segments.size(), 0);
    for (const GfaEnd &j : jobs) {
        if (!g.segments[j.seg].seq) ++r.noSeq;
        else want[j.seg] = 1;
    }
    if (r.noSeq)
        log << "Warning: " << r.noSeq << " of " << jobs.size()
            << " GFA segment(s) had no sequence (*); skipped for telomere annotation.\n";
    const size_t nctx = onDevice && segContext ? teloscope.deviceCount() : 1;
    std::vector<std::vector<uint32_t>> which(nctx);
    std::vector<std::vector<Teloscope::Segment>> segs(nctx);
    if (scannedBases) scannedBases->assign(nctx, 0);
    if (scanMs) scanMs->assign(nctx, 0.0);
    for (uint32_t i = 0; i < g.segments.size(); ++i)
        if (want[i]) {
            const size_t c = nctx > 1 ? (*segContext)[i] : 0;
            which[c].push_back(i);
            segs[c].emplace_back(onDevice ? nullptr : g.segments[i].seq, g.segments[i].len, 0, true);
            if (onDevice) segs[c].back().device = g.segments[i].seq;
            if (scannedBases) (*scannedBases)[c] += g.segments[i].len;
            ++r.scanned;
        }
    if (!r.scanned) return r;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> e(nctx);
    std::vector<std::exception_ptr> errors(nctx);
    auto scan = [&](size_t c, bool ownThread) {
        const auto t0 = std::chrono::steady_clock::now();
        try {
            if (ownThread) ts_bind_thread_to_device(teloscope.context(c));
            e[c] = teloscope.terminalEnds(segs[c], c);
        } catch (...) { errors[c] = std::current_exception(); }
        if (scanMs) (*scanMs)[c] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    size_t busy = 0, only = 0;
    for (size_t c = 0; c < nctx; ++c) if (!segs[c].empty()) { ++busy; only = c; }
    if (busy == 1) scan(only, false);
    else {
        std::vector<std::thread> threads;
        for (size_t c = 0; c < nctx; ++c) if (!segs[c].empty()) threads.emplace_back(scan, c, true);
        for (std::thread &t : threads) t.join();
    }
    for (size_t c = 0; c < nctx; ++c) if (errors[c]) std::rethrow_exception(errors[c]);
    for (size_t c = 0; c < nctx; ++c)
        for (size_t k = 0; k < which[c].size(); ++k) r.ends[which[c][k]] = e[c][k];
    return r;
}

// The input's bytes as the writer sees them: total of them, the last one, and a function that writes bytes [off, off + len) to
// the output.  writeAnnotatedGfa reads GfaGraph::data; annotateGfaDevice hands over the pieces the text arrived in.
struct GfaInputBytes {
    size_t size = 0;
    char last = 0;                                          // (size > 0)
    std::function<void(std::ostream &, size_t off, size_t len)> write;
};

// Writes the annotated graph and its colours file; returns the number of telomere nodes.  ends: per graph segment (GfaEnds).
// Node rules of walkSegment / walkSegmentForPath (src/input.cpp:835-939): a path end keeps the block on the physical side
// isFirst == (orient == '+'), edge orientation orient at a start, its flip at an end; a pathless segment gets a node per side
// that has a block, '+' in the name, edge '+' at the start and '-' at the end.  input: where the input's bytes come from (the form
// without it reads g.data).
inline size_t writeAnnotatedGfa(const GfaGraph &g, const GfaInputBytes &input, const std::vector<GfaEnd> &jobs,
                                const std::vector<std::pair<uint32_t, uint32_t>> &ends,
                                const std::string &outGfa, const std::string &outColors) {
    struct Node { std::string name; uint32_t seg, len; char edge; };
    std::vector<Node> nodes;
    for (const GfaEnd &j : jobs) {
        const std::string &seg = g.segments[j.seg].name;
        const auto &e = ends[j.seg];
        if (j.pathAware) {
            const bool atStart = j.isFirst == (j.orient == '+');
            const uint32_t len = atStart ? e.first : e.second;
            if (!len) continue;
            const char edge = j.isFirst ? j.orient : (j.orient == '+' ? '-' : '+');
            nodes.push_back({"telomere_" + seg + j.orient + (j.isFirst ? "_start" : "_end"), j.seg, len, edge});
        } else {
            if (e.first) nodes.push_back({"telomere_" + seg + "+_start", j.seg, e.first, '+'});
            if (e.second) nodes.push_back({"telomere_" + seg + "+_end", j.seg, e.second, '-'});
        }
    }
    std::ofstream out(outGfa, std::ios::binary);
    if (!out) throw std::runtime_error("could not write " + outGfa);
    if (!g.hasVersion) out << "H\tVN:Z:1.2\n";
    size_t at = 0;
    for (const GfaEdit &ed : g.edits) {
        input.write(out, at, ed.off - at);
        out << ed.text;
        at = ed.off + ed.len;
    }
    input.write(out, at, input.size - at);
    if (input.size && input.last != '\n') out << '\n';
    std::string tail;
    for (const Node &nd : nodes) {
        tail += "S\t" + nd.name + "\t*\tLN:i:6\tRC:i:6000\tTL:i:" + std::to_string(nd.len) + "\n";
        tail += "L\t" + nd.name + "\t+\t" + g.segments[nd.seg].name + "\t" + nd.edge + "\t0M\tRC:i:0\n";
    }
    out << tail;
    out.close();
    if (!out) throw std::runtime_error("could not write " + outGfa);
    std::ofstream colors(outColors, std::ios::binary);
    if (!colors) throw std::runtime_error("could not write " + outColors);
    colors << "node\tcolor\n";
    for (const Node &nd : nodes) colors << nd.name << "\t#008000\n";
    colors.close();
    if (!colors) throw std::runtime_error("could not write " + outColors);
    return nodes.size();
}

inline size_t writeAnnotatedGfa(const GfaGraph &g, const std::vector<GfaEnd> &jobs,
                                const std::vector<std::pair<uint32_t, uint32_t>> &ends,
                                const std::string &outGfa, const std::string &outColors) {
    GfaInputBytes input;
    input.size = g.data.size();
    input.last = g.data.empty() ? 0 : g.data.back();
    input.write = [&g](std::ostream &o, size_t off, size_t len) { o.write(g.data.data() + off, static_cast<std::streamsize>(len)); };
    return writeAnnotatedGfa(g, input, jobs, ends, outGfa, outColors);
}

namespace detail {

// One line of a filtered GFA, its '\r' bytes gone, by the filtered loader's rules (src/input.cpp:206-283): 0, or the first rule
// it breaks, numbered as ts_gfa_chunk_check numbers them (include/teloscan.h)
inline int filteredGfaLineCode(const std::string &line) {
    if (line.empty() || line[0] == '#') return 0;
    if (line.compare(0, 2, "H\t") == 0 && line.find("\tVN:Z:2") != std::string::npos) return 1;
    if (line.size() < 2 || line[1] != '\t') return 2;
    const char type = line[0];
    if (std::strchr("OUEGF", type)) return 3;
    if (type == 'W') return 4;
    if (type == 'C') return 5;
    if (type == 'S') {                                             // S name LEN seq: a GFA 2 segment
        const size_t t2 = line.find('\t', 2), t3 = t2 == std::string::npos ? t2 : line.find('\t', t2 + 1);
        if (t3 != std::string::npos && t3 > t2 + 1 &&
            std::all_of(line.begin() + static_cast<long>(t2) + 1, line.begin() + static_cast<long>(t3),
                        [](char c) { return c >= '0' && c <= '9'; }))
            return 6;
    }
    if (!std::strchr("HSLJP", type)) return 7;
    return 0;
}

// the loader's words for a broken rule (code 1..7) of a line of the given type at line lineNo (from 1)
inline SequenceFilterError filteredGfaError(int code, char type, uint64_t lineNo) {
    const std::string gfa2 = "; use GFA1 P paths or a pathless GFA1 graph.", at = " at line " + std::to_string(lineNo);
    switch (code) {
    case 1: return SequenceFilterError("Assembly record filters do not support GFA2" + at + gfa2);
    case 2: return SequenceFilterError("Assembly record filters found a malformed or unsupported GFA record" + at + ".");
    case 3: return SequenceFilterError(std::string("Assembly record filters do not support GFA2 record type '") + type + "'" + at + gfa2);
    case 4: return SequenceFilterError("Assembly record filters do not support GFA1 W walks" + at + gfa2);
    case 5: return SequenceFilterError("Assembly record filters do not support GFA1 C containment records" + at + ".");
    case 6: return SequenceFilterError("Assembly record filters do not support GFA2 segment records" + at + gfa2);
    default: return SequenceFilterError(std::string("Assembly record filters do not support GFA record type '") + type + "'" + at + ".");
    }
}

// GFA 2 by name: refused before the file is opened
inline void refuseGfa2Name(const std::string &file) {
    if (caseInsensitiveSuffix(file, ".gfa2") || caseInsensitiveSuffix(file, ".gfa2.gz"))
        throw SequenceFilterError("Assembly record filters do not support GFA2; use GFA1 P paths or a pathless GFA1 graph.");
}

}  // namespace detail

// With assembly record filters the input must be a GFA 1 graph with P paths or none (src/input.cpp:206-283): throws a
// SequenceFilterError naming the first line that is not, before the graph is read.  Blank and '#' lines are skipped.
inline void validateFilteredGfa(const std::string &file) {
    detail::refuseGfa2Name(file);
    std::string data;
    try {
        data = detail::gfaReadAll(file);
    } catch (const std::exception &e) {
        throw SequenceFilterError(e.what());
    }
    uint64_t lineNo = 0;
    for (size_t ls = 0; ls < data.size();) {
        const size_t nl = data.find('\n', ls);
        std::string line = data.substr(ls, (nl == std::string::npos ? data.size() : nl) - ls);
        ls = nl == std::string::npos ? data.size() : nl + 1;
        ++lineNo;
        line.erase(std::remove(line.begin(), line.end(), '\r'), line.end());
        const int code = detail::filteredGfaLineCode(line);
        if (code) throw detail::filteredGfaError(code, line[0], lineNo);
    }
}

// The selection of a graph (src/input.cpp:596-623): its P lines' names, or — a pathless graph — its segments' names, each up
// to its first whitespace.  sel.keep is indexed like g.paths, or like g.segments.
inline SequenceSelection selectGfa(const GfaGraph &g, const SequenceSelector &selector) {
    std::vector<std::string> names;
    if (!g.paths.empty())
        for (const GfaPath &p : g.paths) names.push_back(sequenceFilterId(p.name));
    else
        for (const GfaSegment &sg : g.segments) names.push_back(sequenceFilterId(sg.name));
    return selector.select(names, g.paths.empty() ? "segments" : "paths");
}

// teloscope asm.gfa -o outDir on a graph already read: outDir/<name>.telo.annotated.gfa and .colors.csv.  selection: selectGfa's
// (nullptr: every path / segment)
inline GfaAnnotateStats annotateGfa(Teloscope &teloscope, const GfaGraph &g, const SequenceSelection *selection,
                                    const std::string &outDir, std::ostream &log = std::cerr) {
    using Clock = std::chrono::steady_clock;
    auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    GfaAnnotateStats st;
    const auto t1 = Clock::now();
    const std::vector<GfaEnd> jobs = gfaTerminalJobs(g, selection ? &selection->keep : nullptr);
    const GfaEnds e = gfaScanEnds(teloscope, g, jobs, log);
    const auto t2 = Clock::now();
    const std::string stem = outDir + "/" + g.baseName + ".telo.annotated";
    st.nodes = writeAnnotatedGfa(g, jobs, e.ends, stem + ".gfa", stem + ".colors.csv");
    const auto t3 = Clock::now();
    st.segments = g.segments.size();
    st.ends = jobs.size();
    st.scanned = e.scanned;
    st.noSeq = e.noSeq;
    st.scanMs = ms(t1, t2);
    st.writeMs = ms(t2, t3);
    return st;
}

// teloscope asm.gfa -o outDir: outDir/<name>.telo.annotated.gfa and outDir/<name>.telo.annotated.colors.csv
inline GfaAnnotateStats annotateGfa(Teloscope &teloscope, const std::string &file, const std::string &outDir,
                                    std::ostream &log = std::cerr) {
    const auto t0 = std::chrono::steady_clock::now();
    const GfaGraph g = readGfa(file);
    const double parseMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    GfaAnnotateStats st = annotateGfa(teloscope, g, nullptr, outDir, log);
    st.parseMs += parseMs;
    return st;
}

// the same with assembly record filters: validateFilteredGfa (when the selector is active), readGfa, selectGfa — whose line
// goes to `log` — and the annotation of the selected paths / segments.  (A caller that must not touch the device before the
// selection is known runs these steps itself, as the overview above shows.)
inline GfaAnnotateStats annotateGfa(Teloscope &teloscope, const std::string &file, const std::string &outDir,
                                    const SequenceSelector &selector, std::ostream &log = std::cerr) {
    const auto t0 = std::chrono::steady_clock::now();
    if (selector.active()) validateFilteredGfa(file);
    const GfaGraph g = readGfa(file);
    const SequenceSelection sel = selectGfa(g, selector);
    if (selector.active()) log << selectionMessage(sel) << "\n";
    const double parseMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    GfaAnnotateStats st = annotateGfa(teloscope, g, &sel, outDir, log);
    st.parseMs += parseMs;
    return st;
}

// The device route of annotateGfa(teloscope, file, outDir, log), which stays the default: the same two output files byte for
// byte, the same warnings on `log`, the same exceptions and the same GfaAnnotateStats, but no host thread looks for a line end
// or a tab.  The text reaches HBM through detail::ChunkFeed (teloscope_mi355x_io.hpp: a plain file, BGZF members inflated on the
// device, or a stream, here always through zlib, which reads plain bytes through the same calls)
// in chunks of ~chunkBytes bytes, and per chunk ts_gfa_chunk_walk gives the segment table, the P / H lines and the names.  Which
// segments are scanned and which field of an S line is its sequence is known only after the last line (a P or H line may stand
// anywhere), so every walked chunk STAYS RESIDENT; an unfinished last line moves into the next chunk device to device
// (ts_chunk_carry_over).  After the last chunk the host builds the graph exactly as readGfa does (names, hash index, paths,
// version, edits), gfaTerminalJobs picks the ends, and ONE terminalEnds call scans the wanted segments where they lie in the
// chunks (TS_INPUT_DEVICE, no host view; one call per context where the Teloscope has several: below).  The writer takes the input's bytes from the mapping, from the zlib blocks as they were
// produced, or — BGZF — from the chunks, read back piece by piece.
// Assembly record filters: the form with a selector mirrors annotateGfa(teloscope, file, outDir, selector, log).  With an active
// selector the .gfa2 / .gfa2.gz name check comes first; ts_gfa_chunk_check judges every chunk's lines by validateFilteredGfa's
// rules beside the walk (a line with a '\r' inside it is read back and judged by the host's own rule), line numbers running
// over the chunks; after the last chunk the first offence is thrown with validateFilteredGfa's message, then come the graph
// build's errors, selectGfa, its line on `log`, and the ends of the selected paths / segments only.  The text is uploaded and
// indexed once, where the host route reads and walks the file twice.  An inactive selector changes nothing.
// Several contexts (a Teloscope made over a device list with DeviceRoutes::EveryContext — without it such an object is refused
// as before, "runs on one device"; with and without a selector): detail::ChunkRing deals chunk k to
// context k mod N, a thread per context; the new bytes are staged while the chunks before are framed, and the serial section
// carries the unfinished last line over (across contexts), commits, walks, checks and appends the tables in chunk order
// (detail::GfaChunkSteps, for every count: one context fills each chunk in place on the caller's thread).  Every chunk stays
// resident on the context that took it, so N devices hold the text between them; the wanted segments are grouped by the context
// that owns their line and ONE terminalEnds call per context runs, a thread each; the writer reads BGZF pieces back from
// whichever context's chunk holds them.  Files, warnings, exceptions and their order, and GfaAnnotateStats do not depend on N
// (tests/test_gpu_assembly_routes_multi.py).  perDevice, where given, receives one entry per context (AssemblyRouteDeviceStats,
// teloscope_mi355x_io.hpp); TS_TIMING=1 prints a line per context beside the line of totals.
// Limits: a line of more than
// 4 GiB - 2 bytes is refused with its byte offset; a text that does not fit the devices' free memory is refused with a message
// that names annotateGfa, the context that could not allocate and the bytes resident over all contexts; on one context the
// stages run one after the other.  With a GFA 2 input that holds both a foreign record and a segment
// named twice, the foreign record is reported (readGfa reports whichever comes first by its 16 MB parse blocks).
namespace detail {

// annotateGfaDevice's chunk stages, for a Teloscope of any number of contexts.  Every walked chunk stays resident on the context
// that took it, so each chunk is a ts_chunk of its own; the two ways its bytes come in are the read routes'
// (teloscope_mi355x_io.hpp): in place on one context, on the caller's thread, a chunk that holds no whole line growing where it
// is; dealt by detail::ChunkRing on several, chunk k to context k mod N, the new bytes staged while the chunks before it are
// framed.  The serial section places the unfinished last line of chunk k - 1 in front (ts_chunk_carry_over, across contexts),
// commits the staged bytes, walks (ts_gfa_chunk_walk), checks (ts_gfa_chunk_check, with an active selector; line numbers run over
// the chunks) and appends the tables to the host's, in chunk order.  A dealt chunk that holds no whole line hands all of its
// bytes on and is given up once they have moved; judge and emit are empty.
class GfaChunkSteps {
public:
    // the input's bytes for the writer, in the pieces they arrived in: host memory, or bytes [at, at + len) of a chunk
    struct Piece { const char *host; ts_chunk *chunk; uint64_t at, start, len; };
    // what a chunk's walk gave; base: the input offset of the chunk's first byte; context: whose memory the chunk lies in
    struct Walked { ts_chunk *chunk; size_t context; uint64_t base; std::vector<ts_gfa_segment> segs; std::vector<ts_gfa_line> lines; std::vector<char> text; ts_gfa_foreign foreign; };
    struct Held {
        ts_chunk *chunk = nullptr;
        std::atomic<bool> spent{false};                         // all of its bytes moved on: its owner gives it up
        explicit Held(ts_chunk *c) : chunk(c) {}
        Held(const Held &) = delete;
        Held &operator=(const Held &) = delete;
        ~Held() { ts_bam_chunk_destroy(chunk); }
    };
    struct Worker {
        size_t index = 0;
        ts_ctx *ctx = nullptr;
        std::vector<std::unique_ptr<Held>> chunks;              // every one stays until the scan and the write are done
        Held *cur = nullptr;
        ChunkFeed::Fill fill;                                   // a dealt chunk's new bytes
        std::vector<ts_gfa_flagged> flagged = std::vector<ts_gfa_flagged>(64);
        AssemblyRouteDeviceStats st;
    };
    static constexpr uint64_t kChunkLimit = 0xfffffffeull;      // what ts_gfa_chunk_walk takes

    std::vector<std::unique_ptr<Worker>> workers;
    std::vector<Piece> pieces;
    std::vector<std::vector<char>> blocks;                      // zlib's output as it was produced
    uint64_t total = 0;
    std::vector<Walked> walked;
    // filters: the first line that breaks validateFilteredGfa's rules (code 0: none so far), lines counted over the chunks
    int offence = 0;
    char offenceType = 0;
    uint64_t offenceLine = 0;
    std::unique_ptr<ChunkFeed> feed;

    GfaChunkSteps(Teloscope &teloscope, const std::string &file, bool filtered, size_t chunkBytesArg) : file_(file), filtered_(filtered) {
        for (size_t w = 0; w < teloscope.deviceCount(); ++w) {
            workers.emplace_back(new Worker());
            workers.back()->index = w;
            workers.back()->ctx = teloscope.context(w);
            workers.back()->st.device = teloscope.deviceOrdinal(w);
        }
        ChunkFeed::Options options;
        options.cannotOpen = "Could not open assembly input '" + file + "'.";
        options.cannotRead = "Could not read assembly input '" + file + "'.";
        options.zlibAlways = true;
        options.growFailed = "cannot grow a device chunk";
        options.uploadFailed = "upload of the GFA text failed";
        options.noRoom = [this](const char *what) { return noRoom(*workers[0], what); };         // (the in-place fills: context 0's)
        options.sink = [this](const char *host, uint64_t chunkAt, uint64_t len) {
            pieces.push_back({host, host ? nullptr : workers[0]->cur->chunk, chunkAt, total, len});
            total += len;
        };
        if (workers.size() > 1) options.gzipDevice = false;      // (bound to one context: plain gzip is read through zlib)
        feed.reset(new ChunkFeed(workers[0]->ctx, file, options));
        chunkLimit_ = feed->chunkLimit(kChunkLimit);
        chunkBytes_ = static_cast<size_t>(std::min<uint64_t>(std::max<size_t>(chunkBytesArg, 64), chunkLimit_));
        compCap_ = feed->compCap(chunkBytes_);
    }

    // "does not fit the device's free memory": the context that could not allocate, and what is resident over all of them
    std::runtime_error noRoom(const Worker &k, const char *what) const {
        const char *why = ts_last_error(k.ctx);
        return std::runtime_error(std::string("annotateGfaDevice: ") + what + " on context " + std::to_string(k.index) + " of " + std::to_string(workers.size()) +
                                  " (device " + std::to_string(k.st.device) + ") with " + std::to_string(resident_.load()) +
                                  " bytes of the graph's text resident over all contexts (" + (why ? why : "?") +
                                  "): the text does not fit the device's free memory; use annotateGfa, the host route");
    }

    // The whole input as in-place chunks of context 0, on the caller's thread: any source of the feed
    void runInPlace() {
        Worker &k = *workers[0];
        uint64_t held = 0;
        bool atEnd = false, grow = false;
        while (!atEnd) {
            const Clock::time_point t0 = Clock::now();
            uint64_t carry = held;                              // growing: the whole chunk is one unfinished line
            if (!grow) carry = prev_ ? prevSize_ - prevNext_ : 0;
            if (carry >= chunkLimit_) throw lineTooLong();
            // a chunk that held no whole line takes as much again, up to what a chunk may hold
            const size_t want = static_cast<size_t>(std::min<uint64_t>(std::max<uint64_t>(chunkBytes_, grow ? carry : 0), chunkLimit_ - carry));
            std::vector<char> *keep = nullptr;
            if (feed->source() == ChunkFeed::Stream) { blocks.emplace_back(); keep = &blocks.back(); }   // zlib's next block, kept for the writer
            const uint64_t room = feed->read(want, keep);       // (known for a mapped plain file and a block read, a guess for BGZF members)
            if (!grow) {
                make(k, carry + room);
                if (carry && ts_chunk_carry_over(k.cur->chunk, prev_->chunk, prevNext_, nullptr) != TS_OK) throw noRoom(k, "cannot carry a line into the next device chunk");
                ++k.st.chunks;
            }
            atEnd = feed->put(k.cur->chunk, 0);
            k.st.msFill += since(t0);
            const uint64_t now = ts_bam_chunk_size(k.cur->chunk);
            resident_ += now - (grow ? held : 0);
            k.st.bytesReceived += now - carry;
            held = now;
            if (held == 0) continue;
            grow = !walk(k, atEnd, held);                       // no whole line yet: the chunk takes more
        }
    }

    // the ring's steps: a dealt chunk
    void begin(size_t w) { ts_bind_thread_to_device(workers[w]->ctx); }
    RingTake take(size_t w, uint64_t) {
        Worker &k = *workers[w];
        feed->take(chunkBytes_, k.fill);
        return k.fill.atEnd ? RingTake::Last : RingTake::More;
    }
    void stage(size_t w, uint64_t) {
        Worker &k = *workers[w];
        const Clock::time_point t0 = Clock::now();
        k.chunks.erase(std::remove_if(k.chunks.begin(), k.chunks.end(), [](const std::unique_ptr<Held> &h) { return h->spent.load(); }), k.chunks.end());
        make(k, k.fill.n);
        const std::function<std::runtime_error(const char *)> refuse = [&](const char *what) { return noRoom(k, what); };
        feed->stage(k.ctx, k.cur->chunk, k.fill, &refuse);
        resident_ += k.fill.n;
        k.st.msStage += since(t0);
        ++k.st.chunks; k.st.bytesReceived += k.fill.n;
    }
    bool frame(size_t w, uint64_t) {                            // the serial section: carry, commit, walk, check, the tables appended
        Worker &k = *workers[w];
        const uint64_t carry = prev_ ? prevSize_ - prevNext_ : 0;
        if (carry >= chunkLimit_) throw lineTooLong();
        const Clock::time_point t0 = Clock::now();
        if (prev_ && ts_chunk_carry_over(k.cur->chunk, prev_->chunk, prevNext_, nullptr) != TS_OK) throw noRoom(k, "cannot carry a line into the next device chunk");
        if (prev_ && prevWhole_) {                              // all of that chunk's bytes are here now, at the same offsets
            // (the pieces of the unfinished line, which begins at input offset base_, are the list's last ones)
            for (size_t i = pieces.size(); i-- > 0 && pieces[i].start + pieces[i].len > base_;)
                if (pieces[i].chunk == prev_->chunk) pieces[i].chunk = k.cur->chunk;
            resident_ -= prevSize_;
            prev_->spent.store(true);
        }
        if (ts_chunk_commit(k.cur->chunk, nullptr) != TS_OK) throw noRoom(k, "cannot grow a device chunk");
        k.st.msCommit += since(t0);
        resident_ += carry;
        // the new bytes for the writer: where they lie on the host, or behind the carry in the chunk
        if (k.fill.n) {
            if (k.fill.calls.empty()) {
                pieces.push_back({k.fill.host, nullptr, 0, total, k.fill.n});
                if (!k.fill.block.empty()) blocks.push_back(std::move(k.fill.block));    // (its bytes stay where they are)
            } else {
                pieces.push_back({nullptr, k.cur->chunk, carry, total, k.fill.n});
            }
            total += k.fill.n;
        }
        const uint64_t held = ts_bam_chunk_size(k.cur->chunk);
        if (held == 0 || !walk(k, k.fill.atEnd, held)) { prev_ = k.cur; prevNext_ = 0; prevSize_ = held; prevWhole_ = true; }
        return true;
    }
    void judge(size_t, uint64_t) {}                             // (every chunk stays resident on its own context: the scan comes
    void emit(size_t, uint64_t) {}                              // after the last one)

    std::runtime_error chunkError(const Worker &k, const char *what) const { return deviceError(k.ctx, what); }

private:
    using Clock = std::chrono::steady_clock;
    static double since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

    void make(Worker &k, uint64_t room) {
        ts_chunk *made = ts_bam_chunk_create(k.ctx, compCap_, std::max<uint64_t>(room, 64));
        if (!made) throw noRoom(k, "cannot make a device chunk");
        k.chunks.emplace_back(new Held(made));
        k.cur = k.chunks.back().get();
    }
    std::runtime_error lineTooLong() const {
        return std::runtime_error("the line at byte offset " + std::to_string(base_) + " of '" + file_ + "' has more than " + std::to_string(chunkLimit_) +
                                  " bytes and does not fit a device chunk; use annotateGfa, the host route");
    }
    // Segments, P / H lines and names of k's current chunk, which has its `held` bytes; with an active selector its whole lines
    // by the filtered loader's rules; the tables appended and the framing's state moved on.  -> false: the chunk holds no whole
    // line yet, and nothing was appended
    bool walk(Worker &k, bool atEnd, uint64_t held) {
        ts_chunk *cur = k.cur->chunk;
        Clock::time_point t0 = Clock::now();
        Walked w;
        w.chunk = cur; w.context = k.index; w.base = base_;
        w.segs.resize(4096); w.lines.resize(256); w.text.resize(size_t(1) << 16);
        uint64_t nSegs = 0, nLines = 0, textBytes = 0, next = 0;
        int rc = ts_gfa_chunk_walk(cur, atEnd ? 1 : 0, w.segs.data(), w.segs.size(), &nSegs, w.lines.data(), w.lines.size(), &nLines,
                                   w.text.data(), w.text.size(), &textBytes, &next, &w.foreign);
        if (rc == TS_ERR_INVALID_ARG && (nSegs > w.segs.size() || nLines > w.lines.size() || textBytes > w.text.size())) {
            w.segs.resize(static_cast<size_t>(std::max<uint64_t>(nSegs, 1)));
            w.lines.resize(static_cast<size_t>(std::max<uint64_t>(nLines, 1)));
            w.text.resize(static_cast<size_t>(std::max<uint64_t>(textBytes, 1)));
            rc = ts_gfa_chunk_walk(cur, atEnd ? 1 : 0, w.segs.data(), w.segs.size(), &nSegs, w.lines.data(), w.lines.size(), &nLines,
                                   w.text.data(), w.text.size(), &textBytes, &next, &w.foreign);
        }
        if (rc != TS_OK) throw chunkError(k, "GFA walk failed");
        k.st.msIndex += since(t0);
        if (!atEnd && next == 0) return false;
        if (filtered_ && !offence) {                            // the chunk's whole lines by the filtered loader's rules
            t0 = Clock::now();
            uint64_t nFlagged = 0, nChecked = 0;
            rc = ts_gfa_chunk_check(cur, atEnd ? 1 : 0, k.flagged.data(), k.flagged.size(), &nFlagged, &nChecked);
            if (rc == TS_ERR_INVALID_ARG && nFlagged > k.flagged.size()) {
                k.flagged.resize(static_cast<size_t>(nFlagged));
                rc = ts_gfa_chunk_check(cur, atEnd ? 1 : 0, k.flagged.data(), k.flagged.size(), &nFlagged, &nChecked);
            }
            if (rc != TS_OK) throw chunkError(k, "GFA check failed");
            for (uint64_t i = 0; i < nFlagged && !offence; ++i) {
                const ts_gfa_flagged &fl = k.flagged[static_cast<size_t>(i)];
                int code = static_cast<int>(fl.code);
                char type = static_cast<char>(fl.type);
                if (fl.code == TS_GFA_CHECK_HOST_DECIDES) {     // a '\r' inside the line: the host's rule on the line itself
                    std::string line(fl.len, '\0');
                    if (fl.len && ts_bam_chunk_read(cur, fl.off, fl.len, &line[0]) != TS_OK) throw chunkError(k, "cannot read the chunk");
                    line.erase(std::remove(line.begin(), line.end(), '\r'), line.end());
                    code = filteredGfaLineCode(line);
                    type = line.empty() ? 0 : line[0];
                }
                if (code) { offence = code; offenceType = type; offenceLine = linesBefore_ + fl.line + 1; }
            }
            linesBefore_ += nChecked;
            k.st.msIndex += since(t0);
        }
        w.segs.resize(static_cast<size_t>(nSegs)); w.lines.resize(static_cast<size_t>(nLines)); w.text.resize(static_cast<size_t>(textBytes));
        w.segs.shrink_to_fit(); w.lines.shrink_to_fit(); w.text.shrink_to_fit();
        k.st.records += nSegs;
        walked.push_back(std::move(w));
        prev_ = k.cur; prevNext_ = next; prevSize_ = held; prevWhole_ = false;
        base_ += next;
        return true;
    }

    std::string file_;
    bool filtered_;
    uint64_t chunkLimit_ = kChunkLimit, compCap_ = 64;
    size_t chunkBytes_ = 64;
    std::atomic<uint64_t> resident_{0};
    // the framing's state: the chunk framed last, its size, where its unfinished line begins and whether that is all it holds; the
    // input offset of the next chunk's first byte; the lines checked so far
    Held *prev_ = nullptr;
    uint64_t prevNext_ = 0, prevSize_ = 0, base_ = 0, linesBefore_ = 0;
    bool prevWhole_ = false;
};

inline GfaAnnotateStats annotateGfaDeviceWith(Teloscope &teloscope, const std::string &file, const std::string &outDir,
                                              const SequenceSelector *selector, std::ostream &log, size_t chunkBytesArg,
                                              std::vector<AssemblyRouteDeviceStats> *perDevice = nullptr) {
    using Clock = std::chrono::steady_clock;
    auto since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
    const auto tBegin = Clock::now();
    const bool filtered = selector && selector->active();
    if (filtered) detail::refuseGfa2Name(file);
    if (teloscope.deviceCount() > 1 && !teloscope.deviceRoutesUseEveryContext())
        throw std::runtime_error("annotateGfaDevice runs on one device: this Teloscope was made over " + std::to_string(teloscope.deviceCount()) +
                                 " (the graph's text lies in one device's memory); one made with DeviceRoutes::EveryContext has the route "
                                 "deal its chunks to all of them");
    double msGraph = 0;

    GfaChunkSteps steps(teloscope, file, filtered, chunkBytesArg);
    std::unique_ptr<ChunkRing<GfaChunkSteps>> ring;
    if (teloscope.deviceCount() > 1) {
        ring.reset(new ChunkRing<GfaChunkSteps>(teloscope.deviceCount(), 0, steps));
        ring->run();
    } else {
        steps.runInPlace();
    }
    using Walked = GfaChunkSteps::Walked;
    using Piece = GfaChunkSteps::Piece;
    const std::vector<Walked> &walked = steps.walked;
    const std::vector<Piece> &pieces = steps.pieces;
    const uint64_t total = steps.total;
    const int offence = steps.offence;
    const char offenceType = steps.offenceType;
    const uint64_t offenceLine = steps.offenceLine;
    ChunkFeed &feed = *steps.feed;
    auto fail = [&](const char *what) { return detail::deviceError(teloscope.context(0), what); };

    if (offence) throw detail::filteredGfaError(offence, offenceType, offenceLine);

    // the graph, as readGfa builds it
    Clock::time_point t0 = Clock::now();
    GfaGraph g;
    g.file = file;
    const size_t slash = file.find_last_of('/');
    g.baseName = slash == std::string::npos ? file : file.substr(slash + 1);
    std::vector<detail::GfaField> f;
    std::vector<std::pair<size_t, size_t>> headers;             // H lines carrying VN:Z (once per such field): input offset, length
    std::vector<char> headerIsV2;
    size_t nseg = 0;
    for (const Walked &w : walked) {
        nseg += w.segs.size();
        for (const ts_gfa_line &l : w.lines) {
            const char *b = w.text.data() + l.text_at, *e = b + l.len;
            if (l.kind == 'P') {
                detail::gfaFields(b, b, e, f, 4);
                if (f.size() >= 3) g.paths.push_back(detail::gfaCutPath(b, f));
            } else {
                detail::gfaFields(b, b, e, f, size_t(-1));
                for (size_t i = 1; i < f.size(); ++i)
                    if (f[i].len >= 5 && std::memcmp(b + f[i].off, "VN:Z:", 5) == 0) {
                        headers.emplace_back(static_cast<size_t>(w.base + l.off), l.len);
                        headerIsV2.push_back(std::string(b, l.len).find("VN:Z:2") != std::string::npos);
                        g.hasVersion = true;
                        g.version = (f[i].len > 5 && b[f[i].off + 5] == '2') ? 2 : 1;
                    }
            }
        }
    }
    if (g.version == 2)
        for (const Walked &w : walked)
            if (w.foreign.found) {
                std::string type(w.foreign.len, '\0');
                if (w.foreign.len && ts_bam_chunk_read(w.chunk, w.foreign.off, w.foreign.len, &type[0]) != TS_OK)
                    throw detail::deviceError(teloscope.context(w.context), "cannot read the chunk");
                throw std::runtime_error("GFA 2 record type '" + type + "' in '" + file +
                                         "' is not supported: only H and S records of a GFA 2 graph are read.");
            }
    for (size_t i = 0; i < headers.size(); ++i)
        if (headerIsV2[i]) g.edits.push_back({headers[i].first, headers[i].second, "H\tVN:Z:1.2"});
    g.segments.reserve(nseg);
    g.index.reserve(nseg);
    std::vector<uint32_t> segContext;                           // whose memory each segment's line lies in (a line lies in one chunk)
    segContext.reserve(nseg);
    for (const Walked &w : walked) {
        const char *dev = static_cast<const char *>(ts_chunk_data(w.chunk));
        for (const ts_gfa_segment &s : w.segs) {
            GfaSegment seg;
            seg.name.assign(w.text.data() + s.name_at, s.f1_len);
            uint64_t so = s.f2_at, sl = s.f2_len;
            bool star = (s.star & 1u) != 0;
            if (g.version == 2 && s.n_fields >= 4) {                 // S name len seq [tags]: the length goes
                so = s.f3_at; sl = s.f3_len; star = (s.star & 2u) != 0;
                g.edits.push_back({static_cast<size_t>(w.base + s.off + s.f2_at), s.f3_at - s.f2_at, std::string()});
            }
            if (!star) { seg.seq = dev + s.off + so; seg.len = sl; }   // (a device address: gfaScanEnds(..., onDevice))
            if (!g.index.emplace(seg.name, static_cast<uint32_t>(g.segments.size())).second)
                throw std::runtime_error("segment '" + seg.name + "' is defined twice in '" + file + "'.");
            g.segments.push_back(std::move(seg));
            segContext.push_back(static_cast<uint32_t>(w.context));
        }
    }
    std::sort(g.edits.begin(), g.edits.end(), [](const GfaEdit &a, const GfaEdit &b) { return a.off < b.off; });
    msGraph = since(t0);

    SequenceSelection sel;
    if (filtered) {
        sel = selectGfa(g, *selector);
        log << selectionMessage(sel) << "\n";
    }
    GfaAnnotateStats st;
    st.parseMs = since(tBegin);
    const auto t1 = Clock::now();
    const std::vector<GfaEnd> jobs = gfaTerminalJobs(g, filtered ? &sel.keep : nullptr);
    std::vector<uint64_t> scannedBases;
    std::vector<double> scanMs;
    const GfaEnds e = gfaScanEnds(teloscope, g, jobs, log, true, &segContext, &scannedBases, &scanMs);
    const auto t2 = Clock::now();
    for (size_t w = 0; w < steps.workers.size(); ++w) {
        steps.workers[w]->st.basesScanned = w < scannedBases.size() ? scannedBases[w] : 0;
        steps.workers[w]->st.msScan = w < scanMs.size() ? scanMs[w] : 0;          // (its own call; the contexts scan side by side)
    }

    // the input's bytes: host pieces as they lie, chunk pieces read back through a bounce buffer
    GfaInputBytes input;
    input.size = static_cast<size_t>(total);
    std::vector<char> bounce;
    auto readPiece = [&](const Piece &p, uint64_t off, uint64_t n, char *dst) {
        if (ts_bam_chunk_read(p.chunk, p.at + off, n, dst) != TS_OK) throw fail("cannot read the chunk");
    };
    if (total) {
        const Piece &p = pieces.back();
        if (p.host) input.last = p.host[p.len - 1]; else readPiece(p, p.len - 1, 1, &input.last);
    }
    input.write = [&](std::ostream &o, size_t off, size_t len) {
        size_t k = static_cast<size_t>(std::upper_bound(pieces.begin(), pieces.end(), off, [](size_t v, const Piece &p) { return v < p.start; }) - pieces.begin());
        k = k ? k - 1 : 0;
        for (; len && k < pieces.size(); ++k) {
            const Piece &p = pieces[k];
            if (off >= p.start + p.len) continue;
            uint64_t in = off - p.start, n = std::min<uint64_t>(len, p.len - in);
            off += n; len -= n;
            if (p.host) { o.write(p.host + in, static_cast<std::streamsize>(n)); continue; }
            for (; n;) {
                const uint64_t step = std::min<uint64_t>(n, uint64_t(16) << 20);
                bounce.resize(static_cast<size_t>(std::max<uint64_t>(bounce.size(), step)));
                readPiece(p, in, step, bounce.data());
                o.write(bounce.data(), static_cast<std::streamsize>(step));
                in += step; n -= step;
            }
        }
    };
    const std::string stem = outDir + "/" + g.baseName + ".telo.annotated";
    st.nodes = writeAnnotatedGfa(g, input, jobs, e.ends, stem + ".gfa", stem + ".colors.csv");
    const auto t3 = Clock::now();
    st.segments = g.segments.size();
    st.ends = jobs.size();
    st.scanned = e.scanned;
    st.noSeq = e.noSeq;
    st.scanMs = std::chrono::duration<double, std::milli>(t2 - t1).count();
    st.writeMs = std::chrono::duration<double, std::milli>(t3 - t2).count();
    double msUpload = 0, msIndex = 0;
    for (const auto &k : steps.workers) { msUpload += k->st.msFill + k->st.msStage + k->st.msCommit; msIndex += k->st.msIndex; }
    if (std::getenv("TS_TIMING"))
        std::fprintf(stderr, "annotateGfaDevice: upload%s %.0f ms, index %.0f ms, graph (host) %.0f ms, scan %.0f ms, write %.0f ms\n",
                     feed.deviceInflate() ? " + inflate + CRC" : "", msUpload, msIndex, msGraph, st.scanMs, st.writeMs);
    assemblyRouteFigures("annotateGfaDevice", steps.workers, ring.get(), perDevice);
    return st;
}
}  // namespace detail

inline GfaAnnotateStats annotateGfaDevice(Teloscope &teloscope, const std::string &file, const std::string &outDir,
                                          std::ostream &log = std::cerr, size_t chunkBytes = size_t(256) << 20,
                                          std::vector<AssemblyRouteDeviceStats> *perDevice = nullptr) {
    return detail::annotateGfaDeviceWith(teloscope, file, outDir, nullptr, log, chunkBytes, perDevice);
}

// the same with assembly record filters (see above)
inline GfaAnnotateStats annotateGfaDevice(Teloscope &teloscope, const std::string &file, const std::string &outDir,
                                          const SequenceSelector &selector, std::ostream &log = std::cerr,
                                          size_t chunkBytes = size_t(256) << 20,
                                          std::vector<AssemblyRouteDeviceStats> *perDevice = nullptr) {
    return detail::annotateGfaDeviceWith(teloscope, file, outDir, &selector, log, chunkBytes, perDevice);
}

}  // namespace teloscope_mi355x
