// read_ring_host.cpp — the dealing, carry, ordering and error layer of the read routes on several contexts
// (include/teloscope_mi355x_ring.hpp: detail::ChunkRing) without a device: the steps a route gives the ring, restated over host
// buffers.  A stand-in context owns a chunk (contents and staging region, two byte vectors); take cuts the next piece of the
// text, stage copies it into the staging region, frame puts the unfinished record of the chunk framed before in front of it and
// frames FASTQ records by the rule tests/fastqchunk.py pins (ref_walk: blank lines in front of a header skipped, then four lines
// whatever they hold, checked in the host route's order), judge keeps the records whose sequence holds TTAGGG, emit writes.
// Stand-alone, g++ under ASan + UBSan and, a second build, under TSan.
//
//   read_ring_host          runs every case; stdout: one "ok <case> <runs>" line per case, then "ok"; exit 1 and a message
//                           on the first difference
// Cases: every chunk size of a 40-record text on 1-4 contexts; a record that is not valid at every position (so in every chunk
// position of every context); a writer that fails at every write.  What is expected is the result on one context: the output
// bytes, the message, the counts.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/teloscope_mi355x_ring.hpp"

using namespace teloscope_mi355x::detail;

namespace {

enum { OK = 0, TRUNCATED, BAD_HEADER, BAD_SEPARATOR, BAD_LENGTHS };
const char *const kMessages[] = {"", "truncated FASTQ record", "expected header line starting with '@'",
                                 "expected separator line starting with '+'", "sequence and quality length differ"};

struct Rec { size_t off, seqAt, seqLen, size; };
struct Walk { std::vector<Rec> recs; size_t next = 0; int error = OK; };

// ref_walk of tests/fastqchunk.py
Walk walk(const std::string &t, bool atEnd) {
    const size_t n = t.size();
    struct Line { size_t b, e, nx; bool ok; };
    auto line = [&](size_t p) -> Line {
        if (p >= n) return {0, 0, 0, false};
        const size_t nl = t.find('\n', p);
        if (nl == std::string::npos) return atEnd ? Line{p, n, n, true} : Line{0, 0, 0, false};
        return {p, nl, nl + 1, true};
    };
    auto logical = [&](const Line &l) { return l.e > l.b && t[l.e - 1] == '\r' ? l.e - l.b - 1 : l.e - l.b; };
    Walk w;
    size_t pos = 0;
    for (;;) {
        const Line h = line(pos);
        if (!h.ok) break;
        if (logical(h) == 0) { pos = h.nx; continue; }
        const Line s = line(h.nx), p = s.ok ? line(s.nx) : s, q = p.ok ? line(p.nx) : p;
        if (!q.ok) { w.next = h.b; w.error = atEnd ? TRUNCATED : OK; return w; }
        if (t[h.b] != '@') { w.next = h.b; w.error = BAD_HEADER; return w; }
        if (p.e == p.b || t[p.b] != '+') { w.next = h.b; w.error = BAD_SEPARATOR; return w; }
        if (logical(s) != logical(q)) { w.next = h.b; w.error = BAD_LENGTHS; return w; }
        w.recs.push_back({h.b, s.b - h.b, s.e - s.b, q.e - h.b});
        pos = q.nx;
    }
    w.next = pos;
    return w;
}

struct Outcome {
    std::string out, message;                                   // what was written; the exception's text ("" when none)
    size_t kept = 0, total = 0;
    bool operator==(const Outcome &o) const { return out == o.out && message == o.message && kept == o.kept && total == o.total; }
};

struct Writer {
    std::string &out;
    size_t failAt, writes = 0;                                  // the write that fails (counted from 1; 0: none)
    void write(const std::string &s) {
        if (s.empty()) return;
        if (++writes == failAt) throw std::runtime_error("failed while writing FASTQ subset");
        out += s;
    }
};

// the route on one context, without a ring: the loop of fastqSubsetDevice over a host buffer
Outcome oneContext(const std::string &text, size_t chunkBytes, size_t failAt) {
    Outcome o;
    Writer writer{o.out, failAt};
    try {
        std::string chunk;
        size_t at = 0, pos = 0;
        bool first = true, atEnd = false;
        while (!atEnd) {
            const size_t carry = chunk.size() - pos;
            const size_t want = std::max(chunkBytes, pos == 0 ? carry : size_t(0)), n = std::min(want, text.size() - at);
            chunk = chunk.substr(pos) + text.substr(at, n);
            at += n; pos = 0;
            atEnd = at >= text.size();
            if (first) {
                if (chunk.empty()) { if (atEnd) throw std::runtime_error("FASTQ input is empty"); continue; }
                if (chunk[0] != '@') throw std::runtime_error("FASTQ input must start with '@'");
                first = false;
            }
            const Walk w = walk(chunk, atEnd);
            std::string kept;
            for (const Rec &r : w.recs)
                if (chunk.substr(r.off + r.seqAt, r.seqLen).find("TTAGGG") != std::string::npos) { kept += chunk.substr(r.off, r.size) + "\n"; ++o.kept; }
            o.total += w.recs.size();
            writer.write(kept);
            if (w.error) throw std::runtime_error("FASTQ record " + std::to_string(o.total + 1) + ": " + kMessages[w.error]);
            pos = w.next;
        }
    } catch (const std::exception &e) { o.message = e.what(); }
    return o;
}

// the steps of the route on stand-in contexts
struct Steps {
    struct Context {
        std::string chunk, staged, kept;
        Walk w;
        size_t nKept = 0;
        bool atEnd = false;
    };
    const std::string &text;
    size_t chunkBytes;
    Writer writer;
    Outcome &o;
    std::vector<Context> ctx;
    size_t at = 0;                                              // the reader's
    const Context *prev = nullptr;                              // the serial section's
    bool first = true;

    Steps(const std::string &text_, size_t chunkBytes_, size_t contexts, size_t failAt, Outcome &o_)
        : text(text_), chunkBytes(chunkBytes_), writer{o_.out, failAt}, o(o_), ctx(contexts) {}

    void begin(size_t) {}
    RingTake take(size_t w, uint64_t) {
        Context &c = ctx[w];
        const size_t n = std::min(chunkBytes, text.size() - at);
        c.staged = text.substr(at, n);                          // (the reader's half; the copy stands for the stage step below)
        at += n;
        c.atEnd = at >= text.size();
        return c.atEnd ? RingTake::Last : RingTake::More;
    }
    void stage(size_t, uint64_t) {}
    bool frame(size_t w, uint64_t) {
        Context &c = ctx[w];
        const std::string carry = prev ? prev->chunk.substr(prev->w.next) : std::string();     // (prev may be c itself: one context)
        c.chunk = carry + c.staged;
        c.staged.clear();
        prev = &c;
        c.w = Walk();
        if (first) {
            if (c.chunk.empty()) { if (c.atEnd) throw std::runtime_error("FASTQ input is empty"); return true; }
            if (c.chunk[0] != '@') throw std::runtime_error("FASTQ input must start with '@'");
            first = false;
        }
        c.w = walk(c.chunk, c.atEnd);
        return c.w.error == OK;
    }
    void judge(size_t w, uint64_t) {
        Context &c = ctx[w];
        c.kept.clear(); c.nKept = 0;
        for (const Rec &r : c.w.recs)
            if (c.chunk.substr(r.off + r.seqAt, r.seqLen).find("TTAGGG") != std::string::npos) { c.kept += c.chunk.substr(r.off, r.size) + "\n"; ++c.nKept; }
    }
    void emit(size_t w, uint64_t) {
        Context &c = ctx[w];
        o.kept += c.nKept; o.total += c.w.recs.size();
        writer.write(c.kept);
        if (c.w.error) throw std::runtime_error("FASTQ record " + std::to_string(o.total + 1) + ": " + kMessages[c.w.error]);
    }
};

Outcome onRing(const std::string &text, size_t chunkBytes, size_t contexts, size_t failAt) {
    Outcome o;
    Steps steps(text, chunkBytes, contexts, failAt, o);
    try {
        ChunkRing<Steps> ring(contexts, 0, steps);
        ring.run();
    } catch (const std::exception &e) { o.message = e.what(); }
    return o;
}

std::string record(int i, bool telomeric, const char *eol = "\n") {
    std::string seq;
    for (int k = 0; k < 1 + i % 4; ++k) seq += telomeric ? "TTAGGG" : "ACGTC";
    const std::string name = "r" + std::to_string(i);
    return "@" + name + eol + seq + eol + (i % 4 == 2 ? "+" + name : std::string("+")) + eol + std::string(seq.size(), i % 5 == 1 ? '@' : 'I') + eol +
           (i % 13 == 5 ? "\n" : "") + (i % 17 == 9 ? "\r\n\n" : "");
}

bool same(const char *what, const Outcome &got, const Outcome &want, size_t a, size_t b, size_t c) {
    if (got == want) return true;
    // (a failing writer stops the route after a whole number of chunks: the counts are those of the chunks emitted, which differ
    // with the chunk sizes of the two routes only when a record exceeds a chunk — the cases below compare them all the same)
    std::printf("FAILED %s (%zu, %zu, %zu): wrote %zu bytes, kept %zu of %zu, \"%s\"; one context wrote %zu bytes, kept %zu of %zu, \"%s\"\n", what, a, b, c,
                got.out.size(), got.kept, got.total, got.message.c_str(), want.out.size(), want.kept, want.total, want.message.c_str());
    return false;
}

}  // namespace

int main() {
    std::vector<std::string> recs;
    for (int i = 0; i < 40; ++i) recs.push_back(record(i, i % 3 == 0, i % 11 == 4 ? "\r\n" : "\n"));
    std::string text;
    for (const std::string &r : recs) text += r;
    size_t runs = 0;

    // every chunk size: every cut of the text falls on a chunk boundary of some run, records straddle contexts and exceed chunks
    const Outcome whole = oneContext(text, text.size(), 0);
    if (whole.total != 40 || whole.kept != 14 || !whole.message.empty()) { std::printf("FAILED the text itself: kept %zu of %zu\n", whole.kept, whole.total); return 1; }
    for (size_t chunk = 1; chunk <= text.size() + 1; ++chunk)
        for (size_t contexts = 1; contexts <= 4; ++contexts, ++runs)
            if (!same("every cut", onRing(text, chunk, contexts, 0), whole, chunk, contexts, 0)) return 1;
    std::printf("ok every-cut %zu\n", runs);

    // a record that is not valid, at every position; chunks of three sizes, so the record lies in every chunk position
    runs = 0;
    for (size_t bad = 0; bad < recs.size(); ++bad)
        for (int kind = TRUNCATED; kind <= BAD_LENGTHS; ++kind) {
            std::string t;
            for (size_t i = 0; i < recs.size(); ++i) {
                std::string r = recs[i];
                if (i == bad && kind == BAD_HEADER && i > 0) r[0] = 'X';
                if (i == bad && kind == BAD_SEPARATOR) r[r.find("\n+") + 1] = '-';
                if (i == bad && kind == BAD_LENGTHS) r.insert(r.find('\n') + 1, "A");
                if (i == bad && kind == TRUNCATED) { t += r.substr(0, r.find('\n') + 3); break; }
                t += r;
            }
            for (size_t chunk : {size_t(33), size_t(97), size_t(257)}) {
                const Outcome want = oneContext(t, chunk, 0);
                if (want.message.empty() && !(kind == BAD_HEADER && bad == 0)) { std::printf("FAILED: case %zu/%d is no error\n", bad, kind); return 1; }
                for (size_t contexts = 1; contexts <= 4; ++contexts, ++runs)
                    if (!same("a record that is not valid", onRing(t, chunk, contexts, 0), want, bad, size_t(kind), contexts)) return 1;
            }
        }
    std::printf("ok errors %zu\n", runs);

    // a writer that fails at its n-th write: nothing of a later chunk is written
    runs = 0;
    for (size_t chunk : {size_t(129), size_t(257)})              // (above every record: the chunks are those of the loop on one context)
        for (size_t failAt = 1; failAt <= 16; ++failAt) {
            const Outcome want = oneContext(text, chunk, failAt);
            for (size_t contexts = 1; contexts <= 4; ++contexts, ++runs) {
                const Outcome got = onRing(text, chunk, contexts, failAt);
                if (got.out != want.out || got.message != want.message) { same("a failing writer", got, want, chunk, failAt, contexts); return 1; }
            }
        }
    std::printf("ok failing-writer %zu\n", runs);
    std::printf("ok\n");
    return 0;
}
