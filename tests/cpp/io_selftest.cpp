// Host-only self-test of the FASTA reader and the path splitter of include/teloscope_mi355x_io.hpp (no GPU
// call is made): the mapped, multi-threaded reader of plain files must return what the zlib stream reader
// returns for the same text gzip-compressed, and splitPath's 8-bytes-at-a-time scan must equal a per-character
// walk.  And of the device routes' chunk feed: which members of handmade BGZF byte strings one inflate call takes
// (detail::pickBgzfMembers), and which source a file is read as (detail::ChunkFeed::source).
// Usage: io_selftest <scratch directory>
#include "teloscope_mi355x_io.hpp"

#include <cstdlib>
#include <random>

using namespace teloscope_mi355x;

static void check(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "io_selftest: FAILED: %s\n", what); std::exit(1); }
}

// a BGZF member holding `text` (the payload a stored deflate block: nothing here inflates it), the EOF marker, a plain gzip member
static std::string bgzfMember(const std::string &text) {
    auto le = [](uint32_t v, int n) { std::string o; for (int i = 0; i < n; ++i) o += static_cast<char>((v >> (8 * i)) & 0xff); return o; };
    const uint32_t n = static_cast<uint32_t>(text.size());
    const std::string payload = std::string(1, '\1') + le(n, 2) + le(~n, 2) + text;
    return std::string("\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", 16) + le(static_cast<uint32_t>(18 + payload.size() + 8 - 1), 2) + payload +
           le(static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef *>(text.data()), n)), 4) + le(n, 4);
}
static const std::string kBgzfEof("\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0", 28);
static std::string gzipMember(const std::string &text, const std::string &dir) {
    const std::string path = dir + "/member.gz";
    gzFile g = gzopen(path.c_str(), "wb");
    check(g != nullptr, "gzopen");
    gzwrite(g, text.data(), static_cast<unsigned>(text.size()));
    gzclose(g);
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// ---- the member selection of the device routes' fill: first member always, `want`, compCap, foreign and truncated members
static void checkMemberSelection(const std::string &dir) {
    const size_t isize[4] = {30, 50, 70, 100};
    std::string m[4], all;
    for (int i = 0; i < 4; ++i) { m[i] = bgzfMember(std::string(isize[i], "ACGT"[i])); all += m[i]; }
    std::vector<ts_bgzf_block> descs;
    auto pick = [&](const std::string &bytes, size_t at, uint64_t dstBase, uint64_t produced, uint64_t want, uint64_t compCap) {
        return detail::pickBgzfMembers(reinterpret_cast<const unsigned char *>(bytes.data()), bytes.size(), at, dstBase, produced, want, compCap, descs);
    };
    const uint64_t roomy = 1u << 20;
    // want smaller than the first member: it is taken all the same, and the fill is full
    detail::BgzfPick p = pick(all, 0, 0, 0, 5, roomy);
    check(descs.size() == 1 && p.used == m[0].size() && p.made == 30 && p.full && !p.foreign, "first member beyond want");
    check(descs[0].src_off == 18 && descs[0].payload_len == m[0].size() - 26 && descs[0].isize == 30 && descs[0].dst_off == 0, "first member's descriptor");
    // want on a member boundary, and one byte short of it
    p = pick(all, 0, 0, 0, 80, roomy);
    check(descs.size() == 2 && p.used == m[0].size() + m[1].size() && p.made == 80 && p.full && !p.foreign, "want on a member boundary");
    check(descs[1].src_off == m[0].size() + 18 && descs[1].dst_off == 30, "second member's descriptor");
    p = pick(all, 0, 0, 0, 79, roomy);
    check(descs.size() == 1 && p.made == 30 && p.full, "want one byte short of a member boundary");
    // a compressed buffer for one member: the call ends, the fill does not, and dst_off runs on in the next call
    p = pick(all, 0, 7, 0, 1000, m[0].size() + 1);
    check(descs.size() == 1 && p.used == m[0].size() && p.made == 30 && !p.full && !p.foreign && descs[0].dst_off == 7, "compCap of one member, first call");
    p = pick(all, m[0].size(), 7, 30, 1000, m[0].size() + 1);
    check(descs.size() == 1 && p.used == m[1].size() && p.made == 50 && !p.full && !p.foreign, "compCap of one member, second call");
    check(descs[0].dst_off == 7 + 30 && descs[0].src_off == 18 && descs[0].isize == 50, "dst_off runs on, src_off starts again");
    // (the first member of a call is taken even where it alone exceeds compCap, as the first of a fill exceeds want)
    p = pick(all, 0, 0, 0, 1000, 10);
    check(descs.size() == 1 && p.used == m[0].size() && !p.full && !p.foreign, "compCap below one member");
    // the whole file: neither exit, every dst_off shifted by dstBase
    p = pick(all, 0, 1000, 0, 1000, roomy);
    check(descs.size() == 4 && p.used == all.size() && p.made == 250 && !p.full && !p.foreign, "all members");
    for (uint64_t i = 0, off = 1000; i < 4; off += isize[i++]) check(descs[i].dst_off == off && descs[i].isize == isize[i], "dstBase shifts every dst_off");
    // a plain gzip member behind two BGZF members: foreign, used stops in front of it, nothing thrown
    const std::string mixed = m[0] + m[1] + gzipMember("plain gzip text\n", dir);
    p = pick(mixed, 0, 0, 0, 1000, roomy);
    check(descs.size() == 2 && p.used == m[0].size() + m[1].size() && p.made == 80 && p.foreign && !p.full, "gzip member behind BGZF members");
    p = pick(mixed, p.used, 0, 80, 1000, roomy);
    check(descs.empty() && p.used == 0 && p.made == 0 && p.foreign, "a fill that begins at the foreign member");
    // a truncated last member, cut in its payload and in its header
    for (size_t cut : {size_t(5), size_t(11), m[3].size() - 1}) {
        p = pick(all.substr(0, all.size() - m[3].size() + cut), 0, 0, 0, 1000, roomy);
        check(descs.size() == 3 && p.used == all.size() - m[3].size() && p.made == 150 && p.foreign && !p.full, "truncated last member");
    }
    // the EOF marker (isize 0) in the middle, at the end and in front: a member like any other that brings no byte
    const std::string marked = kBgzfEof + m[0] + kBgzfEof + m[1] + kBgzfEof;
    p = pick(marked, 0, 0, 0, 1000, roomy);
    check(descs.size() == 5 && p.used == marked.size() && p.made == 80 && !p.full && !p.foreign, "EOF markers");
    check(descs[0].isize == 0 && descs[2].isize == 0 && descs[2].dst_off == 30 && descs[3].dst_off == 30 && descs[4].isize == 0 && descs[4].dst_off == 80, "EOF markers' descriptors");
    p = pick(marked, 0, 0, 0, 30, roomy);                           // (a marker behind a full fill still fits: it passes nothing)
    check(descs.size() == 3 && p.made == 30 && p.full, "EOF marker behind the last member that fits");
    p = pick(marked, 0, 0, 0, 10, roomy);                           // (a marker in front does not use up the first member's allowance)
    check(descs.size() == 2 && p.made == 30 && p.full, "EOF marker in front of the first member");
}

// ---- which source a file is read as: mapped plain text, mapped BGZF, or a stream (what does not map, or is gzip but not BGZF)
static void checkSourceClassification(const std::string &dir) {
    using Feed = detail::ChunkFeed;
    Feed::Options options;
    options.cannotOpen = "cannot open";
    options.cannotRead = "cannot read";
    const std::string text = "@r\nACGT\n+\nIIII\n";
    auto sourceOf = [&](const std::string &name, const std::string &bytes) {
        { std::ofstream f(dir + "/" + name, std::ios::binary); f << bytes; }
        return Feed(nullptr, dir + "/" + name, options).source();
    };
    check(sourceOf("empty", "") == Feed::Stream, "an empty file is a stream");
    check(sourceOf("plain", text) == Feed::Plain, "a text file is plain");
    check(sourceOf("bgzf", bgzfMember(text) + kBgzfEof) == Feed::Bgzf, "a bgzip-shaped file is BGZF");
    check(sourceOf("gzip", gzipMember(text, dir)) == Feed::Stream, "a plain gzip file is a stream");
    check(sourceOf("magic", "\x1f\x8b") == Feed::Stream, "two bytes of gzip magic are a stream");
    {
        Feed feed(nullptr, dir + "/gzip", options);                     // (a stream is read without a device: through zlib here)
        std::vector<char> block;
        check(feed.read(1000, &block) == text.size() && std::string(block.begin(), block.end()) == text && !feed.deviceInflate(), "the gzip stream's text");
    }
    bool threw = false;
    try { Feed(nullptr, dir + "/is_not_there", options); } catch (const std::runtime_error &e) { threw = std::string(e.what()) == "cannot open"; }
    check(threw, "a missing file is the route's cannot-open exception");
    const std::string fifo = dir + "/fifo";
    if (::mkfifo(fifo.c_str(), 0600) == 0) {                            // (quietly left out where the directory takes no FIFO)
        const int keep = ::open(fifo.c_str(), O_RDWR | O_NONBLOCK);     // a writer, so that the reader's open returns
        check(keep >= 0, "open the FIFO");
        check(Feed(nullptr, fifo, options).source() == Feed::Stream, "a FIFO is a stream");
        ::close(keep);
    }
}

int main(int argc, char **argv) {
    check(argc == 2, "usage: io_selftest <scratch directory>");
    const std::string dir = argv[1];
    std::mt19937_64 rng(11);
    checkMemberSelection(dir);
    checkSourceClassification(dir);
    // ---- splitPath against a per-character walk
    const char alpha[] = "ACGTNnXxYyOoacgtRWm";
    for (int it = 0; it < 20000; ++it) {
        const size_t n = rng() % 200;
        const int mode = static_cast<int>(rng() % 3);
        std::string s(n, 'A');
        for (size_t i = 0; i < n; ++i)
            s[i] = mode == 0 ? alpha[rng() % (sizeof(alpha) - 1)]
                             : (rng() % (mode == 1 ? 7 : 40) == 0 ? "NnXx"[rng() % 4] : alpha[rng() % (sizeof(alpha) - 1)]);
        if (mode == 2 && n > 30) for (size_t i = 5; i < 29; ++i) s[i] = "Nn"[i & 1];
        const std::string view = (std::string(rng() % 8, 'A') + s).substr(0);     // varying alignment of the data
        const PathComponents pc = splitPath(view);
        auto isGap = [](char c) { return c == 'N' || c == 'n' || c == 'X' || c == 'x'; };
        size_t i = 0, gi = 0, si = 0;
        while (i < view.size()) {
            const bool g = isGap(view[i]);
            size_t j = i;
            while (j < view.size() && isGap(view[j]) == g) ++j;
            if (g) { check(gi < pc.gaps.size() && pc.gaps[gi].start == i && pc.gaps[gi].length == j - i, "gap run"); ++gi; }
            else { check(si < pc.segments.size() && pc.segments[si].first == i && pc.segments[si].second == j - i, "segment run"); ++si; }
            i = j;
        }
        check(gi == pc.gaps.size() && si == pc.segments.size(), "run counts");
        // the same record cut into pieces that are scanned independently and stitched (splitPaths): any piece size
        const std::string header = "h";
        for (size_t piece : {size_t(1), size_t(7), size_t(64), size_t(1000), size_t(1) << 20}) {
            if (it % 16 != 0) break;                                   // (each call starts a thread pool)
            const std::vector<PathComponents> got = splitPaths({RecordView{&header, view.data(), view.size()}}, piece);
            check(got.size() == 1 && got[0].segments == pc.segments && got[0].gaps.size() == pc.gaps.size(), "stitched runs");
            for (size_t g = 0; g < pc.gaps.size() && g < got[0].gaps.size(); ++g)
                check(got[0].gaps[g].start == pc.gaps[g].start && got[0].gaps[g].length == pc.gaps[g].length, "stitched gap");
        }
    }
    // ---- readFasta: plain (mapped) vs gzip (stream) on awkward texts
    for (int it = 0; it < 40; ++it) {
        std::string text;
        if (it % 5 == 1) text += "stray line before the first header\n";
        const int nrec = 1 + static_cast<int>(rng() % 6);
        const bool crlf = it % 3 == 1;
        for (int r = 0; r < nrec; ++r) {
            text += ">rec" + std::to_string(r) + (r % 2 ? " description > with a bracket" : "") + (crlf ? "\r\n" : "\n");
            const size_t len = rng() % 5000, width = 1 + rng() % 90;
            for (size_t i = 0; i < len; ++i) {
                text += "ACGTNacgtn>"[rng() % (i % width == 0 ? 10 : 11)];      // '>' never at a line start
                if ((i + 1) % width == 0) text += crlf ? "\r\n" : "\n";
            }
            if (rng() % 3) text += crlf ? "\r\n" : "\n";
            if (rng() % 4 == 0) text += "\n";
        }
        if (it % 7 == 3 && !text.empty() && text.back() == '\n') text.pop_back();     // no newline at the end of the file
        const std::string plain = dir + "/t.fa", packed = dir + "/t.fa.gz";
        { std::ofstream f(plain, std::ios::binary); f << text; }
        { gzFile g = gzopen(packed.c_str(), "wb"); check(g != nullptr, "gzopen"); gzwrite(g, text.data(), static_cast<unsigned>(text.size())); gzclose(g); }
        const std::vector<FastaRecord> a = readFasta(plain), b = readFasta(packed);
        check(a.size() == b.size(), "record count");
        for (size_t i = 0; i < a.size(); ++i) check(a[i].header == b[i].header && a[i].sequence == b[i].sequence, "record content");
        // the streaming reader (groups of records, lines joined in pieces by the thread pool): any group size must
        // give the same records in the same order, from the mapped file and from the gzip stream
        for (const std::string &file : {plain, packed})
            for (size_t groupBytes : {size_t(1), size_t(700), size_t(1) << 20}) {
                FastaGroupReader rd(file, groupBytes, groupBytes == 700 ? size_t(37) : size_t(4) << 20);     // (tiny pieces: every record is stitched)
                detail::FastaGroup g;
                size_t at = 0;
                while (rd.next(g)) {
                    check(g.firstRecord == at, "group order");
                    check(g.comps.size() == g.records.size(), "components per record");
                    for (size_t ri = 0; ri < g.records.size(); ++ri) {
                        const detail::RawRecord &r = g.records[ri];
                        check(at < a.size() && r.header == a[at].header && std::string(r.data.get(), r.size) == a[at].sequence, "streamed record");
                        const PathComponents want = splitPath(a[at].sequence);
                        check(ri < g.comps.size() && g.comps[ri].segments == want.segments && g.comps[ri].gaps.size() == want.gaps.size(), "streamed components");
                        for (size_t q = 0; ri < g.comps.size() && q < want.gaps.size() && q < g.comps[ri].gaps.size(); ++q)
                            check(g.comps[ri].gaps[q].start == want.gaps[q].start && g.comps[ri].gaps[q].length == want.gaps[q].length, "streamed gap");
                        ++at;
                    }
                    for (const FastaRecord &r : g.owned) {
                        check(at < a.size() && r.header == a[at].header && r.sequence == a[at].sequence, "streamed record (zlib)");
                        ++at;
                    }
                }
                check(at == a.size(), "streamed record count");
            }
        // text mode (no lines joined: a record = its text pieces in the mapped file + base counts + N-runs): the pieces
        // must hold exactly the record's bases, the components must equal splitPath of the joined record, and any base
        // range must read back out of the pieces (what -m's matchSeq and the N-cut segments rely on)
        for (size_t pieceBytes : {size_t(1), size_t(53), size_t(4) << 20}) {
            FastaGroupReader rd(plain, 900, pieceBytes, true);
            detail::FastaGroup g;
            size_t at = 0;
            while (rd.next(g)) {
                for (size_t ri = 0; ri < g.records.size(); ++ri, ++at) {
                    const detail::RawRecord &r = g.records[ri];
                    check(at < a.size() && r.header == a[at].header && r.size == a[at].sequence.size(), "text record size");
                    if (at >= a.size()) continue;
                    uint64_t sum = 0;
                    for (const ts_text_piece &t : r.pieces) sum += t.n_bases;
                    check(sum == r.size, "text pieces hold the record's bases");
                    const PathComponents want = splitPath(a[at].sequence);
                    check(g.comps[ri].segments == want.segments && g.comps[ri].gaps.size() == want.gaps.size(), "text components");
                    for (size_t q = 0; q < want.gaps.size() && q < g.comps[ri].gaps.size(); ++q)
                        check(g.comps[ri].gaps[q].start == want.gaps[q].start && g.comps[ri].gaps[q].length == want.gaps[q].length, "text gap");
                    if (r.size) {
                        check(r.lines.size() == r.pieces.size(), "line structure per piece");
                        const Teloscope::Segment seg(r.pieces.data(), r.size, 0, false, (at % 2) ? r.lines.data() : nullptr);
                        for (int probe = 0; probe < 12; ++probe) {
                            const uint64_t pos = rng() % r.size, n = 1 + rng() % std::min<uint64_t>(r.size - pos, 200);
                            std::string want2 = a[at].sequence.substr(pos, n);
                            for (char &ch : want2) if (ch >= 'a' && ch <= 'z') ch = static_cast<char>(ch - 32);
                            check(seg.bases(pos, n) == want2, "bases out of text pieces");
                            check(*detail::textLocate(r.pieces[0].text, r.pieces[0].text_len, 0) == a[at].sequence[0] || r.pieces[0].n_bases == 0, "textLocate");
                        }
                    }
                }
            }
            check(at == a.size(), "text record count");
        }
    }
    // ---- splitFastqRecords (pieces parsed in parallel) against the sequential piece parser on awkward FASTQ texts
    size_t accepted = 0, offered = 0;
    for (int it = 0; it < 24; ++it) {
        std::string text;
        const int nrec = 50 + static_cast<int>(rng() % 400);
        const bool crlf = it % 4 == 1;
        const char *eol = crlf ? "\r\n" : "\n";
        for (int r = 0; r < nrec; ++r) {
            if (rng() % 11 == 0) text += eol;                                   // blank line before a header
            const size_t len = rng() % 300;
            text += "@r" + std::to_string(r) + (r % 3 ? " extra @ + words" : "") + eol;
            for (size_t i = 0; i < len; ++i) text += "ACGTN"[rng() % 5];
            text += eol;
            text += (r % 5 == 0 ? std::string("+r") + std::to_string(r) : std::string("+")) + eol;
            for (size_t i = 0; i < len; ++i) text += (i == 0 && rng() % 3 == 0) ? '@' : static_cast<char>('!' + rng() % 60);   // quality lines may begin with '@' or '+'
            text += eol;
        }
        if (it % 5 == 2) { text.pop_back(); if (crlf) text.pop_back(); }         // no newline at the end of the file
        if (it % 13 == 7) text.insert(text.size() / 2, "garbage line\n");         // malformed: must be refused, not mis-split
        std::vector<detail::FastqRec> seq, par;
        const char *stop = detail::parseFastqPiece(text.data(), text.data() + text.size(), text.data() + text.size(), seq);
        const bool wellFormed = stop == text.data() + text.size();
        for (size_t piece : {size_t(200), size_t(1500), size_t(20000)}) {
            const bool ok = detail::splitFastqRecords(text.data(), text.size(), par, piece);
            if (!wellFormed) { check(!ok, "malformed FASTQ accepted by the parallel splitter"); continue; }
            ++offered;
            if (!ok) continue;                                                  // refusing is always allowed (sequential fallback)
            ++accepted;
            check(par.size() == seq.size(), "parallel FASTQ record count");
            for (size_t i = 0; i < seq.size() && i < par.size(); ++i)
                check(par[i].begin == seq[i].begin && par[i].seq == seq[i].seq && par[i].end == seq[i].end && par[i].seqLen == seq[i].seqLen, "parallel FASTQ record");
        }
    }
    check(offered > 20 && accepted * 10 >= offered * 9, "the parallel splitter refuses well-formed FASTQ too often");
    puts("io_selftest ok");
    return 0;
}
