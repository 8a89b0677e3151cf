// match_format_host.cpp — teloscope_amd/csrc/match_format_core.h on the host: the functions the gfx950 kernels of match_text.hip
// compile, built by g++ under ASan + UBSan and checked against snprintf (tests/test_match_format_core_cpu.py).
//
//   match_format_host               formats generated records through the core and through snprintf("%s\t%llu\t%llu\t") + the
//                                   upper-cased substr of the bases; every line must be equal, of the length the core announced,
//                                   every byte written exactly once and none outside it; the selection rule is held against a
//                                   restatement of scanSegment's routing.  Prints "ok <lines> lines <selections> selections".
//                                   Covered: every digit count of position and end from 1 to 20 with the pairs where they differ;
//                                   sizes 1, 3, 6, 8, 32, 63; names of 1, 15, 16, 17, 70, 300 bytes; lower- and mixed-case bases;
//                                   rel at limit, limit + 1, term_end - 1, term_end; len <= limit; len between limit and 2 limit.
//   match_format_host lines FILE    FILE: u32 limit, n_segs; u64 n, names_len, bases_len; n ts_match of 16 bytes; n_segs segments
//                                   {u64 first_record, n_records, abs_pos, len, base_off, name_off; u32 name_len, tips_only}; the
//                                   names; the bases.  Prints, per file in file order, "#file <f> <bytes> <lines>\n" and its text.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/match_format_core.h"

namespace {

struct CheckedSink {                       // a text of `len` bytes: every put inside it, every byte once
    std::vector<char> text;
    std::vector<unsigned char> hits;
    bool bad = false;
    explicit CheckedSink(uint32_t n) : text(n, 0), hits(n, 0) {}
    void put(uint32_t at, uint32_t byte) {
        if (at >= text.size() || hits[at] || byte > 255u) { bad = true; return; }
        hits[at] = 1;
        text[at] = (char)byte;
    }
    bool complete() const {
        for (unsigned char h : hits) if (!h) return false;
        return !bad;
    }
};
struct StringSink {
    std::string &s;
    size_t base;
    void put(uint32_t at, uint32_t byte) { s.at(base + at) = (char)byte; }
};
struct Bytes {
    const std::vector<char> &v;
    uint32_t byte(uint64_t i) const { return (unsigned char)v.at(i); }
};

uint64_t n_lines = 0, n_selections = 0;

[[noreturn]] void fail(const char *what, const std::string &got, const std::string &want) {
    std::fprintf(stderr, "%s: core \"%s\" expected \"%s\"\n", what, got.c_str(), want.c_str());
    std::exit(1);
}

// one line through the core against snprintf + upper-cased substr
void check_line(const std::vector<char> &names, uint64_t name_off, uint32_t name_len, uint64_t pos, uint32_t size, const std::vector<char> &bases,
                uint64_t base_at) {
    std::string want(names.data() + name_off, name_len);
    char num[64];
    std::snprintf(num, sizeof num, "\t%llu\t%llu\t", (unsigned long long)pos, (unsigned long long)(pos + size));
    want += num;
    std::string seq(bases.data() + base_at, size);
    for (char &c : seq) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    want += seq;
    want += '\n';
    const uint32_t len = tsmatch::line_len(name_len, pos, size);
    CheckedSink s(len);
    tsmatch::put_line(s, 0u, Bytes{names}, name_off, name_len, pos, size, Bytes{bases}, base_at);
    const std::string got(s.text.begin(), s.text.end());
    if (len != want.size() || !s.complete() || got != want) fail("line", got, want);
    ++n_lines;
}

// scanSegment's routing (src/teloscope.cpp:485-509) with isTerminal (:451-459), restated
uint32_t expected_file(bool canonical, uint64_t rel, uint64_t len, uint64_t limit, bool tips) {
    if (tips) return 2u;
    if (canonical) return 0u;
    const bool start_side = rel <= limit;
    const bool end_side = len > limit ? rel >= len - limit : true;
    return start_side || end_side ? 1u : 2u;
}

void check_selection(uint64_t rel, uint64_t len, uint64_t limit) {
    for (int canonical = 0; canonical < 2; ++canonical)
        for (int tips = 0; tips < 2; ++tips) {
            const uint32_t got = tsmatch::select_file(canonical != 0, rel, len, limit, tips != 0), want = expected_file(canonical != 0, rel, len, limit, tips != 0);
            if (got != want) {
                std::fprintf(stderr, "selection: rel %llu len %llu limit %llu canonical %d tips %d: core %u expected %u\n", (unsigned long long)rel,
                             (unsigned long long)len, (unsigned long long)limit, canonical, tips, got, want);
                std::exit(1);
            }
            ++n_selections;
        }
}

int self_check() {
    std::mt19937_64 rng(20261019);
    const uint32_t name_lens[] = {1, 15, 16, 17, 70, 300}, sizes[] = {1, 3, 6, 8, 32, 63};
    std::vector<char> names(400), bases(4096);
    const char letters[] = "ACGTacgtAcGtaCgTNn";
    for (char &c : names) c = (char)('A' + rng() % 50);
    for (char &c : bases) c = letters[rng() % 18];
    std::vector<char> lower(bases);
    for (char &c : lower) if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
    // every digit count of the position from 1 to 20, the end with the same count and with one more
    std::vector<uint64_t> positions = {0, 1, 9};
    uint64_t p10 = 10;
    for (int d = 2; d <= 20; ++d) {                                  // p10 = 10^(d-1): the first position of d digits
        positions.push_back(p10);
        positions.push_back(p10 + 1);
        for (uint32_t back : {1u, 3u, 5u, 6u, 31u, 62u, 63u, 64u}) positions.push_back(p10 - back);     // ... whose end may have d digits
        if (d < 20) p10 *= 10;
    }
    positions.push_back(0xFFFFFFFFull); positions.push_back(0x100000000ull); positions.push_back(0xFFFFFFFFull - 5);
    positions.push_back(~0ull - 63); positions.push_back(~0ull - 64); positions.push_back(~0ull - 1000);
    unsigned seen_pos[21] = {0}, seen_end[21] = {0}, seen_cross = 0;
    for (uint64_t pos : positions)
        for (uint32_t size : sizes) {
            if (pos + size < pos) continue;
            for (uint32_t nl : name_lens) {
                const uint64_t name_off = rng() % (names.size() - nl + 1), base_at = rng() % (bases.size() - size + 1);
                check_line(names, name_off, nl, pos, size, bases, base_at);
                check_line(names, name_off, nl, pos, size, lower, base_at);
            }
            const uint32_t dp = tstrack::u64_digits(pos), de = tstrack::u64_digits(pos + size);
            ++seen_pos[dp]; ++seen_end[de];
            if (dp != de) ++seen_cross;
        }
    for (int d = 1; d <= 20; ++d)
        if (!seen_pos[d] || !seen_end[d]) { std::fprintf(stderr, "digit count %d not covered\n", d); return 1; }
    if (seen_cross < 19) { std::fprintf(stderr, "only %u start/end pairs of different digit counts\n", seen_cross); return 1; }
    // the terminal rule around its four edges, for segments longer than 2 limit, between limit and 2 limit, and up to limit
    typedef unsigned long long u64;
    for (u64 limit : {0ull, 1ull, 300ull, 50000ull, 0x7FFFFFFFull})
        for (u64 len : std::vector<u64>{1, limit / 2 + 1, limit ? limit - 1 : 1, limit + (limit == 0), limit + 1, limit + limit / 2 + 1, 2 * limit, 2 * limit + 1,
                                        2 * limit + 2, 3 * limit + 17, 1ull << 40}) {
            if (!len) continue;
            const u64 term_end = tsmatch::terminal_end(len, limit);
            for (u64 rel : std::vector<u64>{0, limit ? limit - 1 : 0, limit, limit + 1, limit + 2, term_end ? term_end - 1 : 0, term_end, term_end + 1, len - 1})
                if (rel < len) check_selection(rel, len, limit);
        }
    std::printf("ok %" PRIu64 " lines %" PRIu64 " selections\n", n_lines, n_selections);
    return 0;
}

struct Match { uint64_t position; uint16_t size; uint8_t flags; uint8_t reserved[5]; };
static_assert(sizeof(Match) == 16, "ts_match");

int lines_mode(const char *path) {
    FILE *fh = std::fopen(path, "rb");
    if (!fh) { std::perror(path); return 2; }
    uint32_t head32[2];
    uint64_t head64[3];
    if (std::fread(head32, 4, 2, fh) != 2 || std::fread(head64, 8, 3, fh) != 3) { std::fprintf(stderr, "short header\n"); return 2; }
    const uint32_t limit = head32[0], n_segs = head32[1];
    std::vector<Match> records(head64[0]);
    std::vector<tsmatch::Segment> segs(n_segs);
    std::vector<char> names(head64[1]), bases(head64[2]);
    static_assert(sizeof(tsmatch::Segment) == 56, "segment table entry");
    if ((records.size() && std::fread(records.data(), 16, records.size(), fh) != records.size()) ||
        (n_segs && std::fread(segs.data(), sizeof(tsmatch::Segment), n_segs, fh) != n_segs) ||
        (names.size() && std::fread(names.data(), 1, names.size(), fh) != names.size()) ||
        (bases.size() && std::fread(bases.data(), 1, bases.size(), fh) != bases.size())) { std::fprintf(stderr, "short file\n"); return 2; }
    std::fclose(fh);
    std::string text[tsmatch::kFiles];
    uint64_t lines[tsmatch::kFiles] = {0, 0};
    for (const tsmatch::Segment &sg : segs)
        for (uint64_t j = sg.first_record; j < sg.first_record + sg.n_records; ++j) {
            uint64_t w0, w1;
            std::memcpy(&w0, (const char *)&records.at(j), 8);
            std::memcpy(&w1, (const char *)&records.at(j) + 8, 8);
            const tsmatch::Rec r = tsmatch::decode_match(w0, w1);
            const uint64_t rel = r.at - sg.abs_pos;
            const uint32_t f = tsmatch::select_file(r.canonical, rel, sg.len, limit, sg.tips_only != 0);
            if (f == tsmatch::NO_LINE) continue;
            const uint32_t len = tsmatch::line_len(sg.name_len, r.at, r.size);
            const size_t at = text[f].size();
            text[f].resize(at + len);
            StringSink s{text[f], at};
            tsmatch::put_line(s, 0u, Bytes{names}, sg.name_off, sg.name_len, r.at, r.size, Bytes{bases}, sg.base_off + rel);
            check_line(names, sg.name_off, sg.name_len, r.at, r.size, bases, sg.base_off + rel);
            ++lines[f];
        }
    for (uint32_t f = 0; f < tsmatch::kFiles; ++f) {
        std::printf("#file %u %zu %" PRIu64 "\n", f, text[f].size(), lines[f]);
        std::fwrite(text[f].data(), 1, text[f].size(), stdout);
    }
    return 0;
}

// the packed record formats: what the kernels' policies decode
int check_decoders() {
    const tsmatch::Rec a = tsmatch::decode_tiled((12345u << 2) | 2u | 1u, 6u), b = tsmatch::decode_tiled((0x3FFFu << 2) | 2u, 8u);
    const tsmatch::Rec c = tsmatch::decode_general((4095u << 5) | (5u << 2) | 2u | 1u, 5u, 7u), d = tsmatch::decode_general((16383u << 8) | (62u << 2) | 1u, 8u, 63u);
    const unsigned long long lens = 5ull | (6ull << 6) | (63ull << 30);
    if (a.at != 12345u || a.size != 6u || !a.canonical || b.at != 0x3FFFu || b.size != 8u || b.canonical) return 1;
    if (c.at != 4095u || c.size != 5u || !c.canonical || d.at != 16383u || d.size != 62u || d.canonical) return 1;
    if (tsmatch::packed_len(lens, 0) != 5u || tsmatch::packed_len(lens, 1) != 6u || tsmatch::packed_len(lens, 5) != 63u) return 1;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (check_decoders()) { std::fprintf(stderr, "record decoders\n"); return 1; }
    if (argc == 3 && std::strcmp(argv[1], "lines") == 0) return lines_mode(argv[2]);
    if (argc != 1) { std::fprintf(stderr, "usage: match_format_host [lines FILE]\n"); return 2; }
    return self_check();
}
