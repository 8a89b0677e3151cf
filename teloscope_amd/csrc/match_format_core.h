// match_format_core.h — the text of the two match files (_canonical_matches.bed, _noncanonical_matches.bed), one source for the
// gfx950 kernels (match_text.hip) and for a host test program (tests/cpp/match_format_host.cpp, built by g++ under ASan + UBSan).
// Like track_format_core.h, whose integer and prefix routines it uses: no allocation, no library calls, no local arrays.
//
// A line is  name \t position \t position + matchSize \t matchSeq \n  — what BedWriter::format (include/teloscope_mi355x_io.hpp)
// writes per MatchInfo of canonicalMatches / nonCanonicalMatches, in place of the two match loops of the reference's writeBEDFile:
//   matchSeq     the matchSize bases at the match, a..z upper-cased (Teloscope::Segment::bases, src/teloscope.cpp:466-468);
//   which file   scanSegment's routing (src/teloscope.cpp:485-509): a canonical match of a full scan goes to the canonical file, any
//                other match to the non-canonical file if isTerminal(position relative to the SEGMENT) (src/teloscope.cpp:451-459),
//                and nowhere otherwise; a tips-only segment fills neither vector.
//
// Text goes out through a sink S (void put(uint32_t at, uint32_t byte)); names and bases come in through readers
// (uint32_t byte(uint64_t i)), which is what differs between the builds.
#ifndef TS_MATCH_FORMAT_CORE_H
#define TS_MATCH_FORMAT_CORE_H

#include "track_format_core.h"

namespace tsmatch {

// file order everywhere: detail::File's CAN_MATCH, NONCAN_MATCH (include/teloscope_mi355x_io.hpp)
enum File { CANONICAL = 0, NONCANONICAL = 1, kFiles = 2, NO_LINE = 2 };

constexpr uint32_t kMaxSize = 63u;                  // bases of a match: what a ts_pattern holds

// A segment of the table the formatter reads (ts_match_line_segment of include/teloscan.h): its bases are
// bases[base_off, base_off + len), its name names[name_off, name_off + name_len); first_record / n_records say which entries of a
// ts_match array are its matches (the scan's own record streams find their segment through the tile directory instead).
struct Segment {                                    // 56 bytes
    unsigned long long first_record, n_records, abs_pos, len, base_off, name_off;
    uint32_t name_len, tips_only;
};

// isTerminal (src/teloscope.cpp:451-459) of a segment-relative position; term_end = terminal_end(segment length, limit)
TS_THD uint64_t terminal_end(uint64_t seg_len, uint64_t limit) { return seg_len > limit ? seg_len - limit : 0u; }
TS_THD bool is_terminal(uint64_t rel, uint64_t limit, uint64_t term_end) { return rel <= limit || rel >= term_end; }

// the file a full-scan record's line goes to, NO_LINE for none
TS_THD uint32_t select_file(bool canonical, uint64_t rel, uint64_t seg_len, uint64_t limit, bool tips_only) {
    if (tips_only) return NO_LINE;
    if (canonical) return CANONICAL;
    return is_terminal(rel, limit, terminal_end(seg_len, limit)) ? NONCANONICAL : NO_LINE;
}

// ------------------------------------------------------------------------------------------------ records
// What a line needs of a record: where it lies in its tile (or, for a ts_match, its absolute position), its length, its class.
struct Rec { uint64_t at; uint32_t size; bool canonical; };

// the tiled kernel's: (tile-relative position << 2) | forward << 1 | canonical, one pattern length k; 16 or 32 bits
TS_THD Rec decode_tiled(uint32_t rec, uint32_t k) { return Rec{rec >> 2, k, (rec & 1u) != 0u}; }
// the general kernels': (tile-relative position << shift) | length index << 2 | canonical << 1 | forward; shift 5 and a 3-bit
// index (returned: the caller looks the length up), or shift 8 and a 6-bit index in the wide form
TS_THD Rec decode_general(uint32_t rec, uint32_t shift, uint32_t li_mask) { return Rec{rec >> shift, (rec >> 2) & li_mask, (rec & 2u) != 0u}; }
// up to eight lengths, six bits each, index i at bits 6i.. (TsBlockCallParams.gen_lens)
TS_THD uint32_t packed_len(unsigned long long gen_lens, uint32_t li) { return (uint32_t)(gen_lens >> (6u * li)) & 63u; }
// a ts_match as two 64-bit words: {position; match_size | flags << 16}; flag bit 1 is TS_MATCH_CANONICAL
TS_THD Rec decode_match(uint64_t w0, uint64_t w1) { return Rec{w0, (uint32_t)(w1 & 0xFFFFu), ((w1 >> 16) & 2u) != 0u}; }

// ------------------------------------------------------------------------------------------------ lines
TS_THD uint32_t line_len(uint32_t name_len, uint64_t pos, uint32_t size) { return tstrack::prefix_len(name_len, pos, pos + size) + size + 1u; }

// the line's bytes from `at`; the match's bases are bases.byte(base_at + 0 .. size)
template <class S, class N, class B>
TS_THD void put_line(S &s, uint32_t at, const N &names, uint64_t name_off, uint32_t name_len, uint64_t pos, uint32_t size, const B &bases,
                     uint64_t base_at) {
    tstrack::put_prefix(s, at, names, name_off, name_len, pos, pos + size);
    at += tstrack::prefix_len(name_len, pos, pos + size);
    for (uint32_t i = 0; i < size; ++i) {
        uint32_t c = bases.byte(base_at + i);
        if (c >= 'a' && c <= 'z') c -= 32u;
        s.put(at + i, c);
    }
    s.put(at + size, '\n');
}

}  // namespace tsmatch

#endif
