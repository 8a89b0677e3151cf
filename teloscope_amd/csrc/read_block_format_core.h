// read_block_format_core.h — the text of the read block report (include/teloscan.h: "The read block report"), one source for the
// gfx950 kernels (read_blocks.hip), for the host routes (include/teloscope_mi355x_io.hpp) and for a host test program
// (tests/cpp/read_block_format_host.cpp, built by g++ under ASan + UBSan).  Like match_format_core.h, whose integer routines it
// uses: no allocation, no library calls, no local arrays.
//
// A line is
//   name \t start \t end \t block_len \t label \t forward_count \t reverse_count \t canonical_count \t non_canonical_count \t read_len \n
// — the columns the terminal loop of the reference's writeBEDFile (src/teloscope.cpp) prints into _terminal_telomeres.bed, with
// pathSize replaced by the read's length and the scaffold / contig word dropped.  The output is this project's own.
//
// Text goes out through a sink S (void put(uint32_t at, uint32_t byte)); names come in through a reader (uint32_t byte(uint64_t i)).
#ifndef TS_READ_BLOCK_FORMAT_CORE_H
#define TS_READ_BLOCK_FORMAT_CORE_H

#include "track_format_core.h"

namespace tsrb {

// ------------------------------------------------------------------------------------------------ names
// Where a record's name lies, per front end.  `bytes` reads the chunk (or the record's text on the host).

// FASTQ: the header line starts at `off` with '@' and its sequence line at off + seq_at, so the header's bytes behind '@' and in
// front of its '\n' are [off + 1, off + seq_at - 1).  A '\r' right in front of the '\n' does not belong to the line; the name
// ends at the first space or tab, or with the line.  (seq_at >= 2: '@' and '\n'.)
template <class B>
TS_THD uint32_t fastq_name_len(const B &bytes, uint64_t off, uint32_t seq_at) {
    uint32_t n = seq_at >= 2u ? seq_at - 2u : 0u;
    if (n && bytes.byte(off + n) == '\r') --n;
    uint32_t i = 0;
    while (i < n) {
        const uint32_t c = bytes.byte(off + 1u + i);
        if (c == ' ' || c == '\t') break;
        ++i;
    }
    return i;
}
TS_THD uint64_t fastq_name_off(uint64_t off) { return off + 1u; }

// FASTA (the read subset): the header line starts at `off` with '>', and line_len bytes of it lie behind the '>' and in front of
// the line's end (ts_fasta_record's name_len: a '\r' in front of the '\n' is not among them); the name ends at the first space or
// tab, or with the line.  Its first byte is fastq_name_off's.
template <class B>
TS_THD uint32_t fasta_name_len(const B &bytes, uint64_t off, uint32_t line_len) {
    uint32_t i = 0;
    while (i < line_len) {
        const uint32_t c = bytes.byte(off + 1u + i);
        if (c == ' ' || c == '\t') break;
        ++i;
    }
    return i;
}

// SAM: the bytes of the alignment line in front of its first tab (a record of the table has ten tabs or more in front of SEQ, so the
// search ends before seq_at).
template <class B>
TS_THD uint32_t sam_name_len(const B &bytes, uint64_t off, uint32_t seq_at) {
    uint32_t i = 0;
    while (i < seq_at && bytes.byte(off + i) != '\t') ++i;
    return i;
}

// BAM: read_name lies 36 bytes behind the record's block_size field, l_read_name (the byte at 12) long with its NUL.
constexpr uint32_t kBamNameAt = 36u, kBamNameLenAt = 12u;
template <class B>
TS_THD uint32_t bam_name_len(const B &bytes, uint64_t off) {
    const uint32_t l = bytes.byte(off + kBamNameLenAt);
    return l ? l - 1u : 0u;
}
TS_THD uint64_t bam_name_off(uint64_t off) { return off + kBamNameAt; }

// ------------------------------------------------------------------------------------------------ lines
// What a line prints of a block (ts_block of include/teloscan.h) and of its read.
struct Fields {
    uint64_t start;
    uint32_t block_len, forward_count, reverse_count, canonical_count, non_canonical_count, read_len, label;
};

TS_THD uint32_t line_len(uint32_t name_len, const Fields &f) {
    return tstrack::prefix_len(name_len, f.start, f.start + f.block_len) + tstrack::u32_digits(f.block_len) + 3u +
           tstrack::u32_digits(f.forward_count) + 1u + tstrack::u32_digits(f.reverse_count) + 1u + tstrack::u32_digits(f.canonical_count) + 1u +
           tstrack::u32_digits(f.non_canonical_count) + 1u + tstrack::u32_digits(f.read_len) + 1u;
}

// v's digits from `at` and `sep` behind them; returns the place behind the separator
template <class S>
TS_THD uint32_t put_field(S &s, uint32_t at, uint32_t v, uint32_t sep) {
    at += tstrack::u32_digits(v);
    tstrack::put_u64(s, at, v);
    s.put(at, sep);
    return at + 1u;
}

// the line's bytes from `at`
template <class S, class N>
TS_THD void put_line(S &s, uint32_t at, const N &names, uint64_t name_off, uint32_t name_len, const Fields &f) {
    tstrack::put_prefix(s, at, names, name_off, name_len, f.start, f.start + f.block_len);
    at += tstrack::prefix_len(name_len, f.start, f.start + f.block_len);
    at = put_field(s, at, f.block_len, '\t');
    s.put(at, f.label);
    s.put(at + 1u, '\t');
    at += 2u;
    at = put_field(s, at, f.forward_count, '\t');
    at = put_field(s, at, f.reverse_count, '\t');
    at = put_field(s, at, f.canonical_count, '\t');
    at = put_field(s, at, f.non_canonical_count, '\t');
    (void)put_field(s, at, f.read_len, '\n');
}

}  // namespace tsrb

#endif
