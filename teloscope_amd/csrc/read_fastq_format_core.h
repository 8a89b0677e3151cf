// read_fastq_format_core.h — FASTQ text of a kept BAM or SAM record (include/teloscan.h: "FASTQ out of the BAM and SAM subsets"),
// one source for the gfx950 kernels (read_fastq.hip: where a record's fields lie, and every byte outside the 16-byte interior of
// the bases and the quals), for the host routes (include/teloscope_mi355x_io.hpp: bamSubsetFastq, samSubsetFastq) and for a host
// test program (tests/cpp/read_fastq_format_host.cpp, built by g++ under ASan + UBSan).  Like read_block_format_core.h, whose name
// rules it uses: no allocation, no library calls, no local arrays.  Bytes come in through a reader (uint32_t byte(uint64_t i)).
//
// A record's text is
//   '@' name '\n'  bases '\n'  '+' '\n'  quals '\n'
// record_len = name_len + 2 L + 6 bytes, L the number of bases judged.
#ifndef TS_READ_FASTQ_FORMAT_CORE_H
#define TS_READ_FASTQ_FORMAT_CORE_H

#include "read_block_format_core.h"

namespace tsfq {

constexpr uint32_t kPieceBytes = 4096u;            // text a wave of the device formatter writes: a kept record is cut into such pieces
constexpr uint32_t kRestoreStrand = 1u;             // TS_FASTQ_OUT_RESTORE_STRAND
constexpr uint32_t kBam = 0u, kSam = 1u;            // the front ends

// Where a record's fields lie in the bytes, and what its text does with them: 40 bytes, the device formatter's table entry
constexpr uint32_t kReverse = 1u, kQualMissing = 2u, kIsSam = 4u;
struct Rec {
    uint64_t name_off, seq_off, qual_off;           // BAM: seq_off is of the packed SEQ's first byte
    uint32_t name_len, len;                         // len: L
    uint32_t flags, reserved;                       // kReverse | kQualMissing | kIsSam
};

TS_THD uint64_t record_len(uint32_t name_len, uint32_t len) { return (uint64_t)name_len + 2ull * len + 6ull; }
TS_THD uint64_t record_len(const Rec &r) { return record_len(r.name_len, r.len); }

// ------------------------------------------------------------------------------------------------ BAM
constexpr uint32_t kBamFlagAt = 18u, kQualMax = 93u;

// the letter of a 4-bit code, and of the code with its four bits reversed (A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D)
TS_THD uint32_t bam_letter(uint32_t code) {
    const uint64_t lo = 0x56535247'4d43413dull, hi = 0x4e42444b'48595754ull;     // "=ACMGRSV" "TWYHKDBN"
    return (uint32_t)(((code & 8u) ? hi : lo) >> (8u * (code & 7u))) & 255u;
}
TS_THD uint32_t rev4(uint32_t code) { return ((code & 1u) << 3) | ((code & 2u) << 1) | ((code & 4u) >> 1) | ((code & 8u) >> 3); }
TS_THD uint32_t bam_qual(uint32_t byte) { return (byte < kQualMax ? byte : kQualMax) + 33u; }

// The record whose block_size field lies at `off`: block_size bytes behind that field, SEQ at off + seq_at, l_seq bases.  Every
// field is cut at the record's end (a walked record's fields lie inside it; a cut QUAL counts as missing).
template <class B>
TS_THD Rec bam_locate(const B &bytes, uint64_t off, uint32_t block_size, uint32_t seq_at, uint32_t l_seq, uint32_t out_flags) {
    Rec r;
    const uint64_t size = 4ull + block_size;
    const uint32_t name_len = size > tsrb::kBamNameLenAt ? tsrb::bam_name_len(bytes, off) : 0u;
    const uint64_t room = size > tsrb::kBamNameAt ? size - tsrb::kBamNameAt : 0ull;
    r.name_off = tsrb::bam_name_off(off);
    r.name_len = name_len < room ? name_len : (uint32_t)room;
    r.len = l_seq;
    r.seq_off = off + seq_at;
    r.qual_off = r.seq_off + ((uint64_t)l_seq + 1ull) / 2ull;
    const bool fits = (uint64_t)seq_at + ((uint64_t)l_seq + 1ull) / 2ull + l_seq <= size;
    const uint32_t flag = size >= kBamFlagAt + 2u ? bytes.byte(off + kBamFlagAt) | bytes.byte(off + kBamFlagAt + 1u) << 8 : 0u;
    r.flags = 0u;
    if ((out_flags & kRestoreStrand) && (flag & 0x10u)) r.flags |= kReverse;
    if (!fits || l_seq == 0u || bytes.byte(r.qual_off) == 0xffu) r.flags |= kQualMissing;
    r.reserved = 0u;
    return r;
}

// ------------------------------------------------------------------------------------------------ SAM
// the complement of a SEQ byte: the pairs of bam_letter on letters of either case, case kept; U and u as T and t; else the byte
TS_THD uint32_t sam_comp(uint32_t c) {
    const uint32_t up = c & ~32u, low = c & 32u;
    if (up < 'A' || up > 'Z') return c;
    uint32_t to;
    switch (up) {
        case 'A': to = 'T'; break;  case 'T': to = 'A'; break;  case 'U': to = 'A'; break;
        case 'C': to = 'G'; break;  case 'G': to = 'C'; break;
        case 'M': to = 'K'; break;  case 'K': to = 'M'; break;
        case 'R': to = 'Y'; break;  case 'Y': to = 'R'; break;
        case 'V': to = 'B'; break;  case 'B': to = 'V'; break;
        case 'H': to = 'D'; break;  case 'D': to = 'H'; break;
        default: return c;
    }
    return to | low;
}

// FLAG: the decimal value of the leading digits of field 2, at most nine of them; field 2 starts at `at` and the line's content
// ends at `end`
template <class B>
TS_THD uint32_t sam_flag(const B &bytes, uint64_t at, uint64_t end) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < 9u && at + i < end; ++i) {
        const uint32_t c = bytes.byte(at + i);
        if (c < '0' || c > '9') break;
        v = v * 10u + (c - '0');
    }
    return v;
}

// The alignment line at `off` (ts_sam_record: SEQ at off + seq_at, seq_len bytes; `size` bytes of content with a trailing '\r').
// QUAL is field 11: it starts behind the tab behind SEQ and is missing when it is exactly "*" (or does not lie inside the content).
template <class B>
TS_THD Rec sam_locate(const B &bytes, uint64_t off, uint32_t seq_at, uint32_t seq_len, uint32_t size, uint32_t out_flags) {
    Rec r;
    const uint64_t end = off + size - ((size && bytes.byte(off + size - 1u) == '\r') ? 1u : 0u);     // the content's end
    r.name_off = off;
    r.name_len = tsrb::sam_name_len(bytes, off, seq_at);
    r.len = seq_len;
    r.seq_off = off + seq_at;
    r.qual_off = r.seq_off + seq_len + 1ull;
    r.flags = kIsSam;
    if ((out_flags & kRestoreStrand) && (sam_flag(bytes, off + r.name_len + 1ull, end) & 0x10u)) r.flags |= kReverse;
    bool missing = r.qual_off + seq_len > end || seq_len == 0u;
    if (!missing && bytes.byte(r.qual_off) == '*' && (r.qual_off + 1ull >= end || bytes.byte(r.qual_off + 1ull) == '\t')) missing = true;
    if (missing) r.flags |= kQualMissing;
    r.reserved = 0u;
    return r;
}

// ------------------------------------------------------------------------------------------------ the text
// base j and qual j of the text (0 <= j < L), orientation applied
template <class B>
TS_THD uint32_t base_at(const B &bytes, const Rec &r, uint32_t j) {
    const uint32_t i = (r.flags & kReverse) ? r.len - 1u - j : j;
    if (r.flags & kIsSam) {
        const uint32_t c = bytes.byte(r.seq_off + i);
        return (r.flags & kReverse) ? sam_comp(c) : c;
    }
    const uint32_t code = (bytes.byte(r.seq_off + i / 2u) >> ((i & 1u) ? 0u : 4u)) & 15u;
    return bam_letter((r.flags & kReverse) ? rev4(code) : code);
}
template <class B>
TS_THD uint32_t qual_at(const B &bytes, const Rec &r, uint32_t j) {
    if (r.flags & kQualMissing) return '!';
    const uint32_t i = (r.flags & kReverse) ? r.len - 1u - j : j;
    const uint32_t q = bytes.byte(r.qual_off + i);
    return (r.flags & kIsSam) ? q : bam_qual(q);
}

// byte k of the record's text (0 <= k < record_len)
template <class B>
TS_THD uint32_t out_byte(const B &bytes, const Rec &r, uint64_t k) {
    if (k == 0ull) return '@';
    k -= 1ull;
    if (k < r.name_len) return bytes.byte(r.name_off + k);
    k -= r.name_len;
    if (k == 0ull) return '\n';
    k -= 1ull;
    if (k < r.len) return base_at(bytes, r, (uint32_t)k);
    k -= r.len;
    if (k < 3ull) return k == 1ull ? '+' : '\n';
    k -= 3ull;
    if (k < r.len) return qual_at(bytes, r, (uint32_t)k);
    return '\n';
}

}  // namespace tsfq

#endif
