// fastq_pair_core.h — the names of an interleaved pair (include/teloscan.h: "Interleaved paired FASTQ"), one source for the gfx950
// kernel (fastq.hip: ts_fastq_chunk_mates), for the host route (include/teloscope_mi355x_reads_host.hpp: fastqSubsetPaired) and for
// a host test program (tests/cpp/fastq_pairs_host.cpp, built by g++ under ASan + UBSan).  Like read_block_format_core.h, whose
// FASTQ name it takes: no allocation, no library calls, no local arrays.
//
// Bytes come in through a reader (uint32_t byte(uint64_t i)); a record is where its header line starts (`off`, the '@') and where
// its sequence line does (`off + seq_at`), as ts_fastq_record holds them.
#ifndef TS_FASTQ_PAIR_CORE_H
#define TS_FASTQ_PAIR_CORE_H

#include "read_block_format_core.h"

namespace tspair {

// the record's name: the block report's FASTQ name (the bytes behind '@' up to the first space, tab or the line's end, a '\r' in
// front of the '\n' not counted); it starts at tsrb::fastq_name_off(off)
template <class B>
TS_THD uint32_t name_len(const B &bytes, uint64_t off, uint32_t seq_at) { return tsrb::fastq_name_len(bytes, off, seq_at); }

// the mate name: the name without its last two bytes when they are "/1" or "/2", removed once and whichever mate carries them
template <class B>
TS_THD uint32_t mate_name_len(const B &bytes, uint64_t off, uint32_t seq_at) {
    const uint32_t n = name_len(bytes, off, seq_at);
    if (n < 2u) return n;
    const uint64_t at = tsrb::fastq_name_off(off) + n - 2u;
    const uint32_t d = bytes.byte(at + 1u);
    return bytes.byte(at) == '/' && (d == '1' || d == '2') ? n - 2u : n;
}

// whether the records at a and b are mates: their mate names are byte-equal (two empty ones are).  A reader per record, so that
// one that remembers the word it read last serves each name in order; a reader without memory is passed twice.
template <class A, class B>
TS_THD bool mates(const A &a_bytes, uint64_t a_off, uint32_t a_seq_at, const B &b_bytes, uint64_t b_off, uint32_t b_seq_at) {
    const uint32_t n = mate_name_len(a_bytes, a_off, a_seq_at);
    if (n != mate_name_len(b_bytes, b_off, b_seq_at)) return false;
    const uint64_t a = tsrb::fastq_name_off(a_off), b = tsrb::fastq_name_off(b_off);
    for (uint32_t i = 0; i < n; ++i)
        if (a_bytes.byte(a + i) != b_bytes.byte(b + i)) return false;
    return true;
}

}  // namespace tspair

#endif
