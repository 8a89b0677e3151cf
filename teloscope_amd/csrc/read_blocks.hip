// read_blocks.hip — the read block report as text, formatted where a batch's ordered block rows lie (ts_*_chunk_block_lines,
// ts_read_block_lines_format; host side read_blocks.cpp).  The output is this project's own (include/teloscan.h: "The read block
// report"); its columns mirror the terminal loop of the reference's writeBEDFile (src/teloscope.cpp, _terminal_telomeres.bed).
// Which bytes a record's name is, a line's length and a line's bytes are read_block_format_core.h, shared with the host routes
// (include/teloscope_mi355x_io.hpp: detail::ReadBlockReport) and with the host program that checks it against Python; this file
// is the data movement around it, in the shape of tracks.hip and match_text.hip:
//
//   ts_read_block_names  a lane per segment (read): where its name lies in the chunk and how long it is, by the front end's
//                        rule, and the read's length — the table the other two kernels read;
//   ts_read_block_count  a workgroup of ONE wave per 64 rows, a lane per block line: the bytes of the workgroup's lines;
//   (the scan)           tracks.hip's ts_track_scan_blocks over the two columns (bytes, lines): exclusive 64-bit prefix sums, the
//                        totals behind them.  No atomics: the text's order is the rows' order;
//   ts_read_block_write  the same lanes compute the same lengths again, scan them for their place, stage the wave's lines in LDS
//                        and copy them out in aligned 16-byte pieces (ts_text_emit.h says how).  64 lines that exceed the staging
//                        area (names beyond ~70 bytes) are written bytewise.
//
// Vector loads and stores only; names are read bytewise from the chunk through the record table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "read_block_format_core.h"
#include "ts_device.h"
#include "ts_internal.h"
#include "ts_text_emit.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ tsrb::Fields fields_of(const TsReadBlockRow &r, uint32_t read_len) {
    return tsrb::Fields{r.start, r.block_len, r.forward_count, r.reverse_count, r.canonical_count, r.non_canonical_count, read_len,
                        (uint32_t)(unsigned char)r.block_label};
}

// the record tables' entries, as include/teloscan.h lays them out (ts_fastq_record, ts_sam_record: 24 bytes; ts_bam_record: 24;
// ts_fasta_record: 32)
struct RecFastq { u64 off; uint32_t seq_at, seq_len, size, seq_cr; };
struct RecSam { u64 off; uint32_t seq_at, seq_len, size, flags; };
struct RecBam { u64 off; uint32_t block_size, seq_at, l_seq, reserved; };
struct RecFasta { u64 off; uint32_t text_len, body_at, n_bases, name_at, name_len, reserved; };    // (ts_fasta_record: 32 bytes)

__global__ __launch_bounds__(64)
void ts_read_block_names(const void *recs, uint32_t n, uint32_t kind, const unsigned char *chunk, TsReadBlockSeg *segs) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const GlobalBytes bytes{(const TS_GLOBAL unsigned char *)chunk};
    TsReadBlockSeg s;
    if (kind == TS_READ_BLOCK_FASTQ) {
        const RecFastq r = ((const RecFastq *)recs)[i];
        s.name_off = tsrb::fastq_name_off(r.off); s.name_len = tsrb::fastq_name_len(bytes, r.off, r.seq_at); s.read_len = r.seq_len - r.seq_cr;
    } else if (kind == TS_READ_BLOCK_SAM) {
        const RecSam r = ((const RecSam *)recs)[i];
        s.name_off = r.off; s.name_len = tsrb::sam_name_len(bytes, r.off, r.seq_at); s.read_len = r.seq_len;
    } else if (kind == TS_READ_BLOCK_FASTA) {
        const RecFasta r = ((const RecFasta *)recs)[i];
        s.name_off = tsrb::fastq_name_off(r.off); s.name_len = tsrb::fasta_name_len(bytes, r.off, r.name_len); s.read_len = r.n_bases;
    } else {
        const RecBam r = ((const RecBam *)recs)[i];
        // (a walked record's name ends inside it; the cut keeps any other table's reads inside the record too)
        const uint32_t room = r.block_size + 4u - tsrb::kBamNameAt, len = tsrb::bam_name_len(bytes, r.off);
        s.name_off = tsrb::bam_name_off(r.off); s.name_len = len < room ? len : room; s.read_len = r.l_seq;
    }
    segs[i] = s;
}

// A lane's line: its row, its segment's entry, its length (0: no line — a lane behind the last row)
struct Line { TsReadBlockRow row; TsReadBlockSeg seg; uint32_t len; };

__device__ __forceinline__ Line load_line(const TsReadBlockTextParams &P, u64 i) {
    Line L;
    L.len = 0u;
    if (i >= P.n_rows) return L;
    L.row = P.rows[i];
    if (L.row.seg >= P.n_segs) return L;                        // (a row of an overflowed general batch: no line, nothing read)
    L.seg = P.segs[L.row.seg];
    L.len = tsrb::line_len(L.seg.name_len, fields_of(L.row, L.seg.read_len));
    return L;
}

// sums: two columns of n_blocks + 1 values — per workgroup the bytes of its 64 lines, and how many of them there are
__global__ __launch_bounds__(64)
void ts_read_block_count(const TsReadBlockTextParams P) {
    const uint32_t lane = threadIdx.x;
    const Line L = load_line(P, (u64)blockIdx.x * 64u + lane);
    const uint32_t n = wave_total(L.len);
    const unsigned long long lines = __popcll(ballot64(L.len != 0u));
    if (lane == 0u) { P.sums[blockIdx.x] = n; P.sums[(u64)gridDim.x + 1u + blockIdx.x] = lines; }
}

__global__ __launch_bounds__(64)
void ts_read_block_write(const TsReadBlockTextParams P) {
    __shared__ u32x4 stage[kStageVecs];
    const uint32_t lane = threadIdx.x;
    const Line L = load_line(P, (u64)blockIdx.x * 64u + lane);
    const uint32_t incl = wave_scan_add(L.len), excl = incl - L.len;
    const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (!n) return;                                             // (uniform over the wave)
    TS_GLOBAL unsigned char *dst = (TS_GLOBAL unsigned char *)P.out + P.sums[blockIdx.x];
    const GlobalBytes names{(const TS_GLOBAL unsigned char *)P.names};
    if (L.len)
        wave_put(stage, dst, n, excl, [&](const auto &s, uint32_t at) {
            tsrb::put_line(s, at, names, L.seg.name_off, L.seg.name_len, fields_of(L.row, L.seg.read_len));
        });
    __syncthreads();                                            // (a single wave, and n is the same in all its lanes)
    wave_copy_out(stage, dst, n, lane);
}

}  // namespace

int ts_k_launch_read_block_names(const void *recs, uint32_t n, uint32_t kind, const void *chunk, TsReadBlockSeg *segs, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(ts_read_block_names, dim3((n + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, recs, n, kind, (const unsigned char *)chunk, segs);
    return (int)hipGetLastError();
}

int ts_k_launch_read_block_count(const TsReadBlockTextParams *P, uint32_t n_blocks, void *stream) {
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(ts_read_block_count, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, *P);
    const int e = (int)hipGetLastError();
    if (e != 0) return e;
    return ts_k_launch_scan_columns(P->sums, 2u, n_blocks, stream);
}

int ts_k_launch_read_block_write(const TsReadBlockTextParams *P, uint32_t n_blocks, void *stream) {
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(ts_read_block_write, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, *P);
    return (int)hipGetLastError();
}
