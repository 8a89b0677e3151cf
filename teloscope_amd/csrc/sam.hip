// sam.hip — SAM text of a resident chunk (chunk_internal.h) turned into a header extent and a record table on the device.
// One-wave workgroups throughout, like fastq.hip's and gfa.hip's.  The chunk layer's line index and tab index (chunk.hip: the
// byte count, the scan and the byte index for '\n' and for '\t') run in front of everything here; no kernel of this file scans
// the text.
//
//   * kinds: a lane per line.  A line is a header line when its first byte is '@' and an alignment line otherwise; a wave per
//     2 048 lines counts its alignment lines, and the lowest alignment line of the chunk is taken by a 64-bit atomic minimum:
//     the header is every line below it.  The chunk layer's scan turns the counts into every slice's first record.
//   * records: a lane per line again.  An alignment line finds its first tab by a lower bound of its start in the tab offsets
//     and is cut and checked by sam_line_core.h's rule (tabs 9, 10 and 11, only those before the line's end); its number is its
//     slice's first record plus a DPP prefix sum over the wave's kinds.  A header line above the lowest alignment line, or any
//     header line of a chunk that is entered behind the header, is an error.  The lowest bad line wins by a 64-bit atomic
//     minimum of line << 3 | code.
//   * stage and gather are fastq.hip's kernels and chunk.hip's plan: a record is a run of bytes with a '\n' behind it and a
//     sequence inside it in both formats.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teloscan.h"
#include "sam_internal.h"
#include "sam_line_core.h"
#include "ts_device.h"

namespace {

__global__ __launch_bounds__(64)
void ts_sam_kinds_kernel(const unsigned char *first, uint32_t n_lines, uint32_t *counts, unsigned long long *out) {
    uint32_t aligns = 0;
    unsigned long long lowest = ~0ull;
    for (uint32_t s = 0; s < kSamSliceLines; s += 64u) {
        // (in 64 bits: the last slice of a chunk of nearly 2^32 lines would wrap)
        const unsigned long long at = (unsigned long long)blockIdx.x * kSamSliceLines + s + threadIdx.x;
        const bool align = at < n_lines && first[at] != '@';
        const unsigned long long m = ballot64(align);
        // (lines ascend with the lanes and the steps: the first hit is the slice's lowest)
        if (m && lowest == ~0ull) lowest = at - threadIdx.x + (uint32_t)__builtin_ctzll(m);
        aligns += (uint32_t)__popcll(m);
    }
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = aligns;
        if (lowest != ~0ull) atomicMin(&out[kSmFirstAlign], lowest);
    }
}

__global__ __launch_bounds__(64)
void ts_sam_records_kernel(const unsigned char *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                           uint32_t n_lines, uint32_t newlines, const uint32_t *tabs, uint32_t n_tabs, int in_header,
                           const uint32_t *sums, ts_sam_record *recs, uint32_t n_recs, unsigned long long *out) {
    // a header line is in its place below the lowest alignment line of a chunk that is entered inside the header
    const unsigned long long first_align = out[kSmFirstAlign];
    uint32_t base = sums[blockIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) out[kSmLastLine] = lstart[newlines];
    for (uint32_t s = 0; s < kSamSliceLines; s += 64u) {
        const unsigned long long at = (unsigned long long)blockIdx.x * kSamSliceLines + s + threadIdx.x;
        const bool have = at < n_lines;
        const uint32_t i = have ? (uint32_t)at : n_lines;
        const bool align = have && first[i] != '@';
        // (every lane takes part in the scan)
        const uint32_t incl = wave_scan_add(align ? 1u : 0u);
        uint32_t bad = tssam::OK;
        if (align) {
            const uint32_t r = base + incl - 1u;
            const uint32_t ls = lstart[i], end = lstart[i + 1] - 1u - (uint32_t)cr[i];      // without '\n' and the '\r' in front of it
            tssam::Line l;
            bad = tssam::line_rule(plain, ls, end, tabs, n_tabs, tssam::tab_lower_bound(tabs, n_tabs, ls), &l);
            if (r < n_recs) {                                   // (always: the count pass saw the same lines)
                ts_sam_record rec;
                rec.off = ls; rec.seq_at = l.seq_at; rec.seq_len = l.seq_len; rec.size = end + (uint32_t)cr[i] - ls; rec.flags = l.flags;
                recs[r] = rec;
            }
        } else if (have && (!in_header || at > first_align)) {
            bad = tssam::HEADER_AFTER_RECORD;
        }
        const unsigned long long wrong = ballot64(bad != tssam::OK);
        // (lines ascend with the lanes: the lowest lane's is the step's lowest)
        if (wrong && threadIdx.x == (uint32_t)__builtin_ctzll(wrong)) atomicMin(&out[kSmError], (unsigned long long)i << 3 | bad);
        base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
}

}  // namespace

extern "C" {

int ts_k_launch_sam_kinds(const unsigned char *first, uint32_t n_lines, uint32_t *counts, unsigned long long *out, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kSamSliceLines - 1) / kSamSliceLines);
    if (nf == 0) return 0;
    hipLaunchKernelGGL(ts_sam_kinds_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, first, n_lines, counts, out);
    return (int)hipGetLastError();
}

int ts_k_launch_sam_records(const void *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                            uint32_t n_lines, uint32_t newlines, const uint32_t *tabs, uint32_t n_tabs, int in_header,
                            const uint32_t *sums, void *recs, uint32_t n_recs, unsigned long long *out, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kSamSliceLines - 1) / kSamSliceLines);
    if (nf == 0) return 0;
    hipLaunchKernelGGL(ts_sam_records_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, lstart, first, cr,
                       n_lines, newlines, tabs, n_tabs, in_header, sums, (ts_sam_record *)recs, n_recs, out);
    return (int)hipGetLastError();
}

}  // extern "C"
