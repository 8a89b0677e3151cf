// fastq.hip — FASTQ text of a resident chunk (chunk_internal.h) turned into a record table, a read batch's input and the
// passing records' bytes, on the device.  One-wave workgroups throughout, like bgzf.hip's.  The chunk layer's line index
// (chunk.hip: every line's start, its first byte and whether a '\r' stands in front of its '\n') runs in front of everything here.
//
//   * record framing: readFastqRecord's rule is an automaton over lines with four states (0 expect header: a blank line
//     stays, any other line goes to 1; 1, 2, 3 = sequence, separator, quality: one line each, whatever it holds).  A line
//     is a map of the four states, a byte of four 2-bit fields, and maps compose: a prefix scan of the maps — within the
//     wave by six shuffle steps, across waves by a scan of the slices' maps — gives every line its state; no wave walks
//     the records.  A slice of lines also counts its headers for each of the four states it may be entered in, so that the
//     same scan hands every slice the index of its first record.
//   * record table: the lane that holds a header (a non-blank line met in state 0) reads its four lines' starts and checks
//     the record in readFastqRecord's order; the lowest record that fails wins by a 64-bit atomic minimum.
//   * stage and gather: 16 bytes per lane from an unaligned source — five aligned dwords and v_alignbyte_b32
//     (chunk_device.h) — to a 16-byte aligned destination.  The gather's places come from chunk.hip's plan.
//   * interleaved pairs: a lane per pair compares the two mate names by fastq_pair_core.h's rule, read through aligned dwords,
//     and the lowest pair that fails wins by a 64-bit atomic minimum; a byte kernel gives both mates the pair's verdict.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teloscan.h"
#include "chunk_device.h"
#include "fastq_internal.h"
#include "fastq_pair_core.h"
#include "ts_device.h"

namespace {

// ---- the framing automaton.  A map: state s goes to (map >> 2 s) & 3.
constexpr uint32_t kMapIdentity = 0xe4u, kMapBlank = 0x38u, kMapLine = 0x39u;      // {0,1,2,3}, {0,2,3,0}, {1,2,3,0}

__device__ __forceinline__ uint32_t map_then(uint32_t a, uint32_t b) {              // a, then b
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4u; ++s) r |= ((b >> (2u * ((a >> (2u * s)) & 3u))) & 3u) << (2u * s);
    return r;
}
__device__ __forceinline__ uint32_t wave_scan_maps(uint32_t v) {                    // inclusive, lane order
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d);
        if ((int)threadIdx.x >= d) v = map_then(o, v);
    }
    return v;
}
// the map of the lanes below this one (lane 0: the identity)
__device__ __forceinline__ uint32_t maps_below(uint32_t incl) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, 1);
    return threadIdx.x == 0 ? kMapIdentity : o;
}
// line i of n_lines: 0 = there is none, 1 = blank (logical length 0), 2 = any other
__device__ __forceinline__ uint32_t line_kind(const uint32_t *lstart, const unsigned char *cr, uint32_t i, uint32_t n_lines) {
    if (i >= n_lines) return 0u;
    return lstart[i + 1] - 1u - lstart[i] - (uint32_t)cr[i] == 0u ? 1u : 2u;
}

__global__ __launch_bounds__(64)
void ts_fastq_frame_kernel(const uint32_t *lstart, const unsigned char *cr, uint32_t n_lines, FastqFrame *frames) {
    uint32_t before = kMapIdentity, cnt[4] = {0u, 0u, 0u, 0u};
    for (uint32_t s = 0; s < kFastqSliceLines; s += 64u) {
        // (in 64 bits: the last slice of a chunk of nearly 2^32 lines would wrap; n_lines itself is no line)
        const unsigned long long at = (unsigned long long)blockIdx.x * kFastqSliceLines + s + threadIdx.x;
        const uint32_t i = at < n_lines ? (uint32_t)at : n_lines;
        const uint32_t kind = line_kind(lstart, cr, i, n_lines);
        const uint32_t incl = wave_scan_maps(kind == 0u ? kMapIdentity : kind == 1u ? kMapBlank : kMapLine);
        const uint32_t pre = map_then(before, maps_below(incl));
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) cnt[e] += (uint32_t)__popcll(ballot64(kind == 2u && ((pre >> (2u * e)) & 3u) == 0u));
        before = map_then(before, (uint32_t)__builtin_amdgcn_readlane((int)incl, 63));
    }
    if (threadIdx.x == 0) {
        FastqFrame f;
        f.map = before; f.cnt[0] = cnt[0]; f.cnt[1] = cnt[1]; f.cnt[2] = cnt[2]; f.cnt[3] = cnt[3]; f.pad[0] = f.pad[1] = f.pad[2] = 0u;
        frames[blockIdx.x] = f;
    }
}

// the slices' maps scanned from state 0 (one wave, 64 slices per step): every slice's entry state and first record
__global__ __launch_bounds__(64)
void ts_fastq_frame_scan_kernel(const FastqFrame *frames, uint32_t n_frames, const uint32_t *lstart, uint32_t newlines,
                                FastqEntry *entries, unsigned long long *out) {
    uint32_t state = 0, base = 0;
    for (uint32_t b = 0; b < n_frames; b += 64u) {
        const uint32_t i = b + threadIdx.x;
        const bool have = i < n_frames;
        const uint32_t incl = wave_scan_maps(have ? frames[i].map : kMapIdentity);
        const uint32_t in = (maps_below(incl) >> (2u * state)) & 3u;
        const uint32_t c = have ? frames[i].cnt[in] : 0u;
        const uint32_t sum = wave_scan_add(c);
        if (have) { FastqEntry e; e.state = in; e.base = base + sum - c; entries[i] = e; }
        state = ((uint32_t)__builtin_amdgcn_readlane((int)incl, 63) >> (2u * state)) & 3u;
        base += (uint32_t)__builtin_amdgcn_readlane((int)sum, 63);
    }
    if (threadIdx.x == 0) {
        out[kFqHeaders] = base; out[kFqError] = ~0ull; out[kFqOpen] = 0ull; out[kFqOpenOff] = 0ull; out[kFqLastLine] = lstart[newlines];
    }
}

__global__ __launch_bounds__(64)
void ts_fastq_records_kernel(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                             int at_end, const FastqEntry *entries, ts_fastq_record *recs, unsigned long long *out) {
    uint32_t state = entries[blockIdx.x].state, base = entries[blockIdx.x].base;
    for (uint32_t s = 0; s < kFastqSliceLines; s += 64u) {
        // (in 64 bits: the last slice of a chunk of nearly 2^32 lines would wrap; n_lines itself is no line)
        const unsigned long long at = (unsigned long long)blockIdx.x * kFastqSliceLines + s + threadIdx.x;
        const uint32_t i = at < n_lines ? (uint32_t)at : n_lines;
        const uint32_t kind = line_kind(lstart, cr, i, n_lines);
        const uint32_t incl = wave_scan_maps(kind == 0u ? kMapIdentity : kind == 1u ? kMapBlank : kMapLine);
        // (every lane takes part in the shuffle: a lane that sat out would hand its neighbour a zero map)
        const uint32_t below = maps_below(incl);
        const bool header = kind == 2u && ((below >> (2u * state)) & 3u) == 0u;
        const unsigned long long heads = ballot64(header);
        if (header) {
            const uint32_t r = base + (uint32_t)__popcll(heads & low_bits(threadIdx.x));
            const uint32_t s0 = lstart[i];
            if (n_lines - i < 4u) {                             // the lines ran out: the carry, or a truncated record
                out[kFqOpenOff] = s0;                           // (only the last header can be here)
                out[kFqOpen] = 1ull;
                if (at_end) atomicMin(&out[kFqError], (unsigned long long)r << 3 | TS_FASTQ_TRUNCATED);
            } else {
                const uint32_t s1 = lstart[i + 1], s2 = lstart[i + 2], s3 = lstart[i + 3], s4 = lstart[i + 4];
                ts_fastq_record rec;
                rec.off = s0; rec.seq_at = s1 - s0; rec.seq_len = s2 - 1u - s1; rec.size = s4 - 1u - s0; rec.seq_cr = cr[i + 1];
                recs[r] = rec;
                uint32_t bad = TS_FASTQ_OK;
                if (first[i] != '@') bad = TS_FASTQ_BAD_HEADER;
                else if (s3 - 1u - s2 == 0u || first[i + 2] != '+') bad = TS_FASTQ_BAD_SEPARATOR;
                else if (rec.seq_len - rec.seq_cr != s4 - 1u - s3 - (uint32_t)cr[i + 3]) bad = TS_FASTQ_BAD_LENGTHS;
                if (bad) atomicMin(&out[kFqError], (unsigned long long)r << 3 | bad);
            }
        }
        state = ((uint32_t)__builtin_amdgcn_readlane((int)incl, 63) >> (2u * state)) & 3u;
        base += (uint32_t)__popcll(heads);
    }
}

// a piece of a sequence line into a read batch's input buffer: a wave per job, 16 bytes per lane per store
__global__ __launch_bounds__(64)
void ts_fastq_stage_kernel(const unsigned char *plain, const FastqCopyJob *jobs, uint32_t n_jobs, unsigned char *in) {
    if (blockIdx.x >= n_jobs) return;
    const FastqCopyJob job = jobs[blockIdx.x];
    const unsigned char *src = plain + job.src;
    unsigned char *dst = in + job.dst;                          // 16-byte aligned
    for (uint32_t i = threadIdx.x * 16u; i < job.n; i += 1024u) {
        uint4 v = load16_any(src + i);
        const uint32_t left = job.n - i;
        if (left < 16u) {                                       // the bytes behind the read stay zero, as an upload leaves them
            uint32_t o[4] = {v.x, v.y, v.z, v.w};
            zero_tail16(o, left);
            v = make_uint4(o[0], o[1], o[2], o[3]);
        }
        *(uint4 *)(dst + i) = v;
    }
}

// ---- passing records, in input order, each with a '\n' behind it, to the places chunk.hip's plan gave them: a wave per record
__global__ __launch_bounds__(64)
void ts_fastq_gather_kernel(const unsigned char *plain, const ts_fastq_record *recs, const unsigned long long *dst_off,
                            unsigned long long n, unsigned long long cap, unsigned char *out) {
    const unsigned long long r = blockIdx.x;
    if (r >= n) return;
    const unsigned long long to = dst_off[r];
    if (to == ~0ull) return;
    const uint32_t size = recs[r].size;
    if (to > cap || 1ull + size > cap - to) return;             // (the caller has compared the total with cap already)
    const unsigned char *src = plain + recs[r].off;
    unsigned char *dst = out + to;
    copy_record16(dst, src, size, to);
    if (threadIdx.x == 63) dst[size] = '\n';
}

// ---- interleaved pairs (include/teloscan.h: "Interleaved paired FASTQ"): records 2 j and 2 j + 1 of the table are pair j
// The chunk's bytes for one lane, through the aligned dword that holds them, kept until another is asked for (a name is read in
// order).  The chunk's last dword, where the chunk ends inside it, is put together from the bytes that are the chunk's: no load
// touches a byte outside [0, n).
struct MateBytes {
    const unsigned char *plain;                                 // (dword aligned: the chunk's allocation)
    unsigned long long n;
    mutable unsigned long long at;
    mutable uint32_t w;
    __device__ __forceinline__ uint32_t byte(unsigned long long i) const {
        if (i >= n) return 0u;
        const unsigned long long a = i & ~3ull;
        if (a != at) {
            at = a;
            if (n - a >= 4ull) w = *(const uint32_t *)__builtin_assume_aligned(plain + a, 4);
            else {
                w = 0u;
                for (uint32_t k = 0; a + k < n; ++k) w |= (uint32_t)plain[a + k] << (8u * k);
            }
        }
        return (w >> (8u * (uint32_t)(i & 3ull))) & 255u;
    }
};

// a lane per pair: the lowest pair whose records are not mates, by a 64-bit atomic minimum (one atomic per wave)
__global__ __launch_bounds__(64)
void ts_fastq_mates_kernel(const unsigned char *plain, unsigned long long n_bytes, const ts_fastq_record *recs, unsigned long long n_pairs,
                           unsigned long long *lowest) {
    const unsigned long long j = (unsigned long long)blockIdx.x * 64u + threadIdx.x;
    bool bad = false;
    if (j < n_pairs) {
        const ts_fastq_record a = recs[2 * j], b = recs[2 * j + 1];
        const MateBytes ra{plain, n_bytes, ~0ull, 0u}, rb{plain, n_bytes, ~0ull, 0u};
        bad = !tspair::mates(ra, a.off, a.seq_at, rb, b.off, b.seq_at);
    }
    const unsigned long long wrong = ballot64(bad);
    if (wrong && threadIdx.x == (uint32_t)__builtin_ctzll(wrong)) atomicMin(lowest, j);
}

// a lane per pair: both records' bytes of pair_pass are 1 when either mate's own pass byte is set (read_of: a record's index in
// pass, ~0 when it was not judged)
__global__ __launch_bounds__(64)
void ts_fastq_pair_pass_kernel(const uint32_t *read_of, const unsigned char *pass, unsigned long long n_pairs, unsigned char *pair_pass) {
    const unsigned long long j = (unsigned long long)blockIdx.x * 64u + threadIdx.x;
    if (j >= n_pairs) return;
    const uint32_t a = read_of[2 * j], b = read_of[2 * j + 1];
    const bool keep = (a != 0xffffffffu && pass[a] != 0) || (b != 0xffffffffu && pass[b] != 0);
    pair_pass[2 * j] = pair_pass[2 * j + 1] = keep ? 1 : 0;
}

}  // namespace

extern "C" {

int ts_k_launch_fastq_mates(const void *plain, unsigned long long n_bytes, const void *recs, unsigned long long n_pairs,
                            unsigned long long *lowest, void *stream) {
    if (n_pairs == 0) return 0;
    hipLaunchKernelGGL(ts_fastq_mates_kernel, dim3((unsigned)((n_pairs + 63u) / 64u)), dim3(64), 0, (hipStream_t)stream,
                       (const unsigned char *)plain, n_bytes, (const ts_fastq_record *)recs, n_pairs, lowest);
    return (int)hipGetLastError();
}

int ts_k_launch_fastq_pair_pass(const void *read_of, const void *pass, unsigned long long n_pairs, void *pair_pass, void *stream) {
    if (n_pairs == 0) return 0;
    hipLaunchKernelGGL(ts_fastq_pair_pass_kernel, dim3((unsigned)((n_pairs + 63u) / 64u)), dim3(64), 0, (hipStream_t)stream,
                       (const uint32_t *)read_of, (const unsigned char *)pass, n_pairs, (unsigned char *)pair_pass);
    return (int)hipGetLastError();
}

int ts_k_launch_fastq_frames(const uint32_t *lstart, const unsigned char *cr, uint32_t n_lines, uint32_t newlines, void *frames,
                             void *entries, unsigned long long *out, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kFastqSliceLines - 1) / kFastqSliceLines);
    if (nf) hipLaunchKernelGGL(ts_fastq_frame_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, lstart, cr, n_lines, (FastqFrame *)frames);
    hipLaunchKernelGGL(ts_fastq_frame_scan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const FastqFrame *)frames, nf, lstart,
                       newlines, (FastqEntry *)entries, out);
    return (int)hipGetLastError();
}

int ts_k_launch_fastq_records(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                              int at_end, const void *entries, void *recs, unsigned long long *out, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kFastqSliceLines - 1) / kFastqSliceLines);
    if (nf == 0) return 0;
    hipLaunchKernelGGL(ts_fastq_records_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, lstart, first, cr, n_lines, at_end,
                       (const FastqEntry *)entries, (ts_fastq_record *)recs, out);
    return (int)hipGetLastError();
}

int ts_k_launch_fastq_stage(const void *plain, const void *jobs, uint32_t n_jobs, void *in, void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_fastq_stage_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain,
                       (const FastqCopyJob *)jobs, n_jobs, (unsigned char *)in);
    return (int)hipGetLastError();
}

int ts_k_launch_fastq_gather(const void *plain, const void *recs, const void *dst_off, unsigned long long n, unsigned long long cap,
                             void *out, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(ts_fastq_gather_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain,
                       (const ts_fastq_record *)recs, (const unsigned long long *)dst_off, n, cap, (unsigned char *)out);
    return (int)hipGetLastError();
}

}  // extern "C"
