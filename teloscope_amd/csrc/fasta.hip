// fasta.hip — FASTA text of a resident chunk (chunk_internal.h) turned into a record table, the records' header lines, their
// bases joined into one buffer and the runs of gap letters, on the device.  One-wave workgroups throughout, like fastq.hip's.
// The chunk layer's line index (chunk.hip) runs in front of everything here; the sums of the counts are its scan.
//
//   * records: a header line is a line whose first byte is '>'.  A wave per 2 048 lines counts the header lines, the lines
//     that end in "\r\n" and the bytes of the headers' names; one wave sums the counts; a second pass gives every header line
//     its index and the two sums in front of it.  A record's text runs to the next header line, and its number of bases
//     follows from the line index alone: the body's bytes, less one '\n' per body line, less the body lines' '\r'.
//   * join: stream compaction.  The body text is cut at multiples of 16 KB into jobs; a first pass counts every job's kept
//     bytes (not '\n', not a '\r' in front of one or at the input's very end), one wave sums the counts, and the write pass
//     takes 16 source bytes per lane, places the wave's kept bytes in LDS by a DPP prefix sum of the lanes' counts and stores
//     aligned 16-byte rows, 1 KB at a time.  Every byte is read once and written once; there are no per-line copies.
//   * stage: the join's masks and write pass with a read batch's segments as the places (ts_fasta_chunk_stage).  A record inside
//     one slice is one job and is read once, without a count; the jobs of a record that crosses a slice are counted and summed
//     per record, a wave per record.
//   * runs: the same shape over the joined bytes with another predicate: a run starts where "is a gap letter" differs from
//     the byte before, or where a record starts.
//   * strict: the filtered loader's one question about a body (does it hold a byte that is no line end?), the count pass's
//     jobs with a third predicate and no sum: a byte per record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teloscan.h"
#include "chunk_device.h"
#include "fasta_internal.h"
#include "ts_device.h"

namespace {

// bits [lo, hi) of a 16-bit mask (0 <= lo, hi <= 16)
__device__ __forceinline__ uint32_t bit_range(uint32_t lo, uint32_t hi) { return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u; }

// ---- records
__device__ __forceinline__ void line_facts(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t i,
                                           uint32_t n_lines, uint32_t &head, uint32_t &c, uint32_t &name) {
    head = 0u; c = 0u; name = 0u;
    if (i >= n_lines) return;
    c = cr[i];
    if (first[i] == '>') { head = 1u; name = lstart[i + 1] - 1u - lstart[i] - c - 1u; }    // without '>', '\n' and the '\r'
}

__global__ __launch_bounds__(64)
void ts_fasta_frame_kernel(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                           FastaFrame *frames) {
    uint32_t heads = 0, crs = 0, names = 0;
    for (uint32_t s = 0; s < kFastaSliceLines; s += 64u) {
        // (in 64 bits: the last slice of a chunk of nearly 2^32 lines would wrap)
        const unsigned long long at = (unsigned long long)blockIdx.x * kFastaSliceLines + s + threadIdx.x;
        uint32_t h, c, nb;
        line_facts(lstart, first, cr, at < n_lines ? (uint32_t)at : n_lines, n_lines, h, c, nb);
        heads += h; crs += c; names += nb;
    }
    heads = wave_total(heads); crs = wave_total(crs); names = wave_total(names);
    if (threadIdx.x == 0) { FastaFrame f; f.headers = heads; f.crs = crs; f.name_bytes = names; f.pad = 0u; frames[blockIdx.x] = f; }
}

// the slices' sums -> the sums before every slice, in place (one wave, 64 slices per step)
__global__ __launch_bounds__(64)
void ts_fasta_frame_scan_kernel(FastaFrame *frames, uint32_t n_frames, const uint32_t *lstart, uint32_t newlines,
                                unsigned long long *out) {
    uint32_t heads = 0, crs = 0, names = 0;
    for (uint32_t b = 0; b < n_frames; b += 64u) {
        const uint32_t i = b + threadIdx.x;
        FastaFrame f; f.headers = f.crs = f.name_bytes = f.pad = 0u;
        if (i < n_frames) f = frames[i];
        const uint32_t ih = wave_scan_add(f.headers), ic = wave_scan_add(f.crs), in = wave_scan_add(f.name_bytes);
        if (i < n_frames) {
            FastaFrame g; g.headers = heads + ih - f.headers; g.crs = crs + ic - f.crs; g.name_bytes = names + in - f.name_bytes; g.pad = 0u;
            frames[i] = g;
        }
        heads += (uint32_t)__builtin_amdgcn_readlane((int)ih, 63);
        crs += (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
        names += (uint32_t)__builtin_amdgcn_readlane((int)in, 63);
    }
    if (threadIdx.x == 0) { out[kFaHeaders] = heads; out[kFaCrs] = crs; out[kFaNameBytes] = names; out[kFaLastLine] = lstart[newlines]; }
}

__global__ __launch_bounds__(64)
void ts_fasta_heads_kernel(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                           const FastaFrame *frames, FastaHead *heads, uint32_t n_heads, uint32_t all_crs, uint32_t all_names) {
    const FastaFrame f = frames[blockIdx.x];
    uint32_t r0 = f.headers, c0 = f.crs, b0 = f.name_bytes;
    for (uint32_t s = 0; s < kFastaSliceLines; s += 64u) {
        const unsigned long long at = (unsigned long long)blockIdx.x * kFastaSliceLines + s + threadIdx.x;
        const uint32_t i = at < n_lines ? (uint32_t)at : n_lines;
        uint32_t h, c, nb;
        line_facts(lstart, first, cr, i, n_lines, h, c, nb);
        const uint32_t ih = wave_scan_add(h), ic = wave_scan_add(c), in = wave_scan_add(nb);
        const uint32_t r = r0 + ih - h;
        if (h && r < n_heads) {                                 // (always: the count pass saw the same lines)
            FastaHead e; e.line = i; e.crs_before = c0 + ic - c; e.names_before = b0 + in - nb; e.pad = 0u;
            heads[r] = e;
        }
        r0 += (uint32_t)__builtin_amdgcn_readlane((int)ih, 63);
        c0 += (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
        b0 += (uint32_t)__builtin_amdgcn_readlane((int)in, 63);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { FastaHead e; e.line = n_lines; e.crs_before = all_crs; e.names_before = all_names; e.pad = 0u; heads[n_heads] = e; }
}

// a lane per record: from its header line to the next one's (the sentinel: the end of the lines)
__global__ __launch_bounds__(64)
void ts_fasta_records_kernel(unsigned long long size, const uint32_t *lstart, const unsigned char *cr, const FastaHead *heads,
                             uint32_t n_heads, ts_fasta_record *recs) {
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= n_heads) return;
    const FastaHead a = heads[r], b = heads[r + 1u];
    // (a last line without '\n' ends at size + 1 in the index, as if it had one: the sums below count that '\n' like any other)
    const uint32_t l0 = lstart[a.line], l1 = lstart[a.line + 1u], e = lstart[b.line], crh = cr[a.line];
    const uint32_t end = e < size ? e : (uint32_t)size, body = l1 < size ? l1 : (uint32_t)size;
    ts_fasta_record rec;
    rec.off = l0;
    rec.text_len = end - l0;
    rec.body_at = body - l0;
    rec.n_bases = (e - l1) - (b.line - a.line - 1u) - (b.crs_before - a.crs_before - crh);
    rec.name_at = a.names_before;
    rec.name_len = l1 - 1u - l0 - crh - 1u;
    rec.reserved = 0u;
    recs[r] = rec;
}

// a wave per record: its header line without the '>' and the line end
__global__ __launch_bounds__(64)
void ts_fasta_names_kernel(const unsigned char *plain, unsigned long long size, const ts_fasta_record *recs, uint32_t n_heads,
                           unsigned char *names) {
    if (blockIdx.x >= n_heads) return;
    const ts_fasta_record rec = recs[blockIdx.x];
    const unsigned long long from = rec.off + 1ull;
    for (uint32_t i = threadIdx.x; i < rec.name_len; i += 64u)
        if (from + i < size) names[rec.name_at + i] = plain[from + i];
}

// ---- join
// The kept bytes among the 16 at plain + p (p: a multiple of 16) that lie in [a, z), z <= size, as a mask; q = the 16 bytes.
// Dropped: '\n'; a '\r' whose next byte is a '\n' of the chunk; a '\r' that is the input's last byte.
__device__ __forceinline__ uint32_t keep_mask16(const unsigned char *plain, unsigned long long p, unsigned long long a,
                                                unsigned long long z, unsigned long long size, int at_end, uint4 &q) {
    q = make_uint4(0u, 0u, 0u, 0u);
    if (p >= z || p + 16ull <= a) return 0u;
    q = *(const uint4 *)(plain + p);                           // (the chunk's buffer is readable 64 bytes beyond its capacity)
    const uint32_t in_chunk = size - p >= 16ull ? 0xffffu : (1u << (uint32_t)(size - p)) - 1u;
    const uint32_t lf = byte_eq_mask16(q, 0x0a0a0a0au) & in_chunk, cr = byte_eq_mask16(q, 0x0d0d0d0du);
    const uint32_t lf_next = (lf >> 1) | (p + 16ull < size && plain[p + 16ull] == '\n' ? 0x8000u : 0u);
    uint32_t drop = lf | (cr & lf_next);
    if (at_end && size - 1ull >= p && size - 1ull < p + 16ull) drop |= cr & (1u << (uint32_t)(size - 1ull - p));
    const uint32_t lo = a > p ? (uint32_t)(a - p) : 0u, hi = z - p >= 16ull ? 16u : (uint32_t)(z - p);
    return ~drop & bit_range(lo, hi);
}

// the kept bytes of a job's body text (the wave's total, in every lane)
__device__ __forceinline__ uint32_t job_kept(const unsigned char *plain, unsigned long long size, int at_end, const FastaJoinJob &job) {
    const unsigned long long a = job.a, z = job.z < size ? job.z : size;
    uint32_t c = 0;
    for (unsigned long long p0 = a & ~15ull; p0 < z; p0 += 1024ull) {
        uint4 q;
        c += __popc(keep_mask16(plain, p0 + threadIdx.x * 16u, a, z, size, at_end, q));
    }
    return wave_total(c);
}

__global__ __launch_bounds__(64)
void ts_fasta_join_count_kernel(const unsigned char *plain, unsigned long long size, int at_end, const FastaJoinJob *jobs,
                                uint32_t n_jobs, uint32_t *counts) {
    if (blockIdx.x >= n_jobs) return;
    const uint32_t c = job_kept(plain, size, at_end, jobs[blockIdx.x]);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// rows [0, upto) of the staged bytes to out + base (base: a multiple of 16), a 16-byte row per lane; bytes below `lo` (what the
// record's previous job wrote) and at or beyond `limit` (not this record's) are not touched
__device__ __forceinline__ void flush_rows(const unsigned char *buf, unsigned char *out, unsigned long long base, uint32_t lo,
                                           uint32_t upto, unsigned long long limit) {
    const uint32_t b0 = threadIdx.x * 16u;
    if (b0 >= upto) return;
    const uint32_t b1 = b0 + 16u < upto ? b0 + 16u : upto, s = b0 > lo ? b0 : lo;
    if (s == b0 && b1 == b0 + 16u && base + b1 <= limit) { *(uint4 *)(out + base + b0) = *(const uint4 *)(buf + b0); return; }
    for (uint32_t k = s; k < b1; ++k) if (base + k < limit) out[base + k] = buf[k];
}

// a job's kept bytes to out + dst and on, through buf (2 048 bytes of LDS, 16-byte aligned): the write pass of the join and of
// the read stage
__device__ __forceinline__ void job_write(const unsigned char *plain, unsigned long long size, int at_end, const FastaJoinJob &job,
                                          unsigned long long dst, unsigned char *out, unsigned char *buf) {
    const unsigned long long a = job.a, z = job.z < size ? job.z : size;
    uint32_t lo = (uint32_t)(dst & 15ull), fill = lo;          // buf[k] goes to out[base + k]
    unsigned long long base = dst - lo;
    for (unsigned long long p0 = a & ~15ull; p0 < z; p0 += 1024ull) {
        uint4 q;
        const uint32_t m = keep_mask16(plain, p0 + threadIdx.x * 16u, a, z, size, at_end, q);
        const uint32_t c = __popc(m), incl = wave_scan_add(c);
        uint32_t pos = fill + incl - c;                         // (fill < 1024 here, at most 1024 more: inside buf)
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b)
            if ((m >> b) & 1u) buf[pos++] = (unsigned char)(w[b >> 2] >> (8u * (b & 3u)));
        fill += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        __syncthreads();
        if (fill >= 1024u) {                                    // (wave-uniform)
            flush_rows(buf, out, base, lo, 1024u, job.limit);
            const uint4 rest = *(const uint4 *)(buf + 1024u + threadIdx.x * 16u);
            __syncthreads();
            *(uint4 *)(buf + threadIdx.x * 16u) = rest;
            __syncthreads();
            base += 1024ull; fill -= 1024u; lo = 0u;
        }
    }
    flush_rows(buf, out, base, lo, fill, job.limit);
    // the bytes between this record and the next one's 16-byte aligned start are zero, whatever the buffer held before
    if (job.last && threadIdx.x < (uint32_t)(-job.limit & 15ull)) out[job.limit + threadIdx.x] = 0;
}

__global__ __launch_bounds__(64)
void ts_fasta_join_write_kernel(const unsigned char *plain, unsigned long long size, int at_end, const FastaJoinJob *jobs,
                                uint32_t n_jobs, const uint32_t *sums, unsigned char *joined) {
    __shared__ __attribute__((aligned(16))) unsigned char buf[2048];
    if (blockIdx.x >= n_jobs) return;
    const FastaJoinJob job = jobs[blockIdx.x];
    job_write(plain, size, at_end, job, job.dst_rec + (sums[blockIdx.x] - sums[job.first]), joined, buf);
}

// ---- stage (ts_fasta_chunk_stage): the join's jobs with a read batch's segments as their places.  Reads are many and short: a
// record that lies inside one slice is one job, needs no count and no sum, and its text is read once; only the jobs of a record
// that crosses a slice are counted, and their sums are taken per record, a wave each, not over the whole list.
__global__ __launch_bounds__(64)
void ts_fasta_stage_count_kernel(const unsigned char *plain, unsigned long long size, int at_end, const FastaJoinJob *jobs,
                                 uint32_t n_jobs, uint32_t *counts) {
    if (blockIdx.x >= n_jobs) return;
    const FastaJoinJob job = jobs[blockIdx.x];
    if (job.first == blockIdx.x && job.last) return;           // (the record's only job: it goes to the segment's start)
    const uint32_t c = job_kept(plain, size, at_end, job);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// a wave per record of several jobs: its jobs' counts -> the counts before each, in place (64 jobs per step)
__global__ __launch_bounds__(64)
void ts_fasta_stage_scan_kernel(const FastaStageSpan *spans, uint32_t n_spans, uint32_t *counts) {
    if (blockIdx.x >= n_spans) return;
    const FastaStageSpan s = spans[blockIdx.x];
    uint32_t before = 0;
    for (uint32_t b = 0; b < s.n; b += 64u) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t c = i < s.n ? counts[s.first + i] : 0u;
        const uint32_t incl = wave_scan_add(c);
        if (i < s.n) counts[s.first + i] = before + incl - c;
        before += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
}

__global__ __launch_bounds__(64)
void ts_fasta_stage_write_kernel(const unsigned char *plain, unsigned long long size, int at_end, const FastaJoinJob *jobs,
                                 uint32_t n_jobs, const uint32_t *sums, unsigned char *in) {
    __shared__ __attribute__((aligned(16))) unsigned char buf[2048];
    if (blockIdx.x >= n_jobs) return;
    const FastaJoinJob job = jobs[blockIdx.x];
    const uint32_t before = job.first == blockIdx.x ? 0u : sums[blockIdx.x];
    job_write(plain, size, at_end, job, job.dst_rec + before, in, buf);
}

// ---- runs
// gap letters (N n X x) among the 16 joined bytes at p, as a mask
__device__ __forceinline__ uint32_t gap_mask16(uint4 q) {
    const uint4 f = make_uint4(q.x | 0x20202020u, q.y | 0x20202020u, q.z | 0x20202020u, q.w | 0x20202020u);
    return byte_eq_mask16(f, 0x6e6e6e6eu) | byte_eq_mask16(f, 0x78787878u);
}
__device__ __forceinline__ bool is_gap(unsigned char c) { c |= 0x20; return c == 'n' || c == 'x'; }
// the run starts among the 16 joined bytes at p (a multiple of 16, inside [a, z) rounded to 16); g = their gap mask
__device__ __forceinline__ uint32_t run_starts16(const unsigned char *joined, unsigned long long p, const FastaRunJob &job, uint32_t &g) {
    g = 0u;
    if (p >= job.z || p < job.a) return 0u;
    g = gap_mask16(*(const uint4 *)(joined + p));              // (the joined buffer is readable 64 bytes beyond its end)
    const uint32_t before = p > job.rec_begin ? (is_gap(joined[p - 1ull]) ? 1u : 0u) : (~g & 1u);   // a record's first base starts a run
    const uint32_t hi = job.z - p >= 16ull ? 16u : (uint32_t)(job.z - p);
    return (g ^ ((g << 1) | before)) & bit_range(0u, hi);
}

__global__ __launch_bounds__(64)
void ts_fasta_run_count_kernel(const unsigned char *joined, const FastaRunJob *jobs, uint32_t n_jobs, uint32_t *counts) {
    if (blockIdx.x >= n_jobs) return;
    const FastaRunJob job = jobs[blockIdx.x];
    uint32_t c = 0;
    for (unsigned long long p0 = job.a; p0 < job.z; p0 += 1024ull) {
        uint32_t g;
        c += __popc(run_starts16(joined, p0 + threadIdx.x * 16u, job, g));
    }
    c = wave_total(c);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(64)
void ts_fasta_run_write_kernel(const unsigned char *joined, const FastaRunJob *jobs, uint32_t n_jobs, const uint32_t *sums,
                               ts_fasta_run *runs, unsigned long long n_runs) {
    if (blockIdx.x >= n_jobs) return;
    const FastaRunJob job = jobs[blockIdx.x];
    unsigned long long run = sums[blockIdx.x];
    for (unsigned long long p0 = job.a; p0 < job.z; p0 += 1024ull) {
        const unsigned long long p = p0 + threadIdx.x * 16u;
        uint32_t g;
        uint32_t m = run_starts16(joined, p, job, g);
        const uint32_t c = __popc(m), incl = wave_scan_add(c);
        unsigned long long k = run + incl - c;
        while (m) {
            const uint32_t b = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            if (k < n_runs) {                                   // (always: the count pass saw the same bytes)
                ts_fasta_run r; r.record = job.rec; r.is_gap = (g >> b) & 1u; r.start = (uint32_t)(p + b - job.rec_begin); r.len = 0u;
                runs[k] = r;
            }
            ++k;
        }
        run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
}

// a lane per run: it ends where the record's next run starts, the record's last one where the record ends
__global__ __launch_bounds__(64)
void ts_fasta_run_lengths_kernel(ts_fasta_run *runs, unsigned long long n_runs, const ts_fasta_record *recs, uint32_t n_recs) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 64ull + threadIdx.x;
    if (i >= n_runs) return;
    const uint32_t rec = runs[i].record, start = runs[i].start;
    uint32_t end = rec < n_recs ? recs[rec].n_bases : start;
    if (i + 1ull < n_runs && runs[i + 1ull].record == rec) end = runs[i + 1ull].start;
    runs[i].len = end - start;
}

// ---- strict
// a wave per job: does body text [a, z) hold a byte other than '\n' and '\r'?  1 KB per step; the first step that holds one
// ends the job (most bodies: the first)
__global__ __launch_bounds__(64)
void ts_fasta_strict_kernel(const unsigned char *plain, unsigned long long size, const FastaStrictJob *jobs, uint32_t n_jobs,
                            unsigned char *has) {
    if (blockIdx.x >= n_jobs) return;
    const FastaStrictJob job = jobs[blockIdx.x];
    const unsigned long long a = job.a, z = job.z < size ? job.z : size;
    for (unsigned long long p0 = a & ~15ull; p0 < z; p0 += 1024ull) {
        const unsigned long long p = p0 + threadIdx.x * 16u;
        uint32_t m = 0u;
        if (p < z && p + 16ull > a) {
            const uint4 q = *(const uint4 *)(plain + p);       // (the chunk's buffer is readable 64 bytes beyond its capacity)
            const uint32_t lo = a > p ? (uint32_t)(a - p) : 0u, hi = z - p >= 16ull ? 16u : (uint32_t)(z - p);
            m = ~(byte_eq_mask16(q, 0x0a0a0a0au) | byte_eq_mask16(q, 0x0d0d0d0du)) & bit_range(lo, hi);
        }
        if (ballot64(m != 0u) != 0ull) {                        // (wave-uniform; every job of the record stores the same byte)
            if (threadIdx.x == 0) has[job.rec] = 1;
            return;
        }
    }
}

}  // namespace

extern "C" {

int ts_k_launch_fasta_strict(const void *plain, unsigned long long size, const void *jobs, uint32_t n_jobs, unsigned char *has,
                             void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_strict_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, size,
                       (const FastaStrictJob *)jobs, n_jobs, has);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_frames(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                             uint32_t newlines, void *frames, unsigned long long *out, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kFastaSliceLines - 1) / kFastaSliceLines);
    if (nf) hipLaunchKernelGGL(ts_fasta_frame_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, lstart, first, cr, n_lines, (FastaFrame *)frames);
    hipLaunchKernelGGL(ts_fasta_frame_scan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (FastaFrame *)frames, nf, lstart, newlines, out);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_heads(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                            const void *frames, void *heads, uint32_t n_heads, uint32_t crs, uint32_t name_bytes, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kFastaSliceLines - 1) / kFastaSliceLines);
    if (nf == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_heads_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, lstart, first, cr, n_lines,
                       (const FastaFrame *)frames, (FastaHead *)heads, n_heads, crs, name_bytes);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_records(const void *plain, unsigned long long size, const uint32_t *lstart, const unsigned char *cr,
                              const void *heads, uint32_t n_heads, void *recs, void *names, void *stream) {
    if (n_heads == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_records_kernel, dim3((n_heads + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, size, lstart, cr,
                       (const FastaHead *)heads, n_heads, (ts_fasta_record *)recs);
    hipLaunchKernelGGL(ts_fasta_names_kernel, dim3(n_heads), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, size,
                       (const ts_fasta_record *)recs, n_heads, (unsigned char *)names);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_join_count(const void *plain, unsigned long long size, int at_end, const void *jobs, uint32_t n_jobs,
                                 uint32_t *counts, void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_join_count_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, size,
                       at_end, (const FastaJoinJob *)jobs, n_jobs, counts);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_join_write(const void *plain, unsigned long long size, int at_end, const void *jobs, uint32_t n_jobs,
                                 const uint32_t *sums, void *joined, void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_join_write_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, size,
                       at_end, (const FastaJoinJob *)jobs, n_jobs, sums, (unsigned char *)joined);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_stage(const void *plain, unsigned long long size, int at_end, const void *jobs, uint32_t n_jobs,
                            const void *spans, uint32_t n_spans, uint32_t *counts, void *in, void *stream) {
    if (n_jobs == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_spans) {
        hipLaunchKernelGGL(ts_fasta_stage_count_kernel, dim3(n_jobs), dim3(64), 0, st, (const unsigned char *)plain, size, at_end,
                           (const FastaJoinJob *)jobs, n_jobs, counts);
        hipLaunchKernelGGL(ts_fasta_stage_scan_kernel, dim3(n_spans), dim3(64), 0, st, (const FastaStageSpan *)spans, n_spans, counts);
    }
    hipLaunchKernelGGL(ts_fasta_stage_write_kernel, dim3(n_jobs), dim3(64), 0, st, (const unsigned char *)plain, size, at_end,
                       (const FastaJoinJob *)jobs, n_jobs, counts, (unsigned char *)in);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_run_count(const void *joined, const void *jobs, uint32_t n_jobs, uint32_t *counts, void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_run_count_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)joined,
                       (const FastaRunJob *)jobs, n_jobs, counts);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_run_write(const void *joined, const void *jobs, uint32_t n_jobs, const uint32_t *sums, void *runs,
                                unsigned long long n_runs, void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_run_write_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)joined,
                       (const FastaRunJob *)jobs, n_jobs, sums, (ts_fasta_run *)runs, n_runs);
    return (int)hipGetLastError();
}

int ts_k_launch_fasta_run_lengths(void *runs, unsigned long long n_runs, const void *recs, uint32_t n_recs, void *stream) {
    if (n_runs == 0) return 0;
    hipLaunchKernelGGL(ts_fasta_run_lengths_kernel, dim3((unsigned)((n_runs + 63ull) / 64ull)), dim3(64), 0, (hipStream_t)stream,
                       (ts_fasta_run *)runs, n_runs, (const ts_fasta_record *)recs, n_recs);
    return (int)hipGetLastError();
}

}  // extern "C"
