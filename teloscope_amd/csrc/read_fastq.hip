// read_fastq.hip — the kept records of a BAM or SAM chunk as FASTQ text, formatted where the chunk lies (ts_bam_chunk_gather_fastq,
// ts_sam_chunk_gather_fastq; host side read_fastq.cpp).  The output is this project's own (include/teloscan.h: "FASTQ out of the
// BAM and SAM subsets").  Where a record's fields lie and every byte of its text are read_fastq_format_core.h, shared with the
// host routes and with the host program that checks it against Python; this file is the data movement around it:
//
//   ts_read_fastq_sizes  a lane per record: a kept record's table entry (name, SEQ, QUAL, L, reverse, QUAL missing) and the
//                        bytes of its text, name_len + 2 L + 6; 0 when its pass byte is clear;
//   ts_read_fastq_plan   one wave, 64 records per step: prefix sums of the sizes (where a record's text starts) and of the
//                        pieces it is cut into (its first job), the totals.  No atomics: the text's order is the records' order;
//   ts_read_fastq_jobs   a lane per kept record writes its jobs, so that a read of 100 kb is spread over many waves;
//   ts_read_fastq_write  a wave per job.  Pieces are cut at 16-byte boundaries of the output, so a lane's 16 bytes are one aligned
//                        store everywhere but at a record's two ends, where the bytes go out one by one: nothing is stored
//                        outside a record's text.  16 bytes that lie inside the bases or inside the quals are made from aligned
//                        dword loads: BAM bases from nibbles through v_perm_b32 and a letter table (bgzf.hip's decode), a second
//                        table and the reversed byte order for the reverse strand; BAM quals by a saturating add; SAM by byte
//                        copies, reversed and complemented through a table in LDS.  16 bytes that touch the name or a line end
//                        are out_byte's.
//
// Loads: the aligned dwords that hold the bytes wanted (chunk_device.h's load16_any, and three dwords for nine packed bytes).  They
// reach at most 19 bytes beyond a field's last byte, inside the 64 readable bytes behind a chunk's capacity, and never lie in front
// of the field's first byte rounded down to a dword: the backward reads of the reverse form start at the field's base or behind it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk_device.h"
#include "read_fastq_internal.h"
#include "ts_device.h"

namespace {

typedef unsigned long long u64;

struct ChunkBytes {
    const unsigned char *p;
    __device__ __forceinline__ uint32_t byte(u64 i) const { return p[i]; }
};

// the record tables' entries, as include/teloscan.h lays them out (24 bytes each)
struct RecSam { u64 off; uint32_t seq_at, seq_len, size, flags; };
struct RecBam { u64 off; uint32_t block_size, seq_at, l_seq, reserved; };

__device__ __forceinline__ uint32_t pieces_of(u64 size, u64 to) {
    return size ? (uint32_t)((size + (to & 15ull) + tsfq::kPieceBytes - 1ull) / tsfq::kPieceBytes) : 0u;
}

__global__ __launch_bounds__(64)
void ts_read_fastq_sizes(const TsFastqOutParams P) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= P.n) return;
    u64 size = 0;
    if (P.pass[i]) {
        const ChunkBytes bytes{P.chunk};
        tsfq::Rec r;
        if (P.kind == tsfq::kSam) {
            const RecSam s = ((const RecSam *)P.recs)[i];
            r = tsfq::sam_locate(bytes, s.off, s.seq_at, s.seq_len, s.size, P.out_flags);
        } else {
            const RecBam b = ((const RecBam *)P.recs)[i];
            r = tsfq::bam_locate(bytes, b.off, b.block_size, b.seq_at, b.l_seq, P.out_flags);
        }
        P.table[i] = r;
        size = tsfq::record_len(r);
    }
    P.sizes[i] = size;
}

__global__ __launch_bounds__(64)
void ts_read_fastq_plan(const TsFastqOutParams P) {
    u64 run = 0, kept = 0, jobs = 0;
    for (u64 base = 0; base < P.n; base += 64ull) {
        const u64 i = base + threadIdx.x;
        const u64 size = i < P.n ? P.sizes[i] : 0ull;
        u64 total = 0;
        const u64 to = run + wave_excl_scan_u64(size, &total);
        const uint32_t pieces = pieces_of(size, to), incl = wave_scan_add(pieces);
        if (i < P.n) {
            P.dst_off[i] = size ? to : ~0ull;
            P.job_base[i] = (uint32_t)jobs + incl - pieces;
        }
        run += total;
        jobs += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        kept += (u64)__popcll(ballot64(size != 0ull));
    }
    if (threadIdx.x == 0) { P.totals[kFqBytes] = run; P.totals[kFqKept] = kept; P.totals[kFqJobs] = jobs; }
}

__global__ __launch_bounds__(64)
void ts_read_fastq_jobs(const TsFastqOutParams P) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= P.n) return;
    const u64 size = P.sizes[i];
    if (!size) return;
    const uint32_t pieces = pieces_of(size, P.dst_off[i]), first = P.job_base[i];
    for (uint32_t p = 0; p < pieces; ++p)
        if (first + p < P.n_jobs) P.jobs[first + p] = TsFastqOutJob{i, p};     // (always: the plan counted the same pieces)
}

// ---- 16 bytes of the interior of a field
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_amdgcn_perm(0u, x, 0x00010203u); }
__device__ __forceinline__ uint4 reversed16(uint4 v) { return make_uint4(bswap(v.w), bswap(v.z), bswap(v.y), bswap(v.x)); }

// four codes 0..15, one per byte -> their letters, or the letters of the codes with their bits reversed
template <bool Comp>
__device__ __forceinline__ uint32_t letters(uint32_t x) {
    // "=ACM" "GRSV" "TWYH" "KDBN", and "=TGK" "CYSB" "AWRD" "MHVN"
    const uint32_t t0 = Comp ? 0x4b47543du : 0x4d43413du, t1 = Comp ? 0x42535943u : 0x56535247u;
    const uint32_t t2 = Comp ? 0x44525741u : 0x48595754u, t3 = Comp ? 0x4e56484du : 0x4e42444bu;
    const uint32_t sel = x & 0x07070707u;
    const uint32_t a = __builtin_amdgcn_perm(t1, t0, sel), b = __builtin_amdgcn_perm(t3, t2, sel);
    const uint32_t m = ((x >> 3) & 0x01010101u) * 0xffu;
    return (a & ~m) | (b & m);
}

// the codes of bases i0 .. i0 + 15 of the packed SEQ at seq, one per byte: nine bytes from three aligned dwords
__device__ __forceinline__ uint4 codes16(const unsigned char *seq, uint32_t i0) {
    const uintptr_t a = (uintptr_t)(seq + i0 / 2u);
    const uint32_t *q = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3u);
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
    const uint32_t b[3] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), w2 >> (8u * sh)};
    const bool odd = (i0 & 1u) != 0u;
    uint32_t c[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t hi = (b[h] >> 4) & 0x0f0f0f0fu, lo = b[h] & 0x0f0f0f0fu;
        const uint32_t hi_next = (__builtin_amdgcn_alignbyte(b[h + 1], b[h], 1u) >> 4) & 0x0f0f0f0fu;
        // an even start reads high nibble, low nibble; an odd one low nibble, the next byte's high nibble
        const uint32_t first = odd ? lo : hi, second = odd ? hi_next : lo;
        c[2 * h] = __builtin_amdgcn_perm(second, first, 0x05010400u);
        c[2 * h + 1] = __builtin_amdgcn_perm(second, first, 0x07030602u);
    }
    return make_uint4(c[0], c[1], c[2], c[3]);
}

// min(byte, 93) + 33 in every byte: bit 7 of `over` marks the bytes of 94 and more (no carry leaves a byte)
__device__ __forceinline__ uint32_t qual_sat(uint32_t x) {
    const uint32_t over = (((x & 0x7f7f7f7fu) + 0x22222222u) | x) & 0x80808080u;
    const uint32_t m = (over >> 7) * 0xffu;
    return ((x & ~m) | (0x5d5d5d5du & m)) + 0x21212121u;
}

__device__ __forceinline__ uint32_t comp4(const unsigned char *comp, uint32_t x) {
    return (uint32_t)comp[x & 255u] | (uint32_t)comp[(x >> 8) & 255u] << 8 | (uint32_t)comp[(x >> 16) & 255u] << 16 | (uint32_t)comp[x >> 24] << 24;
}

// bases j .. j + 15 of the text (j + 16 <= L)
__device__ __forceinline__ uint4 bases16(const unsigned char *chunk, const tsfq::Rec &r, uint32_t j, const unsigned char *comp) {
    const bool rev = (r.flags & tsfq::kReverse) != 0u;
    const uint32_t i0 = rev ? r.len - 16u - j : j;
    if (r.flags & tsfq::kIsSam) {
        const uint4 v = load16_any(chunk + r.seq_off + i0);
        if (!rev) return v;
        const uint4 w = reversed16(v);
        return make_uint4(comp4(comp, w.x), comp4(comp, w.y), comp4(comp, w.z), comp4(comp, w.w));
    }
    const uint4 c = codes16(chunk + r.seq_off, i0);
    if (!rev) return make_uint4(letters<false>(c.x), letters<false>(c.y), letters<false>(c.z), letters<false>(c.w));
    const uint4 w = reversed16(c);
    return make_uint4(letters<true>(w.x), letters<true>(w.y), letters<true>(w.z), letters<true>(w.w));
}

// quals j .. j + 15 of the text (j + 16 <= L)
__device__ __forceinline__ uint4 quals16(const unsigned char *chunk, const tsfq::Rec &r, uint32_t j) {
    if (r.flags & tsfq::kQualMissing) return make_uint4(0x21212121u, 0x21212121u, 0x21212121u, 0x21212121u);
    const bool rev = (r.flags & tsfq::kReverse) != 0u;
    uint4 v = load16_any(chunk + r.qual_off + (rev ? r.len - 16u - j : j));
    if (rev) v = reversed16(v);
    if (r.flags & tsfq::kIsSam) return v;
    return make_uint4(qual_sat(v.x), qual_sat(v.y), qual_sat(v.z), qual_sat(v.w));
}

__global__ __launch_bounds__(64)
void ts_read_fastq_write(const TsFastqOutParams P) {
    __shared__ unsigned char comp[256];
    if (blockIdx.x >= P.n_jobs) return;
    for (uint32_t c = threadIdx.x; c < 256u; c += 64u) comp[c] = (unsigned char)tsfq::sam_comp(c);
    __syncthreads();
    const TsFastqOutJob job = P.jobs[blockIdx.x];
    if (job.rec >= P.n) return;
    const u64 size = P.sizes[job.rec], to = P.dst_off[job.rec];
    if (!size || to > P.cap || size > P.cap - to) return;       // (the caller has compared the total with cap already)
    const tsfq::Rec r = P.table[job.rec];
    const ChunkBytes bytes{P.chunk};
    const uint32_t shift = (uint32_t)(to & 15ull);
    // positions count from the 16-byte boundary at or in front of the text: byte k of the text is position k + shift
    unsigned char *const line = P.out + (to - shift);
    const u64 end = size + shift, lo = (u64)job.piece * tsfq::kPieceBytes;
    const u64 hi = lo + tsfq::kPieceBytes < end ? lo + tsfq::kPieceBytes : end;
    const u64 bases_at = (u64)r.name_len + 2ull, quals_at = bases_at + r.len + 3ull;
    for (u64 s = lo + threadIdx.x * 16u; s < hi; s += 1024ull) {
        if (s >= shift && s + 16ull <= end) {                   // sixteen bytes of this record: one aligned store
            const u64 k = s - shift;
            uint4 v;
            if (k >= bases_at && k + 16ull <= bases_at + r.len) v = bases16(P.chunk, r, (uint32_t)(k - bases_at), comp);
            else if (k >= quals_at && k + 16ull <= quals_at + r.len) v = quals16(P.chunk, r, (uint32_t)(k - quals_at));
            else {
                uint32_t o[4];
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q)
                    o[q] = tsfq::out_byte(bytes, r, k + 4u * q) | tsfq::out_byte(bytes, r, k + 4u * q + 1u) << 8 |
                           tsfq::out_byte(bytes, r, k + 4u * q + 2u) << 16 | tsfq::out_byte(bytes, r, k + 4u * q + 3u) << 24;
                v = make_uint4(o[0], o[1], o[2], o[3]);
            }
            *(uint4 *)(line + s) = v;
        } else {                                                // the record's first or last bytes: these only
            for (uint32_t b = 0; b < 16u; ++b) {
                const u64 at = s + b;
                if (at >= shift && at < end) line[at] = (unsigned char)tsfq::out_byte(bytes, r, at - shift);
            }
        }
    }
}

}  // namespace

int ts_k_launch_read_fastq_plan(const TsFastqOutParams *P, void *stream) {
    if (P->n == 0) return 0;
    hipLaunchKernelGGL(ts_read_fastq_sizes, dim3((P->n + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, *P);
    hipLaunchKernelGGL(ts_read_fastq_plan, dim3(1), dim3(64), 0, (hipStream_t)stream, *P);
    return (int)hipGetLastError();
}

int ts_k_launch_read_fastq_write(const TsFastqOutParams *P, void *stream) {
    if (P->n == 0 || P->n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_read_fastq_jobs, dim3((P->n + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, *P);
    hipLaunchKernelGGL(ts_read_fastq_write, dim3(P->n_jobs), dim3(64), 0, (hipStream_t)stream, *P);
    return (int)hipGetLastError();
}
