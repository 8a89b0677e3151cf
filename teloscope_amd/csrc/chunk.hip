// chunk.hip — the kernels the device routes over a resident chunk share (chunk_internal.h).  One-wave workgroups throughout.
//   * byte count and byte index: a wave per 16 KB of the chunk, 16 bytes per lane per step.  A first pass counts the byte per
//     slice, one wave sums the counts (the scan), a second pass hands every hit, in order, to a store (a DPP prefix sum of the
//     lanes' counts numbers them; a step without a hit is skipped on a ballot): for '\n' the line index, for '\t' its offset.
//   * gather plan: a prefix sum over the bytes every passing record contributes (one wave, 64 records per step).  The copies
//     are the routes' own kernels around chunk_device.h's copy_record16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teloscan.h"
#include "chunk_device.h"
#include "chunk_internal.h"
#include "ts_device.h"

namespace {

template <unsigned char C>
__global__ __launch_bounds__(64)
void ts_chunk_byte_count_kernel(const unsigned char *plain, unsigned long long n, uint32_t *counts) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kChunkSliceBytes + threadIdx.x * 16u;
    uint32_t c = 0;
#pragma unroll 8
    for (uint32_t s = 0; s < kChunkSliceBytes / 1024u; ++s) c += __popc(byte_mask16<C>(plain, base + 1024ull * s, n));
    c = wave_total(c);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// store.hit(plain, n, k, a, bit): hit k of the chunk is the byte at a + bit; store.finish(plain, n): once per lane, at the end
template <unsigned char C, class Store>
__global__ __launch_bounds__(64)
void ts_chunk_byte_index_kernel(const unsigned char *plain, unsigned long long n, const uint32_t *sums, Store store) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kChunkSliceBytes + threadIdx.x * 16u;
    uint32_t run = sums[blockIdx.x];
    for (uint32_t s = 0; s < kChunkSliceBytes / 1024u; ++s) {
        const unsigned long long a = base + 1024ull * s;
        uint32_t m = byte_mask16<C>(plain, a, n);
        if (ballot64(m != 0u) == 0ull) continue;                // (wave-uniform)
        const uint32_t c = __popc(m), incl = wave_scan_add(c);
        uint32_t k = run + incl - c;                            // the first of this lane's hits is hit k
        while (m) {
            const uint32_t bit = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            store.hit(plain, n, k, a, bit);
            ++k;
        }
        run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    store.finish(plain, n);
}

// '\n' number k ends line k
struct LineStore {
    uint32_t newlines, tail;
    uint32_t *lstart;
    unsigned char *first, *cr;
    __device__ __forceinline__ void hit(const unsigned char *plain, unsigned long long n, uint32_t k, unsigned long long a, uint32_t bit) const {
        const unsigned long long p = a + bit;
        if (k < newlines) {                                     // (always: the count pass saw the same bytes)
            lstart[k + 1] = (uint32_t)(p + 1ull);
            first[k + 1] = p + 1ull < n ? plain[p + 1ull] : (unsigned char)0;
            cr[k] = p > 0ull && plain[p - 1ull] == '\r';
        }
    }
    __device__ __forceinline__ void finish(const unsigned char *plain, unsigned long long n) const {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            lstart[0] = 0u;
            first[0] = n ? plain[0] : (unsigned char)0;
            if (tail) {                                         // the last line has no '\n': it ends at n
                lstart[newlines + 1] = (uint32_t)(n + 1ull);
                cr[newlines] = plain[n - 1ull] == '\r';
            }
        }
    }
};

struct TabStore {
    uint32_t n_tabs;
    uint32_t *tabs;
    __device__ __forceinline__ void hit(const unsigned char *, unsigned long long, uint32_t k, unsigned long long a, uint32_t bit) const {
        const uint32_t p = (uint32_t)a + bit;
        if (k < n_tabs) tabs[k] = p;                            // (always: the count pass saw the same bytes)
    }
    __device__ __forceinline__ void finish(const unsigned char *, unsigned long long) const {}
};

// counts -> exclusive sums in place (one wave, 64 per step); tail(total): what else lane 0 writes behind the total
struct NoTail { __device__ __forceinline__ void operator()(unsigned long long *) const {} };
struct NewlineTail {                    // the line count's second word
    const unsigned char *plain;
    unsigned long long n;
    __device__ __forceinline__ void operator()(unsigned long long *out) const { out[kChunkTail] = n && plain[n - 1] != '\n' ? 1ull : 0ull; }
};

template <class Tail>
__global__ __launch_bounds__(64)
void ts_chunk_scan_kernel(uint32_t *counts, uint32_t n, unsigned long long *total, Tail tail) {
    unsigned long long run = 0;
    for (uint32_t b = 0; b < n; b += 64u) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t c = i < n ? counts[i] : 0u;
        const uint32_t incl = wave_scan_add(c);
        if (i < n) counts[i] = (uint32_t)run + incl - c;        // (a chunk holds less than 4 GiB: the sums fit)
        run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (threadIdx.x == 0) { *total = run; tail(total); }
}

// ---- passing records, in input order: bytes(rec) of every record whose pass byte is set
struct FastqBytes { __device__ __forceinline__ unsigned long long operator()(const ts_fastq_record &r) const { return 1ull + r.size; } };
struct BamBytes { __device__ __forceinline__ uint32_t operator()(const ts_bam_record &r) const { return 4u + r.block_size; } };

template <class Rec, class Bytes>
__global__ __launch_bounds__(64)
void ts_chunk_gather_plan_kernel(const Rec *recs, const unsigned char *pass, unsigned long long n, unsigned long long *dst_off,
                                 unsigned long long *totals) {
    typedef decltype(Bytes()(recs[0])) Size;                    // 32 bits where a record's bytes fit them
    unsigned long long run = 0, kept = 0;
    for (unsigned long long base = 0; base < n; base += 64ull) {
        const unsigned long long i = base + threadIdx.x;
        const bool keep = i < n && pass[i] != 0;
        const Size size = keep ? Bytes()(recs[i]) : (Size)0;
        // (a step's sizes are summed in two halves: 64 records of up to 4 GiB)
        const uint32_t incl_lo = wave_scan_add((uint32_t)(size & 0xffffu)), incl_hi = wave_scan_add((uint32_t)(size >> 16));
        const unsigned long long incl = (unsigned long long)incl_lo + ((unsigned long long)incl_hi << 16);
        if (i < n) dst_off[i] = keep ? run + incl - size : ~0ull;
        run += (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)incl_lo, 63) +
               ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)incl_hi, 63) << 16);
        kept += (unsigned long long)__popcll(ballot64(keep));
    }
    if (threadIdx.x == 0) { totals[0] = run; totals[1] = kept; }
}

template <class Rec, class Bytes>
int launch_gather_plan(const void *recs, const void *pass, unsigned long long n, void *dst_off, void *totals, void *stream) {
    hipLaunchKernelGGL((ts_chunk_gather_plan_kernel<Rec, Bytes>), dim3(1), dim3(64), 0, (hipStream_t)stream, (const Rec *)recs,
                       (const unsigned char *)pass, n, (unsigned long long *)dst_off, (unsigned long long *)totals);
    return (int)hipGetLastError();
}

uint32_t slices_of(unsigned long long n) { return (uint32_t)((n + kChunkSliceBytes - 1) / kChunkSliceBytes); }

}  // namespace

extern "C" {

int ts_k_launch_chunk_newline_count(const void *plain, unsigned long long n, uint32_t *counts, unsigned long long *out, void *stream) {
    const uint32_t slices = slices_of(n);
    if (slices) hipLaunchKernelGGL(ts_chunk_byte_count_kernel<'\n'>, dim3(slices), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, n, counts);
    hipLaunchKernelGGL(ts_chunk_scan_kernel<NewlineTail>, dim3(1), dim3(64), 0, (hipStream_t)stream, counts, slices, out + kChunkNewlines,
                       NewlineTail{(const unsigned char *)plain, n});
    return (int)hipGetLastError();
}

int ts_k_launch_chunk_newline_index(const void *plain, unsigned long long n, const uint32_t *sums, uint32_t newlines, uint32_t tail,
                                    uint32_t *lstart, unsigned char *first, unsigned char *cr, void *stream) {
    const uint32_t slices = slices_of(n);
    if (slices == 0) return 0;
    hipLaunchKernelGGL((ts_chunk_byte_index_kernel<'\n', LineStore>), dim3(slices), dim3(64), 0, (hipStream_t)stream,
                       (const unsigned char *)plain, n, sums, LineStore{newlines, tail, lstart, first, cr});
    return (int)hipGetLastError();
}

int ts_k_launch_chunk_tab_count(const void *plain, unsigned long long n, uint32_t *counts, void *stream) {
    const uint32_t slices = slices_of(n);
    if (slices == 0) return 0;
    hipLaunchKernelGGL(ts_chunk_byte_count_kernel<'\t'>, dim3(slices), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, n, counts);
    return (int)hipGetLastError();
}

int ts_k_launch_chunk_tab_index(const void *plain, unsigned long long n, const uint32_t *sums, uint32_t n_tabs, uint32_t *tabs,
                                void *stream) {
    const uint32_t slices = slices_of(n);
    if (slices == 0 || n_tabs == 0) return 0;
    hipLaunchKernelGGL((ts_chunk_byte_index_kernel<'\t', TabStore>), dim3(slices), dim3(64), 0, (hipStream_t)stream,
                       (const unsigned char *)plain, n, sums, TabStore{n_tabs, tabs});
    return (int)hipGetLastError();
}

int ts_k_launch_chunk_scan(uint32_t *counts, uint32_t n, unsigned long long *total, void *stream) {
    hipLaunchKernelGGL(ts_chunk_scan_kernel<NoTail>, dim3(1), dim3(64), 0, (hipStream_t)stream, counts, n, total, NoTail{});
    return (int)hipGetLastError();
}

int ts_k_launch_chunk_gather_plan_fastq(const void *recs, const void *pass, unsigned long long n, void *dst_off, void *totals, void *stream) {
    return launch_gather_plan<ts_fastq_record, FastqBytes>(recs, pass, n, dst_off, totals, stream);
}
int ts_k_launch_chunk_gather_plan_bam(const void *recs, const void *pass, unsigned long long n, void *dst_off, void *totals, void *stream) {
    return launch_gather_plan<ts_bam_record, BamBytes>(recs, pass, n, dst_off, totals, stream);
}

}  // extern "C"
