// tracks.hip — the five window tracks as text, formatted where the window records lie (ts_window_tracks_format,
// ts_scan_segments_tracks; host side tracks.cpp).  The device side of BedWriter::format's window branch
// (include/teloscope_mi355x_io.hpp), which stands in for the window loops of the reference's writeBEDFile
// (src/teloscope.cpp:785-812).  What a line holds and how a number becomes text is track_format_core.h, shared with the host
// program that checks it against printf; this file is the data movement around it:
//
//   ts_track_count        a lane per window: the length of its line in every enabled track; per workgroup of 256 windows the
//                         five sums (wave scans of ts_device.h, four wave totals through LDS);
//   ts_track_scan_blocks  one wave per track: exclusive 64-bit prefix sums of the workgroup sums, the track's bytes behind them;
//   ts_track_write        the same lane per window computes the same lengths again, once, (a record is 32 bytes, its five offsets
//                         would be 40), scans them for its place and writes its lines.
//
// Stores: a wave stages its 64 lines of one track in LDS and copies them out in aligned 16-byte pieces; ts_text_emit.h says how
// (match_text.hip writes its lines the same way).  A wave's 64 lines exceed the staging area with names beyond ~70 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_format_core.h"
#include "ts_device.h"
#include "ts_internal.h"
#include "ts_text_emit.h"

namespace {

typedef unsigned long long u64;
using tstrack::kTracks;

constexpr uint32_t kBlock = TS_TRACK_BLOCK;                 // windows (threads) per workgroup
constexpr uint32_t kWaves = kBlock / 64u;
constexpr uint32_t kSumsPerThread = 8u;                     // ts_track_scan_blocks: consecutive sums per lane

// What a lane knows about its window before it formats a value.
struct Window {
    tstrack::Record r;
    u64 start, end, name_off;
    uint32_t name_len, size, entropy_bits, prefix;
    bool valid, bad;
};

__device__ __forceinline__ Window load_window(const TsTrackParams &P, u64 i) {
    Window W;
    W.valid = false; W.bad = false;
    W.r = tstrack::Record{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    W.start = W.end = W.name_off = 0; W.name_len = 0; W.size = 1u; W.entropy_bits = 0u; W.prefix = 0u;
    if (i >= P.n) return W;
    const tstrack::Segment *segs = (const tstrack::Segment *)P.segs;
    const tstrack::Segment sg = segs[tstrack::find_segment(segs, P.n_segs, i)];
    const u64 k = i - sg.first_window;
    if (i < sg.first_window || k >= sg.n_windows) return W;      // (a record between two segments' windows: no line)
    W.valid = true;
    const TS_GLOBAL u32x4 *rec = (const TS_GLOBAL u32x4 *)P.records;
    const u32x4 lo = rec[2u * i], hi = rec[2u * i + 1u];
    W.r = tstrack::Record{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    W.start = tstrack::window_start(sg, k, P.step);
    W.size = tstrack::window_size(sg, k, P.w, P.step);
    W.end = W.start + W.size;
    W.name_off = sg.name_off; W.name_len = sg.name_len;
    W.prefix = tstrack::prefix_len(W.name_len, W.start, W.end);
    if (P.on_mask & (1u << tstrack::ENTROPY)) {
        if (P.term && W.size == P.w) {
            W.entropy_bits = tstrack::float_bits(tstrack::entropy_from_terms(W.r, P.term, P.w, &W.bad));
        } else {
            bool found;
            W.entropy_bits = tstrack::find_patch((const tstrack::Patch *)P.patches, P.n_patches, i, &found);
            W.bad = !found;
        }
    }
    return W;
}

// the line's length in track t (0: no line), *bad when the value cannot be printed
__device__ __forceinline__ uint32_t line_len(const Window &W, uint32_t t, tstrack::FloatDec *d, bool *bad) {
    *d = tstrack::float_dec(tstrack::track_value(t, W.r, W.size, W.entropy_bits));
    if (!W.valid) return 0u;
    if (d->kind == tstrack::F_BAD) { *bad = true; return 0u; }
    return W.prefix + tstrack::float_len(*d) + 1u;
}

template <class S>
__device__ __forceinline__ void put_line(const S &s, uint32_t at, const TsTrackParams &P, const Window &W, const tstrack::FloatDec &d) {
    const GlobalBytes names{(const TS_GLOBAL unsigned char *)P.names};
    tstrack::put_prefix(s, at, names, W.name_off, W.name_len, W.start, W.end);
    tstrack::put_float(s, at + W.prefix, d);
    s.put(at + W.prefix + tstrack::float_len(d), '\n');
}

__global__ __launch_bounds__(kBlock)
void ts_track_count(const TsTrackParams P) {
    __shared__ uint32_t tot[kTracks][kWaves];
    const u64 i = P.first + (u64)blockIdx.x * kBlock + threadIdx.x;
    const Window W = load_window(P, i);
    bool bad = W.valid && W.bad;
#pragma unroll
    for (uint32_t t = 0; t < kTracks; ++t) {
        uint32_t len = 0;
        if (P.on_mask & (1u << t)) {
            tstrack::FloatDec d;
            len = line_len(W, t, &d, &bad);
        }
        const uint32_t total = wave_total(len);
        if ((threadIdx.x & 63u) == 0u) tot[t][threadIdx.x >> 6] = total;
    }
    if (bad) atomicMin(P.bad_window, i);
    __syncthreads();
    if (threadIdx.x < kTracks) {
        u64 s = 0;
        for (uint32_t w = 0; w < kWaves; ++w) s += tot[threadIdx.x][w];
        P.block_sums[(u64)threadIdx.x * (P.n_blocks + 1u) + blockIdx.x] = s;
    }
}

// workgroup t, one wave: block_sums[t][0 .. n_blocks) -> their exclusive prefix sums, block_sums[t][n_blocks] = the track's bytes
__global__ __launch_bounds__(64)
void ts_track_scan_blocks(u64 *block_sums, uint32_t n_blocks) {
    u64 *sums = block_sums + (u64)blockIdx.x * (n_blocks + 1u);
    u64 carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 64u * kSumsPerThread) {
        const uint32_t base = b0 + threadIdx.x * kSumsPerThread;
        u64 c[kSumsPerThread], v = 0;
#pragma unroll
        for (uint32_t j = 0; j < kSumsPerThread; ++j) { c[j] = base + j < n_blocks ? sums[base + j] : 0ull; v += c[j]; }
        u64 total;
        u64 run = carry + wave_excl_scan_u64(v, &total);
#pragma unroll
        for (uint32_t j = 0; j < kSumsPerThread; ++j) { if (base + j < n_blocks) sums[base + j] = run; run += c[j]; }
        carry += total;
    }
    if (threadIdx.x == 0) sums[n_blocks] = carry;
}

__global__ __launch_bounds__(kBlock)
void ts_track_write(const TsTrackParams P) {
    __shared__ u32x4 stage[kWaves][kStageVecs];
    __shared__ uint32_t tot[kTracks][kWaves];
    if (*P.bad_window != ~0ull) return;                          // (the host fails the call: nothing is written)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 i = P.first + (u64)blockIdx.x * kBlock + threadIdx.x;
    const Window W = load_window(P, i);
    bool bad = false;
    uint32_t excl[kTracks], wave_bytes[kTracks], lens[kTracks];
    tstrack::FloatDec dec[kTracks];                              // (kept for the second loop: constant indices, registers)
#pragma unroll
    for (uint32_t t = 0; t < kTracks; ++t) {
        uint32_t len = 0;
        dec[t] = tstrack::FloatDec{0u, 1u, 0, tstrack::F_BAD};
        if (P.on_mask & (1u << t)) len = line_len(W, t, &dec[t], &bad);
        lens[t] = len;
        const uint32_t incl = wave_scan_add(len);
        excl[t] = incl - len;
        wave_bytes[t] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (lane == 0u) tot[t][wave] = wave_bytes[t];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < kTracks; ++t) {
        if (!(P.on_mask & (1u << t))) continue;                  // (uniform over the grid)
        u64 off = P.block_sums[(u64)t * (P.n_blocks + 1u) + blockIdx.x];
        for (uint32_t w = 0; w < wave; ++w) off += tot[t][w];
        TS_GLOBAL unsigned char *dst = (TS_GLOBAL unsigned char *)P.out[t] + off;    // the wave's first byte
        const tstrack::FloatDec d = dec[t];
        if (lens[t]) wave_put(stage[wave], dst, wave_bytes[t], excl[t], [&](const auto &s, uint32_t at) { put_line(s, at, P, W, d); });
        __syncthreads();                                         // (outside every condition a wave could differ in: a wave without bytes waits too)
        wave_copy_out(stage[wave], dst, wave_bytes[t], lane);
        __syncthreads();                                         // (the next track reuses the staging area)
    }
}

// patch windows' records, dense: out[j] = records[idx[j]]
__global__ __launch_bounds__(256)
void ts_track_pick(const uint4 *records, const u64 *idx, u64 n, uint4 *out) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u64 i = idx[j];
    out[2u * j] = records[2u * i];
    out[2u * j + 1u] = records[2u * i + 1u];
}

}  // namespace

int ts_k_launch_track_count(const TsTrackParams *P, void *stream) {
    if (P->n_blocks == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ts_track_count, dim3(P->n_blocks), dim3(kBlock), 0, st, *P);
    hipLaunchKernelGGL(ts_track_scan_blocks, dim3(kTracks), dim3(64), 0, st, P->block_sums, P->n_blocks);
    return (int)hipGetLastError();
}

int ts_k_launch_scan_columns(unsigned long long *sums, uint32_t n_columns, uint32_t n_blocks, void *stream) {
    if (n_columns == 0) return 0;
    hipLaunchKernelGGL(ts_track_scan_blocks, dim3(n_columns), dim3(64), 0, (hipStream_t)stream, sums, n_blocks);
    return (int)hipGetLastError();
}

int ts_k_launch_track_write(const TsTrackParams *P, void *stream) {
    if (P->n_blocks == 0) return 0;
    hipLaunchKernelGGL(ts_track_write, dim3(P->n_blocks), dim3(kBlock), 0, (hipStream_t)stream, *P);
    return (int)hipGetLastError();
}

int ts_k_launch_track_pick(const uint32_t *records, const unsigned long long *idx, unsigned long long n, uint32_t *out, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(ts_track_pick, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)records, idx, n,
                       (uint4 *)out);
    return (int)hipGetLastError();
}
