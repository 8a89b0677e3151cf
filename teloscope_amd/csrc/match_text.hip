// match_text.hip — the two match BED files as text, formatted where a scan's match records lie (ts_match_lines_format,
// ts_scan_segments_text; host side match_text.cpp).  The device side of BedWriter::format's match branch
// (include/teloscope_mi355x_io.hpp), which stands in for scanSegment's routing of a match into canonicalMatches /
// nonCanonicalMatches with its matchSeq (src/teloscope.cpp:466-468, 485-509) and for the two match loops of the reference's
// writeBEDFile.  Which record gives a line, and the line's bytes, is match_format_core.h, shared with the host program that
// checks it against snprintf; this file is the data movement around it, in the shape of tracks.hip:
//
//   ts_match_count   a workgroup of ONE wave per tile of the directory; its lanes loop over the tile's records in steps of 64.  Per
//                    workgroup: the bytes of each of the two files and their line counts;
//   (the scan)       tracks.hip's ts_track_scan_blocks over the four columns: exclusive 64-bit prefix sums, the totals behind them.
//                    No atomics: the text's order is the stream's order;
//   ts_match_write   the same lanes compute the same lengths again, scan them for their place, stage the wave's lines of one file
//                    in LDS and copy them out in aligned 16-byte pieces, as tracks.hip does (ts_text_emit.h says how).  64 lines
//                    that exceed the staging area (names beyond ~40 bytes with long matches) are written bytewise.
//
// A workgroup is a single wave because a tile's records are consumed in a loop whose trip count differs from tile to tile:
// the barriers between staging and copy-out are then a wave's own, and waves never wait for a longer neighbour.
//
// Records are read through a policy type, one per format the library has (match_format_core.h decodes): the tiled kernel's 16-
// and 32-bit regions, the general kernels' shift 5 / 3-bit length index, the wide form's shift 8 / 6-bit index — all addressed by
// the scan's own tile directory {tile_off, tile_stats} — and an array of ts_match cut into pseudo-tiles by the host.
// Bases are read bytewise from the input layout at the segment's offset plus the record's segment-relative position: no word
// is touched that holds no base of the match.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_format_core.h"
#include "ts_device.h"
#include "ts_internal.h"
#include "ts_text_emit.h"

namespace {

typedef unsigned long long u64;
using tsmatch::kFiles;

// A tile as the formatter sees it: `count` records from index `first` of the stream, of segment `seg`, their offsets relative to
// segment position `rel0`.
struct Tile { u64 first, rel0; uint32_t count, seg; };
// What a lane knows of its record: segment-relative position, length, class.
struct Match { u64 rel; uint32_t size; bool canonical; };

// ---- the record formats
struct TiledDir {
    __device__ __forceinline__ static Tile tile(const TsMatchTextParams &P, const tsmatch::Segment *segs, uint32_t t) {
        const TsTile T = ((const TsTile *)P.tiles)[t];
        return Tile{P.tile_off[t], T.in_off - segs[T.seg].base_off, P.tile_stats[4ull * t], T.seg};
    }
};
struct Tiled16 : TiledDir {
    __device__ __forceinline__ static Match rec(const TsMatchTextParams &P, const tsmatch::Segment &, const Tile &T, u64 i) {
        const tsmatch::Rec r = tsmatch::decode_tiled(((const uint16_t *)P.records)[i], P.k);
        return Match{T.rel0 + r.at, r.size, r.canonical};
    }
};
struct Tiled32 : TiledDir {
    __device__ __forceinline__ static Match rec(const TsMatchTextParams &P, const tsmatch::Segment &, const Tile &T, u64 i) {
        const tsmatch::Rec r = tsmatch::decode_tiled(((const uint32_t *)P.records)[i], P.k);
        return Match{T.rel0 + r.at, r.size, r.canonical};
    }
};
struct GeneralDir {
    __device__ __forceinline__ static Tile tile(const TsMatchTextParams &P, const tsmatch::Segment *, uint32_t t) {
        const TsGeneralTile *G = (const TsGeneralTile *)P.tiles + t;
        return Tile{P.tile_off[t], G->seg_rel, P.tile_stats[4ull * t], G->seg};
    }
};
struct General : GeneralDir {                                // position << 5 | length index (3 bits) << 2 | canonical << 1 | forward
    __device__ __forceinline__ static Match rec(const TsMatchTextParams &P, const tsmatch::Segment &, const Tile &T, u64 i) {
        const tsmatch::Rec r = tsmatch::decode_general(((const uint32_t *)P.records)[i], 5u, 7u);
        return Match{T.rel0 + r.at, tsmatch::packed_len(P.gen_lens, r.size), r.canonical};
    }
};
struct Wide : GeneralDir {                                   // position << 8 | length index (6 bits) << 2 | canonical << 1 | forward
    __device__ __forceinline__ static Match rec(const TsMatchTextParams &P, const tsmatch::Segment &, const Tile &T, u64 i) {
        const tsmatch::Rec r = tsmatch::decode_general(((const uint32_t *)P.records)[i], 8u, 63u);
        return Match{T.rel0 + r.at, P.wide_len[r.size], r.canonical};
    }
};
struct Array {                                               // ts_match[]; the host cut every segment's records into pseudo-tiles
    __device__ __forceinline__ static Tile tile(const TsMatchTextParams &P, const tsmatch::Segment *, uint32_t t) {
        const TsMatchTile M = ((const TsMatchTile *)P.tiles)[t];
        return Tile{M.first, 0ull, M.count, M.seg};
    }
    __device__ __forceinline__ static Match rec(const TsMatchTextParams &P, const tsmatch::Segment &sg, const Tile &, u64 i) {
        const u32x4 v = ((const TS_GLOBAL u32x4 *)P.records)[i];
        const tsmatch::Rec r = tsmatch::decode_match(((u64)v.y << 32) | v.x, ((u64)v.w << 32) | v.z);
        return Match{r.at - sg.abs_pos, r.size, r.canonical};
    }
};

// A lane's line: which file (NO_LINE: none) and how long.
struct Line { Match m; uint32_t file, len; };

template <class F>
__device__ __forceinline__ Line load_line(const TsMatchTextParams &P, const tsmatch::Segment &sg, const Tile &T, uint32_t i) {
    Line L;
    L.m = Match{0ull, 0u, false}; L.file = tsmatch::NO_LINE; L.len = 0u;
    if (i >= T.count) return L;
    L.m = F::rec(P, sg, T, T.first + i);
    L.file = tsmatch::select_file(L.m.canonical, L.m.rel, sg.len, P.terminal_limit, sg.tips_only != 0u);
    if (L.file != tsmatch::NO_LINE) L.len = tsmatch::line_len(sg.name_len, sg.abs_pos + L.m.rel, L.m.size);
    return L;
}

template <class S>
__device__ __forceinline__ void put_line(const S &s, uint32_t at, const TsMatchTextParams &P, const tsmatch::Segment &sg, const Match &m) {
    const GlobalBytes names{(const TS_GLOBAL unsigned char *)P.names}, bases{(const TS_GLOBAL unsigned char *)P.bases};
    tsmatch::put_line(s, at, names, sg.name_off, sg.name_len, sg.abs_pos + m.rel, m.size, bases, sg.base_off + m.rel);
}

// sums: four columns of n_tiles + 1 values — bytes of the canonical file, of the non-canonical file, their line counts
template <class F>
__global__ __launch_bounds__(64)
void ts_match_count(const TsMatchTextParams P) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= P.n_tiles) return;
    const tsmatch::Segment *segs = (const tsmatch::Segment *)P.segs;
    const Tile T = F::tile(P, segs, t);
    u64 bytes[kFiles] = {0ull, 0ull}, lines[kFiles] = {0ull, 0ull};
    if (T.count && T.seg < P.n_segs) {                          // (uniform over the wave)
        const tsmatch::Segment sg = segs[T.seg];
        if (!sg.tips_only)
            for (uint32_t i0 = 0; i0 < T.count; i0 += 64u) {
                const Line L = load_line<F>(P, sg, T, i0 + lane);
#pragma unroll
                for (uint32_t f = 0; f < kFiles; ++f) {
                    bytes[f] += wave_total(L.file == f ? L.len : 0u);
                    lines[f] += (u64)__popcll(ballot64(L.file == f));
                }
            }
    }
    if (lane == 0u) {
        const u64 col = (u64)P.n_tiles + 1u;
        P.sums[t] = bytes[0]; P.sums[col + t] = bytes[1];
        P.sums[2u * col + t] = lines[0]; P.sums[3u * col + t] = lines[1];
    }
}

// tiles [tile_first, tile_first + gridDim.x): file f's bytes of tile t go to out[f] + (sums[f][t] - slice_base[f])
template <class F>
__global__ __launch_bounds__(64)
void ts_match_write(const TsMatchTextParams P) {
    __shared__ u32x4 stage[kStageVecs];
    const uint32_t t = P.tile_first + blockIdx.x, lane = threadIdx.x;
    if (t >= P.n_tiles) return;
    const tsmatch::Segment *segs = (const tsmatch::Segment *)P.segs;
    const Tile T = F::tile(P, segs, t);
    if (!T.count || T.seg >= P.n_segs) return;                   // (uniform over the wave, as every branch around a barrier below)
    const tsmatch::Segment sg = segs[T.seg];
    if (sg.tips_only) return;
    const u64 col = (u64)P.n_tiles + 1u;
    u64 off[kFiles] = {P.sums[t] - P.slice_base[0], P.sums[col + t] - P.slice_base[1]};
    for (uint32_t i0 = 0; i0 < T.count; i0 += 64u) {
        const Line L = load_line<F>(P, sg, T, i0 + lane);
#pragma unroll
        for (uint32_t f = 0; f < kFiles; ++f) {
            const uint32_t len = L.file == f ? L.len : 0u;
            const uint32_t incl = wave_scan_add(len), excl = incl - len;
            const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (!n) continue;
            TS_GLOBAL unsigned char *dst = (TS_GLOBAL unsigned char *)P.out[f] + off[f];    // the first byte of these lines
            if (len) wave_put(stage, dst, n, excl, [&](const auto &s, uint32_t at) { put_line(s, at, P, sg, L.m); });
            __syncthreads();                                     // (a single wave, and n is the same in all its lanes)
            wave_copy_out(stage, dst, n, lane);
            __syncthreads();                                     // (the next lines reuse the staging area)
            off[f] += n;
        }
    }
}

template <class F>
int launch(const TsMatchTextParams *P, bool write, uint32_t grid, hipStream_t st) {
    if (write) hipLaunchKernelGGL(ts_match_write<F>, dim3(grid), dim3(64), 0, st, *P);
    else hipLaunchKernelGGL(ts_match_count<F>, dim3(grid), dim3(64), 0, st, *P);
    return (int)hipGetLastError();
}

int launch_form(const TsMatchTextParams *P, bool write, uint32_t grid, hipStream_t st) {
    switch (P->form) {
    case TS_MATCH_FORM_TILED16: return launch<Tiled16>(P, write, grid, st);
    case TS_MATCH_FORM_TILED32: return launch<Tiled32>(P, write, grid, st);
    case TS_MATCH_FORM_GENERAL: return launch<General>(P, write, grid, st);
    case TS_MATCH_FORM_WIDE: return launch<Wide>(P, write, grid, st);
    case TS_MATCH_FORM_ARRAY: return launch<Array>(P, write, grid, st);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace

int ts_k_launch_match_count(const TsMatchTextParams *P, void *stream) {
    if (P->n_tiles == 0) return 0;
    const int e = launch_form(P, false, P->n_tiles, (hipStream_t)stream);
    if (e != 0) return e;
    return ts_k_launch_scan_columns(P->sums, 2u * kFiles, P->n_tiles, stream);
}

int ts_k_launch_match_write(const TsMatchTextParams *P, uint32_t n, void *stream) {
    if (n == 0) return 0;
    return launch_form(P, true, n, (hipStream_t)stream);
}
