// general_plan_core.h — what the host plans for the general kernels (generic.hip, and blockcall.hip's walks over their slots),
// one source for every driver: the host entry points' general path (pipeline.cpp), general tips batches (general_batch.cpp), the
// tiled batches' planning and walks (capi.cpp, pipeline.cpp) and a host test program (tests/cpp/general_plan_host.cpp, built
// by g++ under ASan + UBSan).  Plain C++17 over the structures of ts_internal.h: no HIP, no context.
#ifndef TS_GENERAL_PLAN_CORE_H
#define TS_GENERAL_PLAN_CORE_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ts_internal.h"

namespace tsplan {

struct Span { uint64_t start, len; };                       // relative to the segment
struct Regions {
    uint32_t n = 0;
    Span r[2] = {{0, 0}, {0, 0}};
    const Span *begin() const { return r; }
    const Span *end() const { return r + n; }
};

// The scanned regions of a segment of `len` bases, in order: a full scan reads all of it; a tips-only scan the whole segment up
// to 2 x terminal limit, else its two tips — regions exactly as scanSegment picks them (src/teloscope.cpp:576-583; uint32 product)
inline Regions scanned_regions(uint64_t len, bool tips, uint32_t terminal_limit) {
    Regions R;
    const uint32_t twice = 2u * terminal_limit;
    if (tips && len > twice) {
        R.r[R.n++] = {0, terminal_limit};
        R.r[R.n++] = {len - terminal_limit, terminal_limit};
    } else if (len) {
        R.r[R.n++] = {0, len};
    }
    return R;
}

// Appends the tiles of one region: TS_GENERAL_TILE positions each, the last what is left.  in_off: the layout offset of the
// region's first base; seg_start: its position in the segment; halo: the bases a tile may read beyond its own (32, the wide
// form TS_WIDE_HALO) — never beyond the region.  P0 = k_p0 step + r_p0 is divided once and walked from tile to tile.
inline void append_region_tiles(std::vector<TsGeneralTile> &tiles, uint64_t in_off, uint64_t seg_start, uint64_t len, uint32_t seg,
                                uint32_t step, uint32_t halo) {
    uint64_t kq = seg_start / step, kr = seg_start - kq * step;
    for (uint64_t a = 0; a < len; a += TS_GENERAL_TILE) {
        TsGeneralTile T{};
        T.in_off = in_off + a;
        T.seg_rel = seg_start + a;
        T.k_p0 = kq; T.r_p0 = (uint32_t)kr;
        T.n = (uint32_t)std::min<uint64_t>(TS_GENERAL_TILE, len - a);
        T.avail = (uint32_t)std::min<uint64_t>(len - a, (uint64_t)T.n + halo);
        T.seg = seg;
        tiles.push_back(T);
        kr += TS_GENERAL_TILE;
        if (kr >= step) { const uint64_t d = kr / step; kq += d; kr -= d * step; }
    }
}

// The walks' table entry of a segment whose tiles [first_tile, first_tile + n_tiles) are all scanned and owned: both ends its own
inline TsShardSegIn whole_segment_entry(uint64_t in_off, uint64_t len, uint64_t abs_pos, uint32_t first_tile, uint32_t n_tiles, uint32_t seg) {
    TsShardSegIn S{};
    S.in_off = in_off; S.len = len; S.abs_pos = abs_pos;
    S.t0 = S.o0 = first_tile; S.t1 = S.o1 = first_tile + n_tiles;
    S.flags = TS_SEG_F_HAS_START | TS_SEG_F_HAS_END;
    S.lo_rel = 0; S.hi_rel = len; S.seg = seg;
    return S;
}

}  // namespace tsplan

#endif
