// scan_lds_core.h — the LDS layout of ts_scan_tiles (kernels.hip), one source for the kernel that addresses it and for the host
// plan that sizes it (tiled_plan_core.h).  __host__ __device__ under hipcc, plain inline under g++ (the host test programs).
#ifndef TS_SCAN_LDS_CORE_H
#define TS_SCAN_LDS_CORE_H

#include <stdint.h>

#include "ts_internal.h"

#if defined(__HIPCC__)
#define TS_LDS_FN __host__ __device__ inline
#else
#define TS_LDS_FN inline
#endif

constexpr uint32_t TS_CU_LDS_BYTES = 160u * 1024u;          // the LDS of one CU of gfx950: what the workgroups that share a CU divide

TS_LDS_FN uint32_t align16(uint32_t x) { return (x + 15u) & ~15u; }

// LDS: [match table][wave 0 queue][wave 1 queue]...[wave 0 slice][wave 1 slice]...; a slice = codes | rec | wacc | stage
//   codes   2-bit codes of the tile, two dwords per 32 positions (+ one look-ahead dword pair); the per-match pass
//           reads k-mers from it and the window phase counts the nucleotides of every step block in it
//   queue   (its own region) ring of TS_LIST u16 plane coordinates of match positions, appended to by every
//           chunk in position order and consumed 64 at a time, so that the per-match work runs
//           on full wavefronts
//   rec     nucleotide counts {A, C, G, T}, 4 x u32 per step block of the tile (windows + halo) when w is a
//           multiple of s (a window is the sum of w / s rows), else per window
//   wacc    the match fields of the tile's window records while they accumulate: one u64 per step block (w a multiple of s:
//           a window's fields are then the sum of its blocks' minus the matches that run over the end of its last block,
//           which have a row of their own — ONE add per match instead of one per window that contains it) or per window
//           = four 16-bit counters {canonical, non-canonical, forward, reverse}, bumped by ONE
//           ds_add_u64 per (match, window); kept in acc_copies lane-interleaved copies so that the
//           matches of a pass, which mostly fall into the same few windows, do not serialise on one
//           address
//   stage   packed match records waiting to leave in whole coalesced rows at the tile's end (kept out of the
//           chunk loads' counted vmcnt waits), 16 bits each when tile positions allow (P.stage_u16), + one spare slot per lane
//           for predicated-off writes
//   park    eight dwords of per-wave state of the emitting build that only the end of a tile touches (finish_records): kept here,
//           not in scalar registers, so that the chunk loop of the emitting build is the plain build's
struct SliceLayout { uint32_t codes, rec, wacc, stage, park, bytes; };

TS_LDS_FN SliceLayout slice_layout(const TsScanParams &P) {
    SliceLayout s;
    uint32_t o = 0;
    s.codes = o; o += align16((P.nch * 63u + 1u) * 8u);
    s.rec = o; o += (P.windows_on && P.nuc_on) ? align16((P.max_windows + P.halo_blocks) * 16u) : 0u;
    // (per step block when w is a multiple of s: rows for the tile's windows + halo in every copy, then one row per block for
    //  the matches that run over their block's end; else per window)
    s.wacc = o; o += P.windows_on ? align16((P.max_windows + (P.acc_blocks ? P.halo_blocks : 0u)) * 8u * (P.acc_copies + (P.acc_blocks ? 1u : 0u))) : 0u;
    s.stage = o; o += (P.stage_cap + 64u) * (P.stage_u16 ? 2u : 4u);
    s.park = o; o += 32u;                                     // (whether or not this batch emits: one geometry)
    s.bytes = o;
    return s;
}

// The match queues of all waves sit together behind the table, each aligned to its own size, so that a
// queue slot's LDS address is (byte offset & mask) | base: one v_and_or instead of mask, shift and add.
TS_LDS_FN uint32_t queue_region(const TsScanParams &P) {
    const uint32_t a = TS_LIST * 2u;
    return (P.table_rows * 4u + P.fc_bytes + a - 1u) & ~(a - 1u);
}

TS_LDS_FN uint32_t lds_total(const TsScanParams &P) {
    return queue_region(P) + P.waves_per_wg * (TS_LIST * 2u + slice_layout(P).bytes);
}

#endif
