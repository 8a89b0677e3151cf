// tiled_plan_core.h — what the host plans for the tiled scan kernel (kernels.hip: ts_scan_tiles): the tile geometry that fits the
// LDS layout of scan_lds_core.h, the tiles of a batch's segments, what a tile range covers, the launch and capacity sizes, the
// terminal-zone words of the emitting build and the split of a plan into shards with the layout of their messages.  One source
// for capi.cpp (batches), shard.cpp (shards) and a host test program (tests/cpp/tiled_plan_host.cpp, built by g++ under ASan +
// UBSan).  Plain C++17 over the structures of ts_internal.h: no HIP, no context, no batch, no environment.
#ifndef TS_TILED_PLAN_CORE_H
#define TS_TILED_PLAN_CORE_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "general_plan_core.h"
#include "scan_lds_core.h"
#include "ts_internal.h"

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// isTerminal (src/teloscope.cpp:451-459) of a segment-relative position: rel <= t || rel >= N - t, the whole of a segment no
// longer than t; term_end = ts_terminal_end(segment length, limit).  THE statement of the terminal zone: the per-tile thresholds
// below are derived from it.
inline uint64_t ts_terminal_end(uint64_t seg_len, uint64_t terminal_limit) { return seg_len > terminal_limit ? seg_len - terminal_limit : 0; }
inline bool ts_is_terminal(uint64_t rel, uint64_t terminal_limit, uint64_t term_end) { return rel <= terminal_limit || rel >= term_end; }

namespace tsplan {

constexpr uint32_t kMaxBlocksPerTile = 448;
constexpr uint32_t kMaxChunks = 8;             // tiles up to ~16 k positions per wave
constexpr uint32_t kTipsChunks = 8;            // tips-only / read batches: ~16 k positions per tile (15 kb reads, TS_GEOMETRY sweeps: six chunks until round 4;
                                               // eight since the stage's entries are 16 bits — profiles/r05/reads_tilings.txt)

// What a geometry depends on: the parameters, the pattern set as the match-table builders left it, and the knobs the driver
// read from the environment (TS_GEOMETRY, TS_ACC_PER_WINDOW, TS_STAGE_U32).  (TS_VIS_CAP is read whenever a range is sized, not
// once per plan: it is an argument of set_range.)
struct PlanInputs {
    uint32_t step = 0, window_size = 0, terminal_limit = 0, max_match_dist = 0;
    bool fold_case = false, nuc = false;                 // nuc: nucleotide counts wanted (-g / -e)
    uint32_t k = 0;                                      // uniform pattern length
    uint64_t n_patterns = 0, n_canonical = 0;
    uint32_t table_rows = 0, fc_bytes = 0;
    bool fc_byte_table = true, pair_byte_table = false;
    // TS_GEOMETRY="waves,chunks,stage,workgroups" pins the search to one point (0 = any): a test knob for the contract that the
    // output does not depend on the tiling ("independent of GPU count and tile size"); the 4th field: workgroups
    // per CU, for measurements such as 2 x 12 waves
    uint32_t pin_waves = 0, pin_nch = 0, pin_stage = 0, pin_wgs = 0;
    bool acc_per_window = false;                         // TS_ACC_PER_WINDOW=1: A/B
    bool stage_u32 = false;                              // TS_STAGE_U32=1: A/B
};

// (position << 2 | flags) of every position of a tile of nch chunks fits 16 bits: the stage's entries, the visible records, the
// exchange's u16 wire
inline bool positions_fit14(uint32_t nch) { return (uint64_t)nch * TS_CHUNK + 64u <= (1u << 14); }

// Chooses waves per workgroup, chunks per tile and windows per tile so that the match table plus
// one LDS slice per wave fit in 160 KB; false if even one wave cannot hold one window.
inline bool plan_geometry(const PlanInputs &in, bool tips, TsScanParams &kp, uint32_t &wpt) {
    const uint32_t k = in.k;
    kp.k = k;
    kp.table_rows = in.table_rows;
    kp.fc_bytes = in.fc_bytes;
    kp.fc_byte_table = in.fc_byte_table ? 1u : 0u;
    kp.pair_byte_table = in.pair_byte_table ? 1u : 0u;
    kp.fold_mask = in.fold_case ? 0xDFDFDFDFu : 0xFFFFFFFFu;
    kp.emit = 0;                         // (ts_batch_set_emit)
    kp.kdist = in.max_match_dist;
    if (tips) {
        kp.halo_blocks = 0;
        kp.straddle_fix = 0; kp.windows_on = 0; kp.nuc_on = 0; kp.block_sums = 0; kp.acc_blocks = 0;
    } else {
        const uint32_t s = in.step, w = in.window_size;
        kp.s = s; kp.w = w;
        kp.s_inv = (65536u + s - 1u) / s;
        kp.halo_blocks = (w + s - 1) / s - 1;            // window i reaches into step blocks i .. i + ceil(w/s) - 1
        kp.straddle_fix = (w == s) ? 1u : 0u;
        kp.windows_on = 1;
        kp.nuc_on = in.nuc ? 1u : 0u;
        kp.block_sums = (w % s == 0) ? 1u : 0u;
        kp.acc_blocks = (kp.block_sums && !in.acc_per_window) ? 1u : 0u;
    }
    // Search (waves per workgroup, chunks per tile) for the best modelled throughput:
    //   owned bases per tile x occupancy factor / instructions per tile.
    // Instructions: ~470 per 2016-position chunk (decode, probes, planes, per-match pass: the weights of round 1's kernel), ~170 per
    // pass of the window loop (64 window fields per pass), ~100 fixed per tile.  Occupancy factors are
    // measured (profiles/r01/geometry_sweep.txt): against 16 waves per CU the kernel loses 12 % at 12
    // waves and 31 % at 8; more than 16 is not reachable (two workgroups per CU did not co-reside).
    // Round 2: built for 80 VGPRs, two workgroups of 10 waves do share a CU (20 waves; each has its own table copy and half of
    // the LDS, so tiles are shorter): against 16 x 8 chunks, 2 x 10 x 6 chunks measures -3.2 % on configs[1], -1.2 % with the
    // default flags (-8 % and 0 on another box: see `sparse` below); with k = 7 (a table of 20 KB per copy) only
    // 5 chunks and a small record stage fit and it loses 37 %.  So: considered only for window scans with byte tables, at least
    // 6 chunks, a record stage of 256 and all accumulator copies; its factor is what those measurements give under the
    // instruction model below.  (Read batches: +4 % on one box, -1 % on another, where the predicate kernel that runs beside
    // the scan finds fewer free registers; they stay on one workgroup.)
    // What the extra waves hide is the latency chains of the per-match work: the gain needs matches.  On random sequence a
    // position matches with probability patterns / 4^k: 3 % for configs[1] (-2.7 % at 1 Gb) and for a k = 5 motif with one
    // mismatch (-3 %); 0.9 % with the default flags and 0.05 % with -x 0 (both +-1 %): those stay on 16 waves
    // (profiles/r02/planner_check.txt).
    const bool sparse = (double)in.n_patterns < 0.015 * (double)(1ull << (2 * k));
    static const struct { uint32_t waves, wgs; double factor; } kOccupancy[] = {
        {16, 1, 1.0}, {10, 2, 1.06}, {12, 1, 0.88}, {8, 1, 0.69}, {4, 1, 0.43}, {2, 1, 0.22}, {1, 1, 0.11}};
    uint32_t nch_min = 1;
    if (!tips) nch_min = (uint32_t)ceil_div((uint64_t)(1 + kp.halo_blocks) * kp.s + 63, TS_CHUNK);
    const uint32_t pin_waves = in.pin_waves, pin_nch = in.pin_nch, pin_stage = in.pin_stage, pin_wgs = in.pin_wgs;
    const uint32_t nch_max = tips ? std::max(kTipsChunks, pin_nch) : std::max(nch_min, std::max(kMaxChunks, pin_nch));
    double best = 0.0;
    TsScanParams best_kp{};
    uint32_t best_wpt = 0;
    for (const auto &occ : kOccupancy) {
        if (pin_waves && occ.waves != pin_waves) continue;
        const uint32_t wgs = (pin_waves && pin_wgs >= 1 && pin_wgs <= 4) ? pin_wgs : occ.wgs;
        const uint32_t kMaxLds = TS_CU_LDS_BYTES / wgs;
        for (uint32_t nch = nch_min; nch <= nch_max; ++nch) {
            if (nch * TS_CHUNK + 64u > 65535u) break;        // the match queue holds 16-bit plane coordinates
            if (pin_nch && nch != pin_nch) continue;
            TsScanParams cand = kp;
            cand.waves_per_wg = occ.waves;
            cand.wgs_per_cu = wgs;
            cand.nch = nch;
            cand.stage_u16 = (positions_fit14(nch) && !in.stage_u32) ? 1u : 0u;      // (position << 2 | flags) in 16 bits: the stage's entries
            const uint32_t span_max = nch * TS_CHUNK - 63u;
            uint32_t cwpt;
            if (tips) {
                const uint32_t tb = span_max & ~15u;            // one pseudo block per tile
                cand.s = cand.w = tb;
                cand.s_inv = (65536u + tb - 1u) / tb;
                cand.max_windows = 1;
                cwpt = 1;
            } else {
                const uint32_t nblk = span_max / cand.s;
                cwpt = nblk > cand.halo_blocks ? std::min<uint32_t>(nblk - cand.halo_blocks, kMaxBlocksPerTile) : 0u;
                cand.max_windows = cwpt;
            }
            // staging room for match records: what is left of the CU's LDS, 64 .. 1024 records per wave
            cand.stage_cap = 128;
            cand.acc_copies = 4;             // (8 copies measured no better than 4; the LDS goes to the record stage)
            while (cand.acc_copies > 1 && lds_total(cand) > kMaxLds) cand.acc_copies >>= 1;
            if (cwpt < 1 || lds_total(cand) > kMaxLds) continue;
            {
                const uint32_t spare = (kMaxLds - lds_total(cand)) / occ.waves / (cand.stage_u16 ? 2u : 4u);
                cand.stage_cap = std::min<uint32_t>(pin_stage ? pin_stage : 1024u, 128u + (spare & ~15u));
                while (lds_total(cand) > kMaxLds) cand.stage_cap -= 16;
            }
            // (the kernels for the 2-bit tables of k >= 7 need 97 VGPRs: built for 80 they spill)
            if (wgs > 1 && !(kp.pair_byte_table && kp.fc_byte_table)) continue;      // not built: it would spill (kernels.hip: scan_variant)
            if (wgs > 1 && !pin_waves && (tips || sparse || !(kp.pair_byte_table && kp.fc_byte_table) || nch < 6 || cand.stage_cap < 256 || cand.acc_copies < 4)) continue;
            const double passes = tips ? 0.0 : (double)ceil_div((uint64_t)cwpt * 4, 64);
            // fewer accumulator copies serialise the window adds of a pass: 8 chunks with 2 copies measured 2.5 %
            // slower than 7 chunks with 4 on the headline configuration, where the model alone says 1 % faster
            const double copies = cand.acc_copies >= 4 ? 1.0 : cand.acc_copies == 2 ? 0.96 : 0.92;
            // a stage that holds a tile of random sequence whole (its matches at the pattern set's density, + 15 % + most of a pass) lets
            // the records leave once, at the tile's end; a smaller one flushes from inside the chunk loop, where a store sits in
            // the memory queue ahead of the chunk loads that are waited for next
            const double tile_records = (double)in.n_patterns / (double)(1ull << (2 * std::min<uint32_t>(k, 16))) * (double)cwpt * cand.s;
            const double whole = (double)cand.stage_cap >= 1.15 * tile_records + 48.0 ? 1.0 : 0.93;
            const double score = (double)cwpt * cand.s * occ.factor * copies * whole / (470.0 * nch + 170.0 * passes + 100.0);
            if (score > best) { best = score; best_kp = cand; best_wpt = cwpt; }
        }
    }
    if (best <= 0.0) return false;
    kp = best_kp; wpt = best_wpt;
    {   // the exact 22-bit magic of the step, where it exists for every position of a tile (see kernels.hip: the per-match pass)
        const uint64_t s64 = std::max<uint32_t>(kp.s, 1), magic = ((1ull << 22) + s64 - 1) / s64, err = magic * s64 - (1ull << 22);
        const uint64_t max_u = (uint64_t)kp.nch * TS_CHUNK + 64u;
        kp.s_magic22 = (uint32_t)magic;
        kp.div_exact = (!tips && magic < (1u << 24) && max_u < (1u << 24) && max_u * magic < (1ull << 32) && max_u * err < (1ull << 22)) ? 1u : 0u;
    }
    kp.vis_wide = positions_fit14(kp.nch) ? 0u : 1u;
    return true;
}

struct Region {                     // one scanned interval of a segment
    uint64_t start, len;            // relative to the segment
    uint32_t first_tile, n_tiles;
    uint64_t tile_bases;            // owned bases per tile
};

struct SegPlan {
    uint64_t len = 0, abs_pos = 0;
    uint64_t in_off = 0;            // byte offset in the (whole-batch) input layout
    uint64_t win_base = 0, n_windows = 0;
    uint32_t first_tile = 0, n_tiles = 0;
    std::vector<Region> regions;
};

// Grid, waves and per-wave capacities of a launch over a tile range (size_launch)
struct LaunchSizes {
    uint32_t grid = 0, total_waves = 0;
    uint32_t region_cap = 0;                // match records per wave region
    uint32_t vis_cap = 0;                   // visible records per wave region
    uint64_t match_cap = 0;
    bool dealt_tiles = false;               // tiles dealt round-robin instead of taken on demand (see ts_batch_scan)
};

// A PLAN over all the segments of a batch (tiles, window records, input layout), the tile range [tile_lo, tile_hi) it executes
// and the sizes of that range's launch.
struct TiledPlan : LaunchSizes {
    PlanInputs in;
    bool tips = false;
    std::vector<SegPlan> segs;
    std::vector<TsTile> tiles;      // the whole plan
    TsScanParams kp{};
    uint32_t wpt = 1;               // windows per tile
    uint32_t lds_bytes = 0;
    uint64_t total_bases = 0, input_bytes = 0, n_windows = 0, match_cap_request = 0;
    // executed range and what it covers
    uint64_t tile_lo = 0, tile_hi = 0, win_lo = 0, win_hi = 0, in_lo = 0, in_hi = 0, range_bases = 0;
    uint64_t range_tiles() const { return tile_hi - tile_lo; }
    bool whole() const { return tile_lo == 0 && tile_hi == tiles.size(); }
    uint64_t tile_bases() const { return (uint64_t)wpt * kp.s; }        // owned bases of a full tile
};

inline void add_region_tiles(TiledPlan &p, SegPlan &sp, uint32_t seg_index, uint64_t start, uint64_t len,
                             uint64_t tile_bases, uint64_t windows_per_tile, bool windows) {
    Region rg{start, len, (uint32_t)p.tiles.size(), 0, tile_bases};
    const uint64_t nt = ceil_div(len, tile_bases);
    for (uint64_t j = 0; j < nt; ++j) {
        TsTile t{};
        const uint64_t u0 = j * tile_bases;
        const uint64_t rem = len - u0;
        t.in_off = sp.in_off + start + u0;
        t.nrel = (uint32_t)std::min<uint64_t>(rem, 1u << 30);
        if (windows) {
            const uint64_t wins_left = sp.n_windows - j * windows_per_tile;
            t.nwin = (uint32_t)std::min<uint64_t>(wins_left, windows_per_tile);
            t.win_out = sp.win_base + j * windows_per_tile;
        } else {
            t.nwin = 1;
            t.win_out = 0;
        }
        t.own_len = (uint32_t)std::min<uint64_t>(rem, tile_bases);
        t.seg = seg_index;
        p.tiles.push_back(t);
    }
    rg.n_tiles = (uint32_t)nt;
    sp.regions.push_back(rg);
}

// The segments of a plan whose geometry is chosen (kp, wpt): each at the next 16-byte boundary of the input layout, its windows
// behind the previous segment's, its scanned regions cut into tiles.  regions_of(len): the scanned regions of a segment — every
// driver hands over scanned_regions of general_plan_core.h, the rule the tiled batches share with the general kernels' drivers.
// abs_pos may be null.  false: too many tiles in one batch.
template <typename RegionsOf>
bool plan_segments(TiledPlan &p, const uint64_t *seg_lens, const uint64_t *abs_pos, size_t n_segs, RegionsOf regions_of) {
    const uint64_t tile_bases = p.tile_bases();
    uint64_t off = 0, wins = 0;
    p.segs.resize(n_segs);
    for (size_t i = 0; i < n_segs; ++i) {
        SegPlan &sp = p.segs[i];
        sp.len = seg_lens[i];
        sp.abs_pos = abs_pos ? abs_pos[i] : 0;
        sp.in_off = off;
        off += (sp.len + 15) & ~15ull;
        sp.first_tile = (uint32_t)p.tiles.size();
        if (!p.tips) {
            sp.win_base = wins;
            sp.n_windows = ceil_div(sp.len, p.in.step);
            wins += sp.n_windows;
        }
        for (const Span &r : regions_of(sp.len))
            add_region_tiles(p, sp, (uint32_t)i, r.start, r.len, tile_bases, p.tips ? 1 : p.wpt, !p.tips);
        sp.n_tiles = (uint32_t)p.tiles.size() - sp.first_tile;
        p.total_bases += sp.len;
    }
    p.input_bytes = off + TS_IN_PAD;
    p.n_windows = wins;
    return p.tiles.size() < 0x7FFFFFFFull;
}

// What the tile range [lo, hi) covers: window records, bytes of the input layout, owned bases
struct RangeCover { uint64_t window_begin = 0, window_end = 0, input_begin = 0, input_end = 0, bases = 0; };

inline RangeCover range_cover(const TiledPlan &p, uint64_t lo, uint64_t hi) {
    RangeCover r;
    if (lo >= hi) return r;
    const TsTile &first = p.tiles[lo];
    r.window_begin = p.tips ? 0 : first.win_out;
    r.window_end = r.window_begin;
    r.input_begin = first.in_off & ~15ull;
    uint64_t in_end = 0;
    for (uint64_t t = lo; t < hi; ++t) {
        const TsTile &T = p.tiles[t];
        r.bases += T.own_len;
        if (!p.tips) r.window_end = std::max<uint64_t>(r.window_end, T.win_out + T.nwin);
        // what ts_scan_tiles loads for this tile: nch chunks of TS_CHUNK positions from the 16-byte-aligned
        // address at or below its first base, each lane 32 bytes (the last lane reaches 32 bytes past a chunk)
        const uint32_t sh = (uint32_t)(T.in_off & 15ull);
        const uint64_t span = (uint64_t)(T.nwin + p.kp.halo_blocks) * p.kp.s;
        const uint64_t need = sh + std::min<uint64_t>(T.nrel, span + 16u);
        uint64_t nch = (need + 16u + TS_CHUNK - 1u) / TS_CHUNK;
        nch = std::min<uint64_t>(std::max<uint64_t>(nch, 1), p.kp.nch);
        in_end = std::max<uint64_t>(in_end, (T.in_off - sh) + nch * TS_CHUNK + 64u);
    }
    r.input_end = std::min<uint64_t>(in_end, p.input_bytes);
    return r;
}

// ---------------------------------------------------------------------------------------- the terminal zone of a tile
// ts_is_terminal on the tile-relative positions u of the tile that starts at rel0 of a segment of seg_len bases:
// u is terminal iff u < lo || u >= hi
struct TileZone { uint64_t lo, hi; };

inline TileZone tile_zone(uint64_t rel0, uint64_t seg_len, uint64_t terminal_limit) {
    const uint64_t term_end = ts_terminal_end(seg_len, terminal_limit);
    return {rel0 <= terminal_limit ? terminal_limit + 1 - rel0 : 0, term_end > rel0 ? term_end - rel0 : 0};
}
inline TileZone tile_zone(const TiledPlan &p, const TsTile &T) {
    const SegPlan &sp = p.segs[T.seg];
    return tile_zone(T.in_off - sp.in_off, sp.len, p.in.terminal_limit);
}

// ... as the kernel reads it (TsScanParams.tile_zone): two 16-bit thresholds, saturating (tile positions stay below 0xFFFF)
inline uint32_t zone_word(const TileZone &z) {
    return (uint32_t)std::min<uint64_t>(z.lo, 0xFFFF) | ((uint32_t)std::min<uint64_t>(z.hi, 0xFFFF) << 16);
}

// ... and whether one of the tile's owned positions is terminal
inline bool touches_zone(const TileZone &z, uint32_t own_len) { return own_len > 0 && (z.lo > 0 || z.hi < own_len); }

// The zone words of the executed range, + one TS_ZONE_NONE behind them
inline std::vector<uint32_t> zone_words(const TiledPlan &p) {
    const size_t nt = (size_t)p.range_tiles();
    std::vector<uint32_t> zone(nt + 1, TS_ZONE_NONE);
    for (size_t i = 0; i < nt; ++i) zone[i] = zone_word(tile_zone(p, p.tiles[p.tile_lo + i]));
    return zone;
}

// Owned bases of the tiles of [lo, hi) that touch a terminal zone
inline uint64_t zone_bases(const TiledPlan &p, uint64_t lo, uint64_t hi) {
    uint64_t n = 0;
    for (uint64_t t = lo; t < hi; ++t)
        if (touches_zone(tile_zone(p, p.tiles[t]), p.tiles[t].own_len)) n += p.tiles[t].own_len;
    return n;
}

// Visible records (kp.emit) expected of `bases` owned bases, `zone` of them in tiles that touch a terminal zone: canonical matches
// at their density on random sequence (+ 50 %), every match of a terminal zone (a few per cent of its bases; every k-th base
// inside a telomere)
inline uint64_t visible_estimate(const PlanInputs &in, uint64_t bases, uint64_t zone) {
    const double d_canon = (double)std::max<uint64_t>(in.n_canonical, 1) / (double)(1ull << (2 * std::min<uint32_t>(in.k, 16)));
    return (uint64_t)((double)bases * d_canon * 1.5) + zone / 8;
}

// Sizes the launch (one or two persistent workgroups per CU, whose waves take tiles or are dealt them) and the per-wave
// record regions for the tile range [lo, hi) of `bases` owned bases.  Every wave appends to its own region of the match buffer;
// small ranges get the worst case (every base a match), large ones bases/4 spread evenly, grown on overflow
// by ts_batch_sync (worst case for wave w = the owned bases of the tiles it is dealt: t = w, w + waves, ...).
// vis_cap_override: TS_VIS_CAP as the driver read it for this range (tests: force the overflow -> regrow -> rescan path); 0: none
inline LaunchSizes size_launch(const TiledPlan &p, uint64_t lo, uint64_t hi, uint64_t bases, int num_cu, uint64_t vis_cap_override) {
    LaunchSizes L;
    const uint32_t wpw = p.kp.waves_per_wg;
    const uint64_t nt = hi - lo;
    const int ncu = num_cu > 0 ? num_cu : 256;
    L.grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ceil_div(nt, wpw), 1), (uint64_t)ncu * std::max<uint32_t>(p.kp.wgs_per_cu, 1));
    L.total_waves = L.grid * wpw;
    uint64_t worst = 256;
    {
        std::vector<uint64_t> per_wave(L.total_waves, 0);
        for (uint64_t t = 0; t < nt; ++t) per_wave[t % L.total_waves] += p.tiles[lo + t].own_len;
        for (uint64_t v : per_wave) worst = std::max(worst, v);
    }
    const uint64_t want = p.match_cap_request ? p.match_cap_request : bases / 4 + 4096;
    uint64_t cap = ceil_div(want, L.total_waves);
    // Tiles are taken on demand by the waves (see ts_scan_tiles); dealt round-robin to small ranges, whose regions are
    // sized for the worst case of the tiles a wave is dealt, and to the rescans after an overflow.
    L.dealt_tiles = bases <= (64ull << 20) && !p.match_cap_request;
    if (L.dealt_tiles) cap = worst;
    cap = std::min<uint64_t>(std::max<uint64_t>(cap, 256), worst);
    L.region_cap = (uint32_t)((cap + 3) & ~3ull);
    L.match_cap = (uint64_t)L.region_cap * L.total_waves;
    // visible records (kp.emit): twice the even share of the estimate per wave, grown on overflow
    L.vis_cap = 0;
    if (!p.tips) {
        const uint64_t vwant = visible_estimate(p.in, bases, zone_bases(p, lo, hi));
        // (which wave scans which tile is decided at run time: a wave may take several of the few tiles that lie in a telomere,
        // where every k-th base is a visible record — room for a dozen of those per wave, so that an overflow, which costs a
        // rescan with dealt tiles, stays an event for inputs that are telomere through and through)
        const uint64_t tile_bases = (uint64_t)p.wpt * std::max<uint32_t>(p.kp.s, 1);
        uint64_t vcap = 2 * ceil_div(vwant, L.total_waves) + 12 * ceil_div(tile_bases, std::max<uint32_t>(p.in.k, 1)) + 2048;
        if (L.dealt_tiles && !p.match_cap_request) vcap = worst;          // small ranges: the worst case, like the record regions
        vcap = std::min<uint64_t>(vcap, std::max<uint64_t>(worst, 256));
        if (vis_cap_override) vcap = vis_cap_override;
        L.vis_cap = (uint32_t)((vcap + 7) & ~7ull);
    }
    return L;
}

// Makes [lo, hi) the range the plan executes: what it covers and the sizes of its launch
inline void set_range(TiledPlan &p, uint64_t lo, uint64_t hi, int num_cu, uint64_t vis_cap_override) {
    const RangeCover r = range_cover(p, lo, hi);
    p.tile_lo = lo; p.tile_hi = hi;
    p.win_lo = r.window_begin; p.win_hi = r.window_end;
    p.in_lo = r.input_begin; p.in_hi = r.input_end;
    p.range_bases = r.bases;
    if (lo == 0 && hi == p.tiles.size()) {          // the whole plan: every byte of the layout, every window
        p.in_lo = 0; p.in_hi = p.input_bytes;
        p.win_lo = 0; p.win_hi = p.n_windows;
    }
    static_cast<LaunchSizes &>(p) = size_launch(p, lo, hi, p.range_bases, num_cu, vis_cap_override);
}

// The whole plan of a batch, executing all of it.  The caller has set p.in; p is otherwise fresh.
enum class PlanStatus { ok, no_fit, too_many_tiles };

template <typename RegionsOf>
PlanStatus plan_batch(TiledPlan &p, bool tips, const uint64_t *seg_lens, const uint64_t *abs_pos, size_t n_segs, RegionsOf regions_of,
                      uint64_t match_capacity, int num_cu, uint64_t vis_cap_override) {
    p.tips = tips;
    uint32_t wpt = 1;
    if (!plan_geometry(p.in, tips, p.kp, wpt)) return PlanStatus::no_fit;
    p.wpt = wpt;
    p.lds_bytes = lds_total(p.kp);
    p.match_cap_request = match_capacity;
    if (!plan_segments(p, seg_lens, abs_pos, n_segs, regions_of)) return PlanStatus::too_many_tiles;
    set_range(p, 0, p.tiles.size(), num_cu, vis_cap_override);
    return PlanStatus::ok;
}

// After an overflow: the capacity for the fullest wave's count of the scan before (+ 1/8 + 64; the counts of a scan with dealt
// tiles are those of the next)
inline uint32_t regrown_region_cap(uint32_t worst) { return (uint32_t)(((uint64_t)worst + worst / 8 + 64 + 3) & ~3ull); }
inline uint32_t regrown_vis_cap(uint32_t worst_vis) { return (uint32_t)(((uint64_t)worst_vis + worst_vis / 8 + 64 + 7) & ~7ull); }

// Every u32 of the three result arrays fits 16 bits (the exchange's wire).  records: (position << 2 | flags) with
// position < nch * TS_CHUNK + 64 <= 2^14; tile counts <= a tile's bases; window fields: nucleotide counts <= w, covered
// bases = k x matches <= k x w
inline bool wire16_ok(const TiledPlan &p) {
    return positions_fit14(p.kp.nch) && (p.tips || (uint64_t)p.in.k * p.in.window_size <= 65535u);
}

// ------------------------------------------------------------------------------------------------------------ shards
// A shard of a plan (shard.cpp): the tiles it owns, the tiles it scans (owned + context), the segments with an owned tile
struct ShardRange {
    uint64_t own_lo, own_hi, ext_lo, ext_hi;
    uint64_t seg_begin, n_segs;
};
// ... and the layout of its result message
struct ShardLayout {
    uint64_t off_segs, off_windows, off_tilevis, off_visible, off_blocks, bytes;
    uint64_t visible_capacity;
    uint32_t block_capacity, window_bytes, visible_bytes, field_bits;
    uint64_t n_windows;
};

struct ShardGeom { uint64_t tile_bases; uint32_t ctx, zone, margin; };

// context tiles: enough that a record beyond them cannot chain (gap <= -k) to one in an owned tile across an empty
// context, and at least two; zone tiles: those holding positions [0, terminal_limit]
inline ShardGeom shard_geom(const TiledPlan &p) {
    ShardGeom g{};
    g.tile_bases = std::max<uint64_t>((uint64_t)p.wpt * p.kp.s, 1);
    if (p.tips) { g.ctx = 0; g.zone = 0; g.margin = 0; return g; }
    g.ctx = (uint32_t)std::max<uint64_t>(2, ceil_div((uint64_t)p.in.max_match_dist + p.in.k + 1, g.tile_bases) + 1);
    g.zone = (uint32_t)std::min<uint64_t>(ceil_div((uint64_t)p.in.terminal_limit + 1, g.tile_bases), 0x3FFFFFFFull);
    g.margin = g.zone + g.ctx;
    return g;
}

// Boundaries of the split into n_parts: part q owns tiles [out[q], out[q + 1]).  Consecutive ranges of equal owned bases (tiles
// are near-equal work), the boundaries moved — by at most the terminal zone + context of a segment — so that none falls near a
// segment's end.
inline void shard_boundaries(const TiledPlan &p, uint32_t n_parts, std::vector<uint64_t> &out) {
    const ShardGeom g = shard_geom(p);
    const uint64_t nt = p.tiles.size();
    out.assign((size_t)n_parts + 1, nt);
    out[0] = 0;
    uint64_t total = 0;
    for (const TsTile &T : p.tiles) total += T.own_len;
    // where equal bases would cut: the first tile whose preceding owned bases reach q / n_parts of the total
    uint64_t acc = 0, t = 0;
    for (uint32_t q = 1; q < n_parts; ++q) {
        const unsigned __int128 target = (unsigned __int128)total * q;
        for (; t < nt; ++t) {
            if ((unsigned __int128)acc * n_parts >= target) break;
            acc += p.tiles[t].own_len;
        }
        uint64_t cut = t;
        if (cut > 0 && cut < nt) {
            const SegPlan &sp = p.segs[p.tiles[cut].seg];
            const uint64_t f = sp.first_tile, e = f + sp.n_tiles;
            if (cut != f) {
                uint64_t lo, hi;                                     // the allowed positions either side of the cut
                if (p.tips || e - f < 2ull * g.margin) { lo = f; hi = e; }
                else if (cut - f < g.margin) { lo = f; hi = f + g.margin; }
                else if (e - cut < g.margin) { lo = e - g.margin; hi = e; }
                else { lo = hi = cut; }
                cut = (cut - lo <= hi - cut) ? lo : hi;
            }
        }
        out[q] = std::max(cut, out[q - 1]);
    }
}

inline ShardRange shard_range(const TiledPlan &p, uint32_t n_parts, uint32_t part) {
    std::vector<uint64_t> cut;
    shard_boundaries(p, n_parts, cut);
    const ShardGeom g = shard_geom(p);
    ShardRange r{};
    r.own_lo = cut[part]; r.own_hi = cut[part + 1];
    r.ext_lo = r.own_lo; r.ext_hi = r.own_hi;
    if (r.own_hi > r.own_lo) {
        const uint64_t nt = p.tiles.size();
        if (r.own_lo > 0 && p.segs[p.tiles[r.own_lo].seg].first_tile != r.own_lo) r.ext_lo = r.own_lo - g.ctx;
        if (r.own_hi < nt && p.segs[p.tiles[r.own_hi].seg].first_tile != r.own_hi) r.ext_hi = r.own_hi + g.ctx;
        r.seg_begin = p.tiles[r.own_lo].seg;
        r.n_segs = p.tiles[r.own_hi - 1].seg - r.seg_begin + 1;
    }
    return r;
}

inline uint32_t bit_width_u32(uint32_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b ? b : 1u; }
inline uint64_t align16u(uint64_t v) { return (v + 15ull) & ~15ull; }

// Sizes of a shard's message.  The variable sections (visible records, blocks) get capacities estimated from the plan —
// the visible-record estimate of the owned tiles, a block or two per segment — times `scale`; a message that overflows says so
// in its header and the caller packs again with a larger scale.
inline ShardLayout shard_layout(const TiledPlan &p, const ShardRange &r, uint32_t scale) {
    ShardLayout L{};
    if (scale == 0) scale = 1;
    {
        uint64_t w0 = 0, w1 = 0;
        if (!p.tips && r.own_hi > r.own_lo) {
            w0 = p.tiles[r.own_lo].win_out;
            const TsTile &last = p.tiles[r.own_hi - 1];
            w1 = last.win_out + last.nwin;
        }
        L.n_windows = w1 - w0;
    }
    L.field_bits = bit_width_u32(p.in.window_size);
    L.window_bytes = p.tips ? 0u : (uint32_t)(((p.in.nuc ? 7u : 3u) * L.field_bits + 7u) / 8u);
    L.visible_bytes = wire16_ok(p) ? 2u : 4u;
    uint64_t own_bases = 0;
    for (uint64_t t = r.own_lo; t < r.own_hi; ++t) own_bases += p.tiles[t].own_len;
    uint64_t vis = p.tips ? 0 : visible_estimate(p.in, own_bases, zone_bases(p, r.own_lo, r.own_hi)) + 65536;
    vis = std::min<uint64_t>(vis * scale, own_bases + 16);
    L.visible_capacity = (vis + 7ull) & ~7ull;
    L.block_capacity = (uint32_t)std::min<uint64_t>((16ull * r.n_segs + 256ull) * scale, 1u << 24);
    uint64_t o = sizeof(TsShardHeader);
    L.off_segs = o; o = align16u(o + r.n_segs * sizeof(TsShardSeg));
    L.off_windows = o; o = align16u(o + L.n_windows * L.window_bytes);
    L.off_tilevis = o; o = align16u(o + (r.own_hi - r.own_lo) * 2ull);
    L.off_visible = o; o = align16u(o + L.visible_capacity * L.visible_bytes);
    L.off_blocks = o; o = align16u(o + (uint64_t)L.block_capacity * sizeof(TsDevBlock));
    L.bytes = o;
    return L;
}

}  // namespace tsplan

#endif
