// tiled_plan_host.cpp — TEST INFRASTRUCTURE: the host plan of the tiled scan kernel (teloscope_amd/csrc/tiled_plan_core.h over
// the LDS layout of scan_lds_core.h) run by a program of its own under AddressSanitizer and UBSan, so that
// tests/test_tiled_plan_cpu.py can hold the code capi.cpp and shard.cpp call to a plain restatement of the rules.
// Usage: tiled_plan_host < CASES.  One case per line, numbers only behind the kind; one line of output per case.
//   INPUTS = tips step w terminal_limit max_match_dist fold nuc k n_patterns n_canonical table_rows fc_bytes fc_byte pair_byte
//            pin_waves pin_nch pin_stage pin_wgs acc_per_window stage_u32                                   (20 numbers)
//   PLAN   = INPUTS vis_cap_override match_capacity num_cu n_segs len...         (abs_pos of segment i is 7 i)
//   geom INPUTS           ->  geom nofit | geom wgs waves nch wpt lds stage_cap stage_u16 acc_copies div_exact s_magic22 vis_wide
//                             halo s w max_windows acc_blocks block_sums nuc_on windows_on straddle s_inv fold_mask kdist :
//                             codes rec wacc stage park bytes queue_region
//   tiles PLAN            ->  tiles input_bytes n_windows total_bases n : in_off,win_out,nrel,nwin,own_len,seg ... |
//                             len,abs_pos,in_off,win_base,n_windows,first_tile,n_tiles ...
//   cover PLAN            ->  cover n : window_begin,window_end,input_begin,input_end,bases ...    for lo in [0, n], hi in [lo, n]
//   zone PLAN             ->  zone n zone_bases : lo,hi,word,touches ... | the n + 1 zone words of the whole range
//   launch PLAN lo hi     ->  launch grid waves region_cap match_cap dealt vis_cap : win_lo win_hi in_lo in_hi range_bases
//   regrow worst worst_vis -> regrow region_cap vis_cap
//   shard PLAN parts scale -> shard ctx zone margin wire16 : cut ... | own_lo,own_hi,ext_lo,ext_hi,seg_begin,n_segs,off_segs,
//                             off_windows,off_tilevis,off_visible,off_blocks,bytes,visible_capacity,block_capacity,window_bytes,
//                             visible_bytes,field_bits,n_windows ...
//   refusals (geometry that does not fit, too many tiles) print the kind and "nofit" / "toomany"
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/tiled_plan_core.h"

namespace {

typedef unsigned long long ull;

struct Args {
    std::vector<ull> v;
    size_t at = 0;
    ull next() {
        if (at >= v.size()) { std::fprintf(stderr, "short case\n"); std::exit(2); }
        return v[at++];
    }
};

tsplan::PlanInputs read_inputs(Args &a, bool &tips) {
    tsplan::PlanInputs in;
    tips = a.next() != 0;
    in.step = (uint32_t)a.next(); in.window_size = (uint32_t)a.next();
    in.terminal_limit = (uint32_t)a.next(); in.max_match_dist = (uint32_t)a.next();
    in.fold_case = a.next() != 0; in.nuc = a.next() != 0;
    in.k = (uint32_t)a.next(); in.n_patterns = a.next(); in.n_canonical = a.next();
    in.table_rows = (uint32_t)a.next(); in.fc_bytes = (uint32_t)a.next();
    in.fc_byte_table = a.next() != 0; in.pair_byte_table = a.next() != 0;
    in.pin_waves = (uint32_t)a.next(); in.pin_nch = (uint32_t)a.next(); in.pin_stage = (uint32_t)a.next(); in.pin_wgs = (uint32_t)a.next();
    in.acc_per_window = a.next() != 0; in.stage_u32 = a.next() != 0;
    return in;
}

tsplan::PlanStatus read_plan(Args &a, tsplan::TiledPlan &p, int &num_cu, uint64_t &vis_cap) {
    bool tips;
    p.in = read_inputs(a, tips);
    vis_cap = a.next();
    const uint64_t cap = a.next();
    num_cu = (int)a.next();
    const size_t n = (size_t)a.next();
    std::vector<uint64_t> lens(n), pos(n);          // (exactly n long: a read past the segments is a sanitizer error)
    for (size_t i = 0; i < n; ++i) { lens[i] = a.next(); pos[i] = 7 * i; }
    const uint32_t tl = p.in.terminal_limit;
    return tsplan::plan_batch(p, tips, lens.data(), pos.data(), n, [=](uint64_t len) { return tsplan::scanned_regions(len, tips, tl); }, cap, num_cu, vis_cap);
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string kind;
        if (!(ss >> kind)) continue;
        Args a;
        for (ull x; ss >> x;) a.v.push_back(x);
        if (kind == "geom") {
            bool tips;
            const tsplan::PlanInputs in = read_inputs(a, tips);
            TsScanParams kp{};
            uint32_t wpt = 0;
            if (!tsplan::plan_geometry(in, tips, kp, wpt)) { std::printf("geom nofit\n"); continue; }
            const SliceLayout s = slice_layout(kp);
            std::printf("geom %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u : %u %u %u %u %u %u %u\n", kp.wgs_per_cu, kp.waves_per_wg,
                        kp.nch, wpt, lds_total(kp), kp.stage_cap, kp.stage_u16, kp.acc_copies, kp.div_exact, kp.s_magic22, kp.vis_wide,
                        kp.halo_blocks, kp.s, kp.w, kp.max_windows, kp.acc_blocks, kp.block_sums, kp.nuc_on, kp.windows_on, kp.straddle_fix,
                        kp.s_inv, kp.fold_mask, kp.kdist, s.codes, s.rec, s.wacc, s.stage, s.park, s.bytes, queue_region(kp));
            continue;
        }
        if (kind == "regrow") {
            const uint32_t w = (uint32_t)a.next(), wv = (uint32_t)a.next();
            std::printf("regrow %u %u\n", tsplan::regrown_region_cap(w), tsplan::regrown_vis_cap(wv));
            continue;
        }
        tsplan::TiledPlan p;
        int num_cu = 0;
        uint64_t vis_cap = 0;
        const tsplan::PlanStatus st = read_plan(a, p, num_cu, vis_cap);
        if (st != tsplan::PlanStatus::ok) {
            std::printf("%s %s\n", kind.c_str(), st == tsplan::PlanStatus::no_fit ? "nofit" : "toomany");
            continue;
        }
        const uint64_t nt = p.tiles.size();
        if (kind == "tiles") {
            std::printf("tiles %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " :", p.input_bytes, p.n_windows, p.total_bases, nt);
            for (const TsTile &T : p.tiles)
                std::printf(" %" PRIu64 ",%" PRIu64 ",%u,%u,%u,%u", T.in_off, T.win_out, T.nrel, T.nwin, T.own_len, T.seg);
            std::printf(" |");
            for (const tsplan::SegPlan &sp : p.segs)
                std::printf(" %" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%u,%u", sp.len, sp.abs_pos, sp.in_off, sp.win_base, sp.n_windows,
                            sp.first_tile, sp.n_tiles);
            std::printf("\n");
        } else if (kind == "cover") {
            std::printf("cover %" PRIu64 " :", nt);
            for (uint64_t lo = 0; lo <= nt; ++lo)
                for (uint64_t hi = lo; hi <= nt; ++hi) {
                    const tsplan::RangeCover r = tsplan::range_cover(p, lo, hi);
                    std::printf(" %" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64, r.window_begin, r.window_end, r.input_begin, r.input_end, r.bases);
                }
            std::printf("\n");
        } else if (kind == "zone") {
            std::printf("zone %" PRIu64 " %" PRIu64 " :", nt, tsplan::zone_bases(p, 0, nt));
            for (const TsTile &T : p.tiles) {
                const tsplan::TileZone z = tsplan::tile_zone(p, T);
                std::printf(" %" PRIu64 ",%" PRIu64 ",%u,%d", z.lo, z.hi, tsplan::zone_word(z), tsplan::touches_zone(z, T.own_len) ? 1 : 0);
            }
            std::printf(" |");
            for (uint32_t w : tsplan::zone_words(p)) std::printf(" %u", w);
            std::printf("\n");
        } else if (kind == "launch") {
            const uint64_t lo = a.next(), hi = a.next();
            tsplan::set_range(p, lo, hi, num_cu, vis_cap);
            std::printf("launch %u %u %u %" PRIu64 " %d %u : %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.grid, p.total_waves, p.region_cap,
                        p.match_cap, p.dealt_tiles ? 1 : 0, p.vis_cap, p.win_lo, p.win_hi, p.in_lo, p.in_hi, p.range_bases);
        } else if (kind == "shard") {
            const uint32_t parts = (uint32_t)a.next(), scale = (uint32_t)a.next();
            const tsplan::ShardGeom g = tsplan::shard_geom(p);
            std::vector<uint64_t> cut;
            tsplan::shard_boundaries(p, parts, cut);
            std::printf("shard %u %u %u %d :", g.ctx, g.zone, g.margin, tsplan::wire16_ok(p) ? 1 : 0);
            for (uint64_t c : cut) std::printf(" %" PRIu64, c);
            std::printf(" |");
            for (uint32_t q = 0; q < parts; ++q) {
                const tsplan::ShardRange r = tsplan::shard_range(p, parts, q);
                const tsplan::ShardLayout L = tsplan::shard_layout(p, r, scale);
                std::printf(" %" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64
                            ",%" PRIu64 ",%u,%u,%u,%u,%" PRIu64,
                            r.own_lo, r.own_hi, r.ext_lo, r.ext_hi, r.seg_begin, r.n_segs, L.off_segs, L.off_windows, L.off_tilevis, L.off_visible,
                            L.off_blocks, L.bytes, L.visible_capacity, L.block_capacity, L.window_bytes, L.visible_bytes, L.field_bits, L.n_windows);
            }
            std::printf("\n");
        } else {
            std::fprintf(stderr, "bad case: %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
