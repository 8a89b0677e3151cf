// general_batch.cpp — general tips batches: the device-resident read batch of pattern sets the tiled kernel does not take
// (mixed lengths, patterns of 9 bases or more, the wide form's up to 63 lengths of up to 63 bases).
//
// ts_batch_create(ctx, ..., tips_only = 1, ...) returns one on a context whose tips scans go to the general kernels.  It has the
// input layout of a tiled batch — whole segments back to back, each 16-byte aligned, TS_IN_PAD zero bytes behind the last — so
// that ts_batch_upload, ts_fastq_chunk_stage, ts_bam_chunk_decode and a caller's own d_input fill it as they fill any batch.
// Its tiles are TsGeneralTile over the regions scanSegment picks (the whole segment up to 2 x terminal limit, else the two tips);
// ts_batch_scan enqueues the fused tips pass of generic.hip and the slot offsets, ts_batch_read_pass the predicate over the
// records where that pass left them (blockcall.hip: ts_terminal_pass), ts_batch_terminal_ends the same walks in their ENDS form
// (ts_terminal_ends_walk).  For those calls only the fused pass's flag word ever comes back to the host:
// ts_batch_read_pass_status reads it, ts_batch_sync regrows the slots (or leaves the list form) and rescans.
// ts_batch_download_blocks calls the terminal blocks over the same slots and ts_batch_segment_summary adds up the tile directory.
#include "capi_internal.hpp"
#include "general_plan_core.h"

namespace {

const char kWayOut[] = "; the host routes (fastqSubset / bamSubset, ts_filter_reads) scan such a set in groups of bounded size";

// a block of the context's pool, or the batch's own error: an allocation that fails names the way out
int take(ts_ctx *c, size_t bytes, DevBuf &d, const char *what, const TsGeneralBatch &g) {
    if (c->pool.take(bytes, d) == hipSuccess) return TS_OK;
    (void)hipGetLastError();
    return c->fail(TS_ERR_ALLOC, "general read batch: cannot allocate " + std::to_string(bytes) + " bytes of device memory for " + what +
                                 " (" + std::to_string(g.tiles.size()) + " tiles, a slot of " + std::to_string(g.slot_cap) + " records each)" + kWayOut);
}

size_t slot_bytes(const TsGeneralBatch &g) { return std::max<size_t>(g.tiles.size(), 1) * (size_t)g.slot_cap * 4; }

// the walks' per-segment table: every segment with all its tiles, both ends its own
std::vector<TsShardSegIn> segment_table(const ts_batch *b) {
    std::vector<TsShardSegIn> segin(b->segs.size());
    for (size_t i = 0; i < segin.size(); ++i) {
        const SegPlan &sp = b->segs[i];
        segin[i] = tsplan::whole_segment_entry(sp.in_off, sp.len, sp.abs_pos, sp.first_tile, sp.n_tiles, (uint32_t)i);
    }
    return segin;
}

// Device state, once per batch: the tile list, the per-segment table of the fused pass {lengths, window bases, window counts:
// the last two zero for tips} with the flag word behind it, the predicate's tile list and segment table; and the buffers every
// scan writes.
int ensure_device(ts_batch *b) {
    ts_ctx *c = b->ctx;
    TsGeneralBatch &g = *b->gen;
    if (g.uploaded) return TS_OK;
    const size_t ns = b->segs.size(), nt = g.tiles.size();
    g.tab_flag = 3 * ns * 8;
    int rc;
    if ((rc = take(c, std::max<size_t>(nt, 1) * sizeof(TsGeneralTile), g.d_tiles, "the tile list", g)) != TS_OK) return rc;
    if ((rc = take(c, g.tab_flag + 16, g.d_tab, "the segment table", g)) != TS_OK) return rc;
    if ((rc = take(c, (nt + 1) * 16, g.d_stats, "the tile directory", g)) != TS_OK) return rc;
    if ((rc = take(c, (nt + 1) * 8, g.d_off, "the slot offsets", g)) != TS_OK) return rc;
    if ((rc = take(c, std::max<size_t>(nt, 1) * sizeof(TsTile), g.d_bct, "the predicate's tile list", g)) != TS_OK) return rc;
    if ((rc = take(c, std::max<size_t>(ns, 1) * sizeof(TsShardSegIn), g.d_segin, "the predicate's segment table", g)) != TS_OK) return rc;
    if ((rc = take(c, slot_bytes(g), g.d_slots, "the record slots", g)) != TS_OK) return rc;
    std::vector<unsigned long long> tab(3 * ns + 2, 0ull);
    const std::vector<TsShardSegIn> segin = segment_table(b);
    for (size_t i = 0; i < ns; ++i) tab[i] = b->segs[i].len;
    // (the walks take a tile's segment-relative position from in_off - the segment's: the layout's own offsets serve)
    std::vector<TsTile> bct(nt);
    for (size_t t = 0; t < nt; ++t) {
        TsTile &T = bct[t];
        T = TsTile{};
        T.in_off = g.tiles[t].in_off; T.own_len = T.nrel = g.tiles[t].n; T.seg = g.tiles[t].seg;
    }
    if (nt) HIP_TRY(c, hipMemcpy(g.d_tiles.p, g.tiles.data(), nt * sizeof(TsGeneralTile), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(g.d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    if (nt) HIP_TRY(c, hipMemcpy(g.d_bct.p, bct.data(), nt * sizeof(TsTile), hipMemcpyHostToDevice));
    if (ns) HIP_TRY(c, hipMemcpy(g.d_segin.p, segin.data(), ns * sizeof(TsShardSegIn), hipMemcpyHostToDevice));
    g.uploaded = true;
    return TS_OK;
}

// the fused pass's flag word (bit 0: a tile overflowed its slot, bit 1: a candidate list spilled), once the batch's stream is done
int read_flag(ts_batch *b, uint32_t &flag) {
    ts_ctx *c = b->ctx;
    hipStream_t st = (hipStream_t)b->last_stream;
    flag = 0;
    HIP_TRY(c, hipMemcpyAsync(&flag, (char *)b->gen->d_tab.p + b->gen->tab_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->read_batch_stats[3].fetch_add(4, std::memory_order_relaxed);
    return TS_OK;
}

// what the terminal walks read of the batch: the slots through the directory, the context's block parameters
TsBlockCallParams walk_params(const ts_batch *b) {
    const TsGeneralBatch &g = *b->gen;
    TsBlockCallParams Q = ts_general_walk_params(b->ctx, g.gen_lens, g.wide);
    Q.tiles = (const TsTile *)g.d_bct.p;
    Q.tile_off = (const unsigned long long *)g.d_off.p;
    Q.tile_stats = (const uint32_t *)g.d_stats.p;
    Q.matches = (const uint32_t *)g.d_slots.p;
    return Q;
}

}  // namespace

ts_batch *ts_general_batch_create(ts_ctx *ctx, const uint64_t *seg_lens, const uint64_t *abs_pos, size_t n_segs) {
    std::unique_ptr<ts_batch> b(new ts_batch());
    b->ctx = ctx;
    b->tips = true;
    b->gen.reset(new TsGeneralBatch());
    TsGeneralBatch &g = *b->gen;
    g.wide = ctx->gen_wide;
    g.Q = ts_general_geom(ctx);
    g.gen_lens = ts_general_gen_lens(ctx);
    const uint32_t s = std::max<uint32_t>(ctx->params.step, 1u), tl = ctx->params.terminal_limit;
    const uint32_t halo = g.wide ? (uint32_t)TS_WIDE_HALO : 32u;
    uint64_t off = 0, scanned = 0;
    b->segs.resize(n_segs);
    for (size_t i = 0; i < n_segs; ++i) {
        SegPlan &sp = b->segs[i];
        sp.len = seg_lens[i];
        sp.abs_pos = abs_pos ? abs_pos[i] : 0;
        sp.in_off = off;
        off += (sp.len + 15) & ~15ull;
        sp.first_tile = (uint32_t)g.tiles.size();
        for (const tsplan::Span &r : tsplan::scanned_regions(sp.len, true, tl)) {
            Region rg{r.start, r.len, (uint32_t)g.tiles.size(), 0, TS_GENERAL_TILE};
            tsplan::append_region_tiles(g.tiles, sp.in_off + r.start, r.start, r.len, (uint32_t)i, s, halo);
            rg.n_tiles = (uint32_t)g.tiles.size() - rg.first_tile;
            sp.regions.push_back(rg);
            scanned += r.len;
        }
        sp.n_tiles = (uint32_t)g.tiles.size() - sp.first_tile;
        b->total_bases += sp.len;
        if (g.tiles.size() >= 0x7FFFFFFFull) {
            ctx->fail(TS_ERR_UNSUPPORTED, "too many tiles in one batch");
            return nullptr;
        }
    }
    b->input_bytes = off + TS_IN_PAD;
    b->in_lo = 0; b->in_hi = b->input_bytes;
    b->range_bases = scanned;
    uint32_t largest = 0;
    bool aligned = true;
    for (const TsGeneralTile &T : g.tiles) {
        largest = std::max(largest, T.n);
        aligned = aligned && (T.in_off & 15ull) == 0;
    }
    // a slot per tile, sized by the largest tile of THIS batch (reads of 150 bases need no slot of 4096 records): one record per
    // position to begin with (the wide form: four), a record per position and length when that overflowed
    g.slot_unit = std::max<uint32_t>(4u, (largest + 3u) & ~3u);
    g.slot_cap = ts_general_slot_start(ctx, g.slot_unit);
    g.slot_max = ts_general_slot_max(ctx, g.slot_unit);
    // the list form loads a tile's bases 16 aligned bytes at a time: a second tip that starts off a 16-byte boundary (a segment
    // longer than 2 x terminal limit; never a read of a read filter) sends the batch to the strided form
    g.use_list = ts_general_list_form_ok(ctx) && aligned;
    return b.release();
}

void ts_general_batch_release(ts_batch *b) {
    TsGeneralBatch &g = *b->gen;
    for (DevBuf *d : {&g.d_tiles, &g.d_tab, &g.d_slots, &g.d_stats, &g.d_off, &g.d_bct, &g.d_segin, &g.d_sumtab}) b->ctx->pool.give(std::move(*d));
    g.uploaded = false;
}

int ts_general_batch_refuse(const ts_batch *b, const char *call) {
    return b->ctx->fail(TS_ERR_UNSUPPORTED, std::string(call) + ": not served by a general tips batch (the tips-only batch of a pattern set "
                                            "the general kernels scan); it takes ts_batch_segment_offset, _input_ptr, _upload, _scan, "
                                            "_read_pass, _terminal_ends, _read_pass_status, _sync, _download_blocks, "
                                            "_segment_summary, _get_info and _destroy");
}

// The fused tips pass (list or strided form, or the wide form) and the slot offsets, on `stream`; no host synchronisation beyond
// the first call's uploads.  Tips scans are in position order: the records stay in their slots.
int ts_general_batch_scan(ts_batch *b, const void *d_input, void *stream) {
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    TsGeneralBatch &g = *b->gen;
    if (!d_input) d_input = ts_batch_input_ptr(b);
    if (!d_input) return c->fail(TS_ERR_ALLOC, std::string("general read batch: cannot allocate the device input buffer") + kWayOut);
    { const int rc = ensure_device(b); if (rc != TS_OK) return rc; }
    if (!g.d_slots.p) { const int rc = take(c, slot_bytes(g), g.d_slots, "the record slots", g); if (rc != TS_OK) return rc; }   // (a regrow that failed)
    hipStream_t st = (hipStream_t)stream;
    const size_t ns = b->segs.size(), nt = g.tiles.size();
    b->last_input = d_input;
    b->last_stream = stream;
    b->scanned = true;
    b->synced = false;
    b->rb.called = false;
    char *const dt = (char *)g.d_tab.p;
    const unsigned long long *const tab_len = (const unsigned long long *)dt, *const tab_win = tab_len + ns, *const tab_nwin = tab_len + 2 * ns;
    uint32_t *const d_flag = (uint32_t *)(dt + g.tab_flag);
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        HIP_TRY(c, hipMemsetAsync(d_flag, 0, 16, st));
        const int rc = ts_general_launch_fused(c, d_input, (const TsGeneralTile *)g.d_tiles.p, (uint32_t)nt, tab_len, tab_win, tab_nwin, d_flag, true,
                                               g.slot_cap, (uint32_t *)g.d_stats.p, (uint32_t *)g.d_slots.p, nullptr, g.use_list, g.Q, st);
        if (rc != TS_OK) return rc;
        if (ts_k_launch_general_slot_offsets((unsigned long long *)g.d_off.p, (uint32_t)nt, g.slot_cap, st) != 0)
            return c->fail(TS_ERR_HIP, "slot-offset kernel launch failed");
    }
    c->read_batch_stats[0].fetch_add(1, std::memory_order_relaxed);
    return TS_OK;
}

// ReadTelomereFilter::matches (src/read-filter.cpp:37-45, reduced to !terminalBlocks.empty()) per segment: the terminal walks of
// device block calling in their pass form, over the slots.  One byte per segment to d_pass, on the scan's stream.
int ts_general_batch_read_pass(ts_batch *b, void *d_pass, void *stream) {
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    TsGeneralBatch &g = *b->gen;
    if (!b->scanned) return c->fail(TS_ERR_STATE, "ts_batch_read_pass needs a scanned, unrestricted tips-only batch");
    if (stream != b->last_stream) return c->fail(TS_ERR_STATE, "ts_batch_read_pass on a general tips batch: pass the stream of its scan");
    const TsBlockCallParams Q = walk_params(b);
    if (ts_k_launch_read_pass_general(&Q, (const TsShardSegIn *)g.d_segin.p, (uint32_t)b->segs.size(), (uint32_t)g.tiles.size(), g.slot_cap,
                                      (uint32_t *)g.d_stats.p, (unsigned char *)d_pass, stream) != 0)
        return c->fail(TS_ERR_HIP, "general read-pass kernel launch failed");
    c->read_batch_stats[1].fetch_add(b->segs.size(), std::memory_order_relaxed);
    return TS_OK;
}

// walkSegment's per-side maxima (src/input.cpp:835-881) per segment: the same walks in their ENDS form.  Two u32 per segment to
// d_ends, on the scan's stream; after an overflow they mean nothing, as the pass bytes do.
int ts_general_batch_terminal_ends(ts_batch *b, void *d_ends, void *stream) {
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    TsGeneralBatch &g = *b->gen;
    if (!b->scanned) return c->fail(TS_ERR_STATE, "ts_batch_terminal_ends needs a scanned, unrestricted tips-only batch");
    if (stream != b->last_stream) return c->fail(TS_ERR_STATE, "ts_batch_terminal_ends on a general tips batch: pass the stream of its scan");
    const TsBlockCallParams Q = walk_params(b);
    if (ts_k_launch_terminal_ends_general(&Q, (const TsShardSegIn *)g.d_segin.p, (uint32_t)b->segs.size(), (uint32_t)g.tiles.size(), g.slot_cap,
                                          (uint32_t *)g.d_stats.p, (uint32_t *)d_ends, stream) != 0)
        return c->fail(TS_ERR_HIP, "general terminal-ends kernel launch failed");
    c->terminal_ends_stats[1].fetch_add(b->segs.size(), std::memory_order_relaxed);
    return TS_OK;
}

// The terminal blocks of every segment as ordered rows in the batch's device memory (ts_batch_call_read_blocks, which made the
// tables and the rows' room): the same walks in their counting and placing forms, on the scan's stream.  After an overflow or a
// spill the rows mean nothing, as the pass bytes do; the walks stay inside the slots and the rows' room.
int ts_general_batch_call_read_blocks(ts_batch *b, void *stream) {
    ts_ctx *c = b->ctx;
    TsGeneralBatch &g = *b->gen;
    ReadBlocksState &R = b->rb;
    if (!b->scanned) return c->fail(TS_ERR_STATE, "ts_batch_call_read_blocks needs a scanned, unrestricted tips-only batch");
    if (stream != b->last_stream) return c->fail(TS_ERR_STATE, "ts_batch_call_read_blocks on a general tips batch: pass the stream of its scan");
    R.called = false;
    const size_t ns = b->segs.size();
    if (ns) {
        const TsBlockCallParams Q = walk_params(b);
        const ReadBlocksTab T(ns);
        char *const dt = (char *)R.d_tab.p;
        if (ts_k_launch_read_blocks(&Q, (const TsShardSegIn *)g.d_segin.p, (uint32_t)ns, (uint32_t)g.tiles.size(), g.slot_cap, (uint32_t *)g.d_stats.p,
                                    nullptr, 0u, 0u, nullptr, (uint32_t *)dt, (unsigned long long *)(dt + T.places),
                                    (unsigned long long *)(dt + T.first), dt + T.tmp, (TsReadBlockRow *)R.d_rows.p, R.row_cap, stream) != 0)
            return c->fail(TS_ERR_HIP, "general read-block kernel launch failed");
    }
    R.called = true; R.stream = stream;
    return TS_OK;
}

int ts_general_batch_place_read_blocks(ts_batch *b) {
    ts_ctx *c = b->ctx;
    const ReadBlocksState &R = b->rb;
    const TsBlockCallParams Q = walk_params(b);
    if (ts_k_launch_read_blocks_place(&Q, (const TsShardSegIn *)b->gen->d_segin.p, (uint32_t)b->segs.size(), nullptr,
                                      (const unsigned long long *)((char *)R.d_tab.p + ReadBlocksTab(b->segs.size()).places),
                                      (TsReadBlockRow *)R.d_rows.p, R.row_cap, R.stream) != 0)
        return c->fail(TS_ERR_HIP, "general read-block kernel launch failed");
    return TS_OK;
}

// The terminal blocks of every segment, called on the device over the slots in place (a tips scan is in position order: the
// host route's in-place case, pipeline.cpp: gen_blocks) and assembled as that route assembles them: no windows, no matches, no
// interstitial blocks.
int ts_general_batch_download_blocks(ts_batch *b, ts_segment_out *out) {
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    TsGeneralBatch &g = *b->gen;
    if (!b->synced) { const int rc = ts_batch_sync(b); if (rc != TS_OK) return rc; }
    hipStream_t st = (hipStream_t)b->last_stream;
    const size_t ns = b->segs.size(), nt = g.tiles.size();
    if (ts_k_launch_slot_counts((const uint32_t *)g.d_slots.p, g.slot_cap, (uint32_t)nt, (uint32_t *)g.d_stats.p, st) != 0)
        return c->fail(TS_ERR_HIP, "slot-count kernel launch failed");
    std::vector<TsDevBlock> blocks;
    const int rc = ts_device_block_call_raw(c, (const TsTile *)g.d_bct.p, (const unsigned long long *)g.d_off.p, (const uint32_t *)g.d_stats.p,
                                            (const uint32_t *)g.d_slots.p, 0, segment_table(b), nt, true, g.gen_lens, nullptr, nullptr, st,
                                            blocks, nullptr, 0, g.wide ? c->wpat.len : nullptr, false);
    if (rc != TS_OK) return rc;
    HostView v;
    v.tips = true;
    v.blocks = blocks.data(); v.n_blocks = blocks.size();
    v.segs.reserve(ns);
    for (const SegPlan &sp : b->segs) v.segs.push_back({sp.len, sp.abs_pos, 0, 0, sp.first_tile, sp.n_tiles});
    return ts_assemble_general(c, v, out);
}

// {0, matches, canonical, forward} per segment, four u64 each, to d_out on the scan's stream: the tile directory added up (the
// tiled batches' summary kernel; a tips scan has no windows).
int ts_general_batch_segment_summary(ts_batch *b, void *d_out, void *stream) {
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    TsGeneralBatch &g = *b->gen;
    if (!b->scanned) return c->fail(TS_ERR_STATE, "ts_batch_segment_summary needs a scanned batch");
    if (!b->synced) { const int rc = ts_batch_sync(b); if (rc != TS_OK) return rc; }
    if (stream != b->last_stream) return c->fail(TS_ERR_STATE, "ts_batch_segment_summary on a general tips batch: pass the stream of its scan");
    const size_t ns = b->segs.size(), nt = g.tiles.size();
    const size_t bytes_first = ((ns + 1) * 4 + 15) & ~(size_t)15;
    if (!g.d_sumtab.p) {
        std::vector<char> tab(bytes_first + ns * 8 + 16, 0);              // first tile per segment (and the end), then zero windows each
        for (size_t i = 0; i < ns; ++i) ((uint32_t *)tab.data())[i] = b->segs[i].first_tile;
        ((uint32_t *)tab.data())[ns] = (uint32_t)nt;
        { const int rc = take(c, tab.size(), g.d_sumtab, "the summary's segment table", g); if (rc != TS_OK) return rc; }
        HIP_TRY(c, hipMemcpy(g.d_sumtab.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    }
    if (ts_k_launch_slot_counts((const uint32_t *)g.d_slots.p, g.slot_cap, (uint32_t)nt, (uint32_t *)g.d_stats.p, stream) != 0)
        return c->fail(TS_ERR_HIP, "slot-count kernel launch failed");
    if (ts_k_launch_summary((const uint32_t *)g.d_stats.p, (const uint32_t *)g.d_sumtab.p, (const uint64_t *)((char *)g.d_sumtab.p + bytes_first),
                            (uint32_t)ns, (unsigned long long *)d_out, stream) != 0)
        return c->fail(TS_ERR_HIP, "summary kernel launch failed");
    return TS_OK;
}

int ts_general_batch_status(ts_batch *b, int *overflowed) {
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    *overflowed = 0;
    if (!b->scanned) return TS_OK;                                // nothing was ever enqueued
    uint32_t flag = 0;
    { const int rc = read_flag(b, flag); if (rc != TS_OK) return rc; }
    *overflowed = flag ? 1 : 0;
    return TS_OK;
}

// Waits for the scan; after an overflow or a spill grows the slots as the host path's fused stage does (a record per position
// and length, the wide form by fours) or leaves the list form, and rescans until the flag word stays clear.
int ts_general_batch_sync(ts_batch *b) {
    ts_ctx *c = b->ctx;
    if (!b->scanned) return c->fail(TS_ERR_STATE, "ts_batch_sync before ts_batch_scan");
    DEVICE_TRY(c);
    TsGeneralBatch &g = *b->gen;
    for (int attempt = 0;; ++attempt) {
        uint32_t flag = 0;
        { const int rc = read_flag(b, flag); if (rc != TS_OK) return rc; }
        if (!flag) { b->synced = true; return TS_OK; }
        const TsGeneralRescan next = ts_general_after_flag(flag, attempt, g.wide, g.slot_cap, g.slot_max);
        if (next == TsGeneralRescan::Fail)
            return c->fail(TS_ERR_STATE, "general read batch: a tile overflowed a slot that holds every match it can have");
        if (next == TsGeneralRescan::Strided) g.use_list = false;        // a candidate list spilled: the strided form takes the batch
        else {
            c->pool.give(std::move(g.d_slots));
            const int rc = take(c, slot_bytes(g), g.d_slots, "the regrown record slots", g);
            if (rc != TS_OK) return rc;
        }
        c->read_batch_stats[2].fetch_add(1, std::memory_order_relaxed);
        const int rc = ts_general_batch_scan(b, b->last_input, b->last_stream);
        if (rc != TS_OK) return rc;
    }
}

extern "C" int ts_terminal_ends_stats(const ts_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) out[i] = ctx->terminal_ends_stats[i].load(std::memory_order_relaxed);
    return TS_OK;
}

extern "C" int ts_read_batch_stats(const ts_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) out[i] = ctx->read_batch_stats[i].load(std::memory_order_relaxed);
    return TS_OK;
}
