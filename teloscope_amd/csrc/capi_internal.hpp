// capi_internal.hpp — structures shared by the host translation units of libteloscan
// (capi.cpp: contexts and device-resident batches; pipeline.cpp: the host-buffer entry points).
#ifndef TS_CAPI_INTERNAL_HPP
#define TS_CAPI_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "host.hpp"
#include "tiled_plan_core.h"
#include "ts_internal.h"

// A planning-only context (ts_params.device == TS_DEVICE_NONE) never touches HIP: it plans batches
// (tiles, windows, input layout) and every device entry point fails on it with TS_ERR_NO_DEVICE.
constexpr int kNoDevice = TS_DEVICE_NONE;

// Device memory block; move-only, frees itself.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t need) {
        if (need <= bytes && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, need ? need : 16);
        if (e == hipSuccess) bytes = need ? need : 16; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// Pinned host block (hipHostMalloc); move-only, frees itself.
struct PinBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinBuf &operator=(PinBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~PinBuf() { release(); }
    hipError_t ensure(size_t need) {
        if (need <= bytes && p) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc(&p, need ? need : 16, hipHostMallocDefault);
        if (e == hipSuccess) bytes = need ? need : 16; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};

// Device blocks kept between calls: the host entry points plan a batch per group of segments, and a
// hipMalloc / hipFree pair per multi-GB buffer per call costs more than the scan (hipFree also waits for
// the device).  take() hands out the smallest free block that fits within 2x, else allocates.
class BufferPool {
public:
    hipError_t take(size_t need, DevBuf &out);
    void give(DevBuf &&b);
    void clear();
private:
    std::mutex m_;
    std::vector<DevBuf> free_;
    size_t held_ = 0;
    static constexpr size_t kMaxBlocks = 96;
    static constexpr size_t kMaxHeld = 48ull << 30;
};

// Sets the calling thread's HIP device for the scope (every entry point that touches the device: a pool
// thread's current device need not be the context's) and restores the previous one.
class DeviceGuard {
public:
    explicit DeviceGuard(int device) {
        if (device < 0) { err_ = hipErrorNoDevice; return; }
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        err_ = prev_ == device ? hipSuccess : hipSetDevice(device);
        changed_ = err_ == hipSuccess && prev_ != device;
    }
    ~DeviceGuard() { if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_); }
    hipError_t error() const { return err_; }
private:
    int prev_ = -1;
    bool changed_ = false;
    hipError_t err_ = hipSuccess;
};

struct ts_ctx {
    ts_params params{};
    std::vector<ts::Pattern> patterns;
    uint16_t first_pattern_len = 0; // userInput.patterns.front().size(): interstitial blocks are at least twice as long
    uint32_t k = 0;                 // uniform pattern length (0 = mixed)
    uint32_t longest = 0;
    bool fast_ok = false;           // table-driven tiled kernel usable for the pattern set
    std::string why_not;            // reason when a scan mode is unsupported
    int device = 0;                 // HIP ordinal, or kNoDevice for a planning-only context
    int num_cu = 0;
    uint32_t table_rows = 0, fc_bytes = 0;
    bool fc_byte_table = true, pair_byte_table = false;
    // general kernels (generic.hip): sorted 2-bit codes per pattern length
    bool generic_ok = false;
    TsGenericPatterns gpat{};
    DevBuf d_gcodes, d_gflags;
    // ... or, for sets beyond 8 lengths / 32 bases, the wide form's tables (128-bit codes, up to 63 lengths of up to 63 bases)
    bool gen_wide = false;
    TsWidePatterns wpat{};
    std::vector<uint32_t> wide_lens;        // host copy of wpat.len
    DevBuf d_wlo, d_whi, d_wflags, d_wlen, d_wfirst;
    DevBuf d_table;
    mutable std::mutex mtx;         // guards batch planning / launches that read the context's tables
    mutable std::string error;
    bool read_filter = false;
    // measurement / test knobs of the host entry points, read from the environment ONCE, when the context is made (never per call):
    // TS_TIMING (stage times to stderr), TS_GEN_LIST=0 (general path: the strided form), TS_PACKED_UPLOAD=0 (bases cross PCIe
    // as ASCII), TS_PACKED_MIN_BYTES (calls below it go plain), TS_REC32=1 (32-bit records)
    struct Knobs {
        bool timing = false, gen_list = true, packed_upload = true;
        bool rec16 = true;                                    // scans keep 16-bit records where they can (TS_REC32=1: 32-bit)
        uint64_t packed_min_bytes = 1u << 20;                 // small calls are latency, not link time: they go plain
        uint64_t match_slice_bytes = 256ull << 20;            // match lines (match_text.cpp): text of both files formatted per slice (TS_MATCH_SLICE_BYTES)
    } knobs;
    BufferPool pool;
    // host-buffer entry points (pipeline.cpp): pinned staging rings and their streams
    // CPUs of the NUMA node the device is attached to (empty: unknown / TS_NO_NUMA_BIND): the pipeline's own threads run
    // there, and the pinned staging buffers are allocated there — a DMA out of the other socket's memory, or staging
    // threads on the other socket, cost 15-20 % of the PCIe-inclusive rate on a two-socket host
    std::vector<float> entropy_term;      // ts::entropy_terms(window_size): windows of the full size look their terms up
    DevBuf d_entropy_term;                // ... and its copy on the device, made by the first call that formats tracks there (tracks.cpp)
    std::mutex track_mtx;                 // one track-formatting call at a time per context
    std::vector<int> node_cpus;
    void bind_this_thread() const;          // no-op when node_cpus is empty; never widens the thread's current mask
    static constexpr int kUpSlots = 3;
    hipStream_t side_stream = nullptr;          // ts_batch_pack_shard: the terminal walks of every batch's pack (created on first use)
    std::mutex side_mtx;
    // the streams (scan, pack) the side stream has been tried against: HIP puts a process's streams on a few hardware queues, and a
    // side stream that shares the scan stream's queue puts the terminal walks of step i in front of the scan of step i + 1
    // (shard.cpp: side_stream_for)
    std::vector<void *> side_tried;
    PinBuf pin_up[kUpSlots];
    hipEvent_t pin_up_ev[kUpSlots] = {nullptr, nullptr, nullptr};
    DevBuf d_pack[kUpSlots], d_runs[kUpSlots];   // packed upload: a chunk's 2-bit codes and invalid runs on the device
    PinBuf pin_runs[kUpSlots];
    // device pieces (TS_INPUT_DEVICE): the job list of upload_pieces' gather launch — staged in pin_jobs (refilled only once
    // jobs_ev says its previous upload has completed), uploaded to d_jobs (reused under up_stream's order); both grow on demand
    PinBuf pin_jobs;
    DevBuf d_jobs;
    hipEvent_t jobs_ev = nullptr;
    bool jobs_ev_pending = false;
    // ts_device_input_stats: device pieces seen, device-to-device copies issued, gather jobs issued, gather launches — since ts_create
    std::atomic<uint64_t> device_input_stats[4] = {};
    // ts_upload_stats: which way upload_pieces sent its chunks and packed their 16384-position blocks — since ts_create
    std::atomic<uint64_t> upload_stats[8] = {};
    // ts_match_text_stats: formatting calls, canonical lines, non-canonical lines, text bytes — since ts_create
    std::atomic<uint64_t> match_text_stats[4] = {};
    // ts_read_block_text_stats: formatting calls that reached the device, lines, text bytes — since ts_create
    std::atomic<uint64_t> read_block_text_stats[3] = {};
    // ts_read_fastq_text_stats: FASTQ-out gathers that formatted text on the device, records, text bytes — since ts_create
    std::atomic<uint64_t> read_fastq_text_stats[3] = {};
    // ts_gzip_stats: windows, spans probed, spans chained, spans dropped, plain bytes produced, parts the caller handed to zlib — since ts_create
    std::atomic<uint64_t> gzip_stats[6] = {};
    // ts_bam_index_stats: calls, spans the chain entered, spans whose entry was a candidate row, spans settled by the serial
    // rule, records the index wrote, bytes of rows copied device to host — since ts_create
    std::atomic<uint64_t> bam_index_stats[6] = {};
    // ts_bgzf_deflate_stats: device deflate calls, members they wrote, plain bytes in, member bytes out — since ts_create
    std::atomic<uint64_t> bgzf_deflate_stats[4] = {};
    // ts_read_batch_stats: scans enqueued on general tips batches, segments their read pass judged, rescans after an overflow or
    // spill, bytes those calls copied device to host — since ts_create
    std::atomic<uint64_t> read_batch_stats[4] = {};
    // ts_terminal_ends_stats: segments reduced per side by the tiled ENDS walk, by the general ENDS walk, on the host from
    // downloaded blocks; bytes of per-side maxima and flag words copied device to host — since ts_create
    std::atomic<uint64_t> terminal_ends_stats[4] = {};
    hipEvent_t gen_ev[2] = {nullptr, nullptr};   // TS_TIMING: around the general path's kernels
    PinBuf pin_down[2];
    PinBuf pin_off;                              // general path: a group's tile directory lands here (a pageable landing cost 9 ms per MB-sized copy)
    hipStream_t up_stream = nullptr, scan_stream = nullptr, down_stream = nullptr;

    std::mutex down_mtx;            // one download (pinned landing area + its stream) at a time
    mutable std::mutex err_mtx;
    std::mutex api_mtx;             // one pipeline run at a time per context (the runs share the pinned rings and streams)
    // Concurrent callers are COALESCED, not queued one behind the other (the reference calls scanSegment / matches
    // concurrently from its pool workers, src/input.cpp:977, :786): a call that arrives while a run is in flight waits in
    // `sq`; whoever finds no run in flight becomes the leader, takes every waiting call of one kind, runs them as ONE
    // batch and hands each caller its slice (pipeline.cpp: submit_pipeline)
    std::mutex sq_mtx;
    std::condition_variable sq_cv;
    std::deque<struct SubmitReq *> sq;
    bool sq_leader = false;
    int fail(int code, const std::string &msg) const { std::lock_guard<std::mutex> g(err_mtx); error = msg; return code; }
};

// The plan of a tiled batch and of its shards: tiled_plan_core.h
using tsplan::Region;
using tsplan::SegPlan;
using tsplan::ShardRange;
using tsplan::ShardLayout;

// What a GENERAL TIPS BATCH holds beside the segments and the input layout of a ts_batch (general_batch.cpp): a tips-only batch
// of a context whose tips scans go to the general kernels.  Its tiles are TsGeneralTile over the regions scanSegment picks,
// the records stay in the fused pass's per-tile slots, and the read predicate walks them there.
struct TsGeneralBatch {
    std::vector<TsGeneralTile> tiles;
    TsGenericGeom Q{};
    unsigned long long gen_lens = 0;
    bool wide = false, use_list = false;
    uint32_t slot_unit = 0;             // positions of the largest tile, a multiple of 4: what a slot is a multiple of
    uint32_t slot_cap = 0, slot_max = 0;
    // tile list, {segment lengths, zeros, zeros, flag word}, slots, tile directory, slot offsets, the predicate's TsTile list and
    // segment table: all but the slots uploaded or sized once per batch
    DevBuf d_tiles, d_tab, d_slots, d_stats, d_off, d_bct, d_segin;
    DevBuf d_sumtab;                    // ts_batch_segment_summary's table (first tile per segment), made on its first call
    bool uploaded = false;
    size_t tab_flag = 0;                // byte offset of the fused pass's flag word in d_tab
};

// What ts_batch_call_read_blocks leaves in a tips batch, tiled or general: the walks' tables — 2 n x 16 bytes of counts, 2 n + 1
// places, n + 1 first-row indices, the sums' scratch — the rows (room for row_cap of them), and, for a tiled batch, the walks'
// segment table (a general tips batch has its own).  `called`: the rows describe the batch's latest scan.
struct ReadBlocksTab {
    size_t places, first, tmp, bytes;
    explicit ReadBlocksTab(size_t ns) : places(ns * 32), first(places + (((2 * ns + 1) * 8 + 15) & ~(size_t)15)), tmp(first + (((ns + 1) * 8 + 15) & ~(size_t)15)),
                                        bytes(tmp + (size_t)ts_k_scan_tmp_bytes((uint32_t)(2 * ns)) + 16) {}
};
struct ReadBlocksState {
    DevBuf d_tab, d_rows, d_segin;
    uint64_t row_cap = 0;
    bool called = false;                // the rows describe the batch's latest scan
    bool clean = false;                 // ... and ts_batch_read_pass_status has said since that nothing overflowed
    void *stream = nullptr;
};

// A batch is a PLAN over all its segments (tsplan::TiledPlan: tiles, window records, input layout, the tile range
// [tile_lo, tile_hi) it executes and that range's launch sizes) plus the device state of that range: the whole plan by default,
// one rank's shard after ts_batch_restrict, or — on the rank that assembles — results produced elsewhere (ts_batch_adopt).
struct ts_batch : tsplan::TiledPlan {
    ts_ctx *ctx = nullptr;
    std::unique_ptr<TsGeneralBatch> gen;    // non-null: a general tips batch — `tiles` stays empty, only the calls general_batch.cpp serves work
    uint64_t n_matches = 0;
    bool allocated = false;
    double last_ms = 0.0;
    bool scanned = false, synced = false;
    bool dense = false;             // match records form one dense stream in tile order (adopted / exported results)
    const void *last_input = nullptr;
    void *last_stream = nullptr;
    DevBuf d_in, d_tiles, d_windows, d_matches, d_tile_off, d_stats, d_fill, d_tickets, d_segtab, d_dense, d_dense_base, d_scan_tmp, d_readtab;
    // what the scan hands to block calling and to a shard's message (kp.emit): per-wave regions of visible records, the
    // per-tile chain summaries (TsTileChain) and, planned on the host, the terminal-zone word of every tile
    DevBuf d_vis, d_chain, d_zone;
    bool emitted = false;           // the latest scan ran the emitting build: tile_stats word 3, d_chain and d_vis describe it
    bool chain_valid() const { return emitted && !dense && d_chain.p != nullptr; }
    // a shard (ts_batch_restrict_shard): the range the batch executes is its OWNED tiles [own_lo, own_hi) plus context tiles
    uint32_t shard_parts = 0, shard_part = 0, shard_scale = 1;
    uint64_t own_lo = 0, own_hi = 0;
    DevBuf d_shard_segs, d_shard_bounds, d_shard_tmp, d_shard_cand;
    ShardRange shard_r{};
    ShardLayout shard_L{};
    // ts_batch_bind_shard_message: the message buffer the shard's (emitting) scans pack their window records into themselves;
    // msg_windows: the buffer the LATEST scan did so for (null: it wrote 8 x u32 per window, the pack's own kernel packs them)
    void *bound_msg = nullptr;
    const void *msg_windows = nullptr;
    // (ts_batch_pack_shard runs the terminal walks beside the counting / packing kernels on the CONTEXT's side stream: HIP
    // streams share a handful of hardware queues, and kernels of two streams on one queue run one after the other — a side
    // stream per batch, four buffer slots = four more streams, pushed the scan stream onto a shared queue)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // caller-owned result buffers (ts_batch_bind_results / ts_batch_adopt); null = the batch's own
    uint32_t *ext_windows = nullptr, *ext_stats = nullptr;
    const uint32_t *ext_dense = nullptr;
    ReadBlocksState rb;                     // ts_batch_call_read_blocks
    bool all_terminal = false;              // (set with d_readtab) no segment longer than the terminal limit
    uint64_t ticket_seq = 0;                // launches with on-demand tiles so far: parity = the ticket counter in use
    std::vector<uint32_t> wave_fill;
    std::vector<hipEvent_t> evs;                 // ring of {start, stop} pairs, one per enqueued scan
    uint64_t scan_seq = 0, harvested = 0;        // scans enqueued / scans whose time has been read
    uint32_t time_every = 1;                     // ts_batch_set_timing: every n-th scan has a start event too (0: none)
    uint64_t timed_mask = 0;                     // ring slots whose scan was timed (kEventRing = 64 bits)
    double avg_ms = 0.0;
    uint64_t avg_n = 0;

    uint32_t *windows_ptr() const { return ext_windows ? ext_windows : (uint32_t *)d_windows.p; }
    uint32_t *stats_ptr() const { return ext_stats ? ext_stats : (uint32_t *)d_stats.p; }
    bool records16() const { return kp.rec16 != 0u && !dense; }    // the scan's own regions hold 16-bit records (the dense / adopted stream never does)
    const uint32_t *records_ptr() const { return dense ? (ext_dense ? ext_dense : (const uint32_t *)d_dense.p) : (const uint32_t *)d_matches.p; }
    // records that may be read behind records_ptr(): the per-wave regions, or the dense stream
    unsigned long long records_limit() const { return dense ? n_matches : (unsigned long long)region_cap * total_waves; }
};

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return (ctx)->fail(TS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define DEVICE_TRY(ctx)                                                                       \
    if ((ctx)->device == kNoDevice)                                                           \
        return (ctx)->fail(TS_ERR_NO_DEVICE, "planning-only context: no HIP device behind it"); \
    DeviceGuard _dev_guard((ctx)->device);                                                    \
    if (_dev_guard.error() != hipSuccess)                                                     \
        return (ctx)->fail(TS_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_dev_guard.error()))

// pipeline.cpp: per-context pieces of the host pipeline, for multi.cpp
int  ts_scan_segments_unlocked(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, ts_segment_out *out);   // ts_scan_segments for a caller that holds api_mtx
int  ts_pipeline_ensure_streams(ts_ctx *c);
int  ts_pipeline_upload_batch(ts_batch *b, const ts_segment_in *segs, int *slot, bool used[]);   // segs: the batch's segments, in plan order

// capi.cpp internals used by pipeline.cpp
bool ts_full_scan_supported(const ts_ctx *c, std::string &why);
void *ts_alloc_large(size_t bytes);     // malloc-compatible; many-MB arrays on 2 MB pages when the kernel grants them

// --------------------------------------------------------------- SegmentData assembly (capi.cpp), shared by every route
unsigned ts_host_threads();             // host threads of a download's post-processing: TS_HOST_THREADS, default 16

// f(i) for i in [0, n) on up to max_threads host threads (dynamic: an atomic counter hands out the indices)
template <typename F>
void ts_parallel_for(size_t n, unsigned max_threads, F &&f) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = (unsigned)std::min<size_t>({(size_t)max_threads, (size_t)hw, n});
    if (nt <= 1) { for (size_t i = 0; i < n; ++i) f(i); return; }
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&] { for (size_t i; (i = next.fetch_add(1)) < n;) f(i); });
    for (std::thread &th : pool) th.join();
}

// Window kwin of a segment from its eight counts {A, C, G, T, canonical, non-canonical, forward, reverse covered}: the float
// metrics are evaluated on the host from the integer counts, as the reference does
inline void ts_fill_window(const ts_ctx *c, uint64_t kwin, uint64_t seg_len, uint64_t abs_pos, const uint32_t r[8], ts_window &w) {
    const ts_params &P = c->params;
    std::memset(&w, 0, sizeof w);
    const uint64_t ws = kwin * P.step;
    w.window_start = abs_pos + ws;
    w.current_window_size = (uint32_t)std::min<uint64_t>(P.window_size, seg_len - ws);
    if (P.out_gc || P.out_entropy) for (int i = 0; i < 4; ++i) w.nucleotide_counts[i] = r[i];
    if (P.out_gc) w.gc_content = ts::gc_content(w.nucleotide_counts, w.current_window_size);
    if (P.out_entropy) w.shannon_entropy = ts::shannon_entropy_memo(w.nucleotide_counts, w.current_window_size, c->entropy_term);
    w.canonical_covered = r[4];
    w.non_canonical_covered = r[5];
    w.fwd_covered = r[6];
    w.rev_covered = r[7];
}

// A segment's windows / matches arrays (o zeroed first); false when out of host memory
bool ts_alloc_segment(ts_segment_out &o, uint64_t n_windows, uint64_t n_matches);
// The blocks of segments [0, ns), sorted by segment and within one terminal blocks before interstitial ones, into each
// segment's two arrays.  placed: the blocks consumed (fewer than n when one names a segment >= ns).  false when out of memory.
bool ts_split_blocks(const TsDevBlock *blocks, size_t n, ts_segment_out *out, size_t ns, size_t &placed);

// What landed on the host for piece-parallel assembly: per segment its windows (8 x u32 each, at win_base of `wins`) and a
// range of tiles; per tile its records (rec_off, count: a run of `recs`) and the segment-relative position they are relative to.
struct HostView {
    struct Seg { uint64_t len, abs_pos, win_base, n_windows, first_tile, n_tiles; };
    struct Tile { uint64_t rec_off, rel; uint32_t count; };
    std::vector<Seg> segs;
    std::vector<Tile> tiles;                 // empty: no match vectors
    const uint32_t *wins = nullptr, *recs = nullptr;
    uint64_t nrecs = 0;
    bool tips = false;
    bool no_windows = false;                 // the windows stay on the device (ts_scan_segments_tracks): segments get none
    const TsDevBlock *blocks = nullptr;      // sorted as ts_split_blocks reads them
    size_t n_blocks = 0;
};
// SegmentData from the general kernels' records (pipeline.cpp's general path) to out[0, v.segs.size()); frees it on failure
int  ts_assemble_general(ts_ctx *c, const HostView &v, ts_segment_out *out);

// ---- the general kernels' per-context launch geometry: the host entry points' general path (pipeline.cpp) and general tips
// batches (general_batch.cpp) launch the same passes, here; what they plan for them is in general_plan_core.h
inline TsGenericGeom ts_general_geom(const ts_ctx *c) {
    const ts_params &P = c->params;
    const uint32_t s = P.step, w = P.window_size;
    TsGenericGeom Q{};
    Q.s = s; Q.w = w; Q.longest = c->longest; Q.nuc_on = (P.out_gc || P.out_entropy) ? 1u : 0u; Q.fold = P.fold_case;
    Q.s_magic = s >= 2u ? (uint32_t)((1ull << 32) / s + 1ull) : 0u;
    Q.cw = w / s; Q.rw = w - Q.cw * s;
    return Q;
}
// the pattern lengths as block calling reads them (TsBlockCallParams.gen_lens); the wide form: non-zero = "general format"
inline unsigned long long ts_general_gen_lens(const ts_ctx *c) {
    if (c->gen_wide) return 1ull;
    unsigned long long v = 0;
    for (uint32_t li = 0; li < c->gpat.nlen && li < 8u; ++li) v |= (unsigned long long)(c->gpat.len[li] & 63u) << (6u * li);
    if (c->gpat.nlen && c->gpat.len[c->gpat.nlen - 1] > 63u) v = 0;
    return v;
}
// what blockcall.hip's terminal walks read of the context (the record stream and its directory are the caller's to set)
inline TsBlockCallParams ts_general_walk_params(const ts_ctx *c, unsigned long long gen_lens, bool wide) {
    const ts_params &P = c->params;
    TsBlockCallParams Q{};
    Q.terminal_limit = P.terminal_limit; Q.max_match_dist = P.max_match_dist;
    Q.min_block_len = P.min_block_len; Q.max_block_dist = P.max_block_dist;
    Q.min_block_counts = P.min_block_counts; Q.min_block_density = P.min_block_density;
    Q.k = c->k;
    Q.gen_lens = gen_lens;
    Q.wide = wide ? 1u : 0u; Q.wide_len = wide ? c->wpat.len : nullptr;
    return Q;
}
// may a scan start in the list form of the fused pass?  (every tips-only scan that passes this does; a spilled candidate list
// sends it to the strided form)
inline bool ts_general_list_form_ok(const ts_ctx *c) {
    return !c->gen_wide && c->knobs.gen_list && c->params.step >= 2u && c->params.window_size < (1u << 28);
}
// a tile's slot, in units of the positions it holds: what a scan starts with, and what cannot overflow
inline uint32_t ts_general_slot_start(const ts_ctx *c, uint32_t unit) { return c->gen_wide ? unit * std::min<uint32_t>(4u, std::max<uint32_t>(1u, c->wpat.nlen)) : unit; }
inline uint32_t ts_general_slot_max(const ts_ctx *c, uint32_t unit) { return unit * std::max<uint32_t>(1u, c->gen_wide ? c->wpat.nlen : c->gpat.nlen); }
// The fused pass on `st`: the wide form on a context of the wide form, else the list form (use_list) or the strided one.  The
// three tables are per segment (lengths, window bases, window counts); d_flag is the pass's flag word, cleared by the caller,
// who holds c->mtx.  d_win: the window records, nullptr for tips.
inline int ts_general_launch_fused(ts_ctx *c, const void *d_in, const TsGeneralTile *d_tiles, uint32_t nt, const unsigned long long *tab_len,
                                   const unsigned long long *tab_win, const unsigned long long *tab_nwin, uint32_t *d_flag, bool tips, uint32_t slot_cap,
                                   uint32_t *d_stats, uint32_t *d_slots, uint32_t *d_win, bool use_list, const TsGenericGeom &Q, hipStream_t st) {
    if (c->gen_wide) {
        if (ts_k_launch_general_wide((const unsigned char *)d_in, d_tiles, nt, tab_len, tab_win, tab_nwin, &c->wpat, &Q, tips ? 1 : 0, slot_cap,
                                     d_stats, d_slots, d_win, d_flag, st) != 0)
            return c->fail(TS_ERR_HIP, "general wide kernel launch failed");
    } else if (ts_k_launch_general_fused((const unsigned char *)d_in, d_tiles, nt, tab_len, tab_win, tab_nwin, &c->gpat, &Q, tips ? 1 : 0, slot_cap,
                                         d_stats, d_slots, d_win, d_flag, use_list ? 1 : 0, c->num_cu, st) != 0)
        return c->fail(TS_ERR_HIP, "general fused kernel launch failed");
    return TS_OK;
}
// What a driver does once a scan has raised its flag word (bit 0: a tile overflowed its slot, bit 1: a candidate list spilled)
// in scan number `attempt` (from 0): give up at the third scan that raises it (the wide form: the sixth), or when the slot
// already holds every match a tile can have and nothing spilled; after a spill take the strided form and keep the slots; else
// grow the slots to slot_max — the wide form by fours: a slot for every position AND length, 63 of them, is 1 MB per tile —
// which sets slot_cap.
enum class TsGeneralRescan { Fail, Strided, Grown };
inline TsGeneralRescan ts_general_after_flag(uint32_t flag, int attempt, bool wide, uint32_t &slot_cap, uint32_t slot_max) {
    if (attempt > (wide ? 4 : 1) || (slot_cap >= slot_max && !(flag & 2u))) return TsGeneralRescan::Fail;
    if (flag & 2u) return TsGeneralRescan::Strided;
    slot_cap = wide ? std::min<uint32_t>(slot_max, slot_cap * 4u) : slot_max;
    return TsGeneralRescan::Grown;
}

// general_batch.cpp: what the ts_batch_* entry points hand a general tips batch (b->gen != nullptr) to
ts_batch *ts_general_batch_create(ts_ctx *ctx, const uint64_t *seg_lens, const uint64_t *abs_pos, size_t n_segs);
void ts_general_batch_release(ts_batch *b);      // its device blocks back to the pool (ts_batch_destroy)
int  ts_general_batch_scan(ts_batch *b, const void *d_input, void *stream);
int  ts_general_batch_read_pass(ts_batch *b, void *d_pass, void *stream);
int  ts_general_batch_terminal_ends(ts_batch *b, void *d_ends, void *stream);
int  ts_general_batch_download_blocks(ts_batch *b, ts_segment_out *out);
int  ts_general_batch_segment_summary(ts_batch *b, void *d_out, void *stream);
int  ts_general_batch_call_read_blocks(ts_batch *b, void *stream);
int  ts_general_batch_place_read_blocks(ts_batch *b);            // the placing walks again, into b->rb.d_rows as it is now
int  ts_general_batch_status(ts_batch *b, int *overflowed);
int  ts_general_batch_sync(ts_batch *b);
int  ts_general_batch_refuse(const ts_batch *b, const char *call);     // TS_ERR_UNSUPPORTED, the call named in ts_last_error

// pipeline.cpp: after ts_batch_call_read_blocks — waits for its stream, *n_rows = the rows it called; when they are more than the
// buffer held, the buffer is grown and the placing walks run again (same places, same rows).  Then b->rb.d_rows holds them all.
int  ts_batch_settle_read_blocks(ts_batch *b, uint64_t *n_rows);
int  ts_batch_ensure_device(ts_batch *b);        // allocates the range's device state (idempotent)
// block calling on the device over a resident match stream + tile directory (a batch's, or the general kernels' dense stream)
int  ts_device_block_call_raw(ts_ctx *c, const TsTile *d_tiles, const unsigned long long *d_tile_off, const uint32_t *d_stats,
                              const uint32_t *d_matches, uint64_t n_matches_hint, const std::vector<TsShardSegIn> &tab, size_t nt,
                              bool tips, unsigned long long gen_lens, const uint32_t *d_chain, uint32_t *d_work, hipStream_t st,
                              std::vector<TsDevBlock> &blocks, std::vector<unsigned long long> *sums_out, int rec16 = 0,
                              const uint32_t *d_wide_len = nullptr, bool unordered = false);
void ts_batch_release_input(ts_batch *b);        // returns the batch's input buffer to the context's pool
void *ts_batch_input_ptr_nozero(ts_batch *b);
struct ts_fetched;                               // what a download left in host memory, before post-processing
ts_fetched *ts_batch_fetch(ts_batch *b, bool with_matches, int slot, int *rc_out, bool with_windows = true);   // device work + D2H (pinned slot 0/1)
int  ts_batch_finalize(ts_batch *b, ts_fetched *f, ts_segment_out *out);             // host post-processing; frees f
    // the batch's own input buffer, not zero-filled (every byte read is uploaded)

// tracks.cpp: the lines of the window tracks the context has, formatted on the device from `n_records` window records at
// d_records and appended to *out (zeroed by the caller before the first call).  h_records: the same records on the host, or null
// (the few the entropy patch list needs are then picked off the device).  Work and copies run on st; synchronous.
struct ts_track_text;
struct ts_track_segment;
void ts_track_text_begin(const ts_ctx *c, ts_track_text *t);    // a caller's struct (zeroed, or an earlier result: reused) made empty
int  ts_tracks_append(ts_ctx *c, const uint32_t *d_records, const uint32_t *h_records, uint64_t n_records, const ts_track_segment *segs,
                      size_t n_segs, const char *names, uint64_t names_len, hipStream_t st, ts_track_text *out);

// match_text.cpp: the lines of the two match files (contexts with out_matches; others: nothing happens), formatted on the
// device from a record stream that lies there and appended to *out.  The stream: `records` in one of match_text.hip's forms,
// addressed by the directory {tile_off, tile_stats} over `tiles` (TsTile / TsGeneralTile; TS_MATCH_FORM_ARRAY: TsMatchTile and
// no directory); `bases`: what the segments' base_off points into.  segs[i] is the segment the tiles call i.  Work and copies
// run on st; synchronous.
struct ts_match_text;
struct ts_match_line_segment;
struct TsMatchSource {
    uint32_t form = 0;
    const void *records = nullptr, *tiles = nullptr;
    const unsigned long long *tile_off = nullptr;
    const uint32_t *tile_stats = nullptr;
    size_t n_tiles = 0;
    const void *bases = nullptr;
    const uint32_t *wide_len = nullptr;
    unsigned long long gen_lens = 0;
    uint32_t k = 0;
};
void ts_match_text_begin(const ts_ctx *c, ts_match_text *t);    // a caller's struct (zeroed, or an earlier result: reused) made empty
int  ts_matches_append(ts_ctx *c, const TsMatchSource &src, const ts_match_line_segment *segs, size_t n_segs, const char *names,
                       uint64_t names_len, hipStream_t st, ts_match_text *out);

// (struct ts_bam_chunk, the chunk of the device routes: chunk_internal.h)

#endif
