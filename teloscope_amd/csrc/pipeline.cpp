// pipeline.cpp — the host-buffer entry points of libteloscan: ts_scan_segments, ts_scan_segments_blocks,
// ts_filter_reads(_multi), ts_terminal_ends.  Host memory in, host results out.
//
// A call's segments (or reads) are cut into GROUPS of about 256 MB of input and the groups flow through three
// stages that run concurrently, each on its own host thread and HIP stream:
//
//   upload     plan the group's batch, stage its bases into a ring of pinned chunks (several memcpy threads)
//              and DMA them to the device (up_stream)                                 — bound by PCIe
//   scan       ts_scan_tiles on the group (scan_stream), read back the per-wave fill, regrow + rescan on
//              overflow; the group's input buffer goes back to the pool                — ~0.1 ms per group
//   download   mode-specific device work (block calling / read predicate / record compaction), D2H into a
//              pinned landing area, host post-processing on the host threads (down_stream)
//
// so that the wall time of a call is the upload plus the tail of the last group, instead of the sum of the
// three.  Device buffers come from the context's pool: a call neither allocates nor frees device memory once
// the pool is warm.  The reference's own decomposition is one thread-pool job per path (src/input.cpp:719-724)
// and one job per chunk of a 2048-record FASTQ batch (src/input.cpp:753-812); a group is the GPU-sized
// equivalent of such a job, and results come back in input order whatever the grouping.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "capi_internal.hpp"
#include "gather_core.h"
#include "general_plan_core.h"
#include "text_core.h"
#include "upload_stage_core.h"

namespace {

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

uint64_t group_target_bytes() {
    static const uint64_t v = [] {
        // (with the packed upload a group's bases are staged in 128 MB chunks: larger groups, fewer hand-overs between the
        // stages — profiles/r03/packed_upload_rate.txt)
        const char *pk = getenv("TS_PACKED_UPLOAD");
        return (uint64_t)((pk && pk[0] == '0') ? 256 : 512) << 20;
    }();
    return v;
}

template <typename T>
class Channel {                                   // unbounded FIFO between two pipeline stages
public:
    void push(T v) { { std::lock_guard<std::mutex> g(m_); q_.push_back(std::move(v)); } cv_.notify_one(); }
    void close() { { std::lock_guard<std::mutex> g(m_); closed_ = true; } cv_.notify_all(); }
    bool pop(T &out) {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        return true;
    }
private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<T> q_;
    bool closed_ = false;
};

class Semaphore {
public:
    explicit Semaphore(int n) : n_(n) {}
    void acquire() { std::unique_lock<std::mutex> g(m_); cv_.wait(g, [&] { return n_ > 0; }); --n_; }
    void release() { { std::lock_guard<std::mutex> g(m_); ++n_; } cv_.notify_one(); }
private:
    std::mutex m_;
    std::condition_variable cv_;
    int n_;
};

enum class Mode { Matches, Blocks, ReadPass, Ends, Tracks };   // Ends: ts_terminal_ends, 8 bytes per segment back; Tracks: Blocks
                                                                // without window records, the window tracks' text instead (ts_scan_segments_tracks)

struct Item { const char *seq; uint64_t len, abs_pos; uint8_t format; uint32_t n_pieces; };     // format: TS_INPUT_BASES / TS_INPUT_TEXT_PIECES (seq = ts_text_piece[]) /
                                                                                                // TS_INPUT_PACKED2 (seq = ts_packed_seq) / TS_INPUT_DEVICE (seq = device memory)

// Where a call's results go, at the items' indices; null = not asked for.  out: Matches / Blocks; counts: Blocks (optional);
// pass: ReadPass; ends: Ends (two per item).
struct Outputs {
    ts_segment_out *out = nullptr;
    ts_segment_counts *counts = nullptr;
    uint8_t *pass = nullptr;
    uint32_t *ends = nullptr;
    ts_track_text *tracks = nullptr;              // Tracks: every group's lines are appended, in item order (not sliced); names: per item
    const char *const *names = nullptr;
    ts_match_text *matches = nullptr;             // Tracks: the match lines, likewise (ts_scan_segments_text)
    Outputs slice(size_t at) const {
        return {out ? out + at : nullptr, counts ? counts + at : nullptr, pass ? pass + at : nullptr, ends ? ends + 2 * at : nullptr,
                tracks, names ? names + at : nullptr, matches};
    }
};

// The names of a group's segments as the formatters read them: one blob, a name stored once per run of equal ones
// (consecutive segments of one path share a name); made once per group and shared by the track and the match step.
struct NameBlob {
    std::string blob;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
};
int group_names(ts_ctx *c, const char *const *names, size_t n, NameBlob &nb) {
    nb.off.resize(n); nb.len.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const size_t len = std::strlen(names[i]);
        if (len > 0xFFFFFFFFull) return c->fail(TS_ERR_INVALID_ARG, "ts_scan_segments_tracks: a name of 4 GiB or more");
        if (i && nb.len[i - 1] == len && std::memcmp(nb.blob.data() + nb.off[i - 1], names[i], len) == 0) {
            nb.off[i] = nb.off[i - 1];
        } else {
            nb.off[i] = nb.blob.size();
            nb.blob.append(names[i], len);
        }
        nb.len[i] = (uint32_t)len;
    }
    return TS_OK;
}

// Tracks: the lines of a group's windows, formatted where the records lie (tracks.cpp), appended to the call's text.  segs: the
// group's segments with first_window / n_windows / abs_pos / len set; nb: their names.
int group_tracks(ts_ctx *c, const uint32_t *d_windows, uint64_t n_windows, std::vector<ts_track_segment> &segs, const NameBlob &nb,
                 hipStream_t st, ts_track_text *out) {
    for (size_t i = 0; i < segs.size(); ++i) { segs[i].name_off = nb.off[i]; segs[i].name_len = nb.len[i]; }
    return ts_tracks_append(c, d_windows, nullptr, n_windows, segs.data(), segs.size(), nb.blob.data(), nb.blob.size(), st, out);
}

// ... and the lines of its match records, formatted from the record stream and the input buffer where they lie
// (match_text.cpp).  segs: the group's segments with abs_pos / len / base_off set (all of them full scans).
int group_matches(ts_ctx *c, const TsMatchSource &src, std::vector<ts_match_line_segment> &segs, const NameBlob &nb, hipStream_t st,
                  ts_match_text *out) {
    for (size_t i = 0; i < segs.size(); ++i) { segs[i].name_off = nb.off[i]; segs[i].name_len = nb.len[i]; }
    return ts_matches_append(c, src, segs.data(), segs.size(), nb.blob.data(), nb.blob.size(), st, out);
}

struct Group {
    size_t first = 0, count = 0;                  // items [first, first + count) of the call's item list
    ts_batch *b = nullptr;
    hipEvent_t uploaded = nullptr;
    double t_plan = 0, t_upload = 0, t_scan = 0, t_down = 0, t_fetch = 0, t_final = 0, t_text = 0;
    bool input_kept = false;                      // the download stage reads the input buffer (match lines) and releases it
};

int ensure_streams(ts_ctx *c) {
    if (c->up_stream) return TS_OK;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->scan_stream, hipStreamNonBlocking));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
    // the pinned staging ring is allocated — pinning touches the pages, which places them — by a thread on the device's NUMA node
    int rc = TS_OK;
    std::thread alloc([&] {
        c->bind_this_thread();
        DeviceGuard g(c->device);
        for (int i = 0; i < ts_ctx::kUpSlots && rc == TS_OK; ++i) {
            // (+ 4096: a packed chunk of exactly 128 Mi positions that starts off a 64-byte boundary packs to a few bytes more
            // than 32 MiB, and its DMA reads 8 bytes past the last code)
            if (c->pin_up[i].ensure((32u << 20) + 4096u) != hipSuccess) { rc = c->fail(TS_ERR_ALLOC, "cannot allocate the pinned staging ring"); break; }
            if (hipEventCreateWithFlags(&c->pin_up_ev[i], hipEventDisableTiming) != hipSuccess) rc = c->fail(TS_ERR_HIP, "hipEventCreate failed");
        }
    });
    alloc.join();
    return rc;
}

// (a call's pieces, their chunks and everything the staging workers write into a pinned slot: upload_stage_core.h; the walks over
// FASTA body text under it: text_core.h)
using tsstage::UpPiece;
using tstext::text_locate;

constexpr uint32_t kPackRunCap = 1u << 18;                 // invalid runs a packed chunk may carry (more: the chunk goes as ASCII)

// The device pieces (TS_INPUT_DEVICE) of one upload_pieces call, to the device buffer whose byte lo_all lies at din, on
// up_stream.  One device-to-device copy per piece costs ~3 us of issue each (400 000 GFA segments: 1.2 s); instead the pieces
// become a job list — tsgather::Job: source address, offset from din, byte count; a piece longer than a 16 KiB slice is cut
// into sub-jobs at 16-byte boundaries of the destination, so that no wave's work is unbounded — which is staged in pinned
// memory, uploaded once and consumed by ONE launch of ts_gather_pieces_kernel (gather.hip), a wave per job.
// THE RULE, fixed: a piece of kDeviceCopyMin bytes (8 MiB) or more keeps its own device-to-device copy — a blit that long is
// bound by HBM, not by its issue, and a chromosome-sized record need not become 10^5 jobs; every smaller piece is gathered.
// ts_device_input_stats counts both.  The pinned list is refilled only after jobs_ev says its previous upload has completed;
// the device list is reused under the stream's order (growing it frees the old block, which waits for the device).
constexpr uint64_t kDeviceCopyMin = 8ull << 20;
int gather_device_pieces(ts_ctx *c, const std::vector<UpPiece> &on_device, void *din, uint64_t lo_all) {
    if (on_device.empty()) return TS_OK;
    const uint64_t base = (uint64_t)(uintptr_t)din;
    uint64_t n_jobs = 0, n_copies = 0;
    for (const UpPiece &pc : on_device) {
        if (pc.len >= kDeviceCopyMin) ++n_copies;
        else n_jobs += tsgather::split_count(base + (pc.off - lo_all), pc.len, tsgather::kSliceBytes);
    }
    c->device_input_stats[0].fetch_add(on_device.size(), std::memory_order_relaxed);
    if (n_copies) {
        for (const UpPiece &pc : on_device)
            if (pc.len >= kDeviceCopyMin)
                HIP_TRY(c, hipMemcpyAsync((char *)din + (pc.off - lo_all), pc.src, pc.len, hipMemcpyDeviceToDevice, c->up_stream));
        c->device_input_stats[1].fetch_add(n_copies, std::memory_order_relaxed);
    }
    if (!n_jobs) return TS_OK;
    if (n_jobs > 0x7FFFFFFFull) return c->fail(TS_ERR_UNSUPPORTED, "too many device pieces in one group");
    const size_t bytes = (size_t)n_jobs * sizeof(tsgather::Job);
    if (!c->jobs_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->jobs_ev, hipEventDisableTiming));
    if (c->jobs_ev_pending) { HIP_TRY(c, hipEventSynchronize(c->jobs_ev)); c->jobs_ev_pending = false; }
    if ((c->pin_jobs.bytes < bytes && c->pin_jobs.ensure(bytes + bytes / 2) != hipSuccess) ||
        (c->d_jobs.bytes < bytes && c->d_jobs.ensure(bytes + bytes / 2) != hipSuccess)) {
        (void)hipGetLastError();
        return c->fail(TS_ERR_ALLOC, "cannot allocate the job list of the device pieces' gather");
    }
    tsgather::Job *job = (tsgather::Job *)c->pin_jobs.p;
    for (const UpPiece &pc : on_device) {
        if (pc.len >= kDeviceCopyMin) continue;
        tsgather::split_piece((uint64_t)(uintptr_t)pc.src, base + (pc.off - lo_all), pc.len, tsgather::kSliceBytes,
                              [&](uint64_t src, uint64_t dst, uint32_t n) { *job++ = tsgather::Job{src, dst - base, n, 0u}; });
    }
    if ((uint64_t)(job - (tsgather::Job *)c->pin_jobs.p) != n_jobs) return c->fail(TS_ERR_STATE, "device pieces: the job list does not hold what was counted");
    HIP_TRY(c, hipMemcpyAsync(c->d_jobs.p, c->pin_jobs.p, bytes, hipMemcpyHostToDevice, c->up_stream));
    HIP_TRY(c, hipEventRecord(c->jobs_ev, c->up_stream));
    c->jobs_ev_pending = true;
    if (ts_k_launch_gather_pieces(c->d_jobs.p, (uint32_t)n_jobs, din, c->up_stream) != 0)
        return c->fail(TS_ERR_HIP, "gather kernel launch failed");
    c->device_input_stats[2].fetch_add(n_jobs, std::memory_order_relaxed);
    c->device_input_stats[3].fetch_add(1, std::memory_order_relaxed);
    return TS_OK;
}


// Uploads pieces of an input layout to the device buffer that holds its bytes from lo_all on (din = address of byte
// lo_all).  Consecutive pieces that lie close together in the layout (full scans, reads: a few padding bytes apart) are
// mirrored together in one of three pinned 32 MB buffers, filled by several host threads — plain bases by memcpy, FASTA
// text by a copy that skips the line ends — and leave by ONE DMA while the next buffer is being filled (one memcpy
// stream fills pinned memory at ~10 GB/s, a fraction of what the link moves; one copy per read would cost ~10 us each,
// one pageable 3 GB copy ~0.5 s).  Pieces far apart (the two terminal regions of a long contig in tips-only mode) go
// separately.  Bytes between pieces are never read as bases (the kernels mask everything past a region's end).
// Pieces that already lie on the device (TS_INPUT_DEVICE) take no part in any of this: no pinned slot, no host thread —
// gather_device_pieces above, queued on up_stream BEHIND the host pieces' chunks (a chunk's DMA or unpack kernel also writes the
// padding between its pieces, where a device piece may lie; the stream's order makes the device piece's bytes the last written).
// Asynchronous: the DMAs are queued on up_stream.  `pieces` ascend by offset and do not overlap.
// This function drives: the knobs, the slots and their events, the choice between the packed and the ASCII route per chunk, the DMAs
// and the unpack launch, the counters and the timing line.  What a chunk is and every byte that lands in its slot: upload_stage_core.h.
int upload_pieces(ts_ctx *c, const std::vector<UpPiece> &pieces_in, void *din, uint64_t lo_all, int &slot, bool used[]) {
    using tsstage::kChunk;
    using tsstage::kChunkPacked;
    tsstage::CallPieces call;
    if (tsstage::normalise_pieces(pieces_in, kChunk, call) == tsstage::Refused::TextPieceTooLong)
        return c->fail(TS_ERR_INVALID_ARG, "a text piece holds more than 32 MiB of bases");
    const UpPiece *pieces = call.host.data();
    const size_t n_pieces = call.host.size();
    const bool any_packed = call.any_packed;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nthr = std::min(8u, std::max(1u, hw / 2u));
    tsstage::StagePool stage_pool(call.total_bytes >= (8u << 20) ? nthr : 1u);
    const bool pooled = !stage_pool.threads.empty();          // (without threads a chunk's ranges run one after the other on the caller)
    std::atomic<int> bad_text{0};
    const bool fold = c->params.fold_case != 0;
    bool use_packed = (c->knobs.packed_upload && call.total_bytes >= c->knobs.packed_min_bytes) || any_packed;   // (bases that arrive packed leave packed)
    if (use_packed && !c->d_pack[0].p) {                       // the device side of the ring, once per context
        for (int q = 0; q < ts_ctx::kUpSlots && use_packed; ++q) {
            if (c->d_pack[q].ensure((kChunkPacked >> 2) + 4096) != hipSuccess || c->d_runs[q].ensure((size_t)kPackRunCap * 8) != hipSuccess ||
                c->pin_runs[q].ensure((size_t)kPackRunCap * 8) != hipSuccess) { (void)hipGetLastError(); use_packed = false; }
        }
    }
    if (any_packed && !use_packed) return c->fail(TS_ERR_ALLOC, "packed input needs the packed upload's device buffers");
    static const bool stage_timing = getenv("TS_TIMING") != nullptr && getenv("TS_STAGE_TIMING") != nullptr;
    double t_wait = 0, t_pack = 0, t_issue = 0;
    size_t n_chunks = 0;
    struct Report { const bool on; double &w, &p, &i; size_t &n; ~Report() { if (on && n) fprintf(stderr, "  upload_pieces: %zu chunks, waiting for a free slot %.2f ms, packing %.2f ms, runs + DMA + unpack enqueue %.2f ms\n", n, w, p, i); } }
        report{stage_timing, t_wait, t_pack, t_issue, n_chunks};
    for (size_t i = 0; i < n_pieces;) {
        const uint64_t c0 = pieces[i].off;
        const tsstage::Extent ext = tsstage::chunk_extent(pieces, n_pieces, i, use_packed ? kChunkPacked : kChunk, tsstage::kMaxGap);
        const size_t j = ext.end;
        const uint64_t bytes = ext.bytes, hi_pos = pieces[j - 1].off + pieces[j - 1].len;
        const auto tw0 = Clock::now();
        if (used[slot]) HIP_TRY(c, hipEventSynchronize(c->pin_up_ev[slot]));
        if (stage_timing) t_wait += ms_between(tw0, Clock::now());
        ++n_chunks;
        char *dst = (char *)c->pin_up[slot].p;
        const unsigned nt = bytes >= (4u << 20) ? nthr : 1u;
        const bool packed = use_packed && (bytes >= 4096 || any_packed);
        uint64_t add[8] = {0, 1, 0, 0, 0, 0, nt > 1u && pooled ? 1u : 0u, 0};      // (ts_upload_stats; an ASCII chunk's, a packed one fills its own in)
        Clock::time_point tp1;
        if (packed) {
            // the chunk leaves as 2-bit codes + invalid runs, a quarter of the bytes; unpack.hip restores the byte layout on the device
            tsstage::PackedChunk pk(pieces, i, j, nt);
            auto pack = [&](unsigned t) { if (!pk.pack(t, dst, fold)) bad_text.store(1); };
            const auto tp0 = Clock::now();
            if (nt == 1u) pack(0); else stage_pool.run(nt, pack);
            tp1 = Clock::now();
            if (stage_timing) t_pack += ms_between(tp0, tp1);
            const size_t nruns = pk.n_runs();
            if (nruns > kPackRunCap) {
                // a chunk with more invalid runs than the list holds is not sequence data: the rest of the call goes the plain way
                if (any_packed) return c->fail(TS_ERR_INVALID_ARG, "packed input with more invalid runs per 128 Mi bases than the upload carries (2^18)");
                use_packed = false;
                continue;
            }
            const uint64_t pbytes = tsstage::packed_bytes(pk.P);
            if (pbytes + 8 > c->pin_up[slot].bytes || pbytes + 8 > c->d_pack[slot].bytes)
                return c->fail(TS_ERR_STATE, "packed upload: a chunk does not fit its staging slot");
            ts::InvalidRun *hr = (ts::InvalidRun *)c->pin_runs[slot].p;
            pk.finish(dst, hr, pooled, add);
            HIP_TRY(c, hipMemcpyAsync(c->d_pack[slot].p, dst, pbytes + 8, hipMemcpyHostToDevice, c->up_stream));
            if (nruns) HIP_TRY(c, hipMemcpyAsync(c->d_runs[slot].p, hr, nruns * sizeof(ts::InvalidRun), hipMemcpyHostToDevice, c->up_stream));
            if (ts_k_launch_unpack(c->d_pack[slot].p, (uint32_t)(c0 - pk.c0a), (char *)din + (c0 - lo_all), hi_pos - c0, c->d_runs[slot].p, (uint32_t)nruns,
                                   (char *)din + (c0 - lo_all) - (c0 - pk.c0a), c->up_stream) != 0)
                return c->fail(TS_ERR_HIP, "unpack kernel launch failed");
        } else {
            // the chunk leaves as it is: the pieces mirrored in the slot, one DMA
            if (nt == 1u) {
                if (!tsstage::ascii_single(pieces, i, j, c0, dst)) bad_text.store(1);
            } else if (call.any_text) {
                std::atomic<size_t> next{i};
                stage_pool.run(nt, [&](unsigned) { if (!tsstage::ascii_whole_pieces(pieces, j, c0, dst, next)) bad_text.store(1); });
            } else {
                stage_pool.run(nt, [&](unsigned t) { tsstage::ascii_share(pieces, i, j, c0, dst, bytes, nt, t); });
            }
            HIP_TRY(c, hipMemcpyAsync((char *)din + (c0 - lo_all), dst, hi_pos - c0, hipMemcpyHostToDevice, c->up_stream));
        }
        HIP_TRY(c, hipEventRecord(c->pin_up_ev[slot], c->up_stream));
        for (int q = 0; q < 8; ++q) if (add[q]) c->upload_stats[q].fetch_add(add[q], std::memory_order_relaxed);
        if (packed && stage_timing) t_issue += ms_between(tp1, Clock::now());
        used[slot] = true;
        slot = (slot + 1) % ts_ctx::kUpSlots;
        i = j;
    }
    if (bad_text.load()) return c->fail(TS_ERR_INVALID_ARG, "a text piece holds fewer bases than it declares");
    return gather_device_pieces(c, call.on_device, din, lo_all);
}

// The upload pieces of one scanned region of an item: its bases [rg_start, rg_start + rg_len), whose first lies at byte
// layout_off of the input layout, clipped to the layout range [lo, hi) the caller uploads — from whichever of the four
// input formats the item arrived in.
int region_pieces(ts_ctx *c, const Item &it, uint64_t seg_len, uint64_t rg_start, uint64_t rg_len, uint64_t layout_off,
                  uint64_t lo, uint64_t hi, std::vector<UpPiece> &pieces) {
    if (it.format == TS_INPUT_TEXT_PIECES) {
        // the region's bases out of the segment's text pieces
        const ts_text_piece *tp = (const ts_text_piece *)it.seq;
        uint64_t cum = 0, want = rg_start, left = rg_len, off = layout_off;
        for (size_t k = 0; left; ++k) {
            if (k >= it.n_pieces || cum >= seg_len)
                return c->fail(TS_ERR_INVALID_ARG, "text pieces hold fewer bases than the segment's length (or n_pieces is not set)");
            const ts_text_piece &t = tp[k];
            if (t.text_len > (16ull << 20) + 4096) return c->fail(TS_ERR_INVALID_ARG, "a text piece is larger than 16 MiB");
            if (want >= cum + t.n_bases) { cum += t.n_bases; continue; }      // wholly before the region
            const uint64_t skip = want - cum;
            const uint64_t n = std::min<uint64_t>(t.n_bases - skip, left);
            // of these n bases, those the range reads (a shard uploads only its part of a segment)
            const uint64_t a = std::max<uint64_t>(off, lo), z = std::min<uint64_t>(off + n, hi);
            if (z > a) {
                const uint64_t skip2 = skip + (a - off);
                const char *from = skip2 ? text_locate(t.text, t.text_len, skip2) : t.text;
                pieces.push_back({a, from, z - a, (uint64_t)(t.text + t.text_len - from)});
            }
            off += n; left -= n; want += n; cum += t.n_bases;
        }
        return TS_OK;
    }
    const uint64_t s0 = std::max<uint64_t>(layout_off, lo), s1 = std::min<uint64_t>(layout_off + rg_len, hi);
    if (it.format == TS_INPUT_PACKED2) {
        const ts_packed_seq *ps = (const ts_packed_seq *)it.seq;
        if (!ps || (!ps->codes && seg_len) || (ps->n_runs && !ps->runs)) return c->fail(TS_ERR_INVALID_ARG, "packed input: null codes or runs");
        if (s1 > s0) {
            UpPiece pc{s0, nullptr, s1 - s0, 0};
            pc.packed = ps; pc.packed_first = rg_start + (s0 - layout_off);
            pieces.push_back(pc);
        }
        return TS_OK;
    }
    if (s1 > s0) {
        UpPiece pc{s0, it.seq + rg_start + (s0 - layout_off), s1 - s0, 0};
        pc.device = it.format == TS_INPUT_DEVICE;                 // (the same bytes, already in HBM: copied there, never read here)
        pieces.push_back(pc);
    }
    return TS_OK;
}

// Uploads the bases a batch reads: whole segments of a full scan; only the two terminal regions of a long segment
// in tips-only mode — the rest of the layout is never read.
int upload_batch(ts_batch *b, const Item *items, int &slot, bool used[]) {
    ts_ctx *c = b->ctx;
    void *din = ts_batch_input_ptr_nozero(b);
    if (!din) return c->fail(TS_ERR_ALLOC, "cannot allocate device input buffer");
    std::vector<UpPiece> pieces;
    for (size_t i = 0; i < b->segs.size(); ++i) {
        const SegPlan &sp = b->segs[i];
        for (const Region &rg : sp.regions) {
            // (consecutive regions of one segment never overlap: tips regions are [0,t) and [N-t,N) with N > 2t)
            const int rc = region_pieces(c, items[i], sp.len, rg.start, rg.len, sp.in_off + rg.start, b->in_lo, b->in_hi, pieces);
            if (rc != TS_OK) return rc;
        }
    }
    return upload_pieces(c, pieces, din, b->in_lo, slot, used);
}

// Layout of a tips batch's per-read table (d_readtab): the first tile of every read (and the end), in_off and len per read, then
// the list of long reads, its counter and the overflow flag
struct ReadTab {
    size_t in, len, long_list, count, flag, bytes;
    explicit ReadTab(size_t ns) : in(((ns + 1) * 4 + 15) & ~(size_t)15), len(in + ns * 8), long_list(len + ns * 8),
                                  count((long_list + ns * 4 + 15) & ~(size_t)15), flag(count + 16), bytes(flag + 16) {}
};

// the per-read table of a tips batch (ReadTab), built and uploaded once per batch
int ensure_readtab(ts_batch *b, hipStream_t st) {
    ts_ctx *c = b->ctx;
    const size_t ns = b->segs.size();
    const ReadTab T(ns);
    if (!b->d_readtab.p) {
        std::vector<char> tab(T.bytes);
        for (size_t i = 0; i < ns; ++i) {
            ((uint32_t *)tab.data())[i] = b->segs[i].first_tile;
            ((unsigned long long *)(tab.data() + T.in))[i] = b->segs[i].in_off;
            ((unsigned long long *)(tab.data() + T.len))[i] = b->segs[i].len;
        }
        ((uint32_t *)tab.data())[ns] = (uint32_t)b->tiles.size();
        b->all_terminal = true;                                   // every segment terminal zone as a whole: the lean predicate kernel
        for (size_t i = 0; i < ns; ++i) if (b->segs[i].len > c->params.terminal_limit) b->all_terminal = false;
        HIP_TRY(c, c->pool.take(T.bytes, b->d_readtab));
        HIP_TRY(c, hipMemcpyAsync(b->d_readtab.p, tab.data(), T.bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));                    // (tab is a local)
    }
    return TS_OK;
}

// The terminal-block predicate of a scanned tips batch on the device: one byte per read
// (ReadTelomereFilter::matches, src/read-filter.cpp:37-45, reduced to !terminalBlocks.empty()), written to
// d_pass (device).  The per-read table the kernel walks is built once per batch.
// d_ends (instead of a predicate): the same walks reduced to the longest terminal block per side, two u32 per segment
// (ts_terminal_ends); the overflow flag is then left for the caller to read.
int batch_read_pass_device(ts_batch *b, unsigned char *d_pass, hipStream_t st, uint32_t *d_ends = nullptr) {
    ts_ctx *c = b->ctx;
    const size_t ns = b->segs.size();
    if (!ns) return TS_OK;
    const ReadTab T(ns);
    { const int rc = ensure_readtab(b, st); if (rc != TS_OK) return rc; }
    char *const dt = (char *)b->d_readtab.p;
    TsPredParams Q{};
    Q.terminal_limit = c->params.terminal_limit;
    Q.max_match_dist = c->params.max_match_dist;
    Q.min_block_len = c->params.min_block_len;
    Q.max_block_dist = c->params.max_block_dist;
    Q.min_block_counts = c->params.min_block_counts;
    Q.min_block_density = c->params.min_block_density;
    Q.k = c->k;
    Q.long_list = 128;                                        // floor of the per-wave threshold, see ts_terminal_predicate
    // the predicate's or the ends' launcher: the same walks and arguments, one byte or two u32 per segment out
    auto launch = [&](auto launcher, auto *dst) {
        return launcher((const TsTile *)b->d_tiles.p, (const unsigned long long *)b->d_tile_off.p,
                        b->stats_ptr(), b->records_ptr(), b->records_limit(), (const uint32_t *)dt,
                        (const unsigned long long *)(dt + T.in), (const unsigned long long *)(dt + T.len),
                        (uint32_t)ns, &Q, dst, (uint32_t *)(dt + T.long_list), (uint32_t *)(dt + T.count),
                        // the lean kernel: every segment terminal zone as a whole, and the records in the batch's own
                        // regions (16-byte aligned, 16 bytes of slack behind them: whole aligned blocks can be fetched)
                        (b->all_terminal && !b->dense && ((uintptr_t)b->records_ptr() & 15u) == 0) ? 1 : 0,
                        (const uint32_t *)b->d_fill.p, b->dense ? 0xFFFFFFFFu : b->region_cap, b->dense ? 0u : b->total_waves,
                        (uint32_t *)(dt + T.flag), b->records16() ? 1 : 0, st);
    };
    if ((d_ends ? launch(ts_k_launch_terminal_ends, d_ends) : launch(ts_k_launch_predicate, d_pass)) != 0)
        return c->fail(TS_ERR_HIP, d_ends ? "terminal-ends kernel launch failed" : "predicate kernel launch failed");
    return TS_OK;
}

int batch_read_pass(ts_batch *b, uint8_t *pass_out, hipStream_t st) {
    ts_ctx *c = b->ctx;
    const size_t ns = b->segs.size();
    if (!ns) return TS_OK;
    DevBuf d_pass;
    struct Return { ts_ctx *c; DevBuf &a; ~Return() { c->pool.give(std::move(a)); } } give_back{c, d_pass};
    HIP_TRY(c, c->pool.take(ns + 16, d_pass));
    int rc = batch_read_pass_device(b, (unsigned char *)d_pass.p, st);
    if (rc != TS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(pass_out, d_pass.p, ns, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return TS_OK;
}

// the longest terminal block at either side of a segment, from its terminal blocks (start: absolute position)
void reduce_terminal_ends(const ts_segment_out &o, uint64_t len, uint64_t abs_pos, uint32_t *two) {
    two[0] = two[1] = 0u;
    for (uint64_t j = 0; j < o.n_terminal_blocks; ++j) {
        const ts_block &blk = o.terminal_blocks[j];
        const uint64_t rel = blk.start - abs_pos;
        uint32_t &side = two[rel <= len - (rel + blk.block_len) ? 0 : 1];      // walkSegment, src/input.cpp:849-853
        side = std::max(side, blk.block_len);
    }
}

// ts_terminal_ends of a scanned tips batch: the per-side maxima of every segment to ends_out (2 x u32 per segment).  After a
// region overflow in the scan (the guard's flag: the kernel judged nothing) the group's blocks are called and reduced instead.
int batch_terminal_ends(ts_batch *b, uint32_t *ends_out, int slot, hipStream_t st) {
    ts_ctx *c = b->ctx;
    const size_t ns = b->segs.size();
    if (!ns) return TS_OK;
    DevBuf d_ends;
    struct Return { ts_ctx *c; DevBuf &a; ~Return() { c->pool.give(std::move(a)); } } give_back{c, d_ends};
    HIP_TRY(c, c->pool.take(ns * 8 + 16, d_ends));
    int rc = batch_read_pass_device(b, nullptr, st, (uint32_t *)d_ends.p);
    if (rc != TS_OK) return rc;
    char *const flag_at = (char *)b->d_readtab.p + ReadTab(ns).flag;
    uint32_t flag = 0;
    HIP_TRY(c, hipMemcpyAsync(ends_out, d_ends.p, ns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&flag, flag_at, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->terminal_ends_stats[3].fetch_add(ns * 8 + 4, std::memory_order_relaxed);
    c->terminal_ends_stats[flag ? 2 : 0].fetch_add(ns, std::memory_order_relaxed);
    if (!flag) return TS_OK;
    HIP_TRY(c, hipMemsetAsync(flag_at, 0, 4, st));
    ts_fetched *f = ts_batch_fetch(b, false, slot, &rc);
    std::vector<ts_segment_out> tmp(ns);
    if (rc == TS_OK) rc = ts_batch_finalize(b, f, tmp.data());
    if (rc == TS_OK)
        for (size_t i = 0; i < ns; ++i) reduce_terminal_ends(tmp[i], b->segs[i].len, b->segs[i].abs_pos, ends_out + 2 * i);
    ts_free_segments(tmp.data(), ns);
    return rc;
}

int batch_counts(ts_batch *b, ts_segment_counts *counts, bool tips, hipStream_t st) {
    ts_ctx *c = b->ctx;
    const size_t ns = b->segs.size();
    std::vector<unsigned long long> summary(4 * ns);
    DevBuf d_sum;
    struct Return { ts_ctx *c; DevBuf &a; ~Return() { c->pool.give(std::move(a)); } } give_back{c, d_sum};
    HIP_TRY(c, c->pool.take(summary.size() * 8 + 16, d_sum));
    int rc = ts_batch_segment_summary(b, d_sum.p, st);
    if (rc != TS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(summary.data(), d_sum.p, summary.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (size_t i = 0; i < ns; ++i)
        counts[i] = ts_segment_counts{tips ? 0 : summary[4 * i], summary[4 * i + 1], summary[4 * i + 2], summary[4 * i + 3]};
    return TS_OK;
}

// The three-stage pipeline over the groups of one call.  items: the call's segments or reads in input order;
// results go to o at the same indices.
int run_pipeline(ts_ctx *ctx, Mode mode, bool tips, const std::vector<Item> &items, Outputs o) {
    if (items.empty()) return TS_OK;
    if (ctx->device == kNoDevice) return ctx->fail(TS_ERR_NO_DEVICE, "planning-only context: no HIP device behind it");
    const auto t_begin = Clock::now();
    const bool timing = ctx->knobs.timing;                       // stage times to stderr
    const bool match_text = mode == Mode::Tracks && !tips && o.matches && ctx->params.out_matches;   // ts_scan_segments_text under -m
    {
        DeviceGuard g(ctx->device);
        if (g.error() != hipSuccess) return ctx->fail(TS_ERR_HIP, "hipSetDevice failed");
        int rc = ensure_streams(ctx);
        if (rc != TS_OK) return rc;
    }
    // groups of consecutive items, ~256 MB of input layout each (an item larger than that is its own group)
    std::vector<Group> groups;
    {
        const uint64_t target = group_target_bytes();
        uint64_t acc = 0;
        Group g;
        for (size_t i = 0; i < items.size(); ++i) {
            const uint64_t bytes = (items[i].len + 15) & ~15ull;
            if (g.count && acc + bytes > target) { groups.push_back(g); g = Group{}; g.first = i; acc = 0; }
            ++g.count;
            acc += bytes;
        }
        if (g.count) groups.push_back(g);
    }
    std::atomic<int> first_err{TS_OK};
    auto set_err = [&](int rc) { int expected = TS_OK; first_err.compare_exchange_strong(expected, rc); };
    Channel<Group *> to_scan, to_down;
    Semaphore inputs_in_flight(2);                               // device input buffers alive at a time

    // planning (host only: tiles, windows, the input layout of a group) runs a group or more ahead of the upload on a thread
    // of its own: for read batches — hundreds of thousands of segments — it takes as long as the upload itself
    Channel<Group *> to_upload;
    std::thread planner([&] {
        ctx->bind_this_thread();
        DeviceGuard g(ctx->device);
        std::vector<uint64_t> lens, abs;
        for (Group &gr : groups) {
            if (first_err.load() != TS_OK) break;
            const auto t0 = Clock::now();
            lens.resize(gr.count); abs.resize(gr.count);
            for (size_t i = 0; i < gr.count; ++i) { lens[i] = items[gr.first + i].len; abs[i] = items[gr.first + i].abs_pos; }
            gr.b = ts_batch_create(ctx, lens.data(), abs.data(), gr.count, tips ? 1 : 0, 0);
            if (gr.b) (void)ts_batch_set_emit(gr.b, 1);      // every download calls blocks on the device
            gr.t_plan = ms_between(t0, Clock::now());
            if (!gr.b) { set_err(ctx->error.rfind("unsupported", 0) == 0 ? TS_ERR_UNSUPPORTED : TS_ERR_HIP); break; }
            to_upload.push(&gr);
        }
        to_upload.close();
    });

    std::thread uploader([&] {
        ctx->bind_this_thread();
        DeviceGuard g(ctx->device);
        int slot = 0;
        bool used[ts_ctx::kUpSlots] = {false, false, false};
        Group *grp;
        while (to_upload.pop(grp)) {
            Group &gr = *grp;
            if (first_err.load() != TS_OK) { ts_batch_destroy(gr.b); gr.b = nullptr; continue; }
            const auto t0 = Clock::now();
            inputs_in_flight.acquire();
            int rc = ts_batch_ensure_device(gr.b);
            const auto t1 = Clock::now();
            if (rc == TS_OK) rc = upload_batch(gr.b, items.data() + gr.first, slot, used);
            if (rc == TS_OK && hipEventCreateWithFlags(&gr.uploaded, hipEventDisableTiming) != hipSuccess) rc = ctx->fail(TS_ERR_HIP, "hipEventCreate failed");
            if (rc == TS_OK && hipEventRecord(gr.uploaded, ctx->up_stream) != hipSuccess) rc = ctx->fail(TS_ERR_HIP, "hipEventRecord failed");
            gr.t_plan += ms_between(t0, t1);
            gr.t_upload = ms_between(t1, Clock::now());
            if (rc != TS_OK) { set_err(rc); ts_batch_destroy(gr.b); gr.b = nullptr; inputs_in_flight.release(); continue; }
            to_scan.push(&gr);
        }
        (void)hipStreamSynchronize(ctx->up_stream);              // the pinned ring is free again when the call returns
        to_scan.close();
    });

    std::thread scanner([&] {
        ctx->bind_this_thread();
        DeviceGuard g(ctx->device);
        Group *gr;
        while (to_scan.pop(gr)) {
            const auto t0 = Clock::now();
            int rc = first_err.load();
            if (rc == TS_OK && hipStreamWaitEvent(ctx->scan_stream, gr->uploaded, 0) != hipSuccess) rc = ctx->fail(TS_ERR_HIP, "hipStreamWaitEvent failed");
            if (rc == TS_OK) rc = ts_batch_scan(gr->b, nullptr, ctx->scan_stream);
            if (rc == TS_OK) rc = ts_batch_sync(gr->b);          // waits for the scan; regrows + rescans on overflow
            // (match lines are cut out of the input buffer where it lies: the download stage gives it back)
            gr->input_kept = rc == TS_OK && match_text;
            if (!gr->input_kept) { ts_batch_release_input(gr->b); inputs_in_flight.release(); }
            gr->t_scan = ms_between(t0, Clock::now());
            if (rc != TS_OK) set_err(rc);
            to_down.push(gr);
        }
        to_down.close();
    });

    std::thread downloader([&] {
        ctx->bind_this_thread();
        DeviceGuard g(ctx->device);
        std::lock_guard<std::mutex> dl(ctx->down_mtx);           // the pinned landing areas are this call's
        Group *gr;
        std::thread post;                                        // host post-processing of the previous group
        int slot = 0;
        auto release_kept = [&](Group *g2) {
            if (!g2->input_kept) return;
            g2->input_kept = false;
            ts_batch_release_input(g2->b);
            inputs_in_flight.release();
        };
        auto retire = [&](Group *g2, double t_from) {
            release_kept(g2);
            if (g2->uploaded) (void)hipEventDestroy(g2->uploaded);
            ts_batch_destroy(g2->b);
            g2->b = nullptr;
            g2->t_down += t_from;
        };
        while (to_down.pop(gr)) {
            const auto t0 = Clock::now();
            int rc = first_err.load();
            if (rc == TS_OK) gr->b->last_stream = ctx->down_stream;   // the scan is complete (synced): later work runs on this stage's stream
            const Outputs go = o.slice(gr->first);
            if (rc == TS_OK && mode == Mode::ReadPass) {
                rc = batch_read_pass(gr->b, go.pass, ctx->down_stream);
            } else if (rc == TS_OK && mode == Mode::Ends) {
                rc = batch_terminal_ends(gr->b, go.ends, slot, ctx->down_stream);
            } else if (rc == TS_OK) {
                // device work + D2H of this group while the previous group's records are expanded on the host threads
                ts_fetched *f = ts_batch_fetch(gr->b, mode == Mode::Matches, slot, &rc, mode != Mode::Tracks);
                if (rc == TS_OK && (mode == Mode::Blocks || mode == Mode::Tracks) && go.counts) rc = batch_counts(gr->b, go.counts, tips, ctx->down_stream);
                const auto t_text0 = Clock::now();
                NameBlob nb;
                if (rc == TS_OK && mode == Mode::Tracks && !tips && (go.tracks || match_text)) rc = group_names(ctx, go.names, gr->b->segs.size(), nb);
                if (rc == TS_OK && mode == Mode::Tracks && go.tracks && !tips) {
                    std::vector<ts_track_segment> ts(gr->b->segs.size());
                    for (size_t i = 0; i < ts.size(); ++i) {
                        const SegPlan &sp = gr->b->segs[i];
                        ts[i] = ts_track_segment{sp.win_base, sp.n_windows, sp.abs_pos, sp.len, 0, 0, 0};
                    }
                    rc = group_tracks(ctx, gr->b->windows_ptr(), gr->b->n_windows, ts, nb, ctx->down_stream, go.tracks);
                }
                if (rc == TS_OK && match_text) {
                    // the records in the scan's own regions behind its tile directory, the bases in the batch's input buffer
                    ts_batch *b = gr->b;
                    std::vector<ts_match_line_segment> ms(b->segs.size());
                    for (size_t i = 0; i < ms.size(); ++i) ms[i] = ts_match_line_segment{0, 0, b->segs[i].abs_pos, b->segs[i].len, b->segs[i].in_off, 0, 0, 0};
                    TsMatchSource src;
                    src.form = b->records16() ? TS_MATCH_FORM_TILED16 : TS_MATCH_FORM_TILED32;
                    src.records = b->records_ptr(); src.tiles = b->d_tiles.p;
                    src.tile_off = (const unsigned long long *)b->d_tile_off.p; src.tile_stats = b->stats_ptr();
                    src.n_tiles = b->tiles.size(); src.bases = b->d_in.p; src.k = ctx->k;
                    if (!b->d_in.p || !b->whole()) rc = ctx->fail(TS_ERR_STATE, "match lines: the group's input buffer is gone");
                    else rc = group_matches(ctx, src, ms, nb, ctx->down_stream, go.matches);
                }
                release_kept(gr);
                gr->t_text = ms_between(t_text0, Clock::now());
                gr->t_fetch = ms_between(t0, Clock::now());
                if (post.joinable()) post.join();
                if (rc == TS_OK) {
                    Group *g2 = gr;
                    post = std::thread([&, g2, f, go] {
                        DeviceGuard g3(ctx->device);
                        const auto p0 = Clock::now();
                        const int prc = ts_batch_finalize(g2->b, f, go.out);
                        if (prc != TS_OK) set_err(prc);
                        g2->t_final = ms_between(p0, Clock::now());
                        retire(g2, g2->t_final);
                    });
                    slot ^= 1;
                    gr->t_down += ms_between(t0, Clock::now());
                    continue;
                }
                if (f) { std::vector<ts_segment_out> scratch(gr->count); (void)ts_batch_finalize(gr->b, f, scratch.data()); ts_free_segments(scratch.data(), scratch.size()); }
            }
            if (rc != TS_OK) set_err(rc);
            retire(gr, ms_between(t0, Clock::now()));
        }
        if (post.joinable()) post.join();
    });
    planner.join();
    uploader.join();
    scanner.join();
    downloader.join();
    if (timing) {
        double p = 0, u = 0, s = 0, d = 0, f = 0, z = 0, x = 0;
        for (const Group &gr : groups) { p += gr.t_plan; u += gr.t_upload; s += gr.t_scan; d += gr.t_down; f += gr.t_fetch; z += gr.t_final; x += gr.t_text; }
        const char *name = mode == Mode::Matches ? "ts_scan_segments" : mode == Mode::Blocks ? "ts_scan_segments_blocks"
                         : mode == Mode::Tracks ? "ts_scan_segments_tracks" : mode == Mode::Ends ? "ts_terminal_ends" : "ts_filter_reads";
        fprintf(stderr, "%s: %zu items in %zu groups, wall %.1f ms; stage sums (concurrent): plan %.1f ms, stage+upload %.1f ms, "
                        "scan (incl. waiting for the upload) %.1f ms, download + host post-processing %.1f ms (device work + D2H %.1f ms, host expansion %.1f ms)\n",
                name, items.size(), groups.size(), ms_between(t_begin, Clock::now()), p, u, s, d, f, z);
        if (mode == Mode::Tracks)
            fprintf(stderr, "%s: text step (window tracks%s formatted on the device, within the device work above) %.1f ms; bases read back: 0, match records read back: 0\n",
                    name, match_text ? " and match lines" : "", x);
    }
    return first_err.load();
}

// ---------------------------------------------------------------------------------------- coalescing of concurrent callers
}  // namespace
struct SubmitReq {
    int mode; bool tips;
    const std::vector<Item> *items;
    Outputs o;
    int rc = TS_OK; bool done = false;
    std::string error;
};
namespace {

// One pipeline run for the requests of `group` (all of one mode and kind): their items back to back, every caller's slice of
// the results to its own arrays.  When the merged run fails and more than one caller is in it, each request is run on its
// own, so that only the call that brought the bad input fails.
void run_group(ts_ctx *ctx, std::vector<SubmitReq *> &group) {
    std::lock_guard<std::mutex> api(ctx->api_mtx);
    const Mode mode = (Mode)group[0]->mode;
    const bool tips = group[0]->tips;
    if (group.size() == 1) {
        SubmitReq &r = *group[0];
        r.rc = run_pipeline(ctx, mode, tips, *r.items, r.o);
        if (r.rc != TS_OK) r.error = ctx->error;
        return;
    }
    size_t total = 0;
    for (SubmitReq *r : group) total += r->items->size();
    std::vector<Item> items;
    items.reserve(total);
    for (SubmitReq *r : group) items.insert(items.end(), r->items->begin(), r->items->end());
    std::vector<ts_segment_out> out(mode == Mode::ReadPass || mode == Mode::Ends ? 0 : total);
    std::vector<ts_segment_counts> counts(mode == Mode::Blocks ? total : 0);
    std::vector<uint8_t> pass(mode == Mode::ReadPass ? total : 0);
    std::vector<uint32_t> ends(mode == Mode::Ends ? 2 * total : 0);
    const Outputs merged{out.empty() ? nullptr : out.data(), counts.empty() ? nullptr : counts.data(),
                         pass.empty() ? nullptr : pass.data(), ends.empty() ? nullptr : ends.data()};
    const int rc = run_pipeline(ctx, mode, tips, items, merged);
    if (rc == TS_OK) {
        size_t at = 0;
        for (SubmitReq *r : group) {
            const size_t n = r->items->size();
            const Outputs from = merged.slice(at);
            if (r->o.out) std::memcpy(r->o.out, from.out, n * sizeof(ts_segment_out));
            if (r->o.counts) std::memcpy(r->o.counts, from.counts, n * sizeof(ts_segment_counts));
            if (r->o.pass) std::memcpy(r->o.pass, from.pass, n);
            if (r->o.ends) std::memcpy(r->o.ends, from.ends, n * 8);
            r->rc = TS_OK;
            at += n;
        }
        return;
    }
    if (!out.empty()) ts_free_segments(out.data(), out.size());
    for (SubmitReq *r : group) {
        r->rc = run_pipeline(ctx, mode, tips, *r->items, r->o);
        if (r->rc != TS_OK) r->error = ctx->error;
    }
}

// run_pipeline for a caller that does not hold the context's call lock: alone, it runs at once; beside others, it is merged
// with them.  (A merged run is capped at ~8 GB of input: what is left waits for the next one.)
int submit_pipeline(ts_ctx *ctx, Mode mode, bool tips, const std::vector<Item> &items, Outputs o) {
    if (items.empty()) return TS_OK;
    SubmitReq req{(int)mode, tips, &items, o, TS_OK, false, std::string()};
    std::unique_lock<std::mutex> lk(ctx->sq_mtx);
    ctx->sq.push_back(&req);
    while (!req.done) {
        if (ctx->sq_leader) { ctx->sq_cv.wait(lk); continue; }
        ctx->sq_leader = true;
        while (!ctx->sq.empty()) {
            std::vector<SubmitReq *> group;
            const int m = ctx->sq.front()->mode;
            const bool t = ctx->sq.front()->tips;
            uint64_t bytes = 0;
            for (auto it = ctx->sq.begin(); it != ctx->sq.end();) {
                SubmitReq *r = *it;
                if (r->mode != m || r->tips != t) { ++it; continue; }
                uint64_t b = 0;
                for (const Item &x : *r->items) b += x.len;
                if (!group.empty() && bytes + b > (8ull << 30)) { ++it; continue; }
                bytes += b;
                group.push_back(r);
                it = ctx->sq.erase(it);
            }
            lk.unlock();
            // (a throw in here — std::bad_alloc on a merged multi-GB batch — must not leave the context with a leader that
            // no longer exists: every later caller would wait for it forever)
            try {
                run_group(ctx, group);
            } catch (const std::exception &e) {
                for (SubmitReq *r : group)
                    if (!r->done) { r->rc = TS_ERR_ALLOC; r->error = std::string("batched call failed: ") + e.what(); }
            } catch (...) {
                for (SubmitReq *r : group)
                    if (!r->done) { r->rc = TS_ERR_ALLOC; r->error = "batched call failed"; }
            }
            lk.lock();
            for (SubmitReq *r : group) r->done = true;
            ctx->sq_cv.notify_all();
        }
        ctx->sq_leader = false;
        ctx->sq_cv.notify_all();
    }
    if (req.rc != TS_OK && !req.error.empty()) ctx->fail(req.rc, req.error);
    return req.rc;
}

// =========================================================================== general path
// Parameter sets outside the tiled kernel's closed form (mixed-length pattern sets, pattern lengths above 8, or a
// longest pattern exceeding min(step, window-step) where the reference's uint32 start index wraps): the general
// kernels of generic.hip over groups of ~256 MB of regions at a time — match masks, the records the reference pushes
// and the window records all come off the device, and blocks are called on the device; the host assembles SegmentData
// from them (ts_assemble_general).  Group g + 1 is planned, staged and uploaded on a thread of its own while group g's
// kernels, block calling and download run on the calling thread, and group g - 1's host stage runs on a third.

struct GenRegion { uint64_t seg_start, len, layout_off; };                  // a scanned region and where it lies in the layout
struct GenSeg { uint64_t len, abs_pos, layout_off; std::vector<GenRegion> regions; uint64_t first_tile = 0, n_tiles = 0, win_base = 0, n_windows = 0; };

// What a group's host stage reads (it runs while the next group is on the device)
struct GenHost {
    size_t first = 0;                                     // the group's items: [first, first + G.size())
    std::vector<GenSeg> G;
    std::vector<TsGeneralTile> tiles;
    std::vector<unsigned long long> tile_off;
    std::vector<uint32_t> recs_heap, wins_heap;
    const uint32_t *recs = nullptr, *wins = nullptr;      // the landing area: pinned, or the heap vectors
    uint64_t nrecs = 0;                                   // records downloaded
    std::vector<TsDevBlock> blocks;
    std::vector<unsigned long long> sums;
};

// One group on the device: planned and uploaded by gen_prepare, its other buffers taken by gen_fused; all go back to the pool
struct GenGroup {
    ts_ctx *c;
    std::shared_ptr<GenHost> gh;
    DevBuf d_in, d_tiles, d_tab, d_slots, d_stats, d_off, d_tmp, d_rec, d_win;
    uint64_t nwin_total = 0, nrec = 0;
    uint32_t slot_cap = 0;
    const uint32_t *d_records = nullptr;                  // the stream block calling reads: d_rec, or the slots themselves
    Clock::time_point t_dev0;
    double ms_up = 0;
    int rc = TS_OK;
    explicit GenGroup(ts_ctx *c_) : c(c_) {}
    ~GenGroup() { for (DevBuf *d : {&d_in, &d_tiles, &d_tab, &d_slots, &d_stats, &d_off, &d_tmp, &d_rec, &d_win}) c->pool.give(std::move(*d)); }
    // the segment table: len, layout offset, window base, window count per segment (4 x ns u64), the window total, the overflow flag
    size_t tab_win() const { return 2 * gh->G.size() * 8; }
    size_t tab_nwin() const { return 3 * gh->G.size() * 8; }
    size_t tab_flag() const { return 4 * gh->G.size() * 8 + 8; }
};

// The state of one call that its steps share
struct GenCall {
    ts_ctx *c;
    const ts_params &P;
    Mode mode;
    bool tips, blocks_only, wide;
    const std::vector<Item> &items;
    Outputs o;
    TsGenericGeom Q{};
    uint64_t target;                                      // bytes of regions per group
    uint32_t len_spread;
    bool position_order, push_compact;
    // ts_terminal_ends over records that stay in their slots: the walks' ENDS form reduces them on the device (gen_ends) — no
    // directory, no block and no sum is downloaded, and the group has no host stage.  A stream the device would have to put in
    // push order first keeps the blocks path (no tips scan is one: the flag is the fallback's door, not a switch).
    bool ends_device;
    unsigned long long gen_lens = 0;
    // a tile's slot at the start of a group: what the groups before needed (a telomeric tile under a many-length set holds more
    // than a record per position; finding that out again for every group ran half the groups of a call twice)
    uint32_t slot_cap_call;
    // the upload (one group at a time, on the calling thread or the prefetch thread)
    size_t next_item = 0;
    int slot = 0;
    bool used[ts_ctx::kUpSlots] = {false, false, false};
    size_t group_no = 0;
    std::thread host_job;                                 // the host stage of the group before
    std::atomic<int> host_err{TS_OK};
    // TS_TIMING
    bool timing;
    Clock::time_point t_begin = Clock::now();
    double t_up = 0, t_dev = 0, t_host = 0, t_take = 0, t_fused = 0, t_blk = 0, t_d2h = 0, t_wait_next = 0, t_dbg[3] = {0, 0, 0};
    float t_kern = 0;
    uint32_t n_list = 0, n_strided = 0;                   // groups whose fused pass took the list / the position-strided form

    GenCall(ts_ctx *c_, Mode m, bool t, const std::vector<Item> &it, Outputs out)
        : c(c_), P(c_->params), mode(m), tips(t), blocks_only(m != Mode::Matches), wide(c_->gen_wide), items(it), o(out),
          timing(c_->knobs.timing) {
        const uint32_t s = P.step, w = P.window_size;
        Q = ts_general_geom(c);
        // the wide form (sets beyond 8 lengths / 32 bases): its own kernel, a 64-base halo, records with six bits of length index;
        // smaller groups, because a tile's slot may have to grow to a record per position AND length
        target = wide ? std::min<uint64_t>(group_target_bytes(), 256ull << 20) : group_target_bytes();   // (16 - 64 KB of slot per tile: 4 - 17 GB per group)
        // Block calling on the device (blockcall.hip with the general record formats).  The reference calls blocks over allMatches
        // as pushed (src/teloscope.cpp:485-509, :642-657): position order for tips-only scans, for w == s, and under w > s when the
        // pattern lengths differ by at most one (the record that ends later is never pushed earlier: end positions are monotone
        // in stream order, hence so is the pushing window).  Sets with a length gap of two or more under w > s are pushed not
        // quite in position order: for those the compaction writes the dense stream IN PUSH ORDER
        // (ts_general_compact_push) and block calling walks it as the reference does (blockcall.hip, MODE 1: the predecessor as
        // the stream lies, the search range by stream index from a bisection restated probe by probe).  The host's expansion
        // of such a stream needs no ordering pass either.
        len_spread = wide ? (c->wide_lens.empty() ? 0u : c->wide_lens.back() - c->wide_lens.front())
                          : (c->gpat.nlen ? c->gpat.len[c->gpat.nlen - 1] - c->gpat.len[0] : 0u);
        position_order = tips || w == s || len_spread <= 1u;                   // position order IS push order
        push_compact = !position_order;                                         // the device orders the stream
        ends_device = m == Mode::Ends && t && !push_compact;
        gen_lens = ts_general_gen_lens(c);                                      // (wide records: the lengths come from wpat.len; non-zero = "general format")
        slot_cap_call = ts_general_slot_start(c, TS_GENERAL_TILE);
    }
    ~GenCall() { if (host_job.joinable()) host_job.join(); }
};

// Plans a group of consecutive items, ~256 MB of regions (layout = the regions back to back, 16-byte aligned), and uploads its
// bases, tile list and segment table.
int gen_prepare(GenCall &g, GenGroup &gr) {
    ts_ctx *c = g.c;
    const ts_params &P = g.P;
    const uint32_t s = P.step;
    gr.gh = std::make_shared<GenHost>();
    GenHost &h = *gr.gh;
    h.first = g.next_item;
    std::vector<GenSeg> &G = h.G;
    std::vector<TsGeneralTile> &tiles = h.tiles;
    std::vector<UpPiece> pieces;
    uint64_t off = 0, nwin_total = 0;
    while (g.next_item < g.items.size() && (G.empty() || off < g.target)) {
        const Item &it = g.items[g.next_item];
        GenSeg sl{it.len, it.abs_pos, off, {}};
        if (!g.tips) sl.n_windows = ceil_div(it.len, s);
        sl.first_tile = tiles.size();
        for (const tsplan::Span &r : tsplan::scanned_regions(it.len, g.tips, P.terminal_limit)) {
            sl.regions.push_back({r.start, r.len, off});
            const int rc = region_pieces(c, it, it.len, r.start, r.len, off, 0, ~0ull, pieces);
            if (rc != TS_OK) return rc;
            tsplan::append_region_tiles(tiles, off, r.start, r.len, (uint32_t)G.size(), s, g.wide ? (uint32_t)TS_WIDE_HALO : 32u);
            off += (r.len + 15) & ~15ull;
        }
        sl.n_tiles = tiles.size() - sl.first_tile;
        sl.win_base = nwin_total;
        nwin_total += sl.n_windows;
        G.push_back(std::move(sl));
        ++g.next_item;
    }
    gr.nwin_total = nwin_total;
    const uint64_t span = off + 64;
    const size_t ns = G.size(), nt = tiles.size();
    if (nt >= 0x7FFFFFFFull) return c->fail(TS_ERR_UNSUPPORTED, "too many tiles in one group");
    const size_t tab_bytes = 4 * ns * 8 + 8 + 16;
    HIP_TRY(c, c->pool.take(span, gr.d_in));
    HIP_TRY(c, c->pool.take(std::max<size_t>(nt, 1) * sizeof(TsGeneralTile), gr.d_tiles));
    HIP_TRY(c, c->pool.take(tab_bytes, gr.d_tab));
    std::vector<unsigned long long> tab(4 * ns + 3, 0ull);
    for (size_t i = 0; i < ns; ++i) { tab[i] = G[i].len; tab[ns + i] = G[i].layout_off; tab[2 * ns + i] = G[i].win_base; tab[3 * ns + i] = G[i].n_windows; }
    tab[4 * ns] = nwin_total;
    const auto t0 = Clock::now();
    { int rc = upload_pieces(c, pieces, gr.d_in.p, 0, g.slot, g.used); if (rc != TS_OK) return rc; }
    HIP_TRY(c, hipMemcpyAsync(gr.d_tiles.p, tiles.data(), nt * sizeof(TsGeneralTile), hipMemcpyHostToDevice, c->up_stream));
    HIP_TRY(c, hipMemcpyAsync(gr.d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->up_stream));
    HIP_TRY(c, hipStreamSynchronize(c->up_stream));
    gr.ms_up = ms_between(t0, Clock::now());
    return TS_OK;
}

// The fused pass (match masks, records into per-tile slots, window records) and the tile offsets (a prefix sum over the tile
// counts).  A tile's slot holds one record per position — all a single-length set can produce; a mixed-length tile that holds
// more says so, and the group runs again with slots that cannot overflow.
int gen_fused(GenCall &g, GenGroup &gr) {
    ts_ctx *c = g.c;
    GenHost &h = *gr.gh;
    const size_t nt = h.tiles.size();
    const uint32_t s = g.P.step, w = g.P.window_size;
    hipStream_t st = c->scan_stream;
    const auto t0 = Clock::now();
    gr.slot_cap = g.slot_cap_call;
    // the list form of the fused pass (per-candidate work on full wavefronts) when a tile adds to few enough window
    // records for the accumulators it keeps in LDS; a tile dense enough to overflow a wave's candidate list sends the
    // group through the position-strided form instead
    bool use_list = ts_general_list_form_ok(c) && (g.tips || ((uint64_t)TS_GENERAL_TILE + w) / s + 3 <= ts_k_general_list_max_records());
    HIP_TRY(c, c->pool.take(std::max<size_t>(nt, 1) * (size_t)gr.slot_cap * 4, gr.d_slots));
    HIP_TRY(c, c->pool.take((nt + 1) * 16, gr.d_stats));
    HIP_TRY(c, c->pool.take((nt + 1) * 8, gr.d_off));
    HIP_TRY(c, c->pool.take((size_t)ts_k_scan_tmp_bytes((uint32_t)nt), gr.d_tmp));
    if (gr.nwin_total) HIP_TRY(c, c->pool.take(gr.nwin_total * 32, gr.d_win));
    const auto t1 = Clock::now();
    gr.t_dev0 = t1;
    g.t_up += gr.ms_up;
    g.t_take += ms_between(t0, t1);
    char *const dt = (char *)gr.d_tab.p;
    const unsigned long long *const tab_len = (const unsigned long long *)dt, *const tab_win = (const unsigned long long *)(dt + gr.tab_win()),
                             *const tab_nwin = (const unsigned long long *)(dt + gr.tab_nwin());
    uint32_t *const d_flag = (uint32_t *)(dt + gr.tab_flag());
    std::vector<unsigned long long> &tile_off = h.tile_off;
    tile_off.assign(nt + 1, 0);
    for (int attempt = 0;; ++attempt) {
        uint32_t flag = 0;
        {
            std::lock_guard<std::mutex> lk(c->mtx);
            if (g.timing) HIP_TRY(c, hipEventRecord(c->gen_ev[0], st));
            HIP_TRY(c, hipMemsetAsync(d_flag, 0, 16, st));
            if (gr.nwin_total) HIP_TRY(c, hipMemsetAsync(gr.d_win.p, 0, gr.nwin_total * 32, st));
            const int rc = ts_general_launch_fused(c, gr.d_in.p, (const TsGeneralTile *)gr.d_tiles.p, (uint32_t)nt, tab_len, tab_win, tab_nwin, d_flag,
                                                   g.tips, gr.slot_cap, (uint32_t *)gr.d_stats.p, (uint32_t *)gr.d_slots.p, (uint32_t *)gr.d_win.p,
                                                   use_list, g.Q, st);
            if (rc != TS_OK) return rc;
            if (ts_k_launch_tile_offsets((const uint32_t *)gr.d_stats.p, (uint32_t)nt, (unsigned long long *)gr.d_off.p, gr.d_tmp.p, st) != 0)
                return c->fail(TS_ERR_HIP, "tile-offset kernel launch failed");
            if (g.timing) HIP_TRY(c, hipEventRecord(c->gen_ev[1], st));
        }
        const auto te0 = Clock::now();
        // (pinned landing: asynchronous for real, then one memcpy into the group's own vector)
        unsigned long long *land = nullptr;
        if (nt && c->pin_off.ensure(std::max<size_t>((nt + 1) * 8 + 64, 1u << 20)) == hipSuccess) land = (unsigned long long *)c->pin_off.p;
        else (void)hipGetLastError();
        uint32_t *flag_land = land ? (uint32_t *)(land + nt + 1) : &flag;
        // (the ENDS walk reads the records in their slots: the dense stream's offsets have no reader on the host)
        if (nt && !g.ends_device) HIP_TRY(c, hipMemcpyAsync(land ? land : tile_off.data(), gr.d_off.p, (nt + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(flag_land, d_flag, 4, hipMemcpyDeviceToHost, st));
        if (g.mode == Mode::Ends) c->terminal_ends_stats[3].fetch_add(4, std::memory_order_relaxed);
        const auto te1 = Clock::now();
        HIP_TRY(c, hipStreamSynchronize(st));
        if (land) { if (!g.ends_device) std::memcpy(tile_off.data(), land, (nt + 1) * 8); flag = *flag_land; }
        if (g.timing) { g.t_dbg[0] += ms_between(t1, te0); g.t_dbg[1] += ms_between(te0, te1); g.t_dbg[2] += ms_between(te1, Clock::now()); }
        if (g.timing) { float ms = 0; if (hipEventElapsedTime(&ms, c->gen_ev[0], c->gen_ev[1]) == hipSuccess) g.t_kern += ms; }
        if (!flag) break;
        const TsGeneralRescan next = ts_general_after_flag(flag, attempt, g.wide, gr.slot_cap, ts_general_slot_max(c, TS_GENERAL_TILE));
        if (next == TsGeneralRescan::Fail)
            return c->fail(TS_ERR_STATE, "general path: a tile overflowed a slot that holds every match it can have");
        if (next == TsGeneralRescan::Strided) { use_list = false; continue; }   // a candidate list spilled: the strided form takes this group
        g.slot_cap_call = gr.slot_cap;
        c->pool.give(std::move(gr.d_slots));
        HIP_TRY(c, c->pool.take(std::max<size_t>(nt, 1) * (size_t)gr.slot_cap * 4, gr.d_slots));
    }
    ++(use_list ? g.n_list : g.n_strided);
    gr.nrec = tile_off[nt];
    g.t_fused += ms_between(t1, Clock::now());
    return TS_OK;
}

// The walks' per-segment table of a group, and per segment the base its tiles' positions are relative to: the group's layout
// holds the regions back to back, so a tile's segment-relative position is not its layout offset minus the segment's —
// ts_k_launch_general_block_inputs writes tiles whose in_off is base + that position instead.
void gen_segment_table(const GenHost &h, std::vector<unsigned long long> &sbase, std::vector<TsShardSegIn> &segtab) {
    const size_t ns = h.G.size();
    sbase.assign(std::max<size_t>(ns, 1), 0ull);
    segtab.resize(ns);
    unsigned long long X = 0;
    for (size_t i = 0; i < ns; ++i) {
        sbase[i] = X;
        segtab[i] = tsplan::whole_segment_entry(X, h.G[i].len, h.G[i].abs_pos, (uint32_t)h.G[i].first_tile, (uint32_t)h.G[i].n_tiles, (uint32_t)i);
        X += h.G[i].len + 64;
    }
}

// ts_terminal_ends of a group on the device: the directory pointed at the slots, the tiles as blockcall.hip addresses them with
// the canonical / forward counts (one kernel makes both: what ts_slot_counts counts for a batch, whose tile list is made once),
// then the terminal walks in their ENDS form (ts_terminal_ends_walk) and 8 bytes per segment to the caller's array.
int gen_ends(GenCall &g, GenGroup &gr) {
    ts_ctx *c = g.c;
    GenHost &h = *gr.gh;
    const size_t ns = h.G.size(), nt = h.tiles.size();
    hipStream_t st = c->scan_stream;
    const auto t0 = Clock::now();
    DevBuf d_bct, d_tab, d_ends;
    struct Return { ts_ctx *c; DevBuf &a, &b2, &d; ~Return() { for (DevBuf *x : {&a, &b2, &d}) c->pool.give(std::move(*x)); } } give_back{c, d_bct, d_tab, d_ends};
    std::vector<unsigned long long> sbase;
    std::vector<TsShardSegIn> segtab;
    gen_segment_table(h, sbase, segtab);
    const size_t off_segs = (sbase.size() * 8 + 63) & ~(size_t)63;
    HIP_TRY(c, c->pool.take(std::max<size_t>(nt, 1) * sizeof(TsTile), d_bct));
    HIP_TRY(c, c->pool.take(off_segs + std::max<size_t>(ns, 1) * sizeof(TsShardSegIn), d_tab));
    HIP_TRY(c, c->pool.take(ns * 8 + 16, d_ends));
    HIP_TRY(c, hipMemcpyAsync(d_tab.p, sbase.data(), sbase.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync((char *)d_tab.p + off_segs, segtab.data(), ns * sizeof(TsShardSegIn), hipMemcpyHostToDevice, st));
    TsBlockCallParams Q = ts_general_walk_params(c, g.gen_lens, g.wide);
    Q.tiles = (const TsTile *)d_bct.p;
    Q.tile_off = (const unsigned long long *)gr.d_off.p;
    Q.tile_stats = (const uint32_t *)gr.d_stats.p;
    Q.matches = (const uint32_t *)gr.d_slots.p;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (g.timing) HIP_TRY(c, hipEventRecord(c->gen_ev[0], st));
        if (ts_k_launch_general_slot_offsets((unsigned long long *)gr.d_off.p, (uint32_t)nt, gr.slot_cap, st) != 0)
            return c->fail(TS_ERR_HIP, "slot-offset kernel launch failed");
        if (ts_k_launch_general_block_inputs((const TsGeneralTile *)gr.d_tiles.p, (const unsigned long long *)gr.d_off.p, (const uint32_t *)gr.d_slots.p,
                                             (const unsigned long long *)d_tab.p, (uint32_t)nt, (TsTile *)d_bct.p, (uint32_t *)gr.d_stats.p, 0, st) != 0)
            return c->fail(TS_ERR_HIP, "general block-input kernel launch failed");
        if (ts_k_launch_terminal_ends_general(&Q, (const TsShardSegIn *)((char *)d_tab.p + off_segs), (uint32_t)ns, (uint32_t)nt, gr.slot_cap,
                                              nullptr, (uint32_t *)d_ends.p, st) != 0)
            return c->fail(TS_ERR_HIP, "general terminal-ends kernel launch failed");
        if (g.timing) HIP_TRY(c, hipEventRecord(c->gen_ev[1], st));
    }
    HIP_TRY(c, hipMemcpyAsync(g.o.ends + 2 * h.first, d_ends.p, ns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));                        // (sbase and segtab are locals)
    c->terminal_ends_stats[1].fetch_add(ns, std::memory_order_relaxed);
    c->terminal_ends_stats[3].fetch_add(ns * 8, std::memory_order_relaxed);
    if (g.timing) { float ms = 0; if (hipEventElapsedTime(&ms, c->gen_ev[0], c->gen_ev[1]) == hipSuccess) g.t_kern += ms; }
    const auto t1 = Clock::now();
    g.t_blk += ms_between(t0, t1);
    g.t_dev += ms_between(gr.t_dev0, t1);
    return TS_OK;
}

// The slots into one dense stream (in push order where it is not position order), then blocks on the device: the tiles as
// blockcall.hip addresses them, the canonical / forward counts, then the walks.
int gen_blocks(GenCall &g, GenGroup &gr) {
    ts_ctx *c = g.c;
    GenHost &h = *gr.gh;
    const size_t ns = h.G.size(), nt = h.tiles.size();
    hipStream_t st = c->scan_stream;
    const auto t0 = Clock::now();
    // blocks only, over a stream in position order: block calling reads the records where the fused pass wrote them (it
    // addresses them through the tile directory), so there is no dense stream to make — every record used to be read and
    // written once more for nothing
    const bool in_place = g.blocks_only && !g.push_compact;
    if (!in_place) HIP_TRY(c, c->pool.take(std::max<uint64_t>(gr.nrec, 1) * 4, gr.d_rec));
    gr.d_records = in_place ? (const uint32_t *)gr.d_slots.p : (const uint32_t *)gr.d_rec.p;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (g.timing) HIP_TRY(c, hipEventRecord(c->gen_ev[0], st));
        if (in_place) {
            if (ts_k_launch_general_slot_offsets((unsigned long long *)gr.d_off.p, (uint32_t)nt, gr.slot_cap, st) != 0)
                return c->fail(TS_ERR_HIP, "slot-offset kernel launch failed");
        } else
        if (g.push_compact) {
            if (ts_k_launch_general_compact_push((const TsGeneralTile *)gr.d_tiles.p, (const uint32_t *)gr.d_stats.p, (unsigned long long *)gr.d_off.p,
                                                 (const uint32_t *)gr.d_slots.p, gr.slot_cap, (uint32_t)nt, (const unsigned long long *)gr.d_tab.p,
                                                 g.P.window_size, g.P.step, g.len_spread, g.wide ? 1 : 0, g.gen_lens, g.wide ? c->wpat.len : nullptr,
                                                 (uint32_t *)gr.d_rec.p, st) != 0)
                return c->fail(TS_ERR_HIP, "general push-order compact kernel launch failed");
            // (records moved across tile borders: the host stage reads the offsets as they are now)
            if (!g.blocks_only) HIP_TRY(c, hipMemcpyAsync(h.tile_off.data(), gr.d_off.p, (nt + 1) * 8, hipMemcpyDeviceToHost, st));
        } else
        if (ts_k_launch_general_compact((const uint32_t *)gr.d_stats.p, (const unsigned long long *)gr.d_off.p, (const uint32_t *)gr.d_slots.p,
                                        gr.slot_cap, (uint32_t)nt, (uint32_t *)gr.d_rec.p, st) != 0)
            return c->fail(TS_ERR_HIP, "general compact kernel launch failed");
        if (g.timing) HIP_TRY(c, hipEventRecord(c->gen_ev[1], st));
    }
    DevBuf d_bct, d_sbase;
    struct Return { ts_ctx *c; DevBuf &a, &b2; ~Return() { c->pool.give(std::move(a)); c->pool.give(std::move(b2)); } } give_back{c, d_bct, d_sbase};
    HIP_TRY(c, c->pool.take(std::max<size_t>(nt, 1) * sizeof(TsTile), d_bct));
    HIP_TRY(c, c->pool.take(std::max<size_t>(ns, 1) * 8, d_sbase));
    std::vector<unsigned long long> sbase;
    std::vector<TsShardSegIn> segtab;
    gen_segment_table(h, sbase, segtab);
    HIP_TRY(c, hipMemcpyAsync(d_sbase.p, sbase.data(), sbase.size() * 8, hipMemcpyHostToDevice, st));
    if (ts_k_launch_general_block_inputs((const TsGeneralTile *)gr.d_tiles.p, (const unsigned long long *)gr.d_off.p, gr.d_records,
                                         (const unsigned long long *)d_sbase.p, (uint32_t)nt, (TsTile *)d_bct.p, (uint32_t *)gr.d_stats.p,
                                         g.push_compact ? 1 : 0, st) != 0)
        return c->fail(TS_ERR_HIP, "general block-input kernel launch failed");
    const int rc = ts_device_block_call_raw(c, (const TsTile *)d_bct.p, (const unsigned long long *)gr.d_off.p, (const uint32_t *)gr.d_stats.p,
                                            gr.d_records, gr.nrec, segtab, nt, g.tips, g.gen_lens, nullptr, nullptr, st, h.blocks, &h.sums, 0,
                                            g.wide ? c->wpat.len : nullptr, g.push_compact);
    g.t_blk += ms_between(t0, Clock::now());
    return rc;
}

// The records (unless the mode reads none) and the window records to the landing area: the context's pinned download
// buffers, alternating by group (the host stage of group g reads its buffer while group g + 1 lands in the other; it has been
// joined before group g + 2 arrives)
int gen_download(GenCall &g, GenGroup &gr) {
    ts_ctx *c = g.c;
    GenHost &h = *gr.gh;
    hipStream_t st = c->scan_stream;
    const auto t0 = Clock::now();
    h.nrecs = g.blocks_only ? 0 : gr.nrec;
    const size_t rec_bytes = ((size_t)h.nrecs * 4 + 255) & ~(size_t)255, win_bytes = (size_t)gr.nwin_total * 32;
    PinBuf &pb = c->pin_down[g.group_no & 1];
    ++g.group_no;
    uint32_t *hrec, *hwin;
    if (rec_bytes + win_bytes + 256 <= (768ull << 20) && pb.ensure(std::max<size_t>(rec_bytes + win_bytes + 256, 32u << 20)) == hipSuccess) {
        hrec = (uint32_t *)pb.p;
        hwin = (uint32_t *)((char *)pb.p + rec_bytes);
    } else {
        (void)hipGetLastError();
        h.recs_heap.resize(h.nrecs + 1);
        h.wins_heap.resize(gr.nwin_total * 8 + 1);
        hrec = h.recs_heap.data();
        hwin = h.wins_heap.data();
    }
    if (h.nrecs) HIP_TRY(c, hipMemcpyAsync(hrec, gr.d_rec.p, h.nrecs * 4, hipMemcpyDeviceToHost, st));
    const bool text = g.mode == Mode::Tracks;                    // the windows leave as text, formatted where they lie
    if (gr.nwin_total && !text) HIP_TRY(c, hipMemcpyAsync(hwin, gr.d_win.p, gr.nwin_total * 32, hipMemcpyDeviceToHost, st));
    h.recs = hrec;
    h.wins = text ? nullptr : hwin;
    HIP_TRY(c, hipStreamSynchronize(st));
    const bool match_text = text && !g.tips && g.o.matches && g.P.out_matches;
    NameBlob nb;
    if (text && !g.tips && (g.o.tracks || match_text)) { const int rc = group_names(c, g.o.names + h.first, h.G.size(), nb); if (rc != TS_OK) return rc; }
    if (text && g.o.tracks && gr.nwin_total) {
        std::vector<ts_track_segment> ts(h.G.size());
        for (size_t i = 0; i < ts.size(); ++i) ts[i] = ts_track_segment{h.G[i].win_base, h.G[i].n_windows, h.G[i].abs_pos, h.G[i].len, 0, 0, 0};
        const int rc = group_tracks(c, (const uint32_t *)gr.d_win.p, gr.nwin_total, ts, nb, st, g.o.tracks);
        if (rc != TS_OK) return rc;
    }
    if (match_text) {
        // the stream block calling read — the slots in place, or the dense stream in push order — behind the directory as the
        // compaction left it (a record moved across a tile border carries its new tile-relative position); the bases in the
        // group's input layout
        if (!g.wide && !g.gen_lens) return c->fail(TS_ERR_UNSUPPORTED, "match lines: a pattern set whose lengths the record format does not carry");
        std::vector<ts_match_line_segment> ms(h.G.size());
        for (size_t i = 0; i < ms.size(); ++i) ms[i] = ts_match_line_segment{0, 0, h.G[i].abs_pos, h.G[i].len, h.G[i].layout_off, 0, 0, 0};
        TsMatchSource src;
        src.form = g.wide ? TS_MATCH_FORM_WIDE : TS_MATCH_FORM_GENERAL;
        src.records = gr.d_records; src.tiles = gr.d_tiles.p;
        src.tile_off = (const unsigned long long *)gr.d_off.p; src.tile_stats = (const uint32_t *)gr.d_stats.p;
        src.n_tiles = h.tiles.size(); src.bases = gr.d_in.p;
        src.gen_lens = g.gen_lens; src.wide_len = g.wide ? c->wpat.len : nullptr;
        const int rc = group_matches(c, src, ms, nb, st, g.o.matches);
        if (rc != TS_OK) return rc;
    }
    if (g.timing) { float ms = 0; if (hipEventElapsedTime(&ms, c->gen_ev[0], c->gen_ev[1]) == hipSuccess) g.t_kern += ms; }
    const auto t1 = Clock::now();
    g.t_d2h += ms_between(t0, t1);
    g.t_dev += ms_between(gr.t_dev0, t1);
    return TS_OK;
}

// The host stage of a group: SegmentData from what landed (ts_assemble_general), then the mode's outputs — Matches: the
// segments; Blocks: the segments and the counts from the device sums; ReadPass: whether a read has a terminal block; Ends:
// the longest terminal block per side.
int gen_host(GenCall &g, const GenHost &h) {
    const size_t ns = h.G.size();
    HostView v;
    v.tips = g.tips;
    v.wins = h.wins; v.recs = h.recs; v.nrecs = h.nrecs;
    v.no_windows = g.mode == Mode::Tracks;
    v.blocks = h.blocks.data(); v.n_blocks = h.blocks.size();
    v.segs.reserve(ns);
    for (const GenSeg &sg : h.G) v.segs.push_back({sg.len, sg.abs_pos, sg.win_base, sg.n_windows, sg.first_tile, sg.n_tiles});
    if (!g.blocks_only) {
        v.tiles.resize(h.tiles.size());
        for (size_t t = 0; t < h.tiles.size(); ++t) v.tiles[t] = {h.tile_off[t], h.tiles[t].seg_rel, (uint32_t)(h.tile_off[t + 1] - h.tile_off[t])};
    }
    const Outputs o = g.o.slice(h.first);
    std::vector<ts_segment_out> tmp(o.out ? 0 : ns);
    ts_segment_out *const out = o.out ? o.out : tmp.data();
    const int rc = ts_assemble_general(g.c, v, out);
    if (rc != TS_OK) return rc;
    for (size_t i = 0; i < ns; ++i) {
        if (o.counts) o.counts[i] = ts_segment_counts{g.tips ? 0 : h.G[i].n_windows, h.sums[5 * i + 2], h.sums[5 * i + 3], h.sums[5 * i + 4]};
        if (o.pass) o.pass[i] = out[i].n_terminal_blocks != 0;
        if (o.ends) reduce_terminal_ends(out[i], h.G[i].len, h.G[i].abs_pos, o.ends + 2 * i);
    }
    if (o.ends) g.c->terminal_ends_stats[2].fetch_add(ns, std::memory_order_relaxed);
    ts_free_segments(tmp.data(), tmp.size());
    return TS_OK;
}

int scan_general(ts_ctx *c, Mode mode, bool tips, const std::vector<Item> &items, Outputs o) {
    if (items.empty()) return TS_OK;
    if (!c->generic_ok)
        return c->fail(TS_ERR_UNSUPPORTED, "unsupported parameter set: a non-ACGT pattern, or more than 63 pattern lengths / a pattern "
                                           "longer than 63 bases (more than a ts_pattern holds)");
    DEVICE_TRY(c);
    { int rc = ensure_streams(c); if (rc != TS_OK) return rc; }
    if (c->knobs.timing && !c->gen_ev[0]) { HIP_TRY(c, hipEventCreate(&c->gen_ev[0])); HIP_TRY(c, hipEventCreate(&c->gen_ev[1])); }
    GenCall g(c, mode, tips, items, o);
    std::unique_ptr<GenGroup> cur(new GenGroup(c)), nxt;
    std::thread pf;                                               // prefetch: plans and uploads the next group
    struct JoinPf { std::thread &t; ~JoinPf() { if (t.joinable()) t.join(); } } join_pf{pf};
    cur->rc = gen_prepare(g, *cur);
    while (cur) {
        if (cur->rc != TS_OK) return cur->rc;
        if (g.next_item < items.size()) {
            nxt.reset(new GenGroup(c));
            GenGroup *np = nxt.get();
            // (an exception on the thread — std::bad_alloc while planning a group — must come back as an error code, not end the process)
            pf = std::thread([&g, c, np] {
                try { c->bind_this_thread(); DeviceGuard g2(c->device); np->rc = gen_prepare(g, *np); }
                catch (const std::exception &e) { np->rc = c->fail(TS_ERR_ALLOC, std::string("general path: planning / upload of a group failed: ") + e.what()); }
            });
        }
        int rc = gen_fused(g, *cur);
        if (rc == TS_OK && g.ends_device) {
            // the group's answer is on the host already: nothing to download, no host stage
            rc = gen_ends(g, *cur);
            if (rc != TS_OK) return rc;
            const auto t_w = Clock::now();
            if (pf.joinable()) pf.join();
            g.t_wait_next += ms_between(t_w, Clock::now());
            cur = std::move(nxt);
            continue;
        }
        if (rc == TS_OK) rc = gen_blocks(g, *cur);
        if (rc == TS_OK) rc = gen_download(g, *cur);
        if (rc != TS_OK) return rc;
        if (g.host_job.joinable()) g.host_job.join();             // (one host stage at a time: it takes all the host threads)
        if (g.host_err.load() != TS_OK) return g.host_err.load();
        g.host_job = std::thread([&g, gh = cur->gh] {
            int rc2;
            const auto t0 = Clock::now();
            try { rc2 = gen_host(g, *gh); }
            catch (...) { rc2 = g.c->fail(TS_ERR_ALLOC, "general path: the host stage ran out of memory"); }
            if (rc2 != TS_OK) { int e = TS_OK; g.host_err.compare_exchange_strong(e, rc2); }
            g.t_host += ms_between(t0, Clock::now());
        });
        const auto t_w = Clock::now();
        if (pf.joinable()) pf.join();
        g.t_wait_next += ms_between(t_w, Clock::now());
        cur = std::move(nxt);
    }
    if (g.host_job.joinable()) g.host_job.join();
    if (g.host_err.load() != TS_OK) return g.host_err.load();
    if (g.timing) {
        fprintf(stderr, "general path: device stage: buffers %.1f ms, fused pass + tile offsets (synced) %.1f ms, compaction + block calling %.1f ms, D2H %.1f ms, waiting for the next group's upload %.1f ms (fused stage: enqueue %.1f, copies enqueue %.1f, sync %.1f)\n",
                g.t_take, g.t_fused, g.t_blk, g.t_d2h, g.t_wait_next, g.t_dbg[0], g.t_dbg[1], g.t_dbg[2]);
        fprintf(stderr, "general path: route: %s form, blocks called on the device, stream %s\n", g.wide ? "wide" : "table",
                g.position_order ? "in position order" : "written in push order by the device");
        fprintf(stderr, "general path: fused pass: %u groups in the list form, %u in the strided form\n", g.n_list, g.n_strided);
        fprintf(stderr, "general path: %zu segments, wall %.1f ms: upload %.1f ms, kernels + D2H %.1f ms (kernels alone, HIP events: %.2f ms), host stage %.1f ms (on a thread of its own, one group behind)\n",
                items.size(), ms_between(g.t_begin, Clock::now()), g.t_up, g.t_dev, (double)g.t_kern, g.t_host);
    }
    return TS_OK;
}

// =========================================================================== routing of the entry points
Item item_of(const ts_segment_in &s) { return Item{s.seq, s.len, s.abs_pos, s.input_format, s.n_pieces}; }

// A call's items of one kind (all full scans or all tips-only) to the tiled pipeline — merged with concurrent callers unless
// the caller holds the context's call lock — or, for parameter sets the tiled kernel does not take, to the general kernels,
// one call at a time (their groups are not merged across callers).  Results to o at the items' indices.
int route(ts_ctx *ctx, Mode mode, bool tips, const std::vector<Item> &items, Outputs o, bool have_lock) {
    if (items.empty()) return TS_OK;
    std::string why;
    if (tips ? ctx->fast_ok : ts_full_scan_supported(ctx, why)) {
        if (mode == Mode::Tracks && !have_lock) {                // (its text is one stream in group order: not merged with other callers)
            std::lock_guard<std::mutex> api(ctx->api_mtx);
            return run_pipeline(ctx, mode, tips, items, o);
        }
        return have_lock ? run_pipeline(ctx, mode, tips, items, o) : submit_pipeline(ctx, mode, tips, items, o);
    }
    // (an exception — std::bad_alloc while a multi-GB group is planned — must leave as an error code: this is a C boundary)
    try {
        if (have_lock) return scan_general(ctx, mode, tips, items, o);
        std::lock_guard<std::mutex> api(ctx->api_mtx);
        return scan_general(ctx, mode, tips, items, o);
    } catch (const std::exception &e) {
        return ctx->fail(TS_ERR_ALLOC, std::string("general path: ") + e.what());
    }
}

// The checks of the segment entry points; every segment's outputs are cleared before its checks.  tips_only: every segment
// must be a tips-only one (ts_terminal_ends).
int check_segments(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, Outputs o, bool tips_only) {
    for (size_t i = 0; i < n_segs; ++i) {
        if (o.out) std::memset(&o.out[i], 0, sizeof o.out[i]);
        if (o.counts) o.counts[i] = ts_segment_counts{0, 0, 0, 0};
        if (o.ends) o.ends[2 * i] = o.ends[2 * i + 1] = 0u;
        if (tips_only && !segs[i].tips_only) return ctx->fail(TS_ERR_INVALID_ARG, "ts_terminal_ends: every segment must be tips_only");
        if (segs[i].len && !segs[i].seq) return ctx->fail(TS_ERR_INVALID_ARG, "null sequence pointer");
        if (segs[i].input_format > TS_INPUT_DEVICE) return ctx->fail(TS_ERR_INVALID_ARG, "unknown input_format");
    }
    return TS_OK;
}

// ts_scan_segments (Matches) and ts_scan_segments_blocks (Blocks): the full scans, then the tips-only scans, each routed on its
// own into arrays of their own and moved to the segments' places.  have_lock: the caller holds the context's call lock
// (ts_scan_segments_multi).
int scan_segments_impl(ts_ctx *ctx, Mode mode, const ts_segment_in *segs, size_t n_segs, Outputs o, bool have_lock) {
    int rc = check_segments(ctx, segs, n_segs, o, false);
    if (rc != TS_OK) return rc;
    for (const bool tips : {false, true}) {
        std::vector<size_t> which;
        for (size_t i = 0; i < n_segs; ++i) if ((segs[i].tips_only != 0) == tips) which.push_back(i);
        std::vector<Item> items(which.size());
        for (size_t i = 0; i < which.size(); ++i) items[i] = item_of(segs[which[i]]);
        std::vector<ts_segment_out> out(which.size());
        std::vector<ts_segment_counts> counts(o.counts ? which.size() : 0);
        std::vector<const char *> names(o.names ? which.size() : 0);
        for (size_t i = 0; i < names.size(); ++i) names[i] = o.names[which[i]];
        rc = route(ctx, mode, tips, items, Outputs{out.data(), o.counts ? counts.data() : nullptr, nullptr, nullptr, tips ? nullptr : o.tracks,
                                                     names.empty() ? nullptr : names.data(), tips ? nullptr : o.matches}, have_lock);
        if (rc != TS_OK) { ts_free_segments(out.data(), out.size()); break; }
        for (size_t i = 0; i < which.size(); ++i) {
            o.out[which[i]] = out[i];
            if (o.counts) o.counts[which[i]] = counts[i];
        }
    }
    if (rc != TS_OK) ts_free_segments(o.out, n_segs);
    return rc;
}

}  // namespace

int ts_scan_segments_unlocked(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, ts_segment_out *out) {
    return scan_segments_impl(ctx, Mode::Matches, segs, n_segs, Outputs{out}, true);
}

// the pieces of the pipeline that ts_scan_segments_multi (multi.cpp) runs per context
int ts_pipeline_ensure_streams(ts_ctx *c) { return ensure_streams(c); }
int ts_pipeline_upload_batch(ts_batch *b, const ts_segment_in *segs, int *slot, bool used[]) {
    std::vector<Item> items(b->segs.size());
    for (size_t i = 0; i < items.size(); ++i) items[i] = item_of(segs[i]);
    return upload_batch(b, items.data(), *slot, used);
}

// ---- ts_batch_call_read_blocks' helpers (the entry points are below, with ts_batch_read_pass)
namespace {

// what the terminal walks of blockcall.hip read of a tiled tips batch (device_block_call's view, capi.cpp)
TsBlockCallParams tiled_walk_params(const ts_batch *b) {
    const ts_ctx *c = b->ctx;
    const ts_params &P = c->params;
    TsBlockCallParams Q{};
    Q.tiles = (const TsTile *)b->d_tiles.p;
    Q.tile_off = (const unsigned long long *)b->d_tile_off.p;
    Q.tile_stats = b->stats_ptr();
    Q.matches = b->records_ptr();
    Q.terminal_limit = P.terminal_limit; Q.max_match_dist = P.max_match_dist;
    Q.min_block_len = P.min_block_len; Q.max_block_dist = P.max_block_dist;
    Q.min_block_counts = P.min_block_counts; Q.min_block_density = P.min_block_density;
    Q.k = c->k;
    Q.rec16 = b->records16() ? 1u : 0u;
    return Q;
}

// the rows' room: what the batch held before, or a few blocks per read to begin with
int ensure_read_block_rows(ts_batch *b, uint64_t rows) {
    ts_ctx *c = b->ctx;
    ReadBlocksState &R = b->rb;
    if (R.d_rows.p && R.row_cap >= rows) return TS_OK;
    c->pool.give(std::move(R.d_rows));
    R.row_cap = 0;
    HIP_TRY(c, c->pool.take((size_t)rows * sizeof(TsReadBlockRow), R.d_rows));
    R.row_cap = rows;
    return TS_OK;
}

}  // namespace

int ts_batch_settle_read_blocks(ts_batch *b, uint64_t *n_rows) {
    ts_ctx *c = b->ctx;
    ReadBlocksState &R = b->rb;
    *n_rows = 0;
    if (!R.called) return c->fail(TS_ERR_STATE, "the batch's read blocks were not called since its last scan (ts_batch_call_read_blocks)");
    if (!R.clean) return c->fail(TS_ERR_STATE, "the batch's read blocks: ts_batch_read_pass_status has not said since the call that nothing overflowed");
    const size_t ns = b->segs.size();
    if (!ns) return TS_OK;
    hipStream_t st = (hipStream_t)R.stream;
    const ReadBlocksTab T(ns);
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, (char *)R.d_tab.p + T.first + ns * 8, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (total > R.row_cap) {
        { const int rc = ensure_read_block_rows(b, total + total / 4); if (rc != TS_OK) return rc; }
        if (b->gen) { const int rc = ts_general_batch_place_read_blocks(b); if (rc != TS_OK) return rc; }
        else {
            const TsBlockCallParams Q = tiled_walk_params(b);
            const uint32_t *const flag = b->dense ? nullptr : (const uint32_t *)((char *)b->d_readtab.p + ReadTab(ns).flag);
            if (ts_k_launch_read_blocks_place(&Q, (const TsShardSegIn *)R.d_segin.p, (uint32_t)ns, flag,
                                              (const unsigned long long *)((char *)R.d_tab.p + T.places), (TsReadBlockRow *)R.d_rows.p,
                                              R.row_cap, R.stream) != 0)
                return c->fail(TS_ERR_HIP, "read-block kernel launch failed");
        }
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    *n_rows = total;
    return TS_OK;
}

// =========================================================================== scanSegment, batched
extern "C" {

int ts_scan_segments(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, ts_segment_out *out) {
    if (!ctx || (n_segs && (!segs || !out))) return TS_ERR_INVALID_ARG;
    return scan_segments_impl(ctx, Mode::Matches, segs, n_segs, Outputs{out}, false);
}

// scanSegment for callers that do not read the match vectors: scan, block calling and the per-segment
// counts all stay on the device; windows, blocks and four counters per segment cross PCIe.
int ts_scan_segments_blocks(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, ts_segment_out *out,
                            ts_segment_counts *counts) {
    if (!ctx || (n_segs && (!segs || !out))) return TS_ERR_INVALID_ARG;
    return scan_segments_impl(ctx, Mode::Blocks, segs, n_segs, Outputs{out, counts}, false);
}

// ts_scan_segments_blocks without the window records: every group's window lines are formatted on the device (tracks.hip) and
// appended to `tracks` instead; see include/teloscan.h.
int ts_scan_segments_tracks(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, const char *const *names, ts_segment_out *out,
                            ts_segment_counts *counts, ts_track_text *tracks) {
    if (!ctx || !tracks || (n_segs && (!segs || !out || !names))) return TS_ERR_INVALID_ARG;
    ts_track_text_begin(ctx, tracks);
    for (size_t i = 0; i < n_segs; ++i)
        if (!names[i]) return ctx->fail(TS_ERR_INVALID_ARG, "ts_scan_segments_tracks: null name");
    if (ctx->device == kNoDevice) return ctx->fail(TS_ERR_NO_DEVICE, "planning-only context: no HIP device behind it");
    Outputs o{out, counts};
    o.tracks = tracks; o.names = names;
    int rc = scan_segments_impl(ctx, Mode::Tracks, segs, n_segs, o, false);
    if (rc == TS_OK) {                                           // (a call without a full-scan segment: the tracks exist, empty)
        DeviceGuard g(ctx->device);
        rc = ts_tracks_append(ctx, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, tracks);
        if (rc != TS_OK) ts_free_segments(out, n_segs);
    }
    if (rc != TS_OK) ts_free_track_text(tracks);
    return rc;
}

// ts_scan_segments_tracks plus the match lines: every group's match records are formatted where they lie (match_text.hip), from
// the group's input buffer, and appended to `matches`; see include/teloscan.h.
int ts_scan_segments_text(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, const char *const *names, ts_segment_out *out,
                          ts_segment_counts *counts, ts_track_text *tracks, ts_match_text *matches) {
    if (!ctx || (!tracks && !matches) || (n_segs && (!segs || !out || !names))) return TS_ERR_INVALID_ARG;
    if (tracks) ts_track_text_begin(ctx, tracks);
    if (matches) ts_match_text_begin(ctx, matches);
    auto fail = [&](int rc) {
        if (tracks) ts_free_track_text(tracks);
        if (matches) ts_free_match_text(matches);
        return rc;
    };
    for (size_t i = 0; i < n_segs; ++i)
        if (!names[i]) return fail(ctx->fail(TS_ERR_INVALID_ARG, "ts_scan_segments_text: null name"));
    if (ctx->device == kNoDevice) return fail(ctx->fail(TS_ERR_NO_DEVICE, "planning-only context: no HIP device behind it"));
    Outputs o{out, counts};
    o.tracks = tracks; o.names = names; o.matches = matches;
    int rc = scan_segments_impl(ctx, Mode::Tracks, segs, n_segs, o, false);
    if (rc == TS_OK) {                                           // (a call without a full-scan segment: the texts exist, empty)
        DeviceGuard g(ctx->device);
        if (tracks) rc = ts_tracks_append(ctx, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, tracks);
        if (rc == TS_OK && matches) rc = ts_matches_append(ctx, TsMatchSource{}, nullptr, 0, nullptr, 0, nullptr, matches);
        if (rc != TS_OK) ts_free_segments(out, n_segs);
    }
    return rc == TS_OK ? rc : fail(rc);
}

// =========================================================================== ReadTelomereFilter
// Whole-read tips-only scans.  Tiled sets: the terminal-block predicate on the device, one byte per read back.  Other sets
// (mixed lengths, k > 8): the general kernels' blocks; a read passes with a terminal block.
int ts_filter_reads(ts_ctx *ctx, const char *const *seqs, const uint64_t *lens, size_t n_reads,
                    uint8_t *pass) {
    if (!ctx || (n_reads && (!seqs || !lens || !pass))) return TS_ERR_INVALID_ARG;
    if (!ctx->read_filter) return ctx->fail(TS_ERR_STATE, "context was not made by ts_create_read_filter");
    if (n_reads == 0) return TS_OK;
    std::vector<Item> items(n_reads);
    for (size_t i = 0; i < n_reads; ++i) {
        uint64_t n = lens[i];
        if (n && !seqs[i]) return ctx->fail(TS_ERR_INVALID_ARG, "null sequence pointer");
        if (n && seqs[i][n - 1] == '\r') --n;             // src/read-filter.cpp:38-40
        items[i] = Item{seqs[i], n, 0, TS_INPUT_BASES, 0};
    }
    return route(ctx, Mode::ReadPass, true, items, Outputs{nullptr, nullptr, pass}, false);
}

// =========================================================================== GFA annotation: per-end terminal lengths
// ends[2i] / ends[2i+1]: the longest terminal block at the start / end side of segs[i] (walkSegment's rule,
// src/input.cpp:835-881).  Tiled sets: a tips-only batch, the scan, the predicate's walks in their ENDS form
// (predicate.hip) and 8 bytes per segment back.  Other sets: the general kernels' fused pass per group, then the terminal walks of
// device block calling in their ENDS form over the records in their slots (blockcall.hip: ts_terminal_ends_walk) and the same 8
// bytes per segment back; the blocks route (called on the device, reduced on the host) remains behind it.
int ts_terminal_ends(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, uint32_t *ends) {
    if (!ctx || (n_segs && (!segs || !ends))) return TS_ERR_INVALID_ARG;
    const Outputs o{nullptr, nullptr, nullptr, ends};
    const int rc = check_segments(ctx, segs, n_segs, o, true);
    if (rc != TS_OK) return rc;
    std::vector<Item> items(n_segs);
    for (size_t i = 0; i < n_segs; ++i) items[i] = item_of(segs[i]);
    return route(ctx, Mode::Ends, true, items, o, false);
}

// ReadTelomereFilter::matches over a device-resident tips-only batch (reads already in HBM, scanned on `stream`):
// the pass byte of every read to d_pass, asynchronously on the same stream.
int ts_batch_read_pass(ts_batch *b, void *d_pass, void *stream) {
    if (!b || !d_pass) return TS_ERR_INVALID_ARG;
    if (b->gen) return ts_general_batch_read_pass(b, d_pass, stream);
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    if (!b->tips || !b->whole() || !b->scanned) return c->fail(TS_ERR_STATE, "ts_batch_read_pass needs a scanned, unrestricted tips-only batch");
    return batch_read_pass_device(b, (unsigned char *)d_pass, (hipStream_t)stream);
}

// walkSegment's per-side maxima over a device-resident tips-only batch: two u32 per segment to d_ends (device), asynchronously.
// A tiled batch: the predicate's walks in their ENDS form, as ts_terminal_ends runs them per group; a general tips batch: the
// terminal walks of device block calling in theirs.
int ts_batch_terminal_ends(ts_batch *b, void *d_ends, void *stream) {
    if (!b || !d_ends) return TS_ERR_INVALID_ARG;
    ts_ctx *c = b->ctx;
    if (!b->tips) return c->fail(TS_ERR_INVALID_ARG, "ts_batch_terminal_ends needs a tips-only batch");
    if (b->gen) return ts_general_batch_terminal_ends(b, d_ends, stream);
    DEVICE_TRY(c);
    if (!b->whole() || !b->scanned) return c->fail(TS_ERR_STATE, "ts_batch_terminal_ends needs a scanned, unrestricted tips-only batch");
    const int rc = batch_read_pass_device(b, nullptr, (hipStream_t)stream, (uint32_t *)d_ends);
    if (rc == TS_OK) c->terminal_ends_stats[0].fetch_add(b->segs.size(), std::memory_order_relaxed);
    return rc;
}

// The terminal blocks of a device-resident tips-only batch as ordered rows in its own device memory (blockcall.hip's walks in
// their counting and placing forms); asynchronous.  A tiled batch here, a general tips batch in general_batch.cpp.
int ts_batch_call_read_blocks(ts_batch *b, void *stream) {
    if (!b) return TS_ERR_INVALID_ARG;
    ts_ctx *c = b->ctx;
    if (!b->tips) return c->fail(TS_ERR_INVALID_ARG, "ts_batch_call_read_blocks needs a tips-only batch");
    DEVICE_TRY(c);
    ReadBlocksState &R = b->rb;
    const size_t ns = b->segs.size();
    if (ns >= 0x3FFFFFFFull) return c->fail(TS_ERR_UNSUPPORTED, "ts_batch_call_read_blocks: too many segments in one batch");
    if (!b->scanned || (!b->gen && !b->whole())) return c->fail(TS_ERR_STATE, "ts_batch_call_read_blocks needs a scanned, unrestricted tips-only batch");
    if (b->gen && stream != b->last_stream) return c->fail(TS_ERR_STATE, "ts_batch_call_read_blocks on a general tips batch: pass the stream of its scan");
    R.called = R.clean = false;
    if (!R.d_tab.p) HIP_TRY(c, c->pool.take(ReadBlocksTab(ns).bytes, R.d_tab));
    { const int rc = ensure_read_block_rows(b, std::max<uint64_t>(R.row_cap, 2 * (uint64_t)ns + 1024)); if (rc != TS_OK) return rc; }
    if (b->gen) return ts_general_batch_call_read_blocks(b, stream);
    if (!ns) { R.called = true; R.stream = stream; return TS_OK; }
    hipStream_t st = (hipStream_t)stream;
    { const int rc = ensure_readtab(b, st); if (rc != TS_OK) return rc; }
    if (!R.d_segin.p) {
        std::vector<TsShardSegIn> tab(ns);
        for (size_t i = 0; i < ns; ++i) {
            const SegPlan &sp = b->segs[i];
            tab[i] = tsplan::whole_segment_entry(sp.in_off, sp.len, sp.abs_pos, sp.first_tile, sp.n_tiles, (uint32_t)i);
        }
        HIP_TRY(c, c->pool.take(ns * sizeof(TsShardSegIn), R.d_segin));
        HIP_TRY(c, hipMemcpyAsync(R.d_segin.p, tab.data(), ns * sizeof(TsShardSegIn), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));                    // (tab is a local)
    }
    const TsBlockCallParams Q = tiled_walk_params(b);
    const ReadBlocksTab T(ns);
    char *const dt = (char *)R.d_tab.p;
    uint32_t *const flag = (uint32_t *)((char *)b->d_readtab.p + ReadTab(ns).flag);
    if (ts_k_launch_read_blocks(&Q, (const TsShardSegIn *)R.d_segin.p, (uint32_t)ns, (uint32_t)b->tiles.size(), 0u, nullptr,
                                b->dense ? nullptr : (const uint32_t *)b->d_fill.p, b->region_cap, b->total_waves, flag, (uint32_t *)dt,
                                (unsigned long long *)(dt + T.places), (unsigned long long *)(dt + T.first), dt + T.tmp,
                                (TsReadBlockRow *)R.d_rows.p, R.row_cap, stream) != 0)
        return c->fail(TS_ERR_HIP, "read-block kernel launch failed");
    R.called = true; R.stream = stream;
    return TS_OK;
}

int ts_batch_read_blocks(ts_batch *b, ts_read_block *out, uint64_t cap, uint64_t *n) {
    if (!b || !n || (cap && !out)) return TS_ERR_INVALID_ARG;
    ts_ctx *c = b->ctx;
    static_assert(sizeof(ts_read_block) == sizeof(TsReadBlockRow) && offsetof(ts_read_block, block) == offsetof(TsReadBlockRow, start) &&
                  offsetof(ts_block, block_label) + offsetof(ts_read_block, block) == offsetof(TsReadBlockRow, block_label),
                  "a TsReadBlockRow is a ts_read_block");
    DEVICE_TRY(c);
    { const int rc = ts_batch_settle_read_blocks(b, n); if (rc != TS_OK) return rc; }
    if (*n > cap) return c->fail(TS_ERR_INVALID_ARG, "ts_batch_read_blocks: out is too small (*n says what is needed)");
    if (*n) HIP_TRY(c, hipMemcpy(out, b->rb.d_rows.p, (size_t)*n * sizeof(ts_read_block), hipMemcpyDeviceToHost));
    return TS_OK;
}

int ts_batch_read_pass_status(ts_batch *b, int *overflowed) {
    if (!b || !overflowed) return TS_ERR_INVALID_ARG;
    if (b->gen) {
        const int rc = ts_general_batch_status(b, overflowed);
        if (rc == TS_OK && !*overflowed) b->rb.clean = true;     // (rows called since the scan may be read)
        return rc;
    }
    ts_ctx *c = b->ctx;
    DEVICE_TRY(c);
    *overflowed = 0;
    if (!b->d_readtab.p) return TS_OK;                            // no pass was ever enqueued
    char *const flag_at = (char *)b->d_readtab.p + ReadTab(b->segs.size()).flag;
    uint32_t flag = 0;
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(&flag, flag_at, 4, hipMemcpyDeviceToHost));
    if (flag) HIP_TRY(c, hipMemset(flag_at, 0, 4));
    *overflowed = flag ? 1 : 0;
    if (!flag) b->rb.clean = true;                                // (rows called since the scan may be read)
    return TS_OK;
}

int ts_filter_reads_multi(ts_ctx *const *ctxs, size_t n_ctx, const char *const *seqs, const uint64_t *lens,
                          size_t n_reads, uint8_t *pass) {
    if (!ctxs || !n_ctx || (n_reads && (!seqs || !lens || !pass))) return TS_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_ctx; ++i) if (!ctxs[i]) return TS_ERR_INVALID_ARG;
    if (n_ctx == 1 || n_reads < 2 * n_ctx) return ts_filter_reads(ctxs[0], seqs, lens, n_reads, pass);
    // consecutive shards of equal bases: shard d ends at the first read where the running total reaches
    // (d + 1) / n_ctx of all bases; pass[] is written in place, so the result is in input order by construction
    uint64_t total = 0;
    for (size_t i = 0; i < n_reads; ++i) total += lens[i];
    std::vector<size_t> cut(n_ctx + 1, n_reads);
    cut[0] = 0;
    {
        uint64_t acc = 0;
        size_t d = 1;
        for (size_t i = 0; i < n_reads && d < n_ctx; ++i) {
            acc += lens[i];
            while (d < n_ctx && (unsigned __int128)acc * n_ctx >= (unsigned __int128)total * d) cut[d++] = i + 1;
        }
    }
    std::vector<int> rcs(n_ctx, TS_OK);
    std::vector<std::thread> pool;
    for (size_t d = 0; d < n_ctx; ++d)
        pool.emplace_back([&, d] {
            const size_t a = cut[d], z = cut[d + 1];
            if (z > a) rcs[d] = ts_filter_reads(ctxs[d], seqs + a, lens + a, z - a, pass + a);
        });
    for (std::thread &th : pool) th.join();
    for (size_t d = 0; d < n_ctx; ++d)
        if (rcs[d] != TS_OK) {
            if (d != 0) ctxs[0]->fail(rcs[d], std::string("shard on context ") + std::to_string(d) + ": " + ts_last_error(ctxs[d]));
            return rcs[d];
        }
    return TS_OK;
}

}  // extern "C"
