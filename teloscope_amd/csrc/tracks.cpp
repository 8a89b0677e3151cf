// tracks.cpp — host side of the device track formatter (tracks.hip): ts_window_tracks_format, ts_free_track_text and
// ts_tracks_append, the step ts_scan_segments_tracks (pipeline.cpp) runs per group in place of the download of window records.
//
// Per call: the segments that have windows, their names, and the entropy patch list go up; ts_track_count says how many bytes
// every track takes (and whether a value cannot be printed: the call then fails, nothing is written); ts_track_write formats
// into one device block; one copy per track appends it to the caller's text.  Windows go through in slices of kSliceWindows, so
// that the device block stays a few hundred MB whatever the window size.
//
// Entropy without a device logarithm: a window of the full size takes its terms from the context's entropy_term table (uploaded
// once per context); every other window — the trailing windows of a segment, or all of them when the window is too long for a
// table — gets the host's ts::shannon_entropy_memo of its record, as float bits in a sorted patch list.  The host has the
// records at hand (ts_window_tracks_format) or picks the few it needs off the device (ts_track_pick).
#include "text_out.hpp"
#include "track_format_core.h"

#include <cstdio>

static_assert(sizeof(ts_track_segment) == sizeof(tstrack::Segment) && offsetof(ts_track_segment, name_len) == offsetof(tstrack::Segment, name_len) &&
              offsetof(ts_track_segment, abs_pos) == offsetof(tstrack::Segment, abs_pos), "ts_track_segment is tstrack::Segment");
static_assert(TS_N_TRACKS == tstrack::kTracks, "five tracks");

namespace {

constexpr uint64_t kSliceWindows = 1ull << 21;

uint32_t track_mask(const ts_params &P) {
    return (P.out_win_repeats ? 7u : 0u) | (P.out_gc ? 1u << tstrack::GC : 0u) | (P.out_entropy ? 1u << tstrack::ENTROPY : 0u);
}

}  // namespace

int ts_tracks_append(ts_ctx *c, const uint32_t *d_records, const uint32_t *h_records, uint64_t n_records, const ts_track_segment *segs_in,
                     size_t n_segs_in, const char *names, uint64_t names_len, hipStream_t st, ts_track_text *out) {
    const ts_params &P = c->params;
    const uint32_t mask = track_mask(P), w = P.window_size, step = P.step;
    const TextFiles files = text_files(out);
    for (int t = 0; t < TS_N_TRACKS; ++t)
        if ((mask >> t & 1u) && !files.grow(t, 0)) return c->fail(TS_ERR_ALLOC, "out of host memory");
    if (!mask || !n_records || !n_segs_in) return TS_OK;
    if (!w || !step) return c->fail(TS_ERR_INVALID_ARG, "window tracks: the context has no window size or step");

    // the segments that have windows, checked: ascending, inside the record array, every window inside its segment
    std::vector<tstrack::Segment> segs;
    uint64_t next = 0, lines = 0;
    for (size_t i = 0; i < n_segs_in; ++i) {
        const ts_track_segment &s = segs_in[i];
        if (!s.n_windows) continue;
        if (s.first_window < next || s.first_window > n_records || s.n_windows > n_records - s.first_window)
            return c->fail(TS_ERR_INVALID_ARG, "window tracks: segment " + std::to_string(i) + ": its windows overlap the previous segment's or exceed the records");
        if ((unsigned __int128)(s.n_windows - 1) * step >= s.len)
            return c->fail(TS_ERR_INVALID_ARG, "window tracks: segment " + std::to_string(i) + ": more windows than its length holds");
        const int rc = text_check_segment(c, "window tracks", i, s.name_off, s.name_len, names_len, s.abs_pos, s.len);
        if (rc != TS_OK) return rc;
        segs.push_back(tstrack::Segment{s.first_window, s.n_windows, s.abs_pos, s.len, s.name_off, s.name_len, 0u});
        next = s.first_window + s.n_windows;
        lines += s.n_windows;
    }
    if (segs.empty()) return TS_OK;
    if (segs.size() > 0xFFFFFFFFull) return c->fail(TS_ERR_UNSUPPORTED, "window tracks: more than 2^32 segments in one call");

    std::lock_guard<std::mutex> lock(c->track_mtx);
    const auto t_begin = std::chrono::steady_clock::now();
    struct { DevBuf segs, names, idx, picked, patches, sums, text; } D;
    PoolReturn give_back{c, {&D.segs, &D.names, &D.idx, &D.picked, &D.patches, &D.sums, &D.text}};
    const bool table = P.out_entropy && c->entropy_term.size() == (size_t)w + 1;
    if (table && !c->d_entropy_term.p) {
        HIP_TRY(c, c->d_entropy_term.ensure(c->entropy_term.size() * 4));
        const hipError_t e = hipMemcpy(c->d_entropy_term.p, c->entropy_term.data(), c->entropy_term.size() * 4, hipMemcpyHostToDevice);
        // (synchronous, once per context: calls come on different streams, and the table counts as present from here on)
        if (e != hipSuccess) { c->d_entropy_term.release(); return c->fail(TS_ERR_HIP, std::string("window tracks: upload of the entropy terms: ") + hipGetErrorString(e)); }
    }

    // the patch list: the windows whose entropy the host evaluates
    std::vector<tstrack::Patch> patches;
    if (P.out_entropy) {
        std::vector<unsigned long long> idx;
        for (const tstrack::Segment &s : segs) {
            const uint64_t full = !table ? 0 : s.len >= w ? std::min<uint64_t>(s.n_windows, (s.len - w) / step + 1) : 0;
            for (uint64_t k = full; k < s.n_windows; ++k) idx.push_back(s.first_window + k);
        }
        std::vector<uint32_t> picked;
        const uint32_t *rec = h_records;
        if (!idx.empty() && !h_records) {
            picked.resize(idx.size() * 8);
            HIP_TRY(c, c->pool.take(idx.size() * 8, D.idx));
            HIP_TRY(c, c->pool.take(idx.size() * 32, D.picked));
            HIP_TRY(c, hipMemcpyAsync(D.idx.p, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, st));
            if (ts_k_launch_track_pick(d_records, (const unsigned long long *)D.idx.p, idx.size(), (uint32_t *)D.picked.p, st) != 0)
                return c->fail(TS_ERR_HIP, "window tracks: record pick launch failed");
            HIP_TRY(c, hipMemcpyAsync(picked.data(), D.picked.p, idx.size() * 32, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
        }
        patches.resize(idx.size());
        size_t j = 0;
        for (const tstrack::Segment &s : segs) {
            for (; j < idx.size() && idx[j] < s.first_window + s.n_windows; ++j) {
                const uint32_t *r = h_records ? rec + idx[j] * 8 : picked.data() + j * 8;
                const uint32_t size = tstrack::window_size(s, idx[j] - s.first_window, w, step);
                const float e = ts::shannon_entropy_memo(r, size, c->entropy_term);
                patches[j] = tstrack::Patch{idx[j], tstrack::float_bits(e), 0u};
            }
        }
    }

    HIP_TRY(c, c->pool.take(segs.size() * sizeof(tstrack::Segment), D.segs));
    HIP_TRY(c, c->pool.take(names_len + 16, D.names));
    HIP_TRY(c, hipMemcpyAsync(D.segs.p, segs.data(), segs.size() * sizeof(tstrack::Segment), hipMemcpyHostToDevice, st));
    if (names_len) HIP_TRY(c, hipMemcpyAsync(D.names.p, names, names_len, hipMemcpyHostToDevice, st));
    if (!patches.empty()) {
        HIP_TRY(c, c->pool.take(patches.size() * sizeof(tstrack::Patch), D.patches));
        HIP_TRY(c, hipMemcpyAsync(D.patches.p, patches.data(), patches.size() * sizeof(tstrack::Patch), hipMemcpyHostToDevice, st));
    }
    const uint64_t first = segs.front().first_window, last = segs.back().first_window + segs.back().n_windows;
    const uint32_t max_blocks = (uint32_t)ceil_div(kSliceWindows, TS_TRACK_BLOCK);
    const size_t sums_bytes = (size_t)TS_N_TRACKS * (max_blocks + 1) * 8;
    HIP_TRY(c, c->pool.take(sums_bytes + 8, D.sums));
    unsigned long long *const d_bad = (unsigned long long *)((char *)D.sums.p + sums_bytes);

    double ms_count = 0;
    TextTimes ms;
    for (uint64_t a = first; a < last; a += kSliceWindows) {
        const uint64_t z = std::min(last, a + kSliceWindows);
        auto t0 = std::chrono::steady_clock::now();
        TsTrackParams K{};
        K.records = d_records; K.first = a; K.n = z;
        K.segs = D.segs.p; K.names = D.names.p;
        K.term = table ? (const float *)c->d_entropy_term.p : nullptr;
        K.patches = D.patches.p; K.n_patches = patches.size();
        K.block_sums = (unsigned long long *)D.sums.p; K.bad_window = d_bad;
        K.n_segs = (uint32_t)segs.size(); K.n_blocks = (uint32_t)ceil_div(z - a, TS_TRACK_BLOCK);
        K.w = w; K.step = step; K.on_mask = mask;
        HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
        if (ts_k_launch_track_count(&K, st) != 0) return c->fail(TS_ERR_HIP, "window tracks: count launch failed");
        unsigned long long total[TS_N_TRACKS] = {0, 0, 0, 0, 0}, bad = 0;
        for (int t = 0; t < TS_N_TRACKS; ++t)
            HIP_TRY(c, hipMemcpyAsync(&total[t], K.block_sums + (size_t)t * (K.n_blocks + 1) + K.n_blocks, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        ms_count += ms_since(t0);
        if (bad != ~0ull) {
            const tstrack::Segment &s = segs[tstrack::find_segment(segs.data(), (uint32_t)segs.size(), bad)];
            return c->fail(TS_ERR_UNSUPPORTED, "window tracks: window " + std::to_string(bad) + " (window " + std::to_string(bad - s.first_window) + " of '" +
                                                   std::string(names + s.name_off, s.name_len) +
                                                   "'): a column value lies outside what the device formatter prints (0, -1, 2^-32 .. 128), or a count exceeds the window");
        }
        const int rc = text_slice_out(c, "window tracks", st, D.text, files, total, K.out, ms, [&] { return ts_k_launch_track_write(&K, st); });
        if (rc != TS_OK) return rc;
    }
    out->n_lines += lines;
    if (c->knobs.timing)
        fprintf(stderr, "window tracks: %llu windows of %zu segments, %zu patched, %.1f ms (tables up + count %.1f ms, write kernel %.1f ms, text D2H %.1f ms)\n",
                (unsigned long long)lines, segs.size(), patches.size(), ms_since(t_begin), ms_count, ms.write, ms.copy);
    return TS_OK;
}

// A caller's struct at the start of a call (TextFiles::begin); a track this context does not have is freed.
void ts_track_text_begin(const ts_ctx *c, ts_track_text *t) {
    text_files(t).begin(track_mask(c->params));
    t->n_lines = 0;
}

extern "C" {

int ts_window_tracks_format(ts_ctx *ctx, const uint32_t *records, uint64_t n, const ts_track_segment *segs, size_t n_segs, const char *names,
                            uint64_t names_len, ts_track_text *out) {
    if (!ctx || !out || (n && !records) || (n_segs && !segs) || (names_len && !names)) return TS_ERR_INVALID_ARG;
    ts_ctx *c = ctx;
    ts_track_text_begin(c, out);
    DEVICE_TRY(c);
    int rc = ts_pipeline_ensure_streams(c);
    if (rc != TS_OK) return rc;
    hipStream_t st = c->down_stream;
    DevBuf d_rec;
    PoolReturn give_back{c, {&d_rec}};
    if (n) {
        std::lock_guard<std::mutex> dl(c->down_mtx);
        HIP_TRY(c, c->pool.take(n * 32, d_rec));
        HIP_TRY(c, hipMemcpyAsync(d_rec.p, records, n * 32, hipMemcpyHostToDevice, st));
        rc = ts_tracks_append(c, (const uint32_t *)d_rec.p, records, n, segs, n_segs, names, names_len, st, out);
        (void)hipStreamSynchronize(st);
    } else {
        rc = ts_tracks_append(c, nullptr, nullptr, 0, segs, n_segs, names, names_len, st, out);
    }
    if (rc != TS_OK) ts_free_track_text(out);
    return rc;
}

void ts_free_track_text(ts_track_text *t) {
    if (!t) return;
    text_files(t).free_all();
    t->n_lines = 0;
}

}  // extern "C"
