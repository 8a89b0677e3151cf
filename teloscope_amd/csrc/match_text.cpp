// match_text.cpp — host side of the device match-line formatter (match_text.hip): ts_match_lines_format, ts_free_match_text,
// ts_match_text_stats and ts_matches_append, the step ts_scan_segments_text (pipeline.cpp) runs per group in place of the
// download of the match records and of the bases matchSeq is cut from.
//
// Per call: the segment table and the names go up; ts_match_count says how many bytes and lines every tile of the record
// stream's directory contributes to each of the two files, a prefix sum places them; ts_match_write formats into one device
// block per file; one copy per file appends it to the caller's text.  When the two files together exceed the slice limit
// (256 MB; TS_MATCH_SLICE_BYTES) the byte columns of the prefix sums come down and the tiles go through in runs that stay
// below it, so that the device block stays bounded whatever the group holds.
#include "text_out.hpp"
#include "match_format_core.h"

#include <cstdio>

static_assert(sizeof(ts_match_line_segment) == sizeof(tsmatch::Segment) && offsetof(ts_match_line_segment, name_len) == offsetof(tsmatch::Segment, name_len) &&
              offsetof(ts_match_line_segment, base_off) == offsetof(tsmatch::Segment, base_off) &&
              offsetof(ts_match_line_segment, tips_only) == offsetof(tsmatch::Segment, tips_only), "ts_match_line_segment is tsmatch::Segment");
static_assert(TS_N_MATCH_FILES == tsmatch::kFiles, "two match files");
static_assert(sizeof(ts_match) == 16 && offsetof(ts_match, match_size) == 8 && offsetof(ts_match, flags) == 10 && TS_MATCH_CANONICAL == 2,
              "tsmatch::decode_match reads a ts_match as {position; match_size | flags << 16}");

namespace {

constexpr uint32_t kArrayTile = 512;                // records per pseudo-tile of a ts_match array

}  // namespace

int ts_matches_append(ts_ctx *c, const TsMatchSource &src, const ts_match_line_segment *segs, size_t n_segs, const char *names,
                      uint64_t names_len, hipStream_t st, ts_match_text *out) {
    const ts_params &P = c->params;
    if (!P.out_matches) return TS_OK;
    const TextFiles files = text_files(out);
    for (int f = 0; f < TS_N_MATCH_FILES; ++f)
        if (!files.grow(f, 0)) return c->fail(TS_ERR_ALLOC, "out of host memory");
    if (!src.n_tiles || !n_segs) return TS_OK;
    if (src.n_tiles >= 0x7FFFFFFFull || n_segs > 0xFFFFFFFFull) return c->fail(TS_ERR_UNSUPPORTED, "match lines: too many tiles or segments in one call");
    for (size_t i = 0; i < n_segs; ++i) {
        const ts_match_line_segment &s = segs[i];
        const int rc = text_check_segment(c, "match lines", i, s.name_off, s.name_len, names_len, s.abs_pos, s.len);
        if (rc != TS_OK) return rc;
    }

    std::lock_guard<std::mutex> lock(c->track_mtx);
    const auto t_begin = std::chrono::steady_clock::now();
    struct { DevBuf segs, names, sums, text; } D;
    PoolReturn give_back{c, {&D.segs, &D.names, &D.sums, &D.text}};
    const uint32_t nt = (uint32_t)src.n_tiles;
    const size_t col = (size_t)nt + 1;
    HIP_TRY(c, c->pool.take(n_segs * sizeof(tsmatch::Segment), D.segs));
    HIP_TRY(c, c->pool.take(names_len + 16, D.names));
    HIP_TRY(c, c->pool.take(4 * col * 8, D.sums));
    HIP_TRY(c, hipMemcpyAsync(D.segs.p, segs, n_segs * sizeof(tsmatch::Segment), hipMemcpyHostToDevice, st));
    if (names_len) HIP_TRY(c, hipMemcpyAsync(D.names.p, names, names_len, hipMemcpyHostToDevice, st));

    TsMatchTextParams K{};
    K.records = src.records; K.tiles = src.tiles; K.tile_off = src.tile_off; K.tile_stats = src.tile_stats;
    K.segs = D.segs.p; K.names = D.names.p; K.bases = src.bases;
    K.wide_len = src.wide_len; K.gen_lens = src.gen_lens;
    K.sums = (unsigned long long *)D.sums.p;
    K.form = src.form; K.n_tiles = nt; K.n_segs = (uint32_t)n_segs; K.k = src.k; K.terminal_limit = P.terminal_limit;
    if (ts_k_launch_match_count(&K, st) != 0) return c->fail(TS_ERR_HIP, "match lines: count launch failed");
    unsigned long long total[4] = {0, 0, 0, 0};
    for (int j = 0; j < 4; ++j) HIP_TRY(c, hipMemcpyAsync(&total[j], K.sums + (size_t)j * col + nt, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const double ms_count = ms_since(t_begin);

    // the runs of tiles that go through together: all of them, or — beyond the slice limit — as many as stay below it
    std::vector<unsigned long long> pre[TS_N_MATCH_FILES];
    const uint64_t limit = std::max<uint64_t>(c->knobs.match_slice_bytes, 1);
    const bool sliced = total[0] + total[1] > limit;
    if (sliced)
        for (int f = 0; f < TS_N_MATCH_FILES; ++f) {
            pre[f].resize(col);
            HIP_TRY(c, hipMemcpy(pre[f].data(), K.sums + (size_t)f * col, col * 8, hipMemcpyDeviceToHost));
        }
    TextTimes ms;
    uint32_t n_slices = 0;
    for (uint32_t a = 0; a < nt && total[0] + total[1];) {
        uint32_t z = nt;
        if (sliced) {
            z = a + 1;                                                           // (a single tile beyond the limit goes alone)
            while (z < nt && (pre[0][z + 1] - pre[0][a]) + (pre[1][z + 1] - pre[1][a]) <= limit) ++z;
        }
        const unsigned long long base[2] = {sliced ? pre[0][a] : 0ull, sliced ? pre[1][a] : 0ull};
        const unsigned long long bytes[2] = {sliced ? pre[0][z] - base[0] : total[0], sliced ? pre[1][z] - base[1] : total[1]};
        if (bytes[0] + bytes[1]) {
            K.slice_base[0] = base[0]; K.slice_base[1] = base[1];
            K.tile_first = a;
            const int rc = text_slice_out(c, "match lines", st, D.text, files, bytes, K.out, ms, [&] { return ts_k_launch_match_write(&K, z - a, st); });
            if (rc != TS_OK) return rc;
            ++n_slices;
        }
        a = z;
    }
    out->n_lines[0] += total[2]; out->n_lines[1] += total[3];
    c->match_text_stats[0] += 1; c->match_text_stats[1] += total[2]; c->match_text_stats[2] += total[3];
    c->match_text_stats[3] += total[0] + total[1];
    if (c->knobs.timing)
        fprintf(stderr, "match lines: %llu canonical + %llu non-canonical lines of %u tiles, %llu bytes in %u slices, %.1f ms (tables up + count %.1f ms, "
                        "write kernel %.1f ms, text D2H %.1f ms); records and bases read where they lie: 0 bytes of either read back\n",
                total[2], total[3], nt, total[0] + total[1], n_slices, ms_since(t_begin), ms_count, ms.write, ms.copy);
    return TS_OK;
}

// A caller's struct at the start of a call (TextFiles::begin); a context without -m has no match files: freed.
void ts_match_text_begin(const ts_ctx *c, ts_match_text *t) {
    text_files(t).begin(c->params.out_matches ? 3u : 0u);
    t->n_lines[0] = t->n_lines[1] = 0;
}

extern "C" {

int ts_match_lines_format(ts_ctx *ctx, const ts_match *records, uint64_t n, const ts_match_line_segment *segs, size_t n_segs, const char *names,
                          uint64_t names_len, const char *bases, uint64_t bases_len, ts_match_text *out) {
    if (!ctx || !out || (n && !records) || (n_segs && !segs) || (names_len && !names) || (bases_len && !bases)) return TS_ERR_INVALID_ARG;
    ts_ctx *c = ctx;
    ts_match_text_begin(c, out);
    DEVICE_TRY(c);
    int rc = ts_pipeline_ensure_streams(c);
    if (rc != TS_OK) return rc;
    if (!c->params.out_matches) return TS_OK;
    auto bad = [&](int code, const std::string &msg) { ts_free_match_text(out); return c->fail(code, msg); };

    // the table, checked: ascending, inside the record array, the bases inside `bases`, every record inside its segment; and
    // the pseudo-tiles the kernels walk
    std::vector<TsMatchTile> tiles;
    uint64_t next = 0;
    for (size_t i = 0; i < n_segs; ++i) {
        const ts_match_line_segment &s = segs[i];
        if (s.base_off > bases_len || s.len > bases_len - s.base_off)
            return bad(TS_ERR_INVALID_ARG, "match lines: segment " + std::to_string(i) + ": its bases lie outside the bases");
        if (!s.n_records) continue;
        if (s.first_record < next || s.first_record > n || s.n_records > n - s.first_record)
            return bad(TS_ERR_INVALID_ARG, "match lines: segment " + std::to_string(i) + ": its records overlap the previous segment's or exceed the records");
        next = s.first_record + s.n_records;
        if (s.tips_only) continue;
        for (uint64_t j = s.first_record; j < next; ++j) {
            const ts_match &m = records[j];
            if (m.match_size == 0 || m.match_size > tsmatch::kMaxSize || m.position < s.abs_pos || m.position - s.abs_pos > s.len ||
                m.match_size > s.len - (m.position - s.abs_pos))
                return bad(TS_ERR_INVALID_ARG, "match lines: record " + std::to_string(j) + ": a size of 0 or above 63, or it does not lie inside segment " + std::to_string(i));
        }
        for (uint64_t a = s.first_record; a < next; a += kArrayTile)
            tiles.push_back(TsMatchTile{a, (uint32_t)std::min<uint64_t>(kArrayTile, next - a), (uint32_t)i});
    }
    if (tiles.empty()) {
        rc = ts_matches_append(c, TsMatchSource{}, nullptr, 0, nullptr, 0, nullptr, out);
        if (rc != TS_OK) ts_free_match_text(out);
        return rc;
    }
    hipStream_t st = c->down_stream;
    DevBuf d_rec, d_tiles, d_bases;
    PoolReturn give_back{c, {&d_rec, &d_tiles, &d_bases}};
    {
        std::lock_guard<std::mutex> dl(c->down_mtx);
        auto up = [&]() -> int {
            HIP_TRY(c, c->pool.take(n * sizeof(ts_match), d_rec));
            HIP_TRY(c, c->pool.take(tiles.size() * sizeof(TsMatchTile), d_tiles));
            HIP_TRY(c, c->pool.take(bases_len + 16, d_bases));
            HIP_TRY(c, hipMemcpyAsync(d_rec.p, records, n * sizeof(ts_match), hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(d_tiles.p, tiles.data(), tiles.size() * sizeof(TsMatchTile), hipMemcpyHostToDevice, st));
            if (bases_len) HIP_TRY(c, hipMemcpyAsync(d_bases.p, bases, bases_len, hipMemcpyHostToDevice, st));
            return TS_OK;
        };
        rc = up();
        if (rc == TS_OK) {
            TsMatchSource src{};
            src.form = TS_MATCH_FORM_ARRAY; src.records = d_rec.p; src.tiles = d_tiles.p; src.n_tiles = tiles.size(); src.bases = d_bases.p;
            rc = ts_matches_append(c, src, segs, n_segs, names, names_len, st, out);
        }
        (void)hipStreamSynchronize(st);
    }
    if (rc != TS_OK) ts_free_match_text(out);
    return rc;
}

void ts_free_match_text(ts_match_text *t) {
    if (!t) return;
    text_files(t).free_all();
    t->n_lines[0] = t->n_lines[1] = 0;
}

int ts_match_text_stats(const ts_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) out[i] = ctx->match_text_stats[i].load();
    return TS_OK;
}

}  // extern "C"
