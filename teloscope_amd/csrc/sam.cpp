// sam.cpp — host side of the device SAM route (include/teloscan.h: ts_sam_chunk_*): argument checks, buffer sizes, launches and
// the few words that come back.  The chunk, its line index, the tab index's kernels and the gather's host half are the chunk
// layer's (chunk_internal.h); the stage's and the gather's kernels are the FASTQ route's.  Nothing here parses a byte of text.
#include <cstddef>

#include "sam_internal.h"
#include "sam_line_core.h"

namespace {

static_assert(sizeof(ts_sam_record) == 24, "layouts");
// what lets the FASTQ gather (chunk.hip's plan reads `size`, fastq.hip's copy `off` and `size`) take a SAM table
static_assert(sizeof(ts_sam_record) == sizeof(ts_fastq_record) && offsetof(ts_sam_record, off) == offsetof(ts_fastq_record, off) &&
              offsetof(ts_sam_record, size) == offsetof(ts_fastq_record, size), "ts_sam_record is gathered as a ts_fastq_record");
static_assert(TS_SAM_OK == tssam::OK && TS_SAM_HEADER_AFTER_RECORD == tssam::HEADER_AFTER_RECORD && TS_SAM_TOO_FEW_FIELDS == tssam::TOO_FEW_FIELDS &&
              TS_SAM_EMPTY_SEQ == tssam::EMPTY_SEQ && TS_SAM_BAD_LENGTHS == tssam::BAD_LENGTHS, "the rule's codes are the header's");

// a record of the table against the chunk: inside it, SEQ inside the record
bool record_ok(const ts_bam_chunk *ch, const ts_sam_record &r) {
    if (r.off > ch->plain_n || r.size > ch->plain_n - r.off) return false;
    return r.flags <= 1 && (uint64_t)r.seq_at + r.seq_len <= r.size;
}

}  // namespace

extern "C" {

int ts_sam_chunk_walk(ts_chunk *ch, int at_end, int in_header, ts_sam_record *recs, uint64_t cap, uint64_t *n, uint64_t *n_header_lines,
                      uint64_t *header_end, uint64_t *n_lines_out, uint64_t *next, int *error, uint64_t *error_line, uint64_t *error_off) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n || !n_header_lines || !header_end || !n_lines_out || !next || !error || !error_line || !error_off || (cap && !recs) ||
        cap > (1ull << 31))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_walk: null or out-of-range argument");
    if (ch->plain_n >= 0xffffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_walk: the chunk holds 4 GiB or more");
    *n = 0; *n_header_lines = 0; *header_end = 0; *n_lines_out = 0; *next = 0; *error = TS_SAM_OK; *error_line = 0; *error_off = 0;
    const uint64_t size = ch->plain_n;
    if (size == 0) return TS_OK;
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, ch->sam.d_out.ensure(64));
    unsigned long long *d_out = (unsigned long long *)ch->sam.d_out.p;
    unsigned long long out[kSmWords];
    static_assert(sizeof out <= 64 && kSmError == kSmFirstAlign + 1, "the result block has 64 bytes; the two minima lie side by side");

    // tabs and lines: '\t' and '\n' per slice, their sums, every tab's offset and every line's start.
    // The tab count is under way before the line count's words are waited for.
    const uint64_t slices = ceil_div(size, kChunkSliceBytes);
    HIP_TRY(ctx, ch->sam.d_counts.ensure((size_t)slices * 4));
    HIP_TRY(ctx, hipMemsetAsync(d_out + kSmFirstAlign, 0xff, 2 * sizeof(unsigned long long), nullptr));
    if (ts_k_launch_chunk_tab_count(ch->d_plain.p, size, (uint32_t *)ch->sam.d_counts.p, nullptr) != 0 ||
        ts_k_launch_chunk_scan((uint32_t *)ch->sam.d_counts.p, (uint32_t)slices, d_out + kSmTabs, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_sam_chunk_walk: kernel launch failed");
    LineIndex ix;
    { const int rc = ts_chunk_line_index(ch, at_end, "ts_sam_chunk_walk", "line or tab", &ix); if (rc != TS_OK) return rc; }
    unsigned long long n_tabs = 0;
    HIP_TRY(ctx, hipMemcpy(&n_tabs, d_out + kSmTabs, sizeof n_tabs, hipMemcpyDeviceToHost));
    if (n_tabs > size) return ctx->fail(TS_ERR_STATE, "ts_sam_chunk_walk: the line or tab count left the chunk");
    const uint64_t newlines = ix.newlines, n_lines = ix.n_lines;
    if (n_lines == 0) return TS_OK;                            // (an unfinished line and nothing else: all of it is the carry)
    HIP_TRY(ctx, ch->sam.d_tabs.ensure((size_t)std::max<uint64_t>(n_tabs, 1) * 4));
    const uint32_t *tabs = (const uint32_t *)ch->sam.d_tabs.p;
    if (ts_k_launch_chunk_tab_index(ch->d_plain.p, size, (const uint32_t *)ch->sam.d_counts.p, (uint32_t)n_tabs, (uint32_t *)ch->sam.d_tabs.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_sam_chunk_walk: kernel launch failed");

    // kinds: alignment lines per slice of lines, their sums, the lowest alignment line
    const uint64_t n_frames = ceil_div(n_lines, kSamSliceLines);
    HIP_TRY(ctx, ch->sam.d_frames.ensure((size_t)n_frames * 4));
    uint32_t *frames = (uint32_t *)ch->sam.d_frames.p;
    if (ts_k_launch_sam_kinds(ix.first, (uint32_t)n_lines, frames, d_out, nullptr) != 0 ||
        ts_k_launch_chunk_scan(frames, (uint32_t)n_frames, d_out + kSmAligns, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_sam_chunk_walk: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    const uint64_t aligns = out[kSmAligns], first_align = out[kSmFirstAlign];
    if (aligns > n_lines || (aligns == 0) != (first_align == ~0ull) || (aligns && first_align + aligns > n_lines))
        return ctx->fail(TS_ERR_STATE, "ts_sam_chunk_walk: the walk left the chunk");

    // records: every alignment line cut and checked, every header line held against the lowest alignment line
    HIP_TRY(ctx, ch->d_recs.ensure((size_t)std::max<uint64_t>(aligns, 1) * sizeof(ts_sam_record)));
    if (ts_k_launch_sam_records(ch->d_plain.p, ix.lstart, ix.first, ix.cr, (uint32_t)n_lines, (uint32_t)newlines, tabs, (uint32_t)n_tabs,
                                in_header ? 1 : 0, frames, ch->d_recs.p, (uint32_t)aligns, d_out, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_sam_chunk_walk: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    if (out[kSmLastLine] > size) return ctx->fail(TS_ERR_STATE, "ts_sam_chunk_walk: the walk left the chunk");

    auto line_start = [&](uint64_t line, uint64_t *off) -> int {
        uint32_t at = 0;
        HIP_TRY(ctx, hipMemcpy(&at, ix.lstart + line, sizeof at, hipMemcpyDeviceToHost));
        if (at > size) return ctx->fail(TS_ERR_STATE, "ts_sam_chunk_walk: the walk left the chunk");
        *off = at;
        return TS_OK;
    };
    const uint64_t headers = in_header ? std::min<uint64_t>(first_align, n_lines) : 0;
    uint64_t whole = aligns, lines = n_lines;
    *next = at_end ? size : out[kSmLastLine];
    if (in_header) {
        *n_header_lines = headers;
        *header_end = *next;
        if (headers < n_lines) { const int rc = line_start(headers, header_end); if (rc != TS_OK) return rc; }
    }
    if (out[kSmError] != ~0ull) {
        const uint64_t bad = out[kSmError] >> 3;
        // (the lines between the header and the lowest bad line are alignment lines: a header line there would be the lowest)
        if (bad >= n_lines || bad < headers || bad - headers > aligns) return ctx->fail(TS_ERR_STATE, "ts_sam_chunk_walk: the error lies outside the lines");
        *error = (int)(out[kSmError] & 7u);
        *error_line = bad;
        { const int rc = line_start(bad, error_off); if (rc != TS_OK) return rc; }
        whole = bad - headers; lines = bad;
        *next = *error_off;
    }
    *n = whole; *n_lines_out = lines;
    const uint64_t take = std::min(whole, cap);
    if (take) HIP_TRY(ctx, hipMemcpy(recs, ch->d_recs.p, (size_t)take * sizeof(ts_sam_record), hipMemcpyDeviceToHost));
    if (whole > cap) return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_walk: the table is too small (*n says what is needed)");
    return TS_OK;
}

int ts_sam_chunk_stage(ts_chunk *ch, const ts_sam_record *recs, size_t n, ts_batch *reads, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    return ts_chunk_stage_records(ch, "ts_sam_chunk_stage", recs, n, reads, stream, kFastqStagePiece, kFastqStagePiece,
                                  [](const ts_bam_chunk *c, const void *table, size_t i, uint64_t *src, uint32_t *len) {
                                      const ts_sam_record &r = ((const ts_sam_record *)table)[i];
                                      *src = (uint64_t)r.off + r.seq_at; *len = r.seq_len;
                                      return record_ok(c, r) && r.flags == 0;
                                  }, ts_k_launch_fastq_stage);
}

int ts_sam_chunk_gather(ts_chunk *ch, const ts_sam_record *recs, size_t n, const void *d_pass, void *host_out, uint64_t cap,
                        uint64_t *bytes, uint64_t *n_passed, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_gather: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i)
        if (!record_ok(ch, recs[i])) return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_gather: record " + std::to_string(i) + " does not fit the chunk");
    return ts_chunk_gather(ch, "ts_sam_chunk_gather", recs, sizeof(ts_sam_record), n, d_pass, host_out, cap, bytes, n_passed, stream,
                           ts_k_launch_chunk_gather_plan_fastq, ts_k_launch_fastq_gather);
}

}  // extern "C"
