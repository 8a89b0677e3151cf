// gfa.cpp — host side of the device GFA stages (include/teloscan.h: ts_gfa_chunk_walk, ts_gfa_chunk_check): argument checks, buffer
// sizes, launches and the few words that come back.  The chunk, its line index and the tab index's kernels are the chunk layer's
// (chunk_internal.h); nothing here parses a byte of text.
#include "chunk_internal.h"
#include "gfa_internal.h"

namespace {

static_assert(sizeof(ts_gfa_segment) == 48 && sizeof(ts_gfa_line) == 24 && sizeof(ts_gfa_foreign) == 16 && sizeof(GfaFrame) == 16 &&
              sizeof(ts_gfa_flagged) == 24, "layouts");
static_assert(kGfWords * sizeof(unsigned long long) <= 64, "the result block has 64 bytes");

}  // namespace

extern "C" {

int ts_gfa_chunk_walk(ts_chunk *ch, int at_end, ts_gfa_segment *segs, uint64_t seg_cap, uint64_t *n_segs, ts_gfa_line *lines,
                      uint64_t line_cap, uint64_t *n_lines_out, char *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *next,
                      ts_gfa_foreign *foreign) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n_segs || !n_lines_out || !text_bytes || !next || !foreign || (seg_cap && !segs) || (line_cap && !lines) || (text_cap && !text) ||
        seg_cap > (1ull << 31) || line_cap > (1ull << 31))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_gfa_chunk_walk: null or out-of-range argument");
    if (ch->plain_n >= 0xffffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_gfa_chunk_walk: the chunk holds 4 GiB or more");
    *n_segs = 0; *n_lines_out = 0; *text_bytes = 0; *next = 0;
    foreign->off = 0; foreign->len = 0; foreign->found = 0;
    const uint64_t size = ch->plain_n;
    if (size == 0) return TS_OK;
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, ch->gfa.d_out.ensure(64));
    unsigned long long *d_out = (unsigned long long *)ch->gfa.d_out.p;
    unsigned long long out[kGfWords];

    // tabs and lines: '\t' and '\n' per slice, their sums, every tab's offset and every line's start.
    // The tab count is under way before the line count's words are waited for.
    const uint64_t slices = ceil_div(size, kChunkSliceBytes);
    HIP_TRY(ctx, ch->gfa.d_counts.ensure((size_t)slices * 4));
    HIP_TRY(ctx, hipMemsetAsync(d_out + kGfForeignLine, 0xff, sizeof(unsigned long long), nullptr));
    if (ts_k_launch_chunk_tab_count(ch->d_plain.p, size, (uint32_t *)ch->gfa.d_counts.p, nullptr) != 0 ||
        ts_k_launch_chunk_scan((uint32_t *)ch->gfa.d_counts.p, (uint32_t)slices, d_out + kGfTabs, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gfa_chunk_walk: kernel launch failed");
    LineIndex ix;
    { const int rc = ts_chunk_line_index(ch, at_end, "ts_gfa_chunk_walk", "line or tab", &ix); if (rc != TS_OK) return rc; }
    unsigned long long n_tabs = 0;
    HIP_TRY(ctx, hipMemcpy(&n_tabs, d_out + kGfTabs, sizeof n_tabs, hipMemcpyDeviceToHost));
    if (n_tabs > size) return ctx->fail(TS_ERR_STATE, "ts_gfa_chunk_walk: the line or tab count left the chunk");
    const uint64_t newlines = ix.newlines, n_lines = ix.n_lines;
    HIP_TRY(ctx, ch->gfa.d_tabs.ensure((size_t)std::max<uint64_t>(n_tabs, 1) * 4));
    uint32_t *lstart = ix.lstart;
    unsigned char *first = ix.first, *cr = ix.cr;
    const uint32_t *tabs = (const uint32_t *)ch->gfa.d_tabs.p;
    if (ts_k_launch_chunk_tab_index(ch->d_plain.p, size, (const uint32_t *)ch->gfa.d_counts.p, (uint32_t)n_tabs, (uint32_t *)ch->gfa.d_tabs.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gfa_chunk_walk: kernel launch failed");
    // (what ts_gfa_chunk_check works on: both indexes stay where they are until the chunk is indexed again)
    ch->gfa.lines_generation = ch->lines.generation; ch->gfa.n_tabs = n_tabs;

    // kinds: per slice of lines, their sums, the lowest foreign line
    const uint64_t n_frames = ceil_div(n_lines, kGfaSliceLines);
    HIP_TRY(ctx, ch->gfa.d_kinds.ensure((size_t)std::max<uint64_t>(n_lines, 1)));
    HIP_TRY(ctx, ch->gfa.d_frames.ensure((size_t)std::max<uint64_t>(n_frames, 1) * sizeof(GfaFrame)));
    if (ts_k_launch_gfa_kinds(ch->d_plain.p, lstart, first, cr, (uint32_t)n_lines, (uint32_t)newlines, tabs, (uint32_t)n_tabs,
                              (unsigned char *)ch->gfa.d_kinds.p, ch->gfa.d_frames.p, d_out, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gfa_chunk_walk: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    const uint64_t ns = out[kGfSegs], nl = out[kGfLines], nt = out[kGfTextBytes];
    if (ns > n_lines || nl > n_lines || nt > size || out[kGfLastLine] > size || ns + nl > 0x7fffffffull ||
        (out[kGfForeignLine] != ~0ull && (out[kGfForeignLine] >= n_lines || out[kGfForeignOff] + out[kGfForeignLen] > size)))
        return ctx->fail(TS_ERR_STATE, "ts_gfa_chunk_walk: the walk left the chunk");
    *n_segs = ns; *n_lines_out = nl; *text_bytes = nt;
    *next = at_end ? size : out[kGfLastLine];
    if (out[kGfForeignLine] != ~0ull) { foreign->off = out[kGfForeignOff]; foreign->len = (uint32_t)out[kGfForeignLen]; foreign->found = 1; }
    if (ns > seg_cap || nl > line_cap || nt > text_cap)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_gfa_chunk_walk: a table or the text buffer is too small (*n_segs, *n_lines and *text_bytes say what is needed)");
    if (ns + nl == 0) return TS_OK;

    // tables and the gathered text
    HIP_TRY(ctx, ch->gfa.d_segs.ensure((size_t)std::max<uint64_t>(ns, 1) * sizeof(ts_gfa_segment)));
    HIP_TRY(ctx, ch->gfa.d_lines.ensure((size_t)std::max<uint64_t>(nl, 1) * sizeof(ts_gfa_line)));
    HIP_TRY(ctx, ch->gfa.d_text.ensure((size_t)std::max<uint64_t>(nt, 1)));
    if (ts_k_launch_gfa_tables(ch->d_plain.p, lstart, cr, (uint32_t)n_lines, tabs, (uint32_t)n_tabs, (const unsigned char *)ch->gfa.d_kinds.p,
                               ch->gfa.d_frames.p, ch->gfa.d_segs.p, (uint32_t)ns, ch->gfa.d_lines.p, (uint32_t)nl, nullptr) != 0 ||
        ts_k_launch_gfa_gather(ch->d_plain.p, size, ch->gfa.d_segs.p, (uint32_t)ns, ch->gfa.d_lines.p, (uint32_t)nl, ch->gfa.d_text.p, nt,
                               nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gfa_chunk_walk: kernel launch failed");
    if (ns) HIP_TRY(ctx, hipMemcpy(segs, ch->gfa.d_segs.p, (size_t)ns * sizeof(ts_gfa_segment), hipMemcpyDeviceToHost));
    if (nl) HIP_TRY(ctx, hipMemcpy(lines, ch->gfa.d_lines.p, (size_t)nl * sizeof(ts_gfa_line), hipMemcpyDeviceToHost));
    if (nt) HIP_TRY(ctx, hipMemcpy(text, ch->gfa.d_text.p, (size_t)nt, hipMemcpyDeviceToHost));
    return TS_OK;
}

int ts_gfa_chunk_check(ts_chunk *ch, int at_end, ts_gfa_flagged *flagged, uint64_t cap, uint64_t *n_flagged, uint64_t *n_lines_out) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n_flagged || !n_lines_out || (cap && !flagged) || cap > (1ull << 31))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_gfa_chunk_check: null or out-of-range argument");
    *n_flagged = 0; *n_lines_out = 0;
    const uint64_t size = ch->plain_n;
    if (size == 0) return TS_OK;
    if (!ts_chunk_lines_current(ch, ch->gfa.lines_generation, at_end))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_gfa_chunk_check: ts_gfa_chunk_walk has not walked the chunk's bytes with this at_end");
    const LineIndex &ix = ch->lines.ix;
    const uint64_t n_lines = ix.n_lines, n_tabs = ch->gfa.n_tabs;
    *n_lines_out = n_lines;
    if (n_lines == 0) return TS_OK;
    DEVICE_TRY(ctx);
    // the walk's indexes, where it left them
    const uint32_t *lstart = ix.lstart;
    const unsigned char *first = ix.first, *cr = ix.cr;
    const uint32_t *tabs = (const uint32_t *)ch->gfa.d_tabs.p;
    const uint64_t n_frames = ceil_div(n_lines, kGfaSliceLines);
    HIP_TRY(ctx, ch->gfa.d_stray.ensure((size_t)n_lines));
    HIP_TRY(ctx, ch->gfa.d_codes.ensure((size_t)n_lines));
    HIP_TRY(ctx, ch->gfa.d_ccounts.ensure((size_t)n_frames * 4));
    HIP_TRY(ctx, ch->gfa.d_cout.ensure(8));
    HIP_TRY(ctx, hipMemsetAsync(ch->gfa.d_stray.p, 0, (size_t)n_lines, nullptr));
    if (ts_k_launch_gfa_stray_cr(ch->d_plain.p, size, at_end, lstart, (uint32_t)n_lines, (unsigned char *)ch->gfa.d_stray.p, nullptr) != 0 ||
        ts_k_launch_gfa_check(ch->d_plain.p, lstart, first, cr, (uint32_t)n_lines, tabs, (uint32_t)n_tabs, (const unsigned char *)ch->gfa.d_stray.p,
                              (unsigned char *)ch->gfa.d_codes.p, (uint32_t *)ch->gfa.d_ccounts.p, nullptr) != 0 ||
        ts_k_launch_chunk_scan((uint32_t *)ch->gfa.d_ccounts.p, (uint32_t)n_frames, (unsigned long long *)ch->gfa.d_cout.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gfa_chunk_check: kernel launch failed");
    unsigned long long nf = 0;
    HIP_TRY(ctx, hipMemcpy(&nf, ch->gfa.d_cout.p, sizeof nf, hipMemcpyDeviceToHost));
    if (nf > n_lines) return ctx->fail(TS_ERR_STATE, "ts_gfa_chunk_check: more flagged lines than lines");
    *n_flagged = nf;
    if (nf > cap) return ctx->fail(TS_ERR_INVALID_ARG, "ts_gfa_chunk_check: the table is too small (*n_flagged says what is needed)");
    if (nf == 0) return TS_OK;
    HIP_TRY(ctx, ch->gfa.d_flagged.ensure((size_t)nf * sizeof(ts_gfa_flagged)));
    if (ts_k_launch_gfa_flagged(lstart, first, cr, (uint32_t)n_lines, (const unsigned char *)ch->gfa.d_codes.p, (const uint32_t *)ch->gfa.d_ccounts.p,
                                ch->gfa.d_flagged.p, (uint32_t)nf, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gfa_chunk_check: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(flagged, ch->gfa.d_flagged.p, (size_t)nf * sizeof(ts_gfa_flagged), hipMemcpyDeviceToHost));
    return TS_OK;
}

}  // extern "C"
