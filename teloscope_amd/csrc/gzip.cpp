// gzip.cpp — host side of the device route for plain gzip (include/teloscan.h: ts_gzip_decode): staging, the stitch of the span
// table into a chain, the verdict.  Nothing here inflates: the spans are decoded by gzip.hip's kernels or not at all, and what
// their chain does not verify is the caller's to hand to zlib.
#include "chunk_internal.h"
#include "gzip_core.h"

namespace {
struct SpanEntry { uint32_t start_bit, end_bit, n_out, status, final_seen, reserved; };
struct ChainEntry { uint32_t span, n_out, hist_avail, reserved; unsigned long long plain_off; };
struct CrcSlice { unsigned long long off; uint32_t len, crc; };
constexpr uint32_t kSymbolsPerByte = 16;    // a span's room: symbols per compressed byte of a span,
constexpr uint32_t kMinSymbols = 512u << 10; // and this many at least (a span decodes whole blocks, and a block of text is 50 - 200 KB)
constexpr uint64_t kMaxSymbolBytes = 4ull << 30;
constexpr uint32_t kCrcSlice = 65536;
}  // namespace

struct ts_gzip {
    ts_ctx *ctx = nullptr;
    uint32_t span_bytes = 0;
    DevBuf d_comp, d_cand, d_table, d_sym, d_chain, d_hist, d_plain, d_slices, d_flag, d_keep;
    uint64_t plain_n = 0, taken = 0;    // bytes of the last decode, and how many of them ts_gzip_take has moved
    uint32_t keep_len = 0;              // bytes of d_keep (its last ones) that are real: min(32768, bytes in front of end_bit)
};

extern "C" {

ts_gzip *ts_gzip_create(ts_ctx *ctx, uint32_t span_bytes) {
    if (!ctx) return nullptr;
    if (span_bytes < 1024u || span_bytes > (1u << 20) || span_bytes % 1024u) {
        ctx->fail(TS_ERR_INVALID_ARG, "ts_gzip_create: span_bytes must be a multiple of 1024 in 1024 .. 1 MiB");
        return nullptr;
    }
    if (ctx->device == kNoDevice) { ctx->fail(TS_ERR_NO_DEVICE, "planning-only context: no HIP device behind it"); return nullptr; }
    DeviceGuard guard(ctx->device);
    if (guard.error() != hipSuccess) { ctx->fail(TS_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.error())); return nullptr; }
    ts_gzip *gz = new ts_gzip();
    gz->ctx = ctx; gz->span_bytes = span_bytes;
    if (gz->d_keep.ensure(tsgz::kHistory) != hipSuccess || gz->d_flag.ensure(64) != hipSuccess ||
        hipMemset(gz->d_keep.p, 0, tsgz::kHistory) != hipSuccess) {
        ctx->fail(TS_ERR_ALLOC, "ts_gzip_create: device allocation failed");
        delete gz;
        return nullptr;
    }
    return gz;
}

void ts_gzip_destroy(ts_gzip *gz) {
    if (!gz) return;
    DeviceGuard guard(gz->ctx->device);
    (void)hipDeviceSynchronize();
    delete gz;
}

int ts_gzip_decode(ts_gzip *gz, const void *compressed, uint64_t n, uint64_t start_bit, int history_mode, const void *history,
                   uint64_t history_len, ts_gzip_result *res) {
    if (!gz) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = gz->ctx;
    const uint64_t n_spans64 = ceil_div(n, gz->span_bytes);
    if (!res || !compressed || n == 0 || n > (1ull << 28) || n_spans64 > 65535 ||
        n_spans64 * std::max(kSymbolsPerByte * gz->span_bytes, kMinSymbols) * 2 > kMaxSymbolBytes || start_bit >= 8 * std::min<uint64_t>(n, gz->span_bytes) ||
        history_mode < TS_GZIP_HISTORY_EMPTY || history_mode > TS_GZIP_HISTORY_GIVEN ||
        (history_mode == TS_GZIP_HISTORY_GIVEN && (history_len > tsgz::kHistory || (history_len && !history))))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_gzip_decode: null or out-of-range argument");
    DEVICE_TRY(ctx);
    const uint32_t n_spans = (uint32_t)n_spans64, cap = std::max(kSymbolsPerByte * gz->span_bytes, kMinSymbols), window_len = (uint32_t)n;
    const uint32_t hist0_len = history_mode == TS_GZIP_HISTORY_EMPTY ? 0u : history_mode == TS_GZIP_HISTORY_KEPT ? gz->keep_len : (uint32_t)history_len;
    *res = ts_gzip_result{};
    res->end_bit = start_bit; res->status = TS_GZIP_NO_CANDIDATE; res->spans_probed = n_spans - 1u;
    gz->plain_n = 0; gz->taken = 0;
    ctx->gzip_stats[0].fetch_add(1, std::memory_order_relaxed);
    ctx->gzip_stats[1].fetch_add(n_spans - 1u, std::memory_order_relaxed);

    HIP_TRY(ctx, gz->d_comp.ensure((size_t)n + 64));
    HIP_TRY(ctx, gz->d_cand.ensure((size_t)n_spans * 4));
    HIP_TRY(ctx, gz->d_table.ensure((size_t)n_spans * sizeof(SpanEntry)));
    HIP_TRY(ctx, hipMemcpy(gz->d_comp.p, compressed, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset((char *)gz->d_comp.p + n, 0, 64));
    HIP_TRY(ctx, hipMemset(gz->d_cand.p, 0xff, (size_t)n_spans * 4));
    if (ts_k_launch_gzip_probe(gz->d_comp.p, window_len, (uint32_t)start_bit, gz->span_bytes, n_spans, (uint32_t *)gz->d_cand.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gzip_decode: kernel launch failed");
    std::vector<uint32_t> cand(n_spans);
    HIP_TRY(ctx, hipMemcpy(cand.data(), gz->d_cand.p, (size_t)n_spans * 4, hipMemcpyDeviceToHost));
    if (cand[0] != (uint32_t)start_bit) return ctx->fail(TS_ERR_STATE, "ts_gzip_decode: the probe did not run");
    bool any = false;
    for (uint32_t s = 1; s < n_spans; ++s) {
        if (cand[s] == tsgz::kNoCandidate) continue;
        if (cand[s] / 8u / gz->span_bytes != s) return ctx->fail(TS_ERR_STATE, "ts_gzip_decode: a candidate outside its span");
        any = true;
    }
    // the history in front of the window (its real bytes are its last ones) into 32 KiB of device memory
    auto stage_history = [&](void *dst) -> hipError_t {
        if (history_mode == TS_GZIP_HISTORY_KEPT) return dst == gz->d_keep.p ? hipSuccess : hipMemcpy(dst, gz->d_keep.p, tsgz::kHistory, hipMemcpyDeviceToDevice);
        hipError_t e = hipMemset(dst, 0, tsgz::kHistory);
        if (e == hipSuccess && hist0_len) e = hipMemcpy((char *)dst + (tsgz::kHistory - hist0_len), history, hist0_len, hipMemcpyHostToDevice);
        return e;
    };
    // No candidate behind the start in a window of four spans or more: one wave would decode it all.  Where the window begins
    // with a dynamic block it lies inside one or two long blocks and the wave goes on; where it begins with anything else
    // (stored blocks: a file that did not compress) zlib is faster at that, and nothing is decoded.
    const unsigned char *cb = (const unsigned char *)compressed;
    const uint32_t head = (uint32_t)(cb[start_bit / 8] | (start_bit / 8 + 1 < n ? cb[start_bit / 8 + 1] << 8 : 0)) >> (start_bit & 7);
    if (n_spans >= 4 && !any && ((head >> 1) & 3u) != 2u) {
        HIP_TRY(ctx, stage_history(gz->d_keep.p));
        gz->keep_len = hist0_len;
        return TS_OK;
    }

    HIP_TRY(ctx, gz->d_sym.ensure((size_t)n_spans * cap * 2));
    HIP_TRY(ctx, hipMemset(gz->d_table.p, 0xff, (size_t)n_spans * sizeof(SpanEntry)));
    if (ts_k_launch_gzip_decode(gz->d_comp.p, window_len, n_spans, (const uint32_t *)gz->d_cand.p, cap, hist0_len, gz->d_sym.p,
                                gz->d_table.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gzip_decode: kernel launch failed");
    std::vector<SpanEntry> table(n_spans);
    HIP_TRY(ctx, hipMemcpy(table.data(), gz->d_table.p, (size_t)n_spans * sizeof(SpanEntry), hipMemcpyDeviceToHost));

    // the stitch: the first span, then the span that starts where the one before ended
    std::vector<ChainEntry> chain;
    uint32_t cur = 0, dropped = 0, end_status = tsgz::kSpanEdge, max_out = 0;
    uint64_t total = 0, avail = hist0_len, end_bit = start_bit;
    for (;;) {
        const SpanEntry &e = table[cur];
        if (e.start_bit != cand[cur] || e.status > tsgz::kSpanEdge || e.n_out > cap || e.end_bit < e.start_bit || e.end_bit > 8ull * n)
            return ctx->fail(TS_ERR_STATE, "ts_gzip_decode: span " + std::to_string(cur) + " was not decoded");
        chain.push_back(ChainEntry{cur, e.n_out, (uint32_t)std::min<uint64_t>(avail, tsgz::kHistory), 0u, total});
        total += e.n_out; avail += e.n_out; end_bit = e.end_bit; end_status = e.status;
        max_out = std::max(max_out, e.n_out);
        if (e.status != tsgz::kSpanStop) break;
        uint32_t t = cur + 1, skipped = 0;
        for (; t < n_spans && cand[t] != e.end_bit; ++t) if (cand[t] != tsgz::kNoCandidate) ++skipped;
        if (t >= n_spans) { end_status = tsgz::kSpanEdge; break; }      // (no successor starts at its end)
        dropped += skipped;
        cur = t;
    }

    HIP_TRY(ctx, gz->d_chain.ensure(chain.size() * sizeof(ChainEntry)));
    HIP_TRY(ctx, gz->d_hist.ensure((chain.size() + 1) * (size_t)tsgz::kHistory));
    HIP_TRY(ctx, gz->d_plain.ensure((size_t)total + 64));
    std::vector<CrcSlice> slices;
    for (const ChainEntry &c : chain)
        for (uint32_t a = 0; a < c.n_out; a += kCrcSlice) slices.push_back(CrcSlice{c.plain_off + a, std::min(kCrcSlice, c.n_out - a), 0u});
    HIP_TRY(ctx, gz->d_slices.ensure(std::max<size_t>(slices.size(), 1) * sizeof(CrcSlice)));
    HIP_TRY(ctx, hipMemcpy(gz->d_chain.p, chain.data(), chain.size() * sizeof(ChainEntry), hipMemcpyHostToDevice));
    if (!slices.empty()) HIP_TRY(ctx, hipMemcpy(gz->d_slices.p, slices.data(), slices.size() * sizeof(CrcSlice), hipMemcpyHostToDevice));
    HIP_TRY(ctx, stage_history(gz->d_hist.p));
    HIP_TRY(ctx, hipMemset(gz->d_flag.p, 0xff, 4));
    if (ts_k_launch_gzip_resolve(gz->d_sym.p, cap, gz->d_chain.p, (uint32_t)chain.size(), max_out, gz->d_hist.p, gz->d_plain.p, total,
                                 (uint32_t *)gz->d_flag.p, nullptr) != 0 ||
        ts_k_launch_gzip_crc(gz->d_plain.p, total, gz->d_slices.p, (uint32_t)slices.size(), nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_gzip_decode: kernel launch failed");
    uint32_t bad = 0xffffffffu;
    HIP_TRY(ctx, hipMemcpy(&bad, gz->d_flag.p, 4, hipMemcpyDeviceToHost));
    if (!slices.empty()) HIP_TRY(ctx, hipMemcpy(slices.data(), gz->d_slices.p, slices.size() * sizeof(CrcSlice), hipMemcpyDeviceToHost));
    size_t kept = chain.size();
    if (bad != 0xffffffffu) {                                   // a marker in front of the member's first byte: the chain ends before that span
        if (bad >= chain.size()) return ctx->fail(TS_ERR_STATE, "ts_gzip_decode: the resolve step left the chain");
        kept = bad;
        total = chain[bad].plain_off;
        end_bit = table[chain[bad].span].start_bit;
        end_status = tsgz::kSpanBad;
    }
    uint32_t crc = 0;
    for (const CrcSlice &s : slices) if (s.off < total) crc = tsinf::crc_combine(crc, s.crc, s.len);
    HIP_TRY(ctx, hipMemcpy(gz->d_keep.p, (const char *)gz->d_hist.p + kept * (size_t)tsgz::kHistory, tsgz::kHistory, hipMemcpyDeviceToDevice));
    gz->keep_len = (uint32_t)std::min<uint64_t>(tsgz::kHistory, (uint64_t)hist0_len + total);
    gz->plain_n = total;
    res->end_bit = end_bit; res->plain_bytes = total; res->crc32 = crc;
    res->status = end_status == tsgz::kSpanFinal ? TS_GZIP_FINAL_BLOCK : end_status == tsgz::kSpanFull ? TS_GZIP_SPAN_OVERFLOW :
                  end_status == tsgz::kSpanBad ? TS_GZIP_BAD_DEFLATE : TS_GZIP_WINDOW_END;
    res->member_ended = res->status == TS_GZIP_FINAL_BLOCK;
    res->spans_chained = (uint32_t)kept; res->spans_dropped = dropped;
    ctx->gzip_stats[2].fetch_add(kept, std::memory_order_relaxed);
    ctx->gzip_stats[3].fetch_add(dropped, std::memory_order_relaxed);
    ctx->gzip_stats[4].fetch_add(total, std::memory_order_relaxed);
    return TS_OK;
}

int ts_gzip_take(ts_gzip *gz, ts_chunk *ch, uint64_t carry_from, uint64_t want, uint64_t *moved) {
    if (!gz) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = gz->ctx;
    if (!ch || !moved || ch->ctx != ctx || carry_from > ch->plain_n) return ctx->fail(TS_ERR_INVALID_ARG, "ts_gzip_take: null or out-of-range argument");
    const uint64_t m = std::min<uint64_t>(want, gz->plain_n - gz->taken), tail = ch->plain_n - carry_from;
    *moved = 0;
    if (tail + m > ch->plain_cap) { const int rc = ts_chunk_reserve(ch, tail + m); if (rc != TS_OK) return rc; }
    DEVICE_TRY(ctx);
    uint64_t carry = 0;
    { const int rc = ts_chunk_carry(ch, carry_from, nullptr, &carry); if (rc != TS_OK) return rc; }
    if (m) HIP_TRY(ctx, hipMemcpyAsync((char *)ch->d_plain.p + carry, (const char *)gz->d_plain.p + gz->taken, (size_t)m, hipMemcpyDeviceToDevice, nullptr));
    ch->plain_n = carry + m;
    ch->n_blocks = 0;
    HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    gz->taken += m;
    *moved = m;
    return TS_OK;
}

int ts_gzip_read(ts_gzip *gz, uint64_t off, uint64_t n, void *host) {
    if (!gz) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = gz->ctx;
    if ((n && !host) || off > gz->plain_n || n > gz->plain_n - off) return ctx->fail(TS_ERR_INVALID_ARG, "ts_gzip_read: outside the produced bytes");
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (n) HIP_TRY(ctx, hipMemcpy(host, (const char *)gz->d_plain.p + off, (size_t)n, hipMemcpyDeviceToHost));
    return TS_OK;
}

int ts_gzip_history(ts_gzip *gz, void *host, uint64_t *len) {
    if (!gz) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = gz->ctx;
    if (!host || !len) return ctx->fail(TS_ERR_INVALID_ARG, "ts_gzip_history: null argument");
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, hipDeviceSynchronize());
    *len = gz->keep_len;
    if (gz->keep_len) HIP_TRY(ctx, hipMemcpy(host, (const char *)gz->d_keep.p + (tsgz::kHistory - gz->keep_len), gz->keep_len, hipMemcpyDeviceToHost));
    return TS_OK;
}

int ts_gzip_note_fallback(ts_gzip *gz, uint64_t parts) {
    if (!gz) return TS_ERR_INVALID_ARG;
    gz->ctx->gzip_stats[5].fetch_add(parts, std::memory_order_relaxed);
    return TS_OK;
}

int ts_gzip_stats(const ts_ctx *ctx, uint64_t out[6]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 6; ++i) out[i] = ctx->gzip_stats[i].load(std::memory_order_relaxed);
    return TS_OK;
}

}  // extern "C"
