// deflate.cpp — host side of the device BGZF writer (include/teloscan.h: ts_bgzf_deflate, ts_bgzf_deflate_stats; bgzf.cpp's
// ts_bam_chunk_gather_bgzf runs on ts_deflate_members too): argument checks, the members' slots, the packed download.  Nothing
// here deflates: the members are written by deflate.hip's kernel or not at all.  The reference's counterpart is BgzfWriter
// (src/bgzf.cpp:227-276).
#include "chunk_internal.h"

namespace {
constexpr uint32_t kMaxPayload = 0xff00u;
}

int ts_deflate_members(ts_ctx *ctx, const char *who, const void *d_plain, uint64_t n, uint32_t payload_bytes, DeflateBufs &bufs,
                       void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_members, void *stream) {
    const std::string name = who;
    *bytes = 0; *n_members = 0;
    if (payload_bytes == 0 || payload_bytes > kMaxPayload)
        return ctx->fail(TS_ERR_INVALID_ARG, name + ": payload_bytes is 1 .. 65280");
    const uint64_t members = ceil_div(n, payload_bytes);
    // slot: 2 bytes of padding, header, payload (<= payload_bytes + 5), footer; a multiple of 64
    const uint32_t stride = (payload_bytes + 2u + 18u + 5u + 8u + 63u) & ~63u;
    if (members > 0x7fffffffull || members * stride > (1ull << 40)) return ctx->fail(TS_ERR_INVALID_ARG, name + ": too large for one call");
    ctx->bgzf_deflate_stats[0].fetch_add(1, std::memory_order_relaxed);
    if (members == 0) return TS_OK;
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    const size_t slot_bytes = (size_t)members * stride;
    if (bufs.slots.ensure(slot_bytes + 64) != hipSuccess || bufs.sizes.ensure((size_t)members * 4) != hipSuccess ||
        bufs.offs.ensure((size_t)members * 8 + 16) != hipSuccess)
        return ctx->fail(TS_ERR_ALLOC, name + ": device allocation failed");
    unsigned long long *offs = (unsigned long long *)bufs.offs.p, *total = offs + members;
    HIP_TRY(ctx, hipMemsetAsync(bufs.slots.p, 0, slot_bytes + 64, st));
    HIP_TRY(ctx, hipMemsetAsync(bufs.sizes.p, 0, (size_t)members * 4, st));
    if (ts_k_launch_bgzf_deflate(d_plain, n, payload_bytes, (uint32_t)members, bufs.slots.p, stride, (uint32_t *)bufs.sizes.p, offs, total,
                                 stream) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    unsigned long long tz[2] = {0, 0};                          // the members' bytes; members of size zero
    HIP_TRY(ctx, hipMemcpyAsync(tz, total, sizeof tz, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const unsigned long long t = tz[0];
    if (tz[1] != 0 || t < members * 27ull || t > members * (uint64_t)(stride - 2u)) return ctx->fail(TS_ERR_STATE, name + ": a member was not written");
    *bytes = t; *n_members = members;
    if (t > cap) return ctx->fail(TS_ERR_INVALID_ARG, name + ": host_out is too small (*bytes says what is needed)");
    if (bufs.packed.ensure((size_t)t) != hipSuccess) return ctx->fail(TS_ERR_ALLOC, name + ": device allocation failed");
    if (ts_k_launch_deflate_pack(bufs.slots.p, stride, (const uint32_t *)bufs.sizes.p, offs, (uint32_t)members, t, bufs.packed.p, stream) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    HIP_TRY(ctx, hipMemcpyAsync(host_out, bufs.packed.p, (size_t)t, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->bgzf_deflate_stats[1].fetch_add(members, std::memory_order_relaxed);
    ctx->bgzf_deflate_stats[2].fetch_add(n, std::memory_order_relaxed);
    ctx->bgzf_deflate_stats[3].fetch_add(t, std::memory_order_relaxed);
    return TS_OK;
}

extern "C" {

int ts_bgzf_deflate(ts_ctx *ctx, const void *plain, uint64_t n, uint32_t payload_bytes, void *out, uint64_t cap, uint64_t *bytes,
                    uint64_t *n_members) {
    if (!ctx) return TS_ERR_INVALID_ARG;
    if (!bytes || !n_members || (n && !plain) || (cap && !out)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bgzf_deflate: null argument");
    if (n > (1ull << 32)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bgzf_deflate: too large for one call");
    *bytes = 0; *n_members = 0;
    if (payload_bytes == 0 || payload_bytes > kMaxPayload) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bgzf_deflate: payload_bytes is 1 .. 65280");
    DEVICE_TRY(ctx);
    DevBuf d_plain;
    DeflateBufs bufs;
    if (n) {
        if (d_plain.ensure((size_t)n) != hipSuccess) return ctx->fail(TS_ERR_ALLOC, "ts_bgzf_deflate: device allocation failed");
        HIP_TRY(ctx, hipMemcpy(d_plain.p, plain, (size_t)n, hipMemcpyHostToDevice));
    }
    const int rc = ts_deflate_members(ctx, "ts_bgzf_deflate", d_plain.p, n, payload_bytes, bufs, out, cap, bytes, n_members, nullptr);
    (void)hipDeviceSynchronize();                              // (the buffers are freed on return)
    return rc;
}

int ts_bgzf_deflate_stats(const ts_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) out[i] = ctx->bgzf_deflate_stats[i].load(std::memory_order_relaxed);
    return TS_OK;
}

}  // extern "C"
