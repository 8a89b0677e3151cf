// chunk.cpp — the chunk object of the device routes (chunk_internal.h; include/teloscan.h: ts_bam_chunk_create / _destroy / _size /
// _read / _pass_buffer, ts_chunk_*): its buffers, how bytes get into it and are carried from one chunk to the next, the line index
// of the three text walks, the stage and the gather of the record routes.  What a route makes of the bytes is the route's file.
#include "chunk_internal.h"

int ts_chunk_carry(ts_bam_chunk *ch, uint64_t carry_from, hipStream_t st, uint64_t *carry_out) {
    ts_ctx *ctx = ch->ctx;
    const uint64_t carry = ch->plain_n - carry_from;
    *carry_out = carry;
    if (carry && carry_from) {                                   // the tail moves to the front (through a buffer where the two overlap)
        char *p = (char *)ch->d_plain.p;
        if (carry_from >= carry) HIP_TRY(ctx, hipMemcpyAsync(p, p + carry_from, (size_t)carry, hipMemcpyDeviceToDevice, st));
        else {
            HIP_TRY(ctx, ch->d_tmp.ensure((size_t)carry));
            HIP_TRY(ctx, hipMemcpyAsync(ch->d_tmp.p, p + carry_from, (size_t)carry, hipMemcpyDeviceToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(p, ch->d_tmp.p, (size_t)carry, hipMemcpyDeviceToDevice, st));
        }
    }
    return TS_OK;
}

int ts_chunk_stage_reserve(ts_bam_chunk *ch, uint64_t stage_cap) {
    ts_ctx *ctx = ch->ctx;
    if (stage_cap > (1ull << 40)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_chunk_stage: capacity out of range");
    if (stage_cap <= ch->stage_cap && ch->d_stage.p) return TS_OK;
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, hipDeviceSynchronize());
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(stage_cap, 64), ch->stage_cap + ch->stage_cap / 2);
    DevBuf grown;
    if (grown.ensure((size_t)cap + 64) != hipSuccess) return ctx->fail(TS_ERR_ALLOC, "ts_chunk_stage: device allocation failed");
    if (ch->stage_n) HIP_TRY(ctx, hipMemcpy(grown.p, ch->d_stage.p, (size_t)ch->stage_n, hipMemcpyDeviceToDevice));
    ch->d_stage = std::move(grown);
    ch->stage_cap = cap;
    return TS_OK;
}

int ts_chunk_line_index(ts_bam_chunk *ch, int at_end, const char *who, const char *counted, LineIndex *ix) {
    ts_ctx *ctx = ch->ctx;
    ts_bam_chunk::Lines &L = ch->lines;
    const std::string name = who;
    const uint64_t size = ch->plain_n;
    unsigned long long *d_out = (unsigned long long *)ch->d_out.p;
    L.valid = false;                                           // (the index before this one is overwritten from here on)
    HIP_TRY(ctx, L.d_waves.ensure((size_t)ceil_div(size, kChunkSliceBytes) * 4));
    if (ts_k_launch_chunk_newline_count(ch->d_plain.p, size, (uint32_t *)L.d_waves.p, d_out, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    unsigned long long out[kChunkLineWords];
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    const uint64_t newlines = out[kChunkNewlines], tail = out[kChunkTail];
    if (newlines > size || tail > 1) return ctx->fail(TS_ERR_STATE, name + ": the " + counted + " count left the chunk");
    const uint64_t slots = newlines + 2;
    HIP_TRY(ctx, L.d_lines.ensure((size_t)slots * 6));
    ix->newlines = newlines; ix->tail = tail; ix->n_lines = newlines + (at_end ? tail : 0);
    ix->lstart = (uint32_t *)L.d_lines.p;
    ix->first = (unsigned char *)L.d_lines.p + slots * 4; ix->cr = ix->first + slots;
    if (ts_k_launch_chunk_newline_index(ch->d_plain.p, size, (const uint32_t *)L.d_waves.p, (uint32_t)newlines, (uint32_t)tail, ix->lstart,
                                        ix->first, ix->cr, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    L.ix = *ix; L.at_end = at_end ? 1 : 0; L.size = size;
    ++L.generation;
    L.valid = true;
    return TS_OK;
}

int ts_chunk_gather_device(ts_bam_chunk *ch, const char *who, const void *recs, size_t rec_bytes, size_t n, const void *d_pass,
                           uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream, ts_chunk_plan_launch plan,
                           ts_chunk_copy_launch copy) {
    ts_ctx *ctx = ch->ctx;
    const std::string name = who;
    *bytes = 0; *n_passed = 0;
    if (n == 0) return TS_OK;
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, ch->d_recs.ensure(n * rec_bytes));
    HIP_TRY(ctx, ch->d_dst.ensure(n * 8));
    HIP_TRY(ctx, hipMemcpyAsync(ch->d_recs.p, recs, n * rec_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    unsigned long long *totals = (unsigned long long *)ch->d_out.p + 4;
    if (plan(ch->d_recs.p, d_pass, n, ch->d_dst.p, totals, stream) != 0) return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    unsigned long long t[2];
    HIP_TRY(ctx, hipMemcpyAsync(t, totals, sizeof t, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *bytes = t[0]; *n_passed = t[1];
    if (t[0] > cap) return ctx->fail(TS_ERR_INVALID_ARG, name + ": host_out is too small (*bytes says what is needed)");
    if (t[0] == 0) return TS_OK;
    HIP_TRY(ctx, ch->d_gather.ensure((size_t)t[0]));
    if (copy(ch->d_plain.p, ch->d_recs.p, ch->d_dst.p, n, t[0], ch->d_gather.p, stream) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    return TS_OK;
}

int ts_chunk_gather(ts_bam_chunk *ch, const char *who, const void *recs, size_t rec_bytes, size_t n, const void *d_pass,
                    void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream, ts_chunk_plan_launch plan,
                    ts_chunk_copy_launch copy) {
    ts_ctx *ctx = ch->ctx;
    const int rc = ts_chunk_gather_device(ch, who, recs, rec_bytes, n, d_pass, cap, bytes, n_passed, stream, plan, copy);
    if (rc != TS_OK || *bytes == 0) return rc;
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemcpyAsync(host_out, ch->d_gather.p, (size_t)*bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return TS_OK;
}

int ts_chunk_stage_records(ts_bam_chunk *ch, const char *who, const void *recs, size_t n, ts_batch *reads, void *stream, uint32_t piece,
                           uint32_t src_step, ts_chunk_stage_record record, ts_chunk_stage_launch launch) {
    ts_ctx *ctx = ch->ctx;
    const std::string name = who;
    if (!reads || (n && !recs) || reads->ctx != ctx || !reads->tips || !reads->whole() || reads->segs.size() != n)
        return ctx->fail(TS_ERR_INVALID_ARG, name + ": needs an unrestricted tips-only batch of this context with one segment per record");
    std::vector<ChunkStageJob> jobs;
    for (size_t i = 0; i < n; ++i) {
        uint64_t src = 0;
        uint32_t len = 0;
        if (!record(ch, recs, i, &src, &len) || len == 0 || reads->segs[i].len != len)
            return ctx->fail(TS_ERR_INVALID_ARG, name + ": record " + std::to_string(i) + " does not fit the chunk or its segment");
        const uint64_t dst = ts_batch_segment_offset(reads, i);
        for (uint32_t a = 0; a < len; a += piece, src += src_step) jobs.push_back(ChunkStageJob{src, dst + a, std::min(piece, len - a), 0});
    }
    if (jobs.size() > 0x7fffffffull) return ctx->fail(TS_ERR_INVALID_ARG, name + ": too many bases for one call");
    DEVICE_TRY(ctx);
    const bool fresh = reads->d_in.p == nullptr;
    void *in = ts_batch_input_ptr(reads);
    if (!in) return ctx->fail(TS_ERR_ALLOC, name + ": no input buffer");
    if (jobs.empty()) return TS_OK;
    hipStream_t st = (hipStream_t)stream;
    // (a fresh input buffer was just zeroed on the null stream, which a non-blocking `stream` does not wait for)
    if (fresh && st) HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    HIP_TRY(ctx, ch->d_jobs.ensure(jobs.size() * sizeof(ChunkStageJob)));
    HIP_TRY(ctx, hipMemcpyAsync(ch->d_jobs.p, jobs.data(), jobs.size() * sizeof(ChunkStageJob), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (launch(ch->d_plain.p, ch->d_jobs.p, (uint32_t)jobs.size(), in, stream) != 0) return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    return TS_OK;
}

extern "C" {

ts_bam_chunk *ts_bam_chunk_create(ts_ctx *ctx, uint64_t compressed_cap, uint64_t plain_cap) {
    if (!ctx) return nullptr;
    if (compressed_cap == 0 || plain_cap == 0 || compressed_cap > (1ull << 40) || plain_cap > (1ull << 40)) {
        ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_create: capacities out of range");
        return nullptr;
    }
    if (ctx->device == kNoDevice) { ctx->fail(TS_ERR_NO_DEVICE, "planning-only context: no HIP device behind it"); return nullptr; }
    DeviceGuard guard(ctx->device);
    if (guard.error() != hipSuccess) { ctx->fail(TS_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.error())); return nullptr; }
    ts_bam_chunk *ch = new ts_bam_chunk();
    ch->ctx = ctx; ch->comp_cap = compressed_cap; ch->plain_cap = plain_cap;
    // (the kernels read whole aligned words: 64 readable bytes behind both buffers)
    if (ch->d_comp.ensure((size_t)compressed_cap + 64) != hipSuccess || ch->d_plain.ensure((size_t)plain_cap + 64) != hipSuccess ||
        ch->d_out.ensure(64) != hipSuccess || hipMemset((char *)ch->d_plain.p + plain_cap, 0, 64) != hipSuccess) {
        ctx->fail(TS_ERR_ALLOC, "ts_bam_chunk_create: device allocation failed");
        delete ch;
        return nullptr;
    }
    return ch;
}

void ts_bam_chunk_destroy(ts_bam_chunk *ch) {
    if (!ch) return;
    DeviceGuard guard(ch->ctx->device);
    (void)hipDeviceSynchronize();
    delete ch;
}

uint64_t ts_bam_chunk_size(const ts_bam_chunk *ch) { return ch ? ch->plain_n : 0; }

int ts_bam_chunk_read(ts_bam_chunk *ch, uint64_t off, uint64_t n, void *host) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && !host) || off > ch->plain_n || n > ch->plain_n - off) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_read: outside the chunk");
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (n) HIP_TRY(ctx, hipMemcpy(host, (const char *)ch->d_plain.p + off, (size_t)n, hipMemcpyDeviceToHost));
    return TS_OK;
}

void *ts_bam_chunk_pass_buffer(ts_bam_chunk *ch, uint64_t n) {
    if (!ch || n > (1ull << 40)) return nullptr;
    ts_ctx *ctx = ch->ctx;
    DeviceGuard guard(ctx->device);
    if (guard.error() != hipSuccess || hipDeviceSynchronize() != hipSuccess || ch->d_pass.ensure((size_t)n) != hipSuccess) {
        ctx->fail(TS_ERR_ALLOC, "ts_bam_chunk_pass_buffer: device allocation failed");
        return nullptr;
    }
    return ch->d_pass.p;
}

const void *ts_chunk_data(const ts_chunk *ch) { return ch ? ch->d_plain.p : nullptr; }

int ts_chunk_reserve(ts_chunk *ch, uint64_t plain_cap) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (plain_cap > (1ull << 40)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_chunk_reserve: capacity out of range");
    if (plain_cap <= ch->plain_cap) return TS_OK;
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, hipDeviceSynchronize());
    const uint64_t cap = std::max<uint64_t>(plain_cap, ch->plain_cap + ch->plain_cap / 2);
    DevBuf grown;
    if (grown.ensure((size_t)cap + 64) != hipSuccess) return ctx->fail(TS_ERR_ALLOC, "ts_chunk_reserve: device allocation failed");
    if (ch->plain_n) HIP_TRY(ctx, hipMemcpy(grown.p, ch->d_plain.p, (size_t)ch->plain_n, hipMemcpyDeviceToDevice));
    HIP_TRY(ctx, hipMemset((char *)grown.p + cap, 0, 64));     // (the kernels read whole aligned words behind the last byte)
    ch->d_plain = std::move(grown);
    ch->plain_cap = cap;
    return TS_OK;
}

int ts_chunk_upload(ts_chunk *ch, const void *bytes, uint64_t n, uint64_t carry_from, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && !bytes) || n > (1ull << 40) || carry_from > ch->plain_n)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_chunk_upload: null or out-of-range argument");
    const uint64_t tail = ch->plain_n - carry_from;
    if (tail + n > ch->plain_cap) { const int rc = ts_chunk_reserve(ch, tail + n); if (rc != TS_OK) return rc; }
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    uint64_t carry = 0;
    { const int rc = ts_chunk_carry(ch, carry_from, st, &carry); if (rc != TS_OK) return rc; }
    if (n) HIP_TRY(ctx, hipMemcpyAsync((char *)ch->d_plain.p + carry, bytes, (size_t)n, hipMemcpyHostToDevice, st));
    ch->plain_n = carry + n;
    ch->n_blocks = 0;
    HIP_TRY(ctx, hipStreamSynchronize(st));                    // (the bytes are the caller's memory: they have left it when this returns)
    return TS_OK;
}

int ts_chunk_carry_over(ts_chunk *to, ts_chunk *from, uint64_t carry_from, void *stream) {
    if (!to) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = to->ctx;
    if (!from || from == to || from->ctx->device == kNoDevice || carry_from > from->plain_n)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_chunk_carry_over: needs two chunks on devices and an offset inside the source");
    const uint64_t n = from->plain_n - carry_from;
    to->plain_n = 0;                                           // (what the destination held is dropped, not kept by a growth)
    to->n_blocks = 0;
    to->lines.valid = false;
    if (n > to->plain_cap) { const int rc = ts_chunk_reserve(to, n); if (rc != TS_OK) return rc; }
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    const char *src = (const char *)from->d_plain.p + carry_from;
    const int dev_to = ctx->device, dev_from = from->ctx->device;
    if (n && dev_from == dev_to) {                             // one GPU, whichever contexts: device to device
        HIP_TRY(ctx, hipMemcpyAsync(to->d_plain.p, src, (size_t)n, hipMemcpyDeviceToDevice, st));
    } else if (n) {
        // two GPUs: what the source's device still has in flight for these bytes is waited for there, then a peer copy where the
        // destination's device can reach the source's memory, else the bytes bounce through host memory
        { DeviceGuard other(dev_from); HIP_TRY(ctx, other.error()); HIP_TRY(ctx, hipDeviceSynchronize()); }
        int peer = 0;
        HIP_TRY(ctx, hipDeviceCanAccessPeer(&peer, dev_to, dev_from));
        if (peer) HIP_TRY(ctx, hipMemcpyPeerAsync(to->d_plain.p, dev_to, src, dev_from, (size_t)n, st));
        else {
            std::vector<char> bounce((size_t)n);
            HIP_TRY(ctx, hipMemcpy(bounce.data(), src, (size_t)n, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpyAsync(to->d_plain.p, bounce.data(), (size_t)n, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));            // (the bounce buffer ends with this scope)
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    to->plain_n = n;
    return TS_OK;
}

int ts_chunk_stage_upload(ts_chunk *ch, const void *bytes, uint64_t n, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && !bytes) || n > (1ull << 40)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_chunk_stage_upload: null or out-of-range argument");
    { const int rc = ts_chunk_stage_reserve(ch, ch->stage_n + n); if (rc != TS_OK) return rc; }
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    if (n) HIP_TRY(ctx, hipMemcpyAsync((char *)ch->d_stage.p + ch->stage_n, bytes, (size_t)n, hipMemcpyHostToDevice, st));
    ch->stage_n += n;
    ch->n_blocks = 0;
    HIP_TRY(ctx, hipStreamSynchronize(st));                    // (the bytes are the caller's memory: they have left it when this returns)
    return TS_OK;
}

uint64_t ts_chunk_staged(const ts_chunk *ch) { return ch ? ch->stage_n : 0; }

int ts_chunk_commit(ts_chunk *ch, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    const uint64_t n = ch->stage_n;
    if (ch->plain_n + n > ch->plain_cap) { const int rc = ts_chunk_reserve(ch, ch->plain_n + n); if (rc != TS_OK) return rc; }
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    // (the chunk's first byte stays where every kernel expects it; the staged bytes land wherever the carry ends)
    if (n) HIP_TRY(ctx, hipMemcpyAsync((char *)ch->d_plain.p + ch->plain_n, ch->d_stage.p, (size_t)n, hipMemcpyDeviceToDevice, st));
    ch->plain_n += n;
    ch->stage_n = 0;
    ch->lines.valid = false;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return TS_OK;
}

}  // extern "C"
