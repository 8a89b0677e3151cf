// fastq.cpp — host side of the device FASTQ route (include/teloscan.h: ts_chunk_*, ts_fastq_chunk_*): argument checks, buffer
// sizes, launches and the few words that come back.  The chunk is bgzf.cpp's ts_bam_chunk; nothing here parses a byte of text.
#include "capi_internal.hpp"
#include "fastq_internal.h"

namespace {

static_assert(sizeof(ts_fastq_record) == 24 && sizeof(FastqCopyJob) == 24 && sizeof(FastqFrame) == 32 && sizeof(FastqEntry) == 8, "layouts");

// a record of the table against the chunk: inside it, the sequence line inside the record
bool record_ok(const ts_bam_chunk *ch, const ts_fastq_record &r) {
    if (r.off > ch->plain_n || r.size > ch->plain_n - r.off) return false;
    return r.seq_cr <= 1 && r.seq_cr <= r.seq_len && (uint64_t)r.seq_at + r.seq_len <= r.size;
}

}  // namespace

int ts_chunk_line_index(ts_bam_chunk *ch, int at_end, const char *who, const char *counted, FastqLineIndex *ix) {
    ts_ctx *ctx = ch->ctx;
    const std::string name = who;
    const uint64_t size = ch->plain_n;
    unsigned long long *d_out = (unsigned long long *)ch->d_out.p;
    ch->gfa_walked = false;                                    // (ts_gfa_chunk_check reads the index of the GFA walk that made it)
    HIP_TRY(ctx, ch->d_waves.ensure((size_t)ceil_div(size, kFastqSliceBytes) * 4));
    if (ts_k_launch_fastq_count(ch->d_plain.p, size, (uint32_t *)ch->d_waves.p, d_out, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    unsigned long long out[2];
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    const uint64_t newlines = out[kFqNewlines], tail = out[kFqTail];
    if (newlines > size || tail > 1) return ctx->fail(TS_ERR_STATE, name + ": the " + counted + " count left the chunk");
    const uint64_t slots = newlines + 2;
    HIP_TRY(ctx, ch->d_lines.ensure((size_t)slots * 6));
    ix->newlines = newlines; ix->tail = tail; ix->n_lines = newlines + (at_end ? tail : 0);
    ix->lstart = (uint32_t *)ch->d_lines.p;
    ix->first = (unsigned char *)ch->d_lines.p + slots * 4; ix->cr = ix->first + slots;
    if (ts_k_launch_fastq_index(ch->d_plain.p, size, (const uint32_t *)ch->d_waves.p, (uint32_t)newlines, (uint32_t)tail, ix->lstart, ix->first,
                                ix->cr, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    return TS_OK;
}

extern "C" {

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

int ts_fastq_chunk_walk(ts_chunk *ch, int at_end, ts_fastq_record *recs, uint64_t cap, uint64_t *n, uint64_t *next, int *error,
                        uint64_t *error_record, uint64_t *error_off) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n || !next || !error || !error_record || !error_off || (cap && !recs) || cap > (1ull << 31))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_walk: null or out-of-range argument");
    if (ch->plain_n >= 0xffffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_walk: the chunk holds 4 GiB or more");
    *n = 0; *next = 0; *error = TS_FASTQ_OK; *error_record = 0; *error_off = 0;
    const uint64_t size = ch->plain_n;
    if (size == 0) return TS_OK;
    DEVICE_TRY(ctx);
    unsigned long long *d_out = (unsigned long long *)ch->d_out.p;
    unsigned long long out[kFqWords];
    static_assert(sizeof out <= 64, "the chunk's result block has 64 bytes");

    // lines: '\n' per slice, their sums, every line's start
    FastqLineIndex ix;
    { const int rc = ts_chunk_line_index(ch, at_end, "ts_fastq_chunk_walk", "line", &ix); if (rc != TS_OK) return rc; }
    const uint64_t newlines = ix.newlines, n_lines = ix.n_lines;
    uint32_t *lstart = ix.lstart;
    unsigned char *first = ix.first, *cr = ix.cr;

    // records: the slices' maps and header counts, their scan, the table
    const uint64_t n_frames = ceil_div(n_lines, kFastqSliceLines);
    HIP_TRY(ctx, ch->d_frames.ensure((size_t)std::max<uint64_t>(n_frames, 1) * (sizeof(FastqFrame) + sizeof(FastqEntry))));
    void *frames = ch->d_frames.p, *entries = (char *)ch->d_frames.p + std::max<uint64_t>(n_frames, 1) * sizeof(FastqFrame);
    if (ts_k_launch_fastq_frames(lstart, cr, (uint32_t)n_lines, (uint32_t)newlines, frames, entries, d_out, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fastq_chunk_walk: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    const uint64_t headers = out[kFqHeaders];
    if (headers > n_lines) return ctx->fail(TS_ERR_STATE, "ts_fastq_chunk_walk: more records than lines");
    HIP_TRY(ctx, ch->d_recs.ensure((size_t)std::max<uint64_t>(headers, 1) * sizeof(ts_fastq_record)));
    if (ts_k_launch_fastq_records(lstart, first, cr, (uint32_t)n_lines, at_end, entries, ch->d_recs.p, d_out, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fastq_chunk_walk: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));

    const bool open = out[kFqOpen] != 0;
    uint64_t whole = headers - (open ? 1 : 0);
    if (out[kFqOpenOff] > size || out[kFqLastLine] > size || (open && headers == 0))
        return ctx->fail(TS_ERR_STATE, "ts_fastq_chunk_walk: the walk left the chunk");
    *next = open ? out[kFqOpenOff] : at_end ? size : out[kFqLastLine];
    if (out[kFqError] != ~0ull) {
        const uint64_t bad = out[kFqError] >> 3;
        if (bad > whole) return ctx->fail(TS_ERR_STATE, "ts_fastq_chunk_walk: the error lies behind the records");
        *error = (int)(out[kFqError] & 7u);
        *error_record = bad;
        if (*error == TS_FASTQ_TRUNCATED) *error_off = out[kFqOpenOff];
        else {
            ts_fastq_record r;
            HIP_TRY(ctx, hipMemcpy(&r, (const ts_fastq_record *)ch->d_recs.p + bad, sizeof r, hipMemcpyDeviceToHost));
            *error_off = r.off;
        }
        whole = bad;
        *next = *error_off;
    }
    *n = whole;
    const uint64_t take = std::min(whole, cap);
    if (take) HIP_TRY(ctx, hipMemcpy(recs, ch->d_recs.p, (size_t)take * sizeof(ts_fastq_record), hipMemcpyDeviceToHost));
    if (whole > cap) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_walk: the table is too small (*n says what is needed)");
    return TS_OK;
}

int ts_fastq_chunk_stage(ts_chunk *ch, const ts_fastq_record *recs, size_t n, ts_batch *reads, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!reads || (n && !recs) || reads->ctx != ctx || !reads->tips || !reads->whole() || reads->segs.size() != n)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_stage: needs an unrestricted tips-only batch of this context with one segment per record");
    std::vector<FastqCopyJob> jobs;
    for (size_t i = 0; i < n; ++i) {
        const ts_fastq_record &r = recs[i];
        const uint32_t bases = r.seq_len - r.seq_cr;
        if (!record_ok(ch, r) || bases == 0 || reads->segs[i].len != bases)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_stage: record " + std::to_string(i) + " does not fit the chunk or its segment");
        const uint64_t dst = ts_batch_segment_offset(reads, i);
        for (uint32_t a = 0; a < bases; a += kFastqStagePiece)
            jobs.push_back(FastqCopyJob{r.off + r.seq_at + a, dst + a, std::min(kFastqStagePiece, bases - a), 0});
    }
    if (jobs.size() > 0x7fffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_stage: too many bases for one call");
    DEVICE_TRY(ctx);
    const bool fresh = reads->d_in.p == nullptr;
    void *in = ts_batch_input_ptr(reads);
    if (!in) return ctx->fail(TS_ERR_ALLOC, "ts_fastq_chunk_stage: no input buffer");
    if (jobs.empty()) return TS_OK;
    hipStream_t st = (hipStream_t)stream;
    // (a fresh input buffer was just zeroed on the null stream, which a non-blocking `stream` does not wait for)
    if (fresh && st) HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    HIP_TRY(ctx, ch->d_jobs.ensure(jobs.size() * sizeof(FastqCopyJob)));
    HIP_TRY(ctx, hipMemcpyAsync(ch->d_jobs.p, jobs.data(), jobs.size() * sizeof(FastqCopyJob), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ts_k_launch_fastq_stage(ch->d_plain.p, ch->d_jobs.p, (uint32_t)jobs.size(), in, stream) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fastq_chunk_stage: kernel launch failed");
    return TS_OK;
}

int ts_fastq_chunk_gather(ts_chunk *ch, const ts_fastq_record *recs, size_t n, const void *d_pass, void *host_out, uint64_t cap,
                          uint64_t *bytes, uint64_t *n_passed, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_gather: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i)
        if (!record_ok(ch, recs[i])) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_gather: record " + std::to_string(i) + " does not fit the chunk");
    *bytes = 0; *n_passed = 0;
    if (n == 0) return TS_OK;
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, ch->d_recs.ensure(n * sizeof(ts_fastq_record)));
    HIP_TRY(ctx, ch->d_dst.ensure(n * 8));
    HIP_TRY(ctx, hipMemcpyAsync(ch->d_recs.p, recs, n * sizeof(ts_fastq_record), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    unsigned long long *totals = (unsigned long long *)ch->d_out.p + 4;
    if (ts_k_launch_fastq_gather_plan(ch->d_recs.p, d_pass, n, ch->d_dst.p, totals, stream) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fastq_chunk_gather: kernel launch failed");
    unsigned long long t[2];
    HIP_TRY(ctx, hipMemcpyAsync(t, totals, sizeof t, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *bytes = t[0]; *n_passed = t[1];
    if (t[0] > cap) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_gather: host_out is too small (*bytes says what is needed)");
    if (t[0] == 0) return TS_OK;
    HIP_TRY(ctx, ch->d_gather.ensure((size_t)t[0]));
    if (ts_k_launch_fastq_gather(ch->d_plain.p, ch->d_recs.p, ch->d_dst.p, n, t[0], ch->d_gather.p, stream) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fastq_chunk_gather: kernel launch failed");
    HIP_TRY(ctx, hipMemcpyAsync(host_out, ch->d_gather.p, (size_t)t[0], hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return TS_OK;
}

}  // extern "C"
