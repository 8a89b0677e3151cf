// fastq.cpp — host side of the device FASTQ route (include/teloscan.h: ts_fastq_chunk_*): argument checks, buffer sizes,
// launches and the few words that come back.  The chunk, its line index and the gather's host half are the chunk layer's
// (chunk_internal.h); nothing here parses a byte of text.
#include "fastq_internal.h"

namespace {

static_assert(sizeof(ts_fastq_record) == 24 && sizeof(FastqCopyJob) == 24 && sizeof(FastqFrame) == 32 && sizeof(FastqEntry) == 8, "layouts");

// a record of the table against the chunk: inside it, the sequence line inside the record
bool record_ok(const ts_bam_chunk *ch, const ts_fastq_record &r) {
    if (r.off > ch->plain_n || r.size > ch->plain_n - r.off) return false;
    return r.seq_cr <= 1 && r.seq_cr <= r.seq_len && (uint64_t)r.seq_at + r.seq_len <= r.size;
}

}  // namespace

extern "C" {

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
    LineIndex ix;
    { const int rc = ts_chunk_line_index(ch, at_end, "ts_fastq_chunk_walk", "line", &ix); if (rc != TS_OK) return rc; }
    const uint64_t newlines = ix.newlines, n_lines = ix.n_lines;
    uint32_t *lstart = ix.lstart;
    unsigned char *first = ix.first, *cr = ix.cr;

    // records: the slices' maps and header counts, their scan, the table
    const uint64_t n_frames = ceil_div(n_lines, kFastqSliceLines);
    HIP_TRY(ctx, ch->fastq.d_frames.ensure((size_t)std::max<uint64_t>(n_frames, 1) * (sizeof(FastqFrame) + sizeof(FastqEntry))));
    void *frames = ch->fastq.d_frames.p, *entries = (char *)ch->fastq.d_frames.p + std::max<uint64_t>(n_frames, 1) * sizeof(FastqFrame);
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
    return ts_chunk_stage_records(ch, "ts_fastq_chunk_stage", recs, n, reads, stream, kFastqStagePiece, kFastqStagePiece,
                                  [](const ts_bam_chunk *c, const void *table, size_t i, uint64_t *src, uint32_t *len) {
                                      const ts_fastq_record &r = ((const ts_fastq_record *)table)[i];
                                      *src = (uint64_t)r.off + r.seq_at; *len = r.seq_len - r.seq_cr;
                                      return record_ok(c, r);
                                  }, ts_k_launch_fastq_stage);
}

int ts_fastq_chunk_gather(ts_chunk *ch, const ts_fastq_record *recs, size_t n, const void *d_pass, void *host_out, uint64_t cap,
                          uint64_t *bytes, uint64_t *n_passed, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_gather: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i)
        if (!record_ok(ch, recs[i])) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_gather: record " + std::to_string(i) + " does not fit the chunk");
    return ts_chunk_gather(ch, "ts_fastq_chunk_gather", recs, sizeof(ts_fastq_record), n, d_pass, host_out, cap, bytes, n_passed, stream,
                           ts_k_launch_chunk_gather_plan_fastq, ts_k_launch_fastq_gather);
}

int ts_fastq_chunk_mates(ts_chunk *ch, const ts_fastq_record *recs, size_t n, uint64_t *mismatch) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!mismatch || (n && !recs) || (n & 1u) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_mates: null or out-of-range argument, or an odd number of records");
    *mismatch = UINT64_MAX;
    if (n == 0) return TS_OK;
    // (the header line lies inside the record: every byte the kernel reads of it is the chunk's)
    for (size_t i = 0; i < n; ++i)
        if (!record_ok(ch, recs[i]) || recs[i].seq_at < 2) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_mates: record " + std::to_string(i) + " does not fit the chunk");
    DEVICE_TRY(ctx);
    unsigned long long *d_lowest = (unsigned long long *)ch->d_out.p;
    unsigned long long lowest = ~0ull;
    HIP_TRY(ctx, ch->d_recs.ensure(n * sizeof(ts_fastq_record)));
    HIP_TRY(ctx, hipMemcpy(ch->d_recs.p, recs, n * sizeof(ts_fastq_record), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_lowest, &lowest, sizeof lowest, hipMemcpyHostToDevice));
    if (ts_k_launch_fastq_mates(ch->d_plain.p, ch->plain_n, ch->d_recs.p, n / 2, d_lowest, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fastq_chunk_mates: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(&lowest, d_lowest, sizeof lowest, hipMemcpyDeviceToHost));
    if (lowest != ~0ull && lowest >= n / 2) return ctx->fail(TS_ERR_STATE, "ts_fastq_chunk_mates: the pair lies behind the records");
    *mismatch = lowest;
    return TS_OK;
}

int ts_fastq_chunk_pair_pass(ts_chunk *ch, size_t n, const uint32_t *read_of, const void *d_pass, void *d_pair_pass, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && (!read_of || !d_pass || !d_pair_pass)) || (n & 1u) || n > 0x7fffffffull || (n && d_pass == d_pair_pass))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_pair_pass: null, aliased or out-of-range argument, or an odd number of records");
    if (n == 0) return TS_OK;
    // (a record's index in d_pass lies in front of the judged reads' number, which is at most n)
    for (size_t i = 0; i < n; ++i)
        if (read_of[i] != 0xffffffffu && read_of[i] >= n) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_pair_pass: record " + std::to_string(i) + " points behind the judged reads");
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, ch->fastq.d_read_of.ensure(n * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemcpyAsync(ch->fastq.d_read_of.p, read_of, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                    // (read_of is the caller's memory: it has left it when this returns)
    if (ts_k_launch_fastq_pair_pass(ch->fastq.d_read_of.p, d_pass, n / 2, d_pair_pass, stream) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fastq_chunk_pair_pass: kernel launch failed");
    return TS_OK;
}

}  // extern "C"
