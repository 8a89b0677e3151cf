// read_blocks.cpp — host side of the read block report's device formatter (read_blocks.hip): ts_fastq_chunk_block_lines,
// ts_sam_chunk_block_lines, ts_fasta_chunk_block_lines, ts_bam_chunk_block_lines, ts_read_block_lines_format and ts_read_block_text_stats.  The rule of the
// report is include/teloscan.h's; its bytes are read_block_format_core.h's.
//
// Per call: the rows lie where ts_batch_call_read_blocks left them (or go up), a name entry per segment is made from the chunk's
// record table (or goes up), ts_read_block_count says how many bytes every 64 rows give, a prefix sum places them,
// ts_read_block_write formats, one copy brings the text down.  Nothing here parses or prints a byte of text.
#include "chunk_internal.h"
#include "read_block_format_core.h"

static_assert(sizeof(TsReadBlockSeg) == 16 && sizeof(ts_fastq_record) == 24 && sizeof(ts_sam_record) == 24 && sizeof(ts_bam_record) == 24 &&
              sizeof(ts_fasta_record) == 32, "layouts");
static_assert(offsetof(ts_fastq_record, seq_at) == 8 && offsetof(ts_fastq_record, seq_len) == 12 && offsetof(ts_fastq_record, seq_cr) == 20 &&
              offsetof(ts_sam_record, seq_at) == 8 && offsetof(ts_sam_record, seq_len) == 12 && offsetof(ts_bam_record, block_size) == 8 &&
              offsetof(ts_bam_record, l_seq) == 16 && offsetof(ts_fasta_record, n_bases) == 16 && offsetof(ts_fasta_record, name_len) == 24,
              "read_blocks.hip reads the record tables by these offsets");

namespace {

struct TextBufs { DevBuf *sums, *text; };

// The lines of n_rows rows at d_rows to host_out: *bytes of them; more than cap: nothing is copied.  Synchronous on st.
int format_rows(ts_ctx *c, const char *who, const TsReadBlockRow *d_rows, uint64_t n_rows, const TsReadBlockSeg *d_segs, uint32_t n_segs,
                const void *d_names, const TextBufs &B, void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_lines, hipStream_t st) {
    const std::string name = who;
    *bytes = 0; *n_lines = 0;
    if (!n_rows) return TS_OK;
    if (n_rows > (0x7FFFFFFFull << 6)) return c->fail(TS_ERR_UNSUPPORTED, name + ": too many rows for one call");
    const uint32_t n_blocks = (uint32_t)ceil_div(n_rows, 64);
    HIP_TRY(c, B.sums->ensure(((size_t)n_blocks + 1) * 16));
    TsReadBlockTextParams K{};
    K.rows = d_rows; K.segs = d_segs; K.names = d_names;
    K.sums = (unsigned long long *)B.sums->p;
    K.n_rows = n_rows; K.n_segs = n_segs;
    if (ts_k_launch_read_block_count(&K, n_blocks, st) != 0) return c->fail(TS_ERR_HIP, name + ": count launch failed");
    unsigned long long total = 0, lines = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, K.sums + n_blocks, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&lines, K.sums + 2 * (size_t)n_blocks + 1, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    *bytes = total; *n_lines = lines;
    if (total > cap) return c->fail(TS_ERR_INVALID_ARG, name + ": the text does not fit (*bytes says what is needed)");
    if (total) {
        HIP_TRY(c, B.text->ensure((size_t)total + 16));
        K.out = B.text->p;
        if (ts_k_launch_read_block_write(&K, n_blocks, st) != 0) return c->fail(TS_ERR_HIP, name + ": write launch failed");
        HIP_TRY(c, hipMemcpyAsync(host_out, B.text->p, (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    c->read_block_text_stats[0] += 1; c->read_block_text_stats[1] += lines; c->read_block_text_stats[2] += total;
    return TS_OK;
}

// A *_block_lines call behind its record checks: the table goes up, the name entries are made where the chunk lies, the batch's
// rows are settled and formatted.
int chunk_block_lines(ts_bam_chunk *ch, const char *who, const void *recs, size_t rec_bytes, size_t n, uint32_t kind, ts_batch *reads,
                      void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_lines, void *stream) {
    ts_ctx *ctx = ch->ctx;
    const std::string name = who;
    *bytes = 0; *n_lines = 0;
    if (reads->ctx != ctx || !reads->tips || reads->segs.size() != n)
        return ctx->fail(TS_ERR_INVALID_ARG, name + ": needs the tips-only batch of this context that the records were staged into");
    DEVICE_TRY(ctx);
    uint64_t n_rows = 0;
    { const int rc = ts_batch_settle_read_blocks(reads, &n_rows); if (rc != TS_OK) return rc; }
    if (!n_rows) return TS_OK;
    hipStream_t st = (hipStream_t)stream;
    ts_bam_chunk::Blocks &B = ch->blocks;
    HIP_TRY(ctx, B.d_recs.ensure(n * rec_bytes));
    HIP_TRY(ctx, B.d_segs.ensure(n * sizeof(TsReadBlockSeg)));
    HIP_TRY(ctx, hipMemcpyAsync(B.d_recs.p, recs, n * rec_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                      // (the table is the caller's memory)
    if (ts_k_launch_read_block_names(B.d_recs.p, (uint32_t)n, kind, ch->d_plain.p, (TsReadBlockSeg *)B.d_segs.p, stream) != 0)
        return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    const int rc = format_rows(ctx, who, (const TsReadBlockRow *)reads->rb.d_rows.p, n_rows, (const TsReadBlockSeg *)B.d_segs.p, (uint32_t)n,
                               ch->d_plain.p, TextBufs{&B.d_sums, &B.d_text}, host_out, cap, bytes, n_lines, st);
    return rc;
}

}  // namespace

extern "C" {

int ts_fastq_chunk_block_lines(ts_chunk *ch, const ts_fastq_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                               uint64_t *bytes, uint64_t *n_lines, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!reads || !bytes || !n_lines || (n && !recs) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_block_lines: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i) {
        const ts_fastq_record &r = recs[i];
        if (r.off > ch->plain_n || r.size > ch->plain_n - r.off || r.seq_at < 2 || r.seq_at > r.size || r.seq_cr > r.seq_len)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_fastq_chunk_block_lines: record " + std::to_string(i) + " does not fit the chunk");
        // (a name is at most its header line: the device's 32-bit line lengths are made for names of up to 16 MiB, as text_check_segment says)
        if (r.seq_at > TS_TRACK_MAX_NAME)
            return ctx->fail(TS_ERR_UNSUPPORTED, "ts_fastq_chunk_block_lines: record " + std::to_string(i) + ": a header line of more than 16 MiB (2^24 bytes) is not formatted on the device");
    }
    return chunk_block_lines(ch, "ts_fastq_chunk_block_lines", recs, sizeof *recs, n, TS_READ_BLOCK_FASTQ, reads, host_out, cap, bytes, n_lines, stream);
}

int ts_sam_chunk_block_lines(ts_chunk *ch, const ts_sam_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                             uint64_t *bytes, uint64_t *n_lines, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!reads || !bytes || !n_lines || (n && !recs) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_block_lines: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i) {
        const ts_sam_record &r = recs[i];
        if (r.off > ch->plain_n || r.size > ch->plain_n - r.off || r.seq_at > r.size)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_block_lines: record " + std::to_string(i) + " does not fit the chunk");
        if (r.seq_at > TS_TRACK_MAX_NAME)
            return ctx->fail(TS_ERR_UNSUPPORTED, "ts_sam_chunk_block_lines: record " + std::to_string(i) + ": more than 16 MiB (2^24 bytes) in front of SEQ are not formatted on the device");
    }
    return chunk_block_lines(ch, "ts_sam_chunk_block_lines", recs, sizeof *recs, n, TS_READ_BLOCK_SAM, reads, host_out, cap, bytes, n_lines, stream);
}

int ts_fasta_chunk_block_lines(ts_chunk *ch, const ts_fasta_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                               uint64_t *bytes, uint64_t *n_lines, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!reads || !bytes || !n_lines || (n && !recs) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_block_lines: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i) {
        const ts_fasta_record &r = recs[i];
        // ('>' and the header line's name_len bytes lie inside the record's text)
        if (r.off > ch->plain_n || r.text_len > ch->plain_n - r.off || r.name_len >= r.text_len)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_block_lines: record " + std::to_string(i) + " does not fit the chunk");
        if (r.name_len > TS_TRACK_MAX_NAME)
            return ctx->fail(TS_ERR_UNSUPPORTED, "ts_fasta_chunk_block_lines: record " + std::to_string(i) + ": a header line of more than 16 MiB (2^24 bytes) is not formatted on the device");
    }
    return chunk_block_lines(ch, "ts_fasta_chunk_block_lines", recs, sizeof *recs, n, TS_READ_BLOCK_FASTA, reads, host_out, cap, bytes, n_lines, stream);
}

int ts_bam_chunk_block_lines(ts_bam_chunk *ch, const ts_bam_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                             uint64_t *bytes, uint64_t *n_lines, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!reads || !bytes || !n_lines || (n && !recs) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_block_lines: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i) {
        const ts_bam_record &r = recs[i];
        // (the fixed fields and the name's first byte lie inside the record; the kernel cuts the name at the record's end)
        if (r.off > ch->plain_n || r.block_size < 33 || (uint64_t)r.block_size + 4 > ch->plain_n - r.off)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_block_lines: record " + std::to_string(i) + " does not fit the chunk");
    }
    return chunk_block_lines(ch, "ts_bam_chunk_block_lines", recs, sizeof *recs, n, TS_READ_BLOCK_BAM, reads, host_out, cap, bytes, n_lines, stream);
}

int ts_read_block_lines_format(ts_ctx *ctx, const ts_read_block *rows, uint64_t n_rows, const uint64_t *name_off, const uint32_t *name_len,
                               const uint32_t *read_len, const char *names, uint64_t names_len, void *out, uint64_t cap, uint64_t *bytes) {
    if (!ctx || !bytes || (n_rows && (!rows || !name_off || !name_len || !read_len)) || (names_len && !names) || (cap && !out))
        return TS_ERR_INVALID_ARG;
    ts_ctx *c = ctx;
    *bytes = 0;
    DEVICE_TRY(c);
    int rc = ts_pipeline_ensure_streams(c);
    if (rc != TS_OK) return rc;
    if (!n_rows) return TS_OK;
    uint64_t n_segs = 0;
    for (uint64_t i = 0; i < n_rows; ++i) n_segs = std::max<uint64_t>(n_segs, (uint64_t)rows[i].segment + 1);
    if (n_segs > 0x7fffffffull) return c->fail(TS_ERR_INVALID_ARG, "ts_read_block_lines_format: a row's segment is out of range");
    std::vector<TsReadBlockSeg> segs((size_t)n_segs);
    for (uint64_t s = 0; s < n_segs; ++s) segs[s] = TsReadBlockSeg{name_off[s], name_len[s], read_len[s]};
    for (uint64_t i = 0; i < n_rows; ++i) {
        const TsReadBlockSeg &s = segs[rows[i].segment];
        if (s.name_off > names_len || s.name_len > names_len - s.name_off)
            return c->fail(TS_ERR_INVALID_ARG, "ts_read_block_lines_format: row " + std::to_string(i) + ": its segment's name lies outside the names");
        if (s.name_len > TS_TRACK_MAX_NAME)
            return c->fail(TS_ERR_UNSUPPORTED, "ts_read_block_lines_format: a name of more than 16 MiB (2^24 bytes) is not formatted on the device");
    }
    hipStream_t st = c->down_stream;
    uint64_t n_lines = 0;
    DevBuf d_rows, d_segs, d_names, d_sums, d_text;
    std::lock_guard<std::mutex> dl(c->down_mtx);
    auto run = [&]() -> int {
        HIP_TRY(c, d_rows.ensure((size_t)n_rows * sizeof(TsReadBlockRow)));
        HIP_TRY(c, d_segs.ensure(segs.size() * sizeof(TsReadBlockSeg)));
        HIP_TRY(c, d_names.ensure((size_t)names_len + 16));
        HIP_TRY(c, hipMemcpyAsync(d_rows.p, rows, (size_t)n_rows * sizeof(TsReadBlockRow), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(TsReadBlockSeg), hipMemcpyHostToDevice, st));
        if (names_len) HIP_TRY(c, hipMemcpyAsync(d_names.p, names, (size_t)names_len, hipMemcpyHostToDevice, st));
        return format_rows(c, "ts_read_block_lines_format", (const TsReadBlockRow *)d_rows.p, n_rows, (const TsReadBlockSeg *)d_segs.p, (uint32_t)n_segs,
                           d_names.p, TextBufs{&d_sums, &d_text}, out, cap, bytes, &n_lines, st);
    };
    rc = run();
    (void)hipStreamSynchronize(st);
    return rc;
}

int ts_read_block_text_stats(const ts_ctx *ctx, uint64_t out[3]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i) out[i] = ctx->read_block_text_stats[i].load();
    return TS_OK;
}

}  // extern "C"
