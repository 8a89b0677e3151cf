// read_fastq.cpp — host side of the FASTQ-out gathers (read_fastq.hip): ts_bam_chunk_gather_fastq, ts_sam_chunk_gather_fastq and
// ts_read_fastq_text_stats.  The rule of the text is include/teloscan.h's; its bytes are read_fastq_format_core.h's.
//
// Per call: the record table goes up, ts_read_fastq_sizes and ts_read_fastq_plan say where every kept record's text starts and
// how many pieces it is cut into, three words come back and are held against cap, ts_read_fastq_jobs and ts_read_fastq_write
// format, one copy brings the text down.  Nothing here reads or prints a byte of a record.
#include <cstddef>

#include "chunk_internal.h"
#include "read_fastq_internal.h"

static_assert(sizeof(tsfq::Rec) == 40 && sizeof(TsFastqOutJob) == 8 && sizeof(ts_sam_record) == 24 && sizeof(ts_bam_record) == 24, "layouts");
static_assert(offsetof(ts_sam_record, seq_at) == 8 && offsetof(ts_sam_record, seq_len) == 12 && offsetof(ts_sam_record, size) == 16 &&
              offsetof(ts_bam_record, block_size) == 8 && offsetof(ts_bam_record, seq_at) == 12 && offsetof(ts_bam_record, l_seq) == 16,
              "read_fastq.hip reads the record tables by these offsets");
static_assert(TS_FASTQ_OUT_RESTORE_STRAND == tsfq::kRestoreStrand, "the flag is the header's");

namespace {

int gather_fastq(ts_bam_chunk *ch, const char *who, const void *recs, size_t rec_bytes, size_t n, uint32_t kind, const void *d_pass, uint32_t flags,
                 void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream) {
    ts_ctx *ctx = ch->ctx;
    const std::string name = who;
    *bytes = 0; *n_passed = 0;
    if (n == 0) return TS_OK;
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    ts_bam_chunk::FastqOut &F = ch->fastq_out;
    HIP_TRY(ctx, ch->d_recs.ensure(n * rec_bytes));
    HIP_TRY(ctx, ch->d_dst.ensure(n * 8));
    HIP_TRY(ctx, F.d_table.ensure(n * sizeof(tsfq::Rec)));
    HIP_TRY(ctx, F.d_sizes.ensure(n * 8));
    HIP_TRY(ctx, F.d_job_base.ensure(n * 4));
    HIP_TRY(ctx, hipMemcpyAsync(ch->d_recs.p, recs, n * rec_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                      // (the table is the caller's memory)
    TsFastqOutParams K{};
    K.recs = ch->d_recs.p; K.pass = (const unsigned char *)d_pass; K.chunk = (const unsigned char *)ch->d_plain.p;
    K.table = (tsfq::Rec *)F.d_table.p; K.sizes = (unsigned long long *)F.d_sizes.p; K.dst_off = (unsigned long long *)ch->d_dst.p;
    K.job_base = (uint32_t *)F.d_job_base.p;
    K.totals = (unsigned long long *)ch->d_out.p + 4;
    K.n = (uint32_t)n; K.kind = kind; K.out_flags = flags;
    static_assert(4 + kFqWords <= 8, "the result block has 64 bytes");
    if (ts_k_launch_read_fastq_plan(&K, stream) != 0) return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    unsigned long long t[kFqWords];
    HIP_TRY(ctx, hipMemcpyAsync(t, K.totals, sizeof t, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *bytes = t[kFqBytes]; *n_passed = t[kFqKept];
    if (t[kFqBytes] > cap) return ctx->fail(TS_ERR_INVALID_ARG, name + ": host_out is too small (*bytes says what is needed)");
    if (t[kFqBytes] == 0) return TS_OK;
    if (t[kFqJobs] > 0x7fffffffull) return ctx->fail(TS_ERR_UNSUPPORTED, name + ": too much text for one call");
    HIP_TRY(ctx, ch->d_gather.ensure((size_t)t[kFqBytes]));
    HIP_TRY(ctx, F.d_jobs.ensure((size_t)t[kFqJobs] * sizeof(TsFastqOutJob)));
    K.jobs = (TsFastqOutJob *)F.d_jobs.p; K.n_jobs = (uint32_t)t[kFqJobs];
    K.out = (unsigned char *)ch->d_gather.p; K.cap = t[kFqBytes];
    if (ts_k_launch_read_fastq_write(&K, stream) != 0) return ctx->fail(TS_ERR_HIP, name + ": kernel launch failed");
    HIP_TRY(ctx, hipMemcpyAsync(host_out, ch->d_gather.p, (size_t)t[kFqBytes], hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->read_fastq_text_stats[0] += 1; ctx->read_fastq_text_stats[1] += t[kFqKept]; ctx->read_fastq_text_stats[2] += t[kFqBytes];
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_bam_chunk_gather_fastq(ts_bam_chunk *ch, const ts_bam_record *recs, size_t n, const void *d_pass, uint32_t flags, void *host_out,
                              uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull || (flags & ~TS_FASTQ_OUT_RESTORE_STRAND))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_gather_fastq: null or out-of-range argument, or an unknown flag");
    for (size_t i = 0; i < n; ++i) {
        const ts_bam_record &r = recs[i];
        // (the fixed fields, the name's first byte, SEQ and QUAL lie inside the record, the record inside the chunk)
        const bool ok = r.block_size >= 33u && r.block_size <= (256u << 20) && r.off <= ch->plain_n && 4ull + r.block_size <= ch->plain_n - r.off &&
                        r.l_seq <= 0x7fffffffu && (uint64_t)r.seq_at + ((uint64_t)r.l_seq + 1) / 2 + r.l_seq <= 4ull + r.block_size;
        if (!ok) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_gather_fastq: record " + std::to_string(i) + " does not fit the chunk");
    }
    return gather_fastq(ch, "ts_bam_chunk_gather_fastq", recs, sizeof *recs, n, tsfq::kBam, d_pass, flags, host_out, cap, bytes, n_passed, stream);
}

int ts_sam_chunk_gather_fastq(ts_chunk *ch, const ts_sam_record *recs, size_t n, const void *d_pass, uint32_t flags, void *host_out,
                              uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull || (flags & ~TS_FASTQ_OUT_RESTORE_STRAND))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_gather_fastq: null or out-of-range argument, or an unknown flag");
    for (size_t i = 0; i < n; ++i) {
        const ts_sam_record &r = recs[i];
        if (r.off > ch->plain_n || r.size > ch->plain_n - r.off || r.flags > 1 || (uint64_t)r.seq_at + r.seq_len > r.size)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_sam_chunk_gather_fastq: record " + std::to_string(i) + " does not fit the chunk");
    }
    return gather_fastq(ch, "ts_sam_chunk_gather_fastq", recs, sizeof *recs, n, tsfq::kSam, d_pass, flags, host_out, cap, bytes, n_passed, stream);
}

int ts_read_fastq_text_stats(const ts_ctx *ctx, uint64_t out[3]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i) out[i] = ctx->read_fastq_text_stats[i].load();
    return TS_OK;
}

}  // extern "C"
