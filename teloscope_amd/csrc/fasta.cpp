// fasta.cpp — host side of the device FASTA stages (include/teloscan.h: ts_fasta_chunk_*): argument checks, buffer sizes, the
// job lists of the join, the read stage and the run search (a job per 16 KB of a record: arithmetic on the record table), launches
// and the few words that come back.  The read route's gather is the FASTQ route's kernel and chunk.hip's plan over the records'
// spans.  The chunk and its line index are the chunk layer's (chunk_internal.h); nothing here parses a byte of text.
#include "chunk_internal.h"
#include "fasta_internal.h"
#include "fastq_internal.h"

namespace {

static_assert(sizeof(ts_fasta_record) == 32 && sizeof(ts_fasta_run) == 16 && sizeof(FastaFrame) == 16 && sizeof(FastaHead) == 16 &&
              sizeof(FastaJoinJob) == 32 && sizeof(FastaRunJob) == 32 && sizeof(FastaStrictJob) == 16, "layouts");

// a record of the table against the chunk: inside it, the body inside the record, no more bases than body bytes
bool record_ok(const ts_bam_chunk *ch, const ts_fasta_record &r) {
    if (r.off > ch->plain_n || r.text_len > ch->plain_n - r.off) return false;
    return r.body_at <= r.text_len && r.n_bases <= r.text_len - r.body_at;
}

int ensure_out(ts_bam_chunk *ch) {
    if (ch->fasta.d_out.p) return TS_OK;
    ts_ctx *ctx = ch->ctx;
    HIP_TRY(ctx, ch->fasta.d_out.ensure(64));
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_fasta_chunk_walk(ts_chunk *ch, int at_end, ts_fasta_record *recs, uint64_t cap, uint64_t *n, uint64_t *next, char *names,
                        uint64_t names_cap, uint64_t *names_bytes) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n || !next || !names_bytes || (cap && !recs) || (names_cap && !names) || cap > (1ull << 31))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_walk: null or out-of-range argument");
    if (ch->plain_n >= 0xffffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_walk: the chunk holds 4 GiB or more");
    *n = 0; *next = 0; *names_bytes = 0;
    const uint64_t size = ch->plain_n;
    if (size == 0) return TS_OK;
    DEVICE_TRY(ctx);
    { const int rc = ensure_out(ch); if (rc != TS_OK) return rc; }
    unsigned long long *d_out = (unsigned long long *)ch->fasta.d_out.p;
    unsigned long long out[kFaWords];
    static_assert(sizeof out <= 64, "the result block has 64 bytes");

    // lines: the chunk's line index ('\n' per slice, their sums, every line's start, first byte and '\r')
    LineIndex ix;
    { const int rc = ts_chunk_line_index(ch, at_end, "ts_fasta_chunk_walk", "line", &ix); if (rc != TS_OK) return rc; }
    const uint64_t newlines = ix.newlines, n_lines = ix.n_lines;
    uint32_t *lstart = ix.lstart;
    unsigned char *first = ix.first, *cr = ix.cr;

    // header lines: per slice of lines, their sums, every header's place
    const uint64_t n_frames = ceil_div(n_lines, kFastaSliceLines);
    HIP_TRY(ctx, ch->fasta.d_frames.ensure((size_t)std::max<uint64_t>(n_frames, 1) * sizeof(FastaFrame)));
    if (ts_k_launch_fasta_frames(lstart, first, cr, (uint32_t)n_lines, (uint32_t)newlines, ch->fasta.d_frames.p, d_out, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fasta_chunk_walk: kernel launch failed");
    HIP_TRY(ctx, hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    const uint64_t heads = out[kFaHeaders], all_names = out[kFaNameBytes];
    if (heads > n_lines || out[kFaCrs] > n_lines || all_names > size || out[kFaLastLine] > size)
        return ctx->fail(TS_ERR_STATE, "ts_fasta_chunk_walk: the header count left the chunk");
    if (heads == 0) {                                          // no record begins here: whole lines without a '>' belong to none
        *next = at_end ? size : out[kFaLastLine];
        return TS_OK;
    }
    HIP_TRY(ctx, ch->fasta.d_heads.ensure((size_t)(heads + 1) * sizeof(FastaHead)));
    HIP_TRY(ctx, ch->fasta.d_recs.ensure((size_t)heads * sizeof(ts_fasta_record)));
    HIP_TRY(ctx, ch->fasta.d_names.ensure((size_t)std::max<uint64_t>(all_names, 1)));
    if (ts_k_launch_fasta_heads(lstart, first, cr, (uint32_t)n_lines, ch->fasta.d_frames.p, ch->fasta.d_heads.p, (uint32_t)heads,
                                (uint32_t)out[kFaCrs], (uint32_t)all_names, nullptr) != 0 ||
        ts_k_launch_fasta_records(ch->d_plain.p, size, lstart, cr, ch->fasta.d_heads.p, (uint32_t)heads, ch->fasta.d_recs.p,
                                  ch->fasta.d_names.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fasta_chunk_walk: kernel launch failed");

    // without at_end the last record is open: the next chunk may continue it
    const uint64_t whole = at_end ? heads : heads - 1;
    uint64_t name_bytes = all_names;
    *next = size;
    if (whole < heads) {
        ts_fasta_record open;
        HIP_TRY(ctx, hipMemcpy(&open, (const ts_fasta_record *)ch->fasta.d_recs.p + whole, sizeof open, hipMemcpyDeviceToHost));
        if (open.off > size || open.name_at > all_names) return ctx->fail(TS_ERR_STATE, "ts_fasta_chunk_walk: the walk left the chunk");
        *next = open.off;
        name_bytes = open.name_at;
    }
    *n = whole;
    *names_bytes = name_bytes;
    if (whole > cap || name_bytes > names_cap)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_walk: the table or the names buffer is too small (*n and *names_bytes say what is needed)");
    if (whole) HIP_TRY(ctx, hipMemcpy(recs, ch->fasta.d_recs.p, (size_t)whole * sizeof(ts_fasta_record), hipMemcpyDeviceToHost));
    if (name_bytes) HIP_TRY(ctx, hipMemcpy(names, ch->fasta.d_names.p, (size_t)name_bytes, hipMemcpyDeviceToHost));
    return TS_OK;
}

int ts_fasta_chunk_join(ts_chunk *ch, const ts_fasta_record *recs, size_t n, int at_end, const void **d_bases, uint64_t *offsets,
                        uint64_t *total_bytes, uint64_t *n_runs, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!d_bases || !total_bytes || !n_runs || (n && (!recs || !offsets)) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_join: null or out-of-range argument");
    if (ch->plain_n >= 0xffffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_join: the chunk holds 4 GiB or more");
    *d_bases = nullptr; *total_bytes = 0; *n_runs = 0;
    ch->fasta.joined = 0; ch->fasta.runs = 0;
    const uint64_t size = ch->plain_n;
    // where every record goes, and the jobs: a record's body text and its joined bases, each cut at multiples of 16 KB
    std::vector<FastaJoinJob> jobs;
    std::vector<FastaRunJob> run_jobs;
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const ts_fasta_record &r = recs[i];
        if (!record_ok(ch, r)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_join: record " + std::to_string(i) + " does not fit the chunk");
        offsets[i] = total;
        const uint64_t a = r.off + r.body_at, z = r.off + r.text_len, first = jobs.size();
        for (uint64_t p = a; p < z;) {
            const uint64_t q = std::min<uint64_t>(z, (p / kFastaSliceBytes + 1) * kFastaSliceBytes);
            jobs.push_back(FastaJoinJob{(uint32_t)p, (uint32_t)q, (uint32_t)first, 0u, total, total + r.n_bases});
            p = q;
        }
        if (jobs.size() > first) jobs.back().last = 1u;        // it zeroes the bytes between this record and the next
        for (uint64_t p = total; p < total + r.n_bases;) {
            const uint64_t q = std::min<uint64_t>(total + r.n_bases, (p / kFastaSliceBytes + 1) * kFastaSliceBytes);
            run_jobs.push_back(FastaRunJob{p, q, total, (uint32_t)i, 0u});
            p = q;
        }
        total += ((uint64_t)r.n_bases + 15) & ~15ull;
    }
    if (jobs.size() > 0x7fffffffull || run_jobs.size() > 0x7fffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_join: too many bases for one call");
    DEVICE_TRY(ctx);
    { const int rc = ensure_out(ch); if (rc != TS_OK) return rc; }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *d_totals = (unsigned long long *)ch->fasta.d_out.p + kFaTotal;      // {kept bytes, runs}
    HIP_TRY(ctx, ch->fasta.d_bases.ensure((size_t)total + 64));
    HIP_TRY(ctx, hipMemsetAsync((char *)ch->fasta.d_bases.p + total, 0, 64, st));           // (readable, and zero, behind the last record)
    *d_bases = ch->fasta.d_bases.p;
    *total_bytes = total;
    ch->fasta.joined = total;
    if (n == 0) { HIP_TRY(ctx, hipStreamSynchronize(st)); return TS_OK; }
    // both job lists and the table go up together; both count passes and their sums run before the one wait for the totals
    const size_t n_jobs = jobs.size(), n_rjobs = run_jobs.size();
    HIP_TRY(ctx, ch->fasta.d_recs.ensure(n * sizeof(ts_fasta_record)));
    HIP_TRY(ctx, ch->fasta.d_jobs.ensure(std::max<size_t>(1, n_jobs * sizeof(FastaJoinJob) + n_rjobs * sizeof(FastaRunJob))));
    HIP_TRY(ctx, ch->fasta.d_counts.ensure(std::max<size_t>(1, n_jobs + n_rjobs) * 4));
    void *d_jobs = ch->fasta.d_jobs.p, *d_rjobs = (char *)ch->fasta.d_jobs.p + n_jobs * sizeof(FastaJoinJob);
    uint32_t *counts = (uint32_t *)ch->fasta.d_counts.p, *rcounts = counts + n_jobs;
    HIP_TRY(ctx, hipMemcpyAsync(ch->fasta.d_recs.p, recs, n * sizeof(ts_fasta_record), hipMemcpyHostToDevice, st));
    if (n_jobs) HIP_TRY(ctx, hipMemcpyAsync(d_jobs, jobs.data(), n_jobs * sizeof(FastaJoinJob), hipMemcpyHostToDevice, st));
    if (n_rjobs) HIP_TRY(ctx, hipMemcpyAsync(d_rjobs, run_jobs.data(), n_rjobs * sizeof(FastaRunJob), hipMemcpyHostToDevice, st));
    // join: count, sum, write; runs: count, sum
    if (ts_k_launch_fasta_join_count(ch->d_plain.p, size, at_end, d_jobs, (uint32_t)n_jobs, counts, stream) != 0 ||
        ts_k_launch_chunk_scan(counts, (uint32_t)n_jobs, d_totals, stream) != 0 ||
        ts_k_launch_fasta_join_write(ch->d_plain.p, size, at_end, d_jobs, (uint32_t)n_jobs, counts, ch->fasta.d_bases.p, stream) != 0 ||
        ts_k_launch_fasta_run_count(ch->fasta.d_bases.p, d_rjobs, (uint32_t)n_rjobs, rcounts, stream) != 0 ||
        ts_k_launch_chunk_scan(rcounts, (uint32_t)n_rjobs, d_totals + 1, stream) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fasta_chunk_join: kernel launch failed");
    unsigned long long totals[2] = {0, 0}, bases = 0;
    HIP_TRY(ctx, hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                    // (the lists were this call's memory: they have left it too)
    for (size_t i = 0; i < n; ++i) bases += recs[i].n_bases;
    const unsigned long long kept = totals[0], runs = totals[1];
    if (kept != bases) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_join: the records are not the chunk's (their text holds " + std::to_string(kept) + " bases, the table says " + std::to_string(bases) + ")");
    if (runs > total) return ctx->fail(TS_ERR_STATE, "ts_fasta_chunk_join: more runs than bases");
    // runs: write, lengths
    HIP_TRY(ctx, ch->fasta.d_runs.ensure((size_t)std::max<unsigned long long>(runs, 1) * sizeof(ts_fasta_run)));
    if (ts_k_launch_fasta_run_write(ch->fasta.d_bases.p, d_rjobs, (uint32_t)n_rjobs, rcounts, ch->fasta.d_runs.p, runs, stream) != 0 ||
        ts_k_launch_fasta_run_lengths(ch->fasta.d_runs.p, runs, ch->fasta.d_recs.p, (uint32_t)n, stream) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fasta_chunk_join: kernel launch failed");
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ch->fasta.runs = runs;
    *n_runs = runs;
    return TS_OK;
}

int ts_fasta_chunk_stage(ts_chunk *ch, const ts_fasta_record *recs, size_t n, int at_end, ts_batch *reads, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!reads || (n && !recs) || reads->ctx != ctx || !reads->tips || !reads->whole() || reads->segs.size() != n)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_stage: needs an unrestricted tips-only batch of this context with one segment per record");
    if (ch->plain_n >= 0xffffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_stage: the chunk holds 4 GiB or more");
    // the jobs: a record's body text cut at multiples of 16 KB, as the join cuts it, with the record's segment as its place; the
    // records of two jobs or more, whose jobs are counted and summed
    std::vector<FastaJoinJob> jobs;
    std::vector<FastaStageSpan> spans;
    for (size_t i = 0; i < n; ++i) {
        const ts_fasta_record &r = recs[i];
        if (!record_ok(ch, r) || r.n_bases == 0 || reads->segs[i].len != r.n_bases)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_stage: record " + std::to_string(i) + " does not fit the chunk or its segment");
        const uint64_t dst = ts_batch_segment_offset(reads, i), z = r.off + r.text_len, first = jobs.size();
        for (uint64_t p = r.off + r.body_at; p < z;) {
            const uint64_t q = std::min<uint64_t>(z, (p / kFastaSliceBytes + 1) * kFastaSliceBytes);
            jobs.push_back(FastaJoinJob{(uint32_t)p, (uint32_t)q, (uint32_t)first, 0u, dst, dst + r.n_bases});
            p = q;
        }
        jobs.back().last = 1u;                                  // (n_bases > 0: the record has a job) it zeroes the bytes behind the read
        if (jobs.size() - first > 1) spans.push_back(FastaStageSpan{(uint32_t)first, (uint32_t)(jobs.size() - first)});
        if (jobs.size() > 0x7fffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_stage: too many bases for one call");
    }
    DEVICE_TRY(ctx);
    const bool fresh = reads->d_in.p == nullptr;
    void *in = ts_batch_input_ptr(reads);
    if (!in) return ctx->fail(TS_ERR_ALLOC, "ts_fasta_chunk_stage: no input buffer");
    if (jobs.empty()) return TS_OK;
    hipStream_t st = (hipStream_t)stream;
    // (a fresh input buffer was just zeroed on the null stream, which a non-blocking `stream` does not wait for)
    if (fresh && st) HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    const size_t job_bytes = jobs.size() * sizeof(FastaJoinJob);
    HIP_TRY(ctx, ch->fasta.d_jobs.ensure(job_bytes + std::max<size_t>(1, spans.size()) * sizeof(FastaStageSpan)));
    HIP_TRY(ctx, ch->fasta.d_counts.ensure(jobs.size() * 4));
    void *d_spans = (char *)ch->fasta.d_jobs.p + job_bytes;
    HIP_TRY(ctx, hipMemcpyAsync(ch->fasta.d_jobs.p, jobs.data(), job_bytes, hipMemcpyHostToDevice, st));
    if (!spans.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_spans, spans.data(), spans.size() * sizeof(FastaStageSpan), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                    // (the lists are this call's memory)
    if (ts_k_launch_fasta_stage(ch->d_plain.p, ch->plain_n, at_end ? 1 : 0, ch->fasta.d_jobs.p, (uint32_t)jobs.size(), d_spans, (uint32_t)spans.size(),
                                (uint32_t *)ch->fasta.d_counts.p, in, stream) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_fasta_chunk_stage: kernel launch failed");
    return TS_OK;
}

int ts_fasta_chunk_gather(ts_chunk *ch, const ts_fasta_record *recs, size_t n, const void *d_pass, void *host_out, uint64_t cap,
                          uint64_t *bytes, uint64_t *n_passed, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_gather: null or out-of-range argument");
    // a record's text ends with the '\n' in front of the next record's '>'; only the text that ends the chunk may lack it
    bool final_lf = true, looked = false;
    for (size_t i = 0; i < n; ++i) {
        if (!record_ok(ch, recs[i]) || recs[i].text_len == 0)
            return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_gather: record " + std::to_string(i) + " does not fit the chunk");
        if (recs[i].off + recs[i].text_len == ch->plain_n && !looked) {
            unsigned char c = 0;
            looked = true;
            DEVICE_TRY(ctx);
            HIP_TRY(ctx, hipMemcpy(&c, (const char *)ch->d_plain.p + ch->plain_n - 1, 1, hipMemcpyDeviceToHost));
            final_lf = c == '\n';
        }
    }
    // the span gather of the FASTQ and SAM routes: `size` bytes from `off` and a '\n' behind them
    std::vector<ts_fastq_record> spans(n);
    for (size_t i = 0; i < n; ++i) {
        const bool ends_chunk = recs[i].off + recs[i].text_len == ch->plain_n;
        spans[i] = ts_fastq_record{recs[i].off, 0u, 0u, recs[i].text_len - (ends_chunk && !final_lf ? 0u : 1u), 0u};
    }
    return ts_chunk_gather(ch, "ts_fasta_chunk_gather", spans.data(), sizeof(ts_fastq_record), n, d_pass, host_out, cap, bytes, n_passed, stream,
                           ts_k_launch_chunk_gather_plan_fastq, ts_k_launch_fastq_gather);
}

int ts_fasta_chunk_strict(ts_chunk *ch, const ts_fasta_record *recs, size_t n, unsigned char *has_sequence, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && (!recs || !has_sequence)) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_strict: null or out-of-range argument");
    if (ch->plain_n >= 0xffffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_strict: the chunk holds 4 GiB or more");
    if (n == 0) return TS_OK;
    // the jobs: a record's body text cut at multiples of 16 KB, as the join cuts it
    std::vector<FastaStrictJob> jobs;
    for (size_t i = 0; i < n; ++i) {
        const ts_fasta_record &r = recs[i];
        if (!record_ok(ch, r)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_strict: record " + std::to_string(i) + " does not fit the chunk");
        const uint64_t z = r.off + r.text_len;
        for (uint64_t p = r.off + r.body_at; p < z;) {
            const uint64_t q = std::min<uint64_t>(z, (p / kFastaSliceBytes + 1) * kFastaSliceBytes);
            jobs.push_back(FastaStrictJob{(uint32_t)p, (uint32_t)q, (uint32_t)i, 0u});
            p = q;
        }
    }
    if (jobs.size() > 0x7fffffffull) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_strict: too much text for one call");
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, ch->fasta.d_strict.ensure(n));
    HIP_TRY(ctx, hipMemsetAsync(ch->fasta.d_strict.p, 0, n, st));
    if (!jobs.empty()) {
        HIP_TRY(ctx, ch->fasta.d_jobs.ensure(jobs.size() * sizeof(FastaStrictJob)));
        HIP_TRY(ctx, hipMemcpyAsync(ch->fasta.d_jobs.p, jobs.data(), jobs.size() * sizeof(FastaStrictJob), hipMemcpyHostToDevice, st));
        if (ts_k_launch_fasta_strict(ch->d_plain.p, ch->plain_n, ch->fasta.d_jobs.p, (uint32_t)jobs.size(), (unsigned char *)ch->fasta.d_strict.p, stream) != 0)
            return ctx->fail(TS_ERR_HIP, "ts_fasta_chunk_strict: kernel launch failed");
    }
    HIP_TRY(ctx, hipMemcpyAsync(has_sequence, ch->fasta.d_strict.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                    // (the job list was this call's memory: it has left it too)
    return TS_OK;
}

int ts_fasta_chunk_runs(ts_chunk *ch, ts_fasta_run *runs, uint64_t cap, uint64_t *n_runs) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n_runs || (cap && !runs)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_runs: null argument");
    *n_runs = ch->fasta.runs;
    if (ch->fasta.runs > cap) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_runs: the table is too small (*n_runs says what is needed)");
    if (ch->fasta.runs == 0) return TS_OK;
    DEVICE_TRY(ctx);                                           // (the join waited for its stream: a blocking copy is all it takes)
    HIP_TRY(ctx, hipMemcpy(runs, ch->fasta.d_runs.p, (size_t)ch->fasta.runs * sizeof(ts_fasta_run), hipMemcpyDeviceToHost));
    return TS_OK;
}

int ts_fasta_chunk_bases(ts_chunk *ch, uint64_t off, uint64_t n, void *host) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && !host) || off > ch->fasta.joined || n > ch->fasta.joined - off) return ctx->fail(TS_ERR_INVALID_ARG, "ts_fasta_chunk_bases: outside the joined bases");
    if (n == 0) return TS_OK;
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, hipMemcpy(host, (const char *)ch->fasta.d_bases.p + off, (size_t)n, hipMemcpyDeviceToHost));
    return TS_OK;
}

}  // extern "C"
