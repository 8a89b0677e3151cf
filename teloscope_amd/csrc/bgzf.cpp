// bgzf.cpp — host side of the device BGZF route (include/teloscan.h: ts_bgzf_inflate): descriptor checks, staging, the
// verdict.  Nothing here inflates: the members are decoded by bgzf.hip's kernel or not at all.
#include "chunk_internal.h"
#include "bam_walk_core.h"

#include <numeric>

namespace {

// src_off + payload_len <= n, sizes <= 64 KB, dst_off + isize <= plain_cap, outputs disjoint
bool descriptors_ok(const ts_bgzf_block *blocks, size_t n_blocks, uint64_t n, uint64_t plain_cap, std::string &why,
                    uint64_t dst_floor = 0) {
    for (size_t i = 0; i < n_blocks; ++i) {
        const ts_bgzf_block &b = blocks[i];
        if (b.dst_off < dst_floor) { why = "block " + std::to_string(i) + ": output inside the carried bytes"; return false; }
        if (b.payload_len > 65536u || b.isize > 65536u) { why = "block " + std::to_string(i) + ": payload_len or isize above 65536"; return false; }
        if (b.src_off > n || b.payload_len > n - b.src_off) { why = "block " + std::to_string(i) + ": payload outside the compressed bytes"; return false; }
        if (b.dst_off > plain_cap || b.isize > plain_cap - b.dst_off) { why = "block " + std::to_string(i) + ": output outside plain_out"; return false; }
    }
    std::vector<uint32_t> order;
    for (size_t i = 0; i < n_blocks; ++i) if (blocks[i].isize) order.push_back((uint32_t)i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return blocks[a].dst_off < blocks[b].dst_off; });
    for (size_t k = 1; k < order.size(); ++k) {
        const ts_bgzf_block &a = blocks[order[k - 1]], &b = blocks[order[k]];
        if (a.dst_off + a.isize > b.dst_off) { why = "blocks " + std::to_string(order[k - 1]) + " and " + std::to_string(order[k]) + ": outputs overlap"; return false; }
    }
    return true;
}

}  // namespace

extern "C" int ts_bgzf_inflate(ts_ctx *ctx, const void *compressed, uint64_t n, const ts_bgzf_block *blocks, size_t n_blocks,
                               void *plain_out, uint64_t plain_cap, ts_bgzf_status *first_bad) {
    if (!ctx) return TS_ERR_INVALID_ARG;
    if (!first_bad || (n && !compressed) || (n_blocks && !blocks) || (plain_cap && !plain_out))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bgzf_inflate: null argument");
    if (n_blocks > 0xffffffffull || n > (1ull << 40) || plain_cap > (1ull << 40))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bgzf_inflate: too large for one call");
    std::string why;
    if (!descriptors_ok(blocks, n_blocks, n, plain_cap, why)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bgzf_inflate: " + why);
    DEVICE_TRY(ctx);
    first_bad->code = TS_BGZF_OK; first_bad->reserved = 0; first_bad->block = n_blocks;
    if (n_blocks == 0) { if (plain_cap) memset(plain_out, 0, (size_t)plain_cap); return TS_OK; }

    // the buffers go back to the context's pool on every return path
    struct Lease {
        ts_ctx *c; DevBuf b;
        explicit Lease(ts_ctx *c_) : c(c_) {}
        ~Lease() { if (b.p) c->pool.give(std::move(b)); }
    } d_comp(ctx), d_blocks(ctx), d_plain(ctx), d_result(ctx);
    HIP_TRY(ctx, ctx->pool.take((size_t)n + 16, d_comp.b));                     // (the kernel reads whole aligned dwords)
    HIP_TRY(ctx, ctx->pool.take(n_blocks * sizeof(ts_bgzf_block), d_blocks.b));
    HIP_TRY(ctx, ctx->pool.take((size_t)plain_cap + 16, d_plain.b));
    HIP_TRY(ctx, ctx->pool.take(n_blocks * 4, d_result.b));
    if (n) HIP_TRY(ctx, hipMemcpy(d_comp.b.p, compressed, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset((char *)d_comp.b.p + n, 0, 16));
    HIP_TRY(ctx, hipMemcpy(d_blocks.b.p, blocks, n_blocks * sizeof(ts_bgzf_block), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(d_plain.b.p, 0, (size_t)plain_cap + 16));
    HIP_TRY(ctx, hipMemset(d_result.b.p, 0xff, n_blocks * 4));
    if (ts_k_launch_bgzf_inflate(d_comp.b.p, d_blocks.b.p, (uint32_t)n_blocks, d_plain.b.p, (uint32_t *)d_result.b.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_bgzf_inflate: kernel launch failed");
    HIP_TRY(ctx, hipDeviceSynchronize());
    std::vector<uint32_t> result(n_blocks);
    HIP_TRY(ctx, hipMemcpy(result.data(), d_result.b.p, n_blocks * 4, hipMemcpyDeviceToHost));
    if (plain_cap) HIP_TRY(ctx, hipMemcpy(plain_out, d_plain.b.p, (size_t)plain_cap, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_blocks; ++i) {
        if (result[i] > TS_BGZF_BAD_CRC) return ctx->fail(TS_ERR_STATE, "ts_bgzf_inflate: block " + std::to_string(i) + " was not judged");
        if (result[i] != TS_BGZF_OK && first_bad->code == TS_BGZF_OK) { first_bad->code = (int32_t)result[i]; first_bad->block = i; }
    }
    // (a member that is not ok may have written some of its bytes: they are not its output)
    for (size_t i = 0; i < n_blocks; ++i)
        if (result[i] != TS_BGZF_OK && blocks[i].isize) memset((char *)plain_out + blocks[i].dst_off, 0, blocks[i].isize);
    return TS_OK;
}

// ===================================================================== the resident form: a chunk of a BAM on the device
// (struct ts_bam_chunk: chunk_internal.h; the object itself: chunk.cpp)
namespace {
constexpr uint32_t kDecodePiece = 2048;

// a record of the table against the chunk: inside it, SEQ inside the record
bool record_ok(const ts_bam_chunk *ch, const ts_bam_record &r) {
    if (r.block_size < 32u || r.block_size > (256u << 20)) return false;
    if (r.off > ch->plain_n || 4ull + r.block_size > ch->plain_n - r.off) return false;
    if (r.l_seq > 0x7fffffffu) return false;
    return (uint64_t)r.seq_at + ((uint64_t)r.l_seq + 1) / 2 <= 4ull + r.block_size;
}
}  // namespace

extern "C" {

int ts_bam_chunk_inflate(ts_bam_chunk *ch, const void *compressed, uint64_t n, const ts_bgzf_block *blocks, size_t n_blocks,
                         uint64_t carry_from, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && !compressed) || (n_blocks && !blocks) || n > ch->comp_cap || n_blocks > 0xffffffffull || carry_from > ch->plain_n)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_inflate: null or out-of-range argument");
    const uint64_t carry = ch->plain_n - carry_from;
    std::string why;
    if (!descriptors_ok(blocks, n_blocks, n, ch->plain_cap, why, carry)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_inflate: " + why);
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    { uint64_t moved = 0; const int rc = ts_chunk_carry(ch, carry_from, st, &moved); if (rc != TS_OK) return rc; }
    uint64_t end = carry;
    for (size_t i = 0; i < n_blocks; ++i) end = std::max<uint64_t>(end, blocks[i].dst_off + blocks[i].isize);
    ch->plain_n = end;
    ch->n_blocks = n_blocks;
    if (n_blocks) {
        HIP_TRY(ctx, ch->bam.d_blocks.ensure(n_blocks * sizeof(ts_bgzf_block)));
        HIP_TRY(ctx, ch->bam.d_result.ensure(n_blocks * 4));
        if (n) HIP_TRY(ctx, hipMemcpyAsync(ch->d_comp.p, compressed, (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync((char *)ch->d_comp.p + n, 0, 16, st));
        HIP_TRY(ctx, hipMemcpyAsync(ch->bam.d_blocks.p, blocks, n_blocks * sizeof(ts_bgzf_block), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(ch->bam.d_result.p, 0xff, n_blocks * 4, st));
        // (the descriptors are the caller's memory: they have left it when this returns)
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (ts_k_launch_bgzf_inflate(ch->d_comp.p, ch->bam.d_blocks.p, (uint32_t)n_blocks, ch->d_plain.p, (uint32_t *)ch->bam.d_result.p, stream) != 0)
            return ctx->fail(TS_ERR_HIP, "ts_bam_chunk_inflate: kernel launch failed");
    }
    return TS_OK;
}

int ts_chunk_stage_inflate(ts_bam_chunk *ch, const void *compressed, uint64_t n, const ts_bgzf_block *blocks, size_t n_blocks,
                           void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if ((n && !compressed) || (n_blocks && !blocks) || n > ch->comp_cap || n_blocks > 0xffffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_chunk_stage_inflate: null or out-of-range argument");
    uint64_t end = ch->stage_n;
    for (size_t i = 0; i < n_blocks; ++i)
        if (blocks[i].dst_off < (1ull << 40) && blocks[i].isize <= 65536u) end =std::max<uint64_t>(end, blocks[i].dst_off + blocks[i].isize);
    { const int rc = ts_chunk_stage_reserve(ch, end); if (rc != TS_OK) return rc; }
    std::string why;
    if (!descriptors_ok(blocks, n_blocks, n, ch->stage_cap, why, ch->stage_n)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_chunk_stage_inflate: " + why);
    DEVICE_TRY(ctx);
    hipStream_t st = (hipStream_t)stream;
    ch->stage_n = end;
    ch->n_blocks = n_blocks;
    if (n_blocks) {
        HIP_TRY(ctx, ch->bam.d_blocks.ensure(n_blocks * sizeof(ts_bgzf_block)));
        HIP_TRY(ctx, ch->bam.d_result.ensure(n_blocks * 4));
        if (n) HIP_TRY(ctx, hipMemcpyAsync(ch->d_comp.p, compressed, (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync((char *)ch->d_comp.p + n, 0, 16, st));
        HIP_TRY(ctx, hipMemcpyAsync(ch->bam.d_blocks.p, blocks, n_blocks * sizeof(ts_bgzf_block), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(ch->bam.d_result.p, 0xff, n_blocks * 4, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                // (the descriptors are the caller's memory, as for ts_bam_chunk_inflate)
        if (ts_k_launch_bgzf_inflate(ch->d_comp.p, ch->bam.d_blocks.p, (uint32_t)n_blocks, ch->d_stage.p, (uint32_t *)ch->bam.d_result.p, stream) != 0)
            return ctx->fail(TS_ERR_HIP, "ts_chunk_stage_inflate: kernel launch failed");
    }
    return TS_OK;
}

int ts_bam_chunk_status(ts_bam_chunk *ch, ts_bgzf_status *first_bad) {
    if (!ch || !first_bad) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    DEVICE_TRY(ctx);
    first_bad->code = TS_BGZF_OK; first_bad->reserved = 0; first_bad->block = ch->n_blocks;
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (!ch->n_blocks) return TS_OK;
    std::vector<uint32_t> result(ch->n_blocks);
    HIP_TRY(ctx, hipMemcpy(result.data(), ch->bam.d_result.p, ch->n_blocks * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ch->n_blocks; ++i) {
        if (result[i] > TS_BGZF_BAD_CRC) return ctx->fail(TS_ERR_STATE, "ts_bam_chunk_status: block " + std::to_string(i) + " was not judged");
        if (result[i] != TS_BGZF_OK) { first_bad->code = (int32_t)result[i]; first_bad->block = i; break; }
    }
    return TS_OK;
}

int ts_bam_chunk_walk(ts_bam_chunk *ch, uint64_t from, ts_bam_record *recs, uint64_t cap, uint64_t *n, uint64_t *next,
                      int *error, uint64_t *error_off) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n || !next || !error || !error_off || (cap && !recs) || from > ch->plain_n || cap > (1ull << 31))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_walk: null or out-of-range argument");
    DEVICE_TRY(ctx);
    HIP_TRY(ctx, ch->d_recs.ensure((size_t)std::max<uint64_t>(cap, 1) * sizeof(ts_bam_record)));
    if (ts_k_launch_bam_walk(ch->d_plain.p, ch->plain_n, from, cap, ch->d_recs.p, ch->d_out.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_bam_chunk_walk: kernel launch failed");
    HIP_TRY(ctx, hipDeviceSynchronize());
    unsigned long long out[4];
    HIP_TRY(ctx, hipMemcpy(out, ch->d_out.p, sizeof out, hipMemcpyDeviceToHost));
    if (out[0] > cap || out[1] > ch->plain_n) return ctx->fail(TS_ERR_STATE, "ts_bam_chunk_walk: the walk left the chunk");
    if (out[0]) HIP_TRY(ctx, hipMemcpy(recs, ch->d_recs.p, (size_t)out[0] * sizeof(ts_bam_record), hipMemcpyDeviceToHost));
    *n = out[0]; *next = out[1]; *error = (int)out[2]; *error_off = out[3];
    return TS_OK;
}

int ts_bam_chunk_set_index_geometry(ts_bam_chunk *ch, uint32_t span_bytes, uint32_t candidates) {
    if (!ch) return TS_ERR_INVALID_ARG;
    if (span_bytes < tsbam::kMinSpan || span_bytes > tsbam::kMaxSpan || (span_bytes & (span_bytes - 1u)) != 0u || candidates < 1u ||
        candidates > tsbam::kMaxCandidates)
        return ch->ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_set_index_geometry: span_bytes is a power of two of 64 .. 2^30, candidates 1 .. 8");
    uint32_t lg = 0;
    while ((1u << lg) < span_bytes) ++lg;
    ch->bam.index_span_log2 = lg;
    ch->bam.index_candidates = candidates;
    return TS_OK;
}

// The parallel form of ts_bam_chunk_walk (bam_walk_core.h): candidates per span on the device, the chain here from the
// downloaded rows, the table written on the device by a wave per entered span.
int ts_bam_chunk_index(ts_bam_chunk *ch, uint64_t from, ts_bam_record *recs, uint64_t cap, uint64_t *n, uint64_t *next,
                       int *error, uint64_t *error_off) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!n || !next || !error || !error_off || (cap && !recs) || from > ch->plain_n || cap > (1ull << 31))
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_index: null or out-of-range argument");
    DEVICE_TRY(ctx);
    const uint32_t lg = ch->bam.index_span_log2, K = ch->bam.index_candidates;
    const uint64_t size = ch->plain_n;
    ctx->bam_index_stats[0].fetch_add(1, std::memory_order_relaxed);
    *n = 0; *next = from; *error = TS_BAM_OK; *error_off = 0;
    if (cap == 0 || size - from < 4) return TS_OK;
    const uint64_t first = from >> lg, n_spans = ((size - 1) >> lg) - first + 1;
    if (n_spans > (1ull << 26)) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_index: the span size is too small for this chunk");
    const size_t row_bytes = (size_t)n_spans * K * sizeof(tsbam::Row);
    HIP_TRY(ctx, ch->bam.d_idx_rows.ensure(row_bytes));
    if (ts_k_launch_bam_index_candidates(ch->d_plain.p, size, from, lg, K, first, (uint32_t)n_spans, ch->bam.d_idx_rows.p, nullptr) != 0)
        return ctx->fail(TS_ERR_HIP, "ts_bam_chunk_index: kernel launch failed");
    ch->bam.h_idx_rows.resize(row_bytes);
    HIP_TRY(ctx, hipMemcpy(ch->bam.h_idx_rows.data(), ch->bam.d_idx_rows.p, row_bytes, hipMemcpyDeviceToHost));     // (waits for the kernel)
    const tsbam::Row *rows = (const tsbam::Row *)ch->bam.h_idx_rows.data();
    std::vector<tsbam::Task> tasks;
    hipError_t bad = hipSuccess;
    int launch_failed = 0;
    const tsbam::ChainResult c = tsbam::chain(
        size, from, cap, lg, K, [&](uint64_t k) { return rows + (size_t)(k - first) * K; },
        [&](uint64_t entry, uint64_t span_end) {
            tsbam::SpanResult s;
            s.exit = entry; s.records = 0; s.stop = tsbam::kShort;      // (after a failure: the chain ends here)
            unsigned long long out[3] = {0, 0, 0};
            if (bad != hipSuccess || launch_failed) return s;
            if (ts_k_launch_bam_index_settle(ch->d_plain.p, size, entry, span_end, ch->d_out.p, nullptr) != 0) { launch_failed = 1; return s; }
            bad = hipMemcpy(out, ch->d_out.p, sizeof out, hipMemcpyDeviceToHost);
            if (bad != hipSuccess) return s;
            s.exit = out[0]; s.records = out[1]; s.stop = (uint32_t)out[2];
            return s;
        },
        [&](const tsbam::Task &t) { tasks.push_back(t); });
    if (launch_failed) return ctx->fail(TS_ERR_HIP, "ts_bam_chunk_index: kernel launch failed");
    HIP_TRY(ctx, bad);
    ctx->bam_index_stats[1].fetch_add(c.entered, std::memory_order_relaxed);
    ctx->bam_index_stats[2].fetch_add(c.hits, std::memory_order_relaxed);
    ctx->bam_index_stats[3].fetch_add(c.settled, std::memory_order_relaxed);
    ctx->bam_index_stats[5].fetch_add(row_bytes, std::memory_order_relaxed);
    if (c.n > cap || c.next > size) return ctx->fail(TS_ERR_STATE, "ts_bam_chunk_index: the chain left the chunk");
    unsigned long long next_at = c.next;
    if (c.n) {
        // (the write pass is told c.n, not cap: it stores nothing beyond what the chain counted, whatever it meets)
        HIP_TRY(ctx, ch->d_recs.ensure((size_t)c.n * sizeof(ts_bam_record)));
        HIP_TRY(ctx, ch->bam.d_idx_tasks.ensure(tasks.size() * sizeof(tsbam::Task)));
        HIP_TRY(ctx, hipMemcpy(ch->bam.d_idx_tasks.p, tasks.data(), tasks.size() * sizeof(tsbam::Task), hipMemcpyHostToDevice));
        if (ts_k_launch_bam_index_write(ch->d_plain.p, size, ch->bam.d_idx_tasks.p, (uint32_t)tasks.size(), lg, c.n, ch->d_recs.p, ch->d_out.p, nullptr) != 0)
            return ctx->fail(TS_ERR_HIP, "ts_bam_chunk_index: kernel launch failed");
        HIP_TRY(ctx, hipMemcpy(recs, ch->d_recs.p, (size_t)c.n * sizeof(ts_bam_record), hipMemcpyDeviceToHost));
        if (c.next_in_span) {
            HIP_TRY(ctx, hipMemcpy(&next_at, ch->d_out.p, sizeof next_at, hipMemcpyDeviceToHost));
            if (next_at > size) return ctx->fail(TS_ERR_STATE, "ts_bam_chunk_index: the walk left the chunk");
        }
    }
    ctx->bam_index_stats[4].fetch_add(c.n, std::memory_order_relaxed);
    *n = c.n; *next = next_at; *error = (int)c.error; *error_off = c.error_off;
    return TS_OK;
}

int ts_bam_index_stats(const ts_ctx *ctx, uint64_t out[6]) {
    if (!ctx || !out) return TS_ERR_INVALID_ARG;
    for (int i = 0; i < 6; ++i) out[i] = ctx->bam_index_stats[i].load(std::memory_order_relaxed);
    return TS_OK;
}

int ts_bam_chunk_decode(ts_bam_chunk *ch, const ts_bam_record *recs, size_t n, ts_batch *reads, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    // (a job's kDecodePiece bases are packed two to a byte)
    return ts_chunk_stage_records(ch, "ts_bam_chunk_decode", recs, n, reads, stream, kDecodePiece, kDecodePiece / 2,
                                  [](const ts_bam_chunk *c, const void *table, size_t i, uint64_t *src, uint32_t *len) {
                                      const ts_bam_record &r = ((const ts_bam_record *)table)[i];
                                      *src = (uint64_t)r.off + r.seq_at; *len = r.l_seq;
                                      return record_ok(c, r);
                                  }, ts_k_launch_bam_decode);
}

int ts_bam_chunk_gather(ts_bam_chunk *ch, const ts_bam_record *recs, size_t n, const void *d_pass, void *host_out, uint64_t cap,
                        uint64_t *bytes, uint64_t *n_passed, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_gather: null or out-of-range argument");
    for (size_t i = 0; i < n; ++i)
        if (!record_ok(ch, recs[i])) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_gather: record " + std::to_string(i) + " does not fit the chunk");
    return ts_chunk_gather(ch, "ts_bam_chunk_gather", recs, sizeof(ts_bam_record), n, d_pass, host_out, cap, bytes, n_passed, stream,
                           ts_k_launch_chunk_gather_plan_bam, ts_k_launch_bam_gather);
}

// ts_bam_chunk_gather with the passing records left on the device, deflated there (deflate.cpp, deflate.hip) and downloaded as
// BGZF members: what the reference's BgzfWriter makes of them with zlib (src/bgzf.cpp:227-276).
int ts_bam_chunk_gather_bgzf(ts_bam_chunk *ch, const ts_bam_record *recs, size_t n, const void *d_pass, uint32_t payload_bytes,
                             void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_passed, uint64_t *plain_bytes, void *stream) {
    if (!ch) return TS_ERR_INVALID_ARG;
    ts_ctx *ctx = ch->ctx;
    if (!bytes || !n_passed || !plain_bytes || (n && (!recs || !d_pass)) || (cap && !host_out) || n > 0x7fffffffull)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_gather_bgzf: null or out-of-range argument");
    *bytes = 0; *n_passed = 0; *plain_bytes = 0;
    if (payload_bytes == 0 || payload_bytes > 0xff00u)
        return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_gather_bgzf: payload_bytes is 1 .. 65280");
    for (size_t i = 0; i < n; ++i)
        if (!record_ok(ch, recs[i])) return ctx->fail(TS_ERR_INVALID_ARG, "ts_bam_chunk_gather_bgzf: record " + std::to_string(i) + " does not fit the chunk");
    const int rc = ts_chunk_gather_device(ch, "ts_bam_chunk_gather_bgzf", recs, sizeof(ts_bam_record), n, d_pass, ~0ull, plain_bytes, n_passed,
                                          stream, ts_k_launch_chunk_gather_plan_bam, ts_k_launch_bam_gather);
    if (rc != TS_OK || *plain_bytes == 0) return rc;
    uint64_t members = 0;
    return ts_deflate_members(ctx, "ts_bam_chunk_gather_bgzf", ch->d_gather.p, *plain_bytes, payload_bytes, ch->bam.deflate, host_out, cap,
                              bytes, &members, stream);
}

}  // extern "C"
