// chunk_internal.h — the chunk layer under the BAM, FASTQ, SAM, FASTA and GFA device stages: a chunk of an uncompressed stream
// resident on the device (struct ts_bam_chunk: the public header names the type; ts_chunk is the same type), the line index the
// four text walks begin with, the gather the record routes end with, and the launchers of the kernels the routes share
// (chunk.hip).  chunk.cpp owns the object and the functions declared here; a route file (bgzf.cpp, fastq.cpp, sam.cpp, fasta.cpp,
// gfa.cpp) touches the common part and its own group.
#pragma once

#include "capi_internal.hpp"

constexpr uint32_t kChunkSliceBytes = 16384;        // bytes of the chunk a wave of a byte count or a byte index takes
// the line count's two words at the front of a result block (unsigned long long each)
enum { kChunkNewlines = 0, kChunkTail, kChunkLineWords };

// The line index: line i starts at lstart[i] and begins with first[i]; cr[i] = 1 when a '\r' stands before its end.  n_lines counts
// the unfinished last line (tail = 1: the last byte is no '\n') with at_end only.
struct LineIndex { uint64_t newlines, tail, n_lines; uint32_t *lstart; unsigned char *first, *cr; };

// the buffers of one device deflate (deflate.cpp: ts_deflate_members) — the members' slots, their sizes and offsets (the total
// behind the offsets), the packed members
struct DeflateBufs { DevBuf slots, sizes, offs, packed; };

struct ts_bam_chunk {
    // ---- what every route uses
    ts_ctx *ctx = nullptr;
    uint64_t comp_cap = 0, plain_cap = 0;
    uint64_t plain_n = 0;               // bytes the chunk holds: the carried tail, then the members' output or the uploaded bytes
    size_t n_blocks = 0;                // members of the last inflate, judged by ts_bam_chunk_status (0: the bytes came another way)
    // the compressed and the plain bytes (both readable 64 bytes beyond their capacity), the carry's bounce buffer, a result block
    // of 64 bytes, the caller's pass bytes; the record table of a walk or a gather, the passing records' places and bytes; the
    // jobs of a stage (ts_chunk_stage_records)
    DevBuf d_comp, d_plain, d_tmp, d_out, d_pass, d_recs, d_dst, d_gather, d_jobs;
    // the staging region (ts_chunk_stage_upload / ts_chunk_stage_inflate): new bytes that wait for the carry they go behind
    // (ts_chunk_commit); readable 64 bytes beyond stage_cap, as d_plain is
    DevBuf d_stage;
    uint64_t stage_cap = 0, stage_n = 0;
    // the line index (ts_chunk_line_index) and the record of what it indexed: `ix` describes the chunk's bytes as long as `valid`
    // holds, plain_n == size and the caller's at_end is the one it was made with; every index made has another generation
    struct Lines {
        DevBuf d_lines, d_waves;        // lstart / first / cr, and the per-slice newline counts
        LineIndex ix{};
        bool valid = false;
        int at_end = 0;
        uint64_t size = 0, generation = 0;
    } lines;
    // ---- BAM (bgzf.cpp): the members' descriptors and verdicts; the parallel record index
    // (ts_bam_chunk_index): its span size (log2) and candidates per span, the candidate rows, the tasks of the write pass, and the
    // host copy of the rows
    struct Bam {
        DevBuf d_blocks, d_result;
        uint32_t index_span_log2 = 18, index_candidates = 4;
        DevBuf d_idx_rows, d_idx_tasks;
        std::vector<unsigned char> h_idx_rows;
        DeflateBufs deflate;                // ts_bam_chunk_gather_bgzf's buffers (deflate.cpp)
    } bam;
    // ---- FASTQ (fastq.cpp): the framing results; of the paired route, where a sub-batch's records lie among its judged reads
    struct Fastq { DevBuf d_frames, d_read_of; } fastq;
    // ---- FASTA (fasta.cpp): the header counts per slice, the walk's header table, record table and names; the join's jobs, their
    // counts, the joined bases and runs; a byte per record of the strict check
    struct Fasta {
        DevBuf d_frames, d_heads, d_recs, d_names, d_jobs, d_counts, d_bases, d_runs, d_out, d_strict;
        uint64_t joined = 0, runs = 0;  // bytes of the last join, its runs
    } fasta;
    // ---- GFA (gfa.cpp): the tab counts per slice and the tabs' offsets, the lines' kind bytes and their per-slice counts, the two
    // tables and the gathered text; of the check the lines' stray-'\r' and code bytes, the flagged lines per slice, their total and
    // the flagged table.  lines_generation: the line index the tab index was made beside (ts_gfa_chunk_check works on both)
    struct Gfa {
        DevBuf d_counts, d_tabs, d_kinds, d_frames, d_segs, d_lines, d_text, d_out, d_stray, d_codes, d_ccounts, d_cout, d_flagged;
        uint64_t lines_generation = 0, n_tabs = 0;
    } gfa;
    // ---- SAM (sam.cpp): the tab counts per slice and the tabs' offsets, the alignment lines per slice of lines, the walk's
    // result block of 64 bytes
    struct Sam { DevBuf d_counts, d_tabs, d_frames, d_out; } sam;
    // ---- the read block report (read_blocks.cpp): the record table of a *_block_lines call, the segments' name entries, the
    // workgroups' sums and the text
    struct Blocks { DevBuf d_recs, d_segs, d_sums, d_text; } blocks;
    // ---- FASTQ out of a BAM or SAM chunk (read_fastq.cpp): the kept records' table entries, their text's sizes, their first
    // jobs and the jobs
    struct FastqOut { DevBuf d_table, d_sizes, d_job_base, d_jobs; } fastq_out;
};

// the tail [carry_from, plain_n) of the chunk's bytes to its front, on st (through d_tmp where the two overlap); -> the tail's length
int  ts_chunk_carry(ts_bam_chunk *ch, uint64_t carry_from, hipStream_t st, uint64_t *carry);

// room for stage_cap staged bytes (what is staged is kept); waits for the device when the region grows
int  ts_chunk_stage_reserve(ts_bam_chunk *ch, uint64_t stage_cap);

// The line index of the chunk's bytes, on the null stream: '\n' counted per slice and summed (its two words come back through
// ch->d_out and are checked against the chunk), then every line's start, first byte and '\r' flag into ch->lines.d_lines
// (launched, not waited for).  *ix = ch->lines.ix.  A failure is "<who>: ..." in the context's error; `counted` names what "left
// the chunk".
int  ts_chunk_line_index(ts_bam_chunk *ch, int at_end, const char *who, const char *counted, LineIndex *ix);
// does line index `generation` still describe the chunk's bytes, read with this at_end?
inline bool ts_chunk_lines_current(const ts_bam_chunk *ch, uint64_t generation, int at_end) {
    const ts_bam_chunk::Lines &l = ch->lines;
    return l.valid && l.generation == generation && l.size == ch->plain_n && (l.at_end != 0) == (at_end != 0);
}

// The host half of ts_bam_chunk_gather and ts_fastq_chunk_gather behind their argument checks: the table of n records of rec_bytes
// each goes up, `plan` places the passing records, its totals come back as *bytes / *n_passed and are held against cap, `copy`
// moves the records, the bytes come down.  Failures are "<who>: ...".
typedef int (*ts_chunk_plan_launch)(const void *recs, const void *pass, unsigned long long n, void *dst_off, void *totals, void *stream);
typedef int (*ts_chunk_copy_launch)(const void *plain, const void *recs, const void *dst_off, unsigned long long n,
                                    unsigned long long cap, void *out, void *stream);
int  ts_chunk_gather(ts_bam_chunk *ch, const char *who, const void *recs, size_t rec_bytes, size_t n, const void *d_pass,
                     void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream, ts_chunk_plan_launch plan,
                     ts_chunk_copy_launch copy);
// ... up to the copy kernel: the passing records' bytes stay in ch->d_gather (launched on `stream`, not waited for); cap bounds
// *bytes as above
int  ts_chunk_gather_device(ts_bam_chunk *ch, const char *who, const void *recs, size_t rec_bytes, size_t n, const void *d_pass,
                            uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream, ts_chunk_plan_launch plan,
                            ts_chunk_copy_launch copy);

// The host half of ts_fastq_chunk_stage, ts_sam_chunk_stage and ts_bam_chunk_decode behind their null check: `reads` must be an
// unrestricted tips-only batch of the chunk's context with one segment per record; record(ch, recs, i, &src, &len) holds record i
// against the chunk by the route's rule and says where its len bases begin in the chunk; every record becomes jobs of `piece` bases
// whose sources lie src_step bytes apart; the jobs go up into ch->d_jobs and `launch` is called on `stream` (not waited for).
// Failures are "<who>: ...".
struct ChunkStageJob { unsigned long long src, dst; uint32_t n, pad; };     // n bases from plain + src -> in + dst (16-byte aligned)
typedef bool (*ts_chunk_stage_record)(const ts_bam_chunk *ch, const void *recs, size_t i, uint64_t *src, uint32_t *len);
typedef int (*ts_chunk_stage_launch)(const void *plain, const void *jobs, uint32_t n_jobs, void *in, void *stream);
int  ts_chunk_stage_records(ts_bam_chunk *ch, const char *who, const void *recs, size_t n, ts_batch *reads, void *stream, uint32_t piece,
                            uint32_t src_step, ts_chunk_stage_record record, ts_chunk_stage_launch launch);

// ---- deflate.cpp
// d_plain[0, n) (device memory of ctx's device) cut into payloads of payload_bytes (1 .. 0xff00), each deflated into one BGZF
// member on the device (deflate.hip), the members packed and downloaded to host_out: *bytes of them, *n_members.  When *bytes >
// cap nothing is copied: TS_ERR_INVALID_ARG.  Ordered on `stream`; waits for it.  Counts into ctx->bgzf_deflate_stats.
int  ts_deflate_members(ts_ctx *ctx, const char *who, const void *d_plain, uint64_t n, uint32_t payload_bytes, DeflateBufs &bufs,
                        void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_members, void *stream);

// ---- chunk.hip
extern "C" {
// '\n' per slice of kChunkSliceBytes -> counts[n_slices]; then (one wave) counts -> exclusive sums in place,
// out[kChunkNewlines] = their total, out[kChunkTail] = 1 when the last byte is not '\n'
int ts_k_launch_chunk_newline_count(const void *plain, unsigned long long n, uint32_t *counts, unsigned long long *out, void *stream);
// the line index from the sums: newlines + 2 entries each
int ts_k_launch_chunk_newline_index(const void *plain, unsigned long long n, const uint32_t *sums, uint32_t newlines, uint32_t tail,
                                    uint32_t *lstart, unsigned char *first, unsigned char *cr, void *stream);
// '\t' per slice of kChunkSliceBytes -> counts[n_slices]
int ts_k_launch_chunk_tab_count(const void *plain, unsigned long long n, uint32_t *counts, void *stream);
// every tab's offset in order (sums: the exclusive sums of the counts)
int ts_k_launch_chunk_tab_index(const void *plain, unsigned long long n, const uint32_t *sums, uint32_t n_tabs, uint32_t *tabs,
                                void *stream);
// counts[n] -> exclusive sums in place (one wave), *total = their sum
int ts_k_launch_chunk_scan(uint32_t *counts, uint32_t n, unsigned long long *total, void *stream);
// dst_off[i] = where passing record i goes (~0: it does not pass), totals = {bytes, records}: 1 + size per ts_fastq_record (a
// '\n' behind each), 4 + block_size per ts_bam_record
int ts_k_launch_chunk_gather_plan_fastq(const void *recs, const void *pass, unsigned long long n, void *dst_off, void *totals, void *stream);
int ts_k_launch_chunk_gather_plan_bam(const void *recs, const void *pass, unsigned long long n, void *dst_off, void *totals, void *stream);
}
