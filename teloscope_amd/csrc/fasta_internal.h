// fasta_internal.h — what fasta.cpp (host glue) and fasta.hip (kernels) of the device FASTA route share: the launchers and
// the layouts both sides count with.  The line index underneath and the sums of the join's and the runs' counts are the chunk
// layer's (chunk_internal.h).
#pragma once

#include <stdint.h>

constexpr uint32_t kFastaSliceLines = 2048;         // lines a wave of the header scan takes
constexpr uint32_t kFastaSliceBytes = 16384;        // bytes of body text (join) or of joined bases (runs) a wave takes
// words of the FASTA result block (unsigned long long each)
enum { kFaHeaders = 0, kFaCrs, kFaNameBytes, kFaLastLine, kFaTotal, kFaRunTotal, kFaWords };
struct FastaFrame { uint32_t headers, crs, name_bytes, pad; };       // a slice of lines: its header lines, its lines that end in "\r\n",
                                                                      // the bytes of its headers' names; after the scan: those before it
struct FastaHead { uint32_t line, crs_before, names_before, pad; };  // a header line: its index, the "\r\n" lines and name bytes before it
// body text [a, z) of the chunk, a piece of one record that lies inside one 16 KB slice: its kept bytes go to
// dst_rec + (kept bytes of the record's jobs before this one), and never to or beyond limit; the record's last job also
// zeroes the bytes from limit to the next multiple of 16, where the next record begins
struct FastaJoinJob { uint32_t a, z, first, last; unsigned long long dst_rec, limit; };
// the jobs [first, first + n) of the stage's list are one record's, n >= 2: what its segmented sum runs over
struct FastaStageSpan { uint32_t first, n; };
// joined bases [a, z) of one record, which begins at rec_begin (a multiple of 16), inside one 16 KB slice of the joined buffer
struct FastaRunJob { unsigned long long a, z, rec_begin; uint32_t rec, pad; };
// body text [a, z) of the chunk, a piece of record `rec` of the strict check's table that lies inside one 16 KB slice
struct FastaStrictJob { uint32_t a, z, rec, pad; };

extern "C" {
// header lines, "\r\n" lines and name bytes per slice of kFastaSliceLines -> frames; then (one wave) frames -> exclusive sums in
// place, out[kFaHeaders / kFaCrs / kFaNameBytes] = the totals, out[kFaLastLine] = lstart[newlines]
int ts_k_launch_fasta_frames(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                             uint32_t newlines, void *frames, unsigned long long *out, void *stream);
// heads[r] for every header line in order, and the sentinel heads[n_heads] = {n_lines, all crs, all name bytes}
int ts_k_launch_fasta_heads(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                            const void *frames, void *heads, uint32_t n_heads, uint32_t crs, uint32_t name_bytes, void *stream);
// the record table from the heads (a lane per record), then the names gathered (a wave per record)
int ts_k_launch_fasta_records(const void *plain, unsigned long long size, const uint32_t *lstart, const unsigned char *cr,
                              const void *heads, uint32_t n_heads, void *recs, void *names, void *stream);
// kept bytes per join job -> counts[n_jobs]
int ts_k_launch_fasta_join_count(const void *plain, unsigned long long size, int at_end, const void *jobs, uint32_t n_jobs,
                                 uint32_t *counts, void *stream);
int ts_k_launch_fasta_join_write(const void *plain, unsigned long long size, int at_end, const void *jobs, uint32_t n_jobs,
                                 const uint32_t *sums, void *joined, void *stream);
// The read stage: the jobs are the join's, dst_rec / limit a segment of a read batch's input buffer `in`; spans names the records
// of two jobs or more.  Their jobs are counted into counts[n_jobs], summed per record in place, and every job's kept bytes are
// written (a record's only job without a count).  Launched on `stream`, not waited for.
int ts_k_launch_fasta_stage(const void *plain, unsigned long long size, int at_end, const void *jobs, uint32_t n_jobs,
                            const void *spans, uint32_t n_spans, uint32_t *counts, void *in, void *stream);
// run starts per run job -> counts[n_jobs]; after the scan, the runs' {record, is_gap, start}; then every run's length
int ts_k_launch_fasta_run_count(const void *joined, const void *jobs, uint32_t n_jobs, uint32_t *counts, void *stream);
int ts_k_launch_fasta_run_write(const void *joined, const void *jobs, uint32_t n_jobs, const uint32_t *sums, void *runs,
                                unsigned long long n_runs, void *stream);
int ts_k_launch_fasta_run_lengths(void *runs, unsigned long long n_runs, const void *recs, uint32_t n_recs, void *stream);
// has[job.rec] = 1 for every job whose body text holds a byte other than '\n' and '\r' (has: a byte per record, zero before)
int ts_k_launch_fasta_strict(const void *plain, unsigned long long size, const void *jobs, uint32_t n_jobs, unsigned char *has,
                             void *stream);
}
