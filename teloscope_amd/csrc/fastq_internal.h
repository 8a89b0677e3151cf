// fastq_internal.h — what fastq.cpp (host glue) and fastq.hip (kernels) of the device FASTQ route share: the launchers and the
// sizes both sides count with.
#pragma once

#include <stdint.h>

constexpr uint32_t kFastqSliceBytes = 16384;        // bytes of the chunk a wave of the line index takes
constexpr uint32_t kFastqSliceLines = 2048;         // lines a wave of the framing scan takes
constexpr uint32_t kFastqStagePiece = 8192;         // bytes of a sequence a wave of the stage copies
// words of the walk's result block (unsigned long long each)
enum { kFqNewlines = 0, kFqTail, kFqHeaders, kFqError, kFqOpen, kFqOpenOff, kFqLastLine, kFqWords };
struct FastqFrame { uint32_t map, cnt[4], pad[3]; };        // a slice of lines: its transition map, its headers per entry state
struct FastqEntry { uint32_t state, base; };                // a slice's entry state and the index of its first record
struct FastqCopyJob { unsigned long long src, dst; uint32_t n, pad; };       // n bytes at plain + src -> in + dst (16-byte aligned)

// The line index the FASTQ, FASTA and GFA walks begin with (fastq.cpp), on the null stream: '\n' counted per slice and summed
// (ts_k_launch_fastq_count; its two words come back through ch->d_out and are checked against the chunk), then every line's
// start, first byte and '\r' flag into ch->d_lines (ts_k_launch_fastq_index: launched, not waited for).  n_lines counts the
// unfinished last line with at_end only.  A failure is "<who>: ..." in the context's error; `counted` names what "left the chunk".
struct ts_bam_chunk;
struct FastqLineIndex { uint64_t newlines, tail, n_lines; uint32_t *lstart; unsigned char *first, *cr; };
int ts_chunk_line_index(ts_bam_chunk *ch, int at_end, const char *who, const char *counted, FastqLineIndex *ix);

extern "C" {
// '\n' per slice of kFastqSliceBytes -> counts[n_slices]; then (one wave) counts -> exclusive sums in place,
// out[kFqNewlines] = their total, out[kFqTail] = 1 when the last byte is not '\n'
int ts_k_launch_fastq_count(const void *plain, unsigned long long n, uint32_t *counts, unsigned long long *out, void *stream);
// line i starts at lstart[i] and begins with first[i]; cr[i] = 1 when a '\r' stands before its end; lines = newlines + 2 entries
int ts_k_launch_fastq_index(const void *plain, unsigned long long n, const uint32_t *bases, uint32_t newlines, uint32_t tail,
                            uint32_t *lstart, unsigned char *first, unsigned char *cr, void *stream);
// the framing automaton over n_lines lines: frames per slice of kFastqSliceLines, their scan (entry states and record bases,
// out[kFqHeaders], out[kFqLastLine] = lstart[newlines]; the error and open-record words are reset), then the record table
int ts_k_launch_fastq_frames(const uint32_t *lstart, const unsigned char *cr, uint32_t n_lines, uint32_t newlines, void *frames,
                             void *entries, unsigned long long *out, void *stream);
int ts_k_launch_fastq_records(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                              int at_end, const void *entries, void *recs, unsigned long long *out, void *stream);
int ts_k_launch_fastq_stage(const void *plain, const void *jobs, uint32_t n_jobs, void *in, void *stream);
int ts_k_launch_fastq_gather_plan(const void *recs, const void *pass, unsigned long long n, void *dst_off, void *totals, void *stream);
int ts_k_launch_fastq_gather(const void *plain, const void *recs, const void *dst_off, unsigned long long n, unsigned long long cap,
                             void *out, void *stream);
}
