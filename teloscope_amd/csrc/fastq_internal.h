// fastq_internal.h — what fastq.cpp (host glue) and fastq.hip (kernels) of the device FASTQ route share: the launchers and the
// sizes both sides count with.
#pragma once

#include <stdint.h>

#include "chunk_internal.h"

constexpr uint32_t kFastqSliceLines = 2048;         // lines a wave of the framing scan takes
constexpr uint32_t kFastqStagePiece = 8192;         // bytes of a sequence a wave of the stage copies
// words of the walk's result block (unsigned long long each), behind the line count's
enum { kFqHeaders = kChunkLineWords, kFqError, kFqOpen, kFqOpenOff, kFqLastLine, kFqWords };
struct FastqFrame { uint32_t map, cnt[4], pad[3]; };        // a slice of lines: its transition map, its headers per entry state
struct FastqEntry { uint32_t state, base; };                // a slice's entry state and the index of its first record
using FastqCopyJob = ChunkStageJob;                         // the stage kernel's job: n bytes at plain + src -> in + dst

extern "C" {
// the framing automaton over n_lines lines: frames per slice of kFastqSliceLines, their scan (entry states and record bases,
// out[kFqHeaders], out[kFqLastLine] = lstart[newlines]; the error and open-record words are reset), then the record table
int ts_k_launch_fastq_frames(const uint32_t *lstart, const unsigned char *cr, uint32_t n_lines, uint32_t newlines, void *frames,
                             void *entries, unsigned long long *out, void *stream);
int ts_k_launch_fastq_records(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                              int at_end, const void *entries, void *recs, unsigned long long *out, void *stream);
int ts_k_launch_fastq_stage(const void *plain, const void *jobs, uint32_t n_jobs, void *in, void *stream);
int ts_k_launch_fastq_gather(const void *plain, const void *recs, const void *dst_off, unsigned long long n, unsigned long long cap,
                             void *out, void *stream);
// interleaved pairs: *lowest = min(*lowest, the lowest j < n_pairs for which recs[2 j] and recs[2 j + 1] are not mates); both bytes
// of a pair in pair_pass from the mates' own pass bytes
int ts_k_launch_fastq_mates(const void *plain, unsigned long long n_bytes, const void *recs, unsigned long long n_pairs,
                            unsigned long long *lowest, void *stream);
int ts_k_launch_fastq_pair_pass(const void *read_of, const void *pass, unsigned long long n_pairs, void *pair_pass, void *stream);
}
