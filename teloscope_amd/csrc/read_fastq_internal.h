// read_fastq_internal.h — what read_fastq.cpp (host glue) and read_fastq.hip (kernels) of the FASTQ-out gathers share: the
// launchers' parameters and the words that come back.  The text's rule is read_fastq_format_core.h.
#pragma once

#include <stdint.h>

#include "read_fastq_format_core.h"

// a piece of a kept record's text: piece `piece` of record `rec` (pieces are cut at multiples of tsfq::kPieceBytes of the output
// counted from the 16-byte boundary at or in front of the record's first byte, so every piece but a record's first starts on one)
struct TsFastqOutJob { uint32_t rec, piece; };
// words of the plan's result (unsigned long long each): text bytes, kept records, jobs
enum { kFqBytes = 0, kFqKept, kFqJobs, kFqWords };

struct TsFastqOutParams {
    const void *recs;                   // the chunk's record table: ts_bam_record or ts_sam_record by `kind` (tsfq::kBam / kSam)
    const unsigned char *pass;
    const unsigned char *chunk;
    tsfq::Rec *table;                   // per record: where its fields lie (written for kept records only)
    unsigned long long *sizes;          // per record: its text's bytes, 0 when its pass byte is clear
    unsigned long long *dst_off;        // per record: where its text starts in out (~0: not kept)
    uint32_t *job_base;                 // per record: its first job
    unsigned long long *totals;         // kFqWords
    TsFastqOutJob *jobs;
    unsigned char *out;                 // 16-byte aligned
    unsigned long long cap;             // bytes of out
    uint32_t n, kind, out_flags, n_jobs;
};

// sizes and table (a lane per record), then the plan (one wave): dst_off, job_base, totals
int ts_k_launch_read_fastq_plan(const TsFastqOutParams *P, void *stream);
// the job list (a lane per record), then the text (a wave per job)
int ts_k_launch_read_fastq_write(const TsFastqOutParams *P, void *stream);
