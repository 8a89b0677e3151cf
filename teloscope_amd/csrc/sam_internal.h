// sam_internal.h — what sam.cpp (host glue) and sam.hip (kernels) of the device SAM route share: the launchers and the sizes
// both sides count with.  The stage's jobs and kernel and the gather's plan and copy are the FASTQ route's (fastq_internal.h,
// chunk_internal.h): ts_sam_record has ts_fastq_record's layout where those kernels read it (off, size).
#pragma once

#include <stdint.h>

#include "fastq_internal.h"

constexpr uint32_t kSamSliceLines = 2048;           // lines a wave of the kind count and of the record pass takes
// words of the walk's result block (unsigned long long each): the chunk's tabs, the lowest alignment line (~0: none), the lowest
// bad line << 3 | its code (~0: none), the alignment lines, the end of the whole lines
enum { kSmTabs = 0, kSmFirstAlign, kSmError, kSmAligns, kSmLastLine, kSmWords };

extern "C" {
// alignment lines (first byte not '@') per slice of kSamSliceLines -> counts[n_slices]; the lowest one into out[kSmFirstAlign]
// by an atomic minimum (the caller has set the word to ~0)
int ts_k_launch_sam_kinds(const unsigned char *first, uint32_t n_lines, uint32_t *counts, unsigned long long *out, void *stream);
// the record table from the counts' exclusive sums: alignment line number r of the chunk -> recs[r] when r < n_recs; the lowest
// line that fails a check into out[kSmError] by an atomic minimum (the caller has set the word to ~0); out[kSmLastLine] =
// lstart[newlines]
int ts_k_launch_sam_records(const void *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                            uint32_t n_lines, uint32_t newlines, const uint32_t *tabs, uint32_t n_tabs, int in_header,
                            const uint32_t *sums, void *recs, uint32_t n_recs, unsigned long long *out, void *stream);
}
