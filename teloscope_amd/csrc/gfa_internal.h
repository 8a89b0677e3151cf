// gfa_internal.h — what gfa.cpp (host glue) and gfa.hip (kernels) of the device GFA route share: the launchers and the layouts
// both sides count with.  The line index underneath, the tab index and the sums of the counts are the chunk layer's
// (chunk_internal.h).
#pragma once

#include <stdint.h>

#include "chunk_internal.h"

constexpr uint32_t kGfaSliceLines = 2048;           // lines a wave of the kind passes takes
// words of the GFA result block (unsigned long long each)
enum { kGfSegs = 0, kGfLines, kGfTextBytes, kGfForeignLine, kGfForeignOff, kGfForeignLen, kGfTabs, kGfLastLine, kGfWords };
// a line's kind byte: bits 0..1 what the tables keep of it, bit 7 "foreign" (readGfa's rule for a GFA 2 input)
constexpr uint32_t kGfaNothing = 0, kGfaSegment = 1, kGfaPath = 2, kGfaHeader = 3, kGfaForeign = 0x80;
// a slice of lines: its segments, its P / H lines and the bytes they gather; after the scan: those before it
struct GfaFrame { uint32_t segs, lines, text_bytes, pad; };

extern "C" {
// every line's kind byte and the counts per slice of kGfaSliceLines -> frames, the lowest foreign line by an atomic minimum on
// out[kGfForeignLine] (set to ~0 before); then (one wave) frames -> exclusive sums in place, out[kGfSegs / kGfLines / kGfTextBytes]
// = the totals, out[kGfForeignOff / kGfForeignLen] = the lowest foreign line's offset and first field, out[kGfLastLine] =
// lstart[newlines]
int ts_k_launch_gfa_kinds(const void *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                          uint32_t n_lines, uint32_t newlines, const uint32_t *tabs, uint32_t n_tabs, unsigned char *kinds,
                          void *frames, unsigned long long *out, void *stream);
// the segment table and the P / H line table, every entry with its place in the gathered text
int ts_k_launch_gfa_tables(const void *plain, const uint32_t *lstart, const unsigned char *cr, uint32_t n_lines,
                           const uint32_t *tabs, uint32_t n_tabs, const unsigned char *kinds, const void *frames, void *segs,
                           uint32_t n_segs, void *lines, uint32_t n_kept, void *stream);
// the segments' names and the P / H lines whole into text (a wave per item)
int ts_k_launch_gfa_gather(const void *plain, unsigned long long size, const void *segs, uint32_t n_segs, const void *lines,
                           uint32_t n_kept, void *text, unsigned long long text_bytes, void *stream);
// the filtered loader's check (ts_gfa_chunk_check).  stray[i] = 1 for every line that holds a '\r' anywhere but as the last byte
// of its content (stray: a byte per line, zero before): a wave per slice of kChunkSliceBytes, the line found by a search of lstart
int ts_k_launch_gfa_stray_cr(const void *plain, unsigned long long n, int at_end, const uint32_t *lstart, uint32_t n_lines,
                             unsigned char *stray, void *stream);
// every line's code byte (0: nothing to say) and the flagged lines per slice of kGfaSliceLines -> counts
int ts_k_launch_gfa_check(const void *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                          uint32_t n_lines, const uint32_t *tabs, uint32_t n_tabs, const unsigned char *stray, unsigned char *codes,
                          uint32_t *counts, void *stream);
// the flagged lines in input order (sums: the exclusive sums of the counts)
int ts_k_launch_gfa_flagged(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                            const unsigned char *codes, const uint32_t *sums, void *flagged, uint32_t n_flagged, void *stream);
}
