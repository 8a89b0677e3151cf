/*
 * teloscan.h — C-ABI of libteloscan.so: the MI355X (gfx950) implementation of
 * Teloscope's telomeric-motif scan path.
 *
 * This is the drop-in boundary.  The reference has no plugin registry; the seam
 * is two C++ member functions,
 *
 *     SegmentData Teloscope::scanSegment(std::string&, uint64_t absPos, bool tipsOnly);
 *                                                   (include/teloscope.h:260, src/teloscope.cpp:537)
 *     bool        ReadTelomereFilter::matches(std::string);
 *                                                   (include/read-filter.h:16, src/read-filter.cpp:37)
 *
 * and every entry point below names the reference interface it replaces.
 * Plain pointers and sizes only; no C++ or torch types.  All functions that
 * return int return TS_OK (0) or a negative ts_status; ts_last_error() gives
 * the text.  The library never calls exit().
 *
 * There is no CPU fallback: if no HIP device is usable, ts_create() fails
 * with TS_ERR_NO_DEVICE.
 */
#ifndef TELOSCAN_H
#define TELOSCAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TELOSCAN_ABI_VERSION 4

/* ts_params.device value of a PLANNING-ONLY context: no HIP call is ever made behind it.  It plans batches
 * (ts_batch_create, ts_batch_get_info, ts_batch_get_tiles, ts_batch_partition, ts_batch_range_info) so that a
 * host without a GPU — the rank that only merges, a test — sees the same tiling as the ranks that scan; every
 * entry point that needs the device fails on it with TS_ERR_NO_DEVICE.  It is not a CPU scan path. */
#define TS_DEVICE_NONE (-2)

typedef enum ts_status {
    TS_OK               =  0,
    TS_ERR_INVALID_ARG  = -1,
    TS_ERR_NO_DEVICE    = -2,   /* no usable HIP device (no CPU fallback exists) */
    TS_ERR_HIP          = -3,   /* a HIP runtime call failed */
    TS_ERR_ALLOC        = -4,
    TS_ERR_UNSUPPORTED  = -5,   /* parameter set no device path implements (pattern > 32 bases, > 8 lengths, ...) */
    TS_ERR_STATE        = -6
} ts_status;

/* ScaffoldType, include/tools.h:13-19 (same enumerator order). */
typedef enum ts_scaffold_type {
    TS_T2T = 0, TS_GAPPED_T2T, TS_MISASSEMBLY, TS_GAPPED_MISASSEMBLY,
    TS_INCOMPLETE, TS_GAPPED_INCOMPLETE, TS_NONE, TS_GAPPED_NONE,
    TS_DISCORDANT, TS_GAPPED_DISCORDANT
} ts_scaffold_type;

/* One expanded search pattern = one element of UserInputTeloscope::patternInfo
 * plus the isCanonical flag the Teloscope ctor derives (include/teloscope.h:241-247). */
typedef struct ts_pattern {
    char    seq[64];        /* NUL-terminated, A/C/G/T only */
    uint8_t len;
    uint8_t is_forward;
    uint8_t is_canonical;
    uint8_t reserved;
} ts_pattern;

/* The fields of UserInputTeloscope (include/input.h:15-64) the scan path reads. */
typedef struct ts_params {
    uint32_t struct_size;        /* = sizeof(ts_params), for ABI growth */
    uint32_t window_size;        /* -w, default 1000 */
    uint32_t step;               /* -s, default 1000, must be <= window_size */
    uint32_t terminal_limit;     /* -t, default 50000 */
    uint16_t max_match_dist;     /* -k, default 50 */
    uint16_t min_block_len;      /* -l, default 300 */
    uint16_t max_block_dist;     /* -d, default 500 */
    uint16_t min_block_counts;   /* default 2 */
    float    min_block_density;  /* -y, default 0.5 */
    uint16_t canonical_size;     /* strlen(canonical) */
    uint8_t  out_gc;             /* -g : nucleotide counts + gc_content are produced */
    uint8_t  out_entropy;        /* -e : nucleotide counts + shannon_entropy */
    uint8_t  out_matches;        /* -m */
    uint8_t  out_its;            /* -i */
    uint8_t  fold_case;          /* 1: a/c/g/t match like A/C/G/T (what every reference
                                       caller gets by calling unmaskSequence first);
                                    0: strict scanSegment semantics (lower case = non-ACGT) */
    uint8_t  out_win_repeats;    /* -r : read only by the window tracks' formatter (ts_window_tracks_format, ts_scan_segments_tracks): the
                                    density, canonical-ratio and strand-ratio tracks exist.  (Was reserved and zero: no other entry
                                    point looks at it — the covered counts of a window are always produced.) */
    int32_t  device;             /* HIP device ordinal, -1 = current device, TS_DEVICE_NONE = planning only */
    uint32_t reserved1;
} ts_params;

/* MatchInfo, include/teloscope.h:89-95 (matchSeq is seq.substr(position-absPos, match_size)). */
#define TS_MATCH_FORWARD   0x1u
#define TS_MATCH_CANONICAL 0x2u
#define TS_MATCH_TERMINAL  0x4u   /* isTerminal of src/teloscope.cpp:451-459 */
typedef struct ts_match {
    uint64_t position;
    uint16_t match_size;
    uint8_t  flags;
    uint8_t  reserved[5];
} ts_match;

/* WindowData, include/teloscope.h:119-137, without the fields no writer reads. */
typedef struct ts_window {
    uint64_t window_start;           /* absolute (absPos + window offset) */
    uint32_t current_window_size;
    uint32_t nucleotide_counts[4];   /* A C G T; zero unless out_gc || out_entropy */
    float    gc_content;             /* getGCContent, include/teloscope.h:211 (if out_gc) */
    float    shannon_entropy;        /* getShannonEntropy, include/teloscope.h:199 (if out_entropy) */
    uint32_t canonical_covered;
    uint32_t non_canonical_covered;
    uint32_t fwd_covered;
    uint32_t rev_covered;
    uint32_t reserved;
} ts_window;

/* TelomereBlock, include/teloscope.h:103-117. */
typedef struct ts_block {
    uint64_t start;
    uint32_t block_len;
    uint32_t block_counts;
    uint32_t forward_count;
    uint32_t reverse_count;
    uint32_t canonical_count;
    uint32_t non_canonical_count;
    uint32_t total_covered;
    uint32_t fwd_covered;
    uint32_t can_covered;
    uint8_t  has_valid_or;
    uint8_t  is_longest;
    char     block_label;
    uint8_t  reserved;
} ts_block;

/* One scanSegment() call: (sequence, absPos, tipsOnly).
 *
 * input_format TS_INPUT_BASES (0): `seq` points to the segment's `len` bases.
 * input_format TS_INPUT_TEXT_PIECES: `seq` points to a ts_text_piece array instead — FASTA body text as it lies in the
 * file, line ends included; the pieces, in order, hold the segment's `len` bases.  The library skips the line ends while
 * it stages the bases for upload, so a front end never has to join the lines of a record into one buffer (what gfalibs
 * does before walkPath, and the largest host cost once the scan itself takes milliseconds).  The entry points read
 * pieces until `len` bases are covered (at most `n_pieces` of them); of the last piece only what is needed. */
#define TS_INPUT_BASES       0
#define TS_INPUT_TEXT_PIECES 1
#define TS_INPUT_PACKED2     2
#define TS_INPUT_DEVICE      3
typedef struct ts_text_piece {
    const char *text;        /* text_len bytes: n_bases bases and the line ends between / behind them ('\n', and a '\r'
                                right before one or at the very end of the piece) */
    uint64_t    text_len;    /* at most 16 MiB */
    uint64_t    n_bases;
} ts_text_piece;
/* input_format TS_INPUT_PACKED2: `seq` points to ONE ts_packed_seq — the segment's bases already as 2-bit codes (four per
 * byte, base i at bits 2 (i & 3) of byte i >> 2; A 0, C 1, T 2, G 3: what ts_pack_bases writes) plus the runs of positions
 * that are not A/C/G/T (after case folding, if the context folds case), ascending and non-overlapping, segment-relative.
 * A front end that parses FASTA touches every base once anyway: packing there (ts_pack_bases, or its own loop) means the
 * bases are read from host memory ONCE between the file and the PCIe link — the library's staging threads then copy a
 * quarter of the bytes instead of reading the ASCII a second time, which is what bounds the host entry points once the
 * link carries packed bases.  Results cannot depend on the input format: the device restores the same
 * byte layout ('N' over the runs) that TS_INPUT_BASES uploads.  Tiled kernel's parameter sets only, like the text pieces. */
/* input_format TS_INPUT_DEVICE: `seq` is a DEVICE pointer, on the context's device, to the segment's `len` bases — raw ASCII in
 * any case, non-ACGT bytes as they are: exactly the bytes TS_INPUT_BASES would have uploaded, so results are byte-equal to
 * that format's.  The bases are gathered on the device into the scan's input layout (no pinned buffer, no host thread, nothing
 * over PCIe): all the device segments of a call by ONE kernel over a job list, a wave per 16 KiB at most — 10^5 small segments
 * cost one launch, not 10^5 copies; a piece of 8 MiB or more keeps a device-to-device copy of its own (ts_device_input_stats
 * counts both).  Any address will do — the kernel reads no aligned word that holds no byte of the segment, so the allocation
 * may end with the segment's last byte — and the writes that produced them must be complete when the call is made (the gather
 * runs on a stream of the library's own).  Any parameter set, full and tips-only scans, mixed freely with host segments in one call; not
 * ts_scan_segments_multi (the pointer belongs to one device).  Stands in for the std::string& that scanSegment borrows
 * (include/teloscope.h:260) when a front end has produced the bases on the device (the FASTA route's joined records). */
typedef struct ts_packed_run { uint64_t start, len; } ts_packed_run;
typedef struct ts_packed_seq {
    const uint8_t       *codes;     /* (len + 3) / 4 bytes */
    const ts_packed_run *runs;      /* may be NULL when n_runs == 0 */
    uint64_t             n_runs;
} ts_packed_seq;
typedef struct ts_segment_in {
    const char *seq;        /* borrowed for the duration of the call; need not be NUL-terminated (TS_INPUT_DEVICE: device memory) */
    uint64_t    len;
    uint64_t    abs_pos;
    uint8_t     tips_only;
    uint8_t     input_format;   /* TS_INPUT_BASES / TS_INPUT_TEXT_PIECES / TS_INPUT_PACKED2 / TS_INPUT_DEVICE (any parameter set the library scans) */
    uint8_t     reserved[2];
    uint32_t    n_pieces;       /* TS_INPUT_TEXT_PIECES: entries of the ts_text_piece array (the walk never reads past it;
                                   pieces that hold fewer than `len` bases are TS_ERR_INVALID_ARG) */
} ts_segment_in;

/* SegmentData, include/teloscope.h:139-148.  `matches` holds what the
 * reference pushes to allMatches (full scan) or to fwdMatches+revMatches
 * (tips-only), in the reference's push order; the other reference vectors are
 * subsequences selected by flags:
 *   canonicalMatches     = flags & CANONICAL                  (full scan only)
 *   nonCanonicalMatches  = !(flags & CANONICAL) && TERMINAL   (full scan only)
 *   fwdMatches / revMatches = flags & FORWARD / not
 * Arrays are owned by the library until ts_free_segments(). */
typedef struct ts_segment_out {
    ts_window *windows;             uint64_t n_windows;
    ts_match  *matches;             uint64_t n_matches;
    ts_block  *terminal_blocks;     uint64_t n_terminal_blocks;
    ts_block  *interstitial_blocks; uint64_t n_interstitial_blocks;
} ts_segment_out;

typedef struct ts_ctx   ts_ctx;
typedef struct ts_batch ts_batch;

int         ts_abi_version(void);
const char *ts_last_error(const ts_ctx *ctx);      /* ctx may be NULL: last create error */
int         ts_device_count(void);                 /* usable HIP devices, 0 if none */

/* ---- pattern preparation: expandPatternsWithOrientation, src/tools.cpp:201-283,
 *      plus the canonical-orientation rule of src/main.cpp:287-296. ---------------- */
/* canonical_in: the -c argument (upper-cased by the callee). Writes the
 * lexicographically smaller of (canonical, revcomp) to fwd_out, the other to rev_out
 * (each >= 64 bytes). */
int ts_canonical_orientation(const char *canonical_in, char *fwd_out, char *rev_out);
/* raw_csv: comma-separated -p list (IUPAC allowed). On success *out is a malloc'd
 * array of *n_out patterns sorted like the reference's patternInfo; free with
 * ts_free_patterns(). */
int  ts_expand_patterns(const char *raw_csv, int edit_distance, const char *canonical_fwd,
                        ts_pattern **out, size_t *n_out);
void ts_free_patterns(ts_pattern *p);

/* ---- context: the Teloscope object (ctor include/teloscope.h:241-247). Builds the
 *      k-mer match tables on the device.  Thread-safe for concurrent scan/filter calls, and made for them: the reference
 *      calls scanSegment / matches from all its pool workers at once (src/input.cpp:977, :786, src/bam.cpp:217-220), and
 *      calls that arrive while the device is busy are COALESCED — the next run takes every waiting call of one kind
 *      (ts_scan_segments, ts_scan_segments_blocks, ts_filter_reads; full scans and tips-only apart) as one batch and hands
 *      each caller its own results.  Sixty-four threads with one segment each cost about what one call with sixty-four
 *      segments costs; results never depend on who was merged with whom.
 *      LIMITS of the pattern set (the reference's trie has none, include/teloscope.h:40-57): what a ts_pattern[] can express — a
 *      pattern of up to 63 bases, hence up to 63 distinct lengths — is scanned; a longer pattern is refused by ts_create and by
 *      ts_expand_patterns (never truncated), a non-ACGT pattern makes every scan fail with TS_ERR_UNSUPPORTED (loudly: there
 *      is no CPU path to fall back to).  Uniform-length sets of 3..8 bases under w == s or k <= min(s, w - s) take the tiled
 *      kernel; sets of up to 8 distinct lengths of up to 32 bases the general kernels' table forms; everything else the
 *      general kernels' wide form (128-bit codes; a correct path for rare sets, not a fast one). */
ts_ctx *ts_create(const ts_params *params, const ts_pattern *patterns, size_t n_patterns);
void    ts_destroy(ts_ctx *ctx);
/* 1 if full scans with this (window, step, patterns) run on the tiled uniform-k kernel,
 * 0 if on the general kernels (mixed-length sets, k > 9, or a longest pattern exceeding
 * min(step, window-step), where the reference's start-index arithmetic wraps). */
int     ts_uses_fast_path(const ts_ctx *ctx);
/* Measurement aid (no counterpart in the reference): what THIS device issues — wave-instructions per ns of hand-written
 * independent integer instructions at four waves per SIMD — and streams — read + write bytes per ns of a 1 GiB copy —, so that
 * a benchmark line from a box that runs everything a few per cent slower can be told from a slower kernel (bench.py: roofline.box). */
int     ts_box_probe(ts_ctx *ctx, double *valu_wave_instr_per_ns, double *copy_bytes_per_ns);
/* 1 if segments of this kind (full scan / tips-only) may come as TS_INPUT_TEXT_PIECES, TS_INPUT_PACKED2 or TS_INPUT_DEVICE:
 * every parameter set the library scans (until ABI 3 the general kernels wanted the bases joined). */
int     ts_takes_text_input(const ts_ctx *ctx, int tips_only);
/* Measurement aid (no counterpart in the reference): what the context has done with TS_INPUT_DEVICE segments since ts_create —
 * out[0] device pieces seen (a segment scanned fully is one piece per pipeline group it lies in, a long segment's tips are two),
 * out[1] device-to-device copies issued (pieces of 8 MiB or more), out[2] gather jobs issued (a smaller piece is one job per
 * 16 KiB), out[3] gather kernel launches (one per pipeline group that holds such a piece).  Cumulative, monotonic and atomic:
 * concurrent calls are coalesced, so "the last call's" numbers would be nobody's; take the difference around a call. */
int     ts_device_input_stats(const ts_ctx *ctx, uint64_t out[4]);
/* Measurement aid (no counterpart in the reference): which way the host-to-device upload of the host entry points went since
 * ts_create — out[0] chunks sent packed (2-bit codes + invalid runs, restored on the device), out[1] chunks sent as ASCII; of the
 * packed chunks' blocks of 16384 positions: out[2] packed from one piece of plain bases, out[3] packed straight from one piece of
 * FASTA text, out[4] copied codes (every piece the block touches arrived as TS_INPUT_PACKED2), out[5] mixed (several pieces, or
 * padding: spelled out as letters, then packed); out[6] chunks staged by more than one worker thread; out[7] launches of the
 * unpack kernel for a chunk whose first base is not on a 64-position boundary of the layout.  Cumulative, monotonic and atomic,
 * like ts_device_input_stats: take the difference around a call. */
int     ts_upload_stats(const ts_ctx *ctx, uint64_t out[8]);
/* Measurement aid (no counterpart in the reference): what the context's GENERAL TIPS BATCHES (see the batch section below) have
 * done since ts_create — out[0] scans enqueued on them, rescans included, out[1] segments ts_batch_read_pass judged on them,
 * out[2] rescans ts_batch_sync made after a tile overflowed its slot or a candidate list spilled, out[3] bytes these calls
 * copied device to host: the fused pass's flag word, four bytes per ts_batch_read_pass_status and per round of ts_batch_sync —
 * no record and no block is ever downloaded.  Cumulative, monotonic and atomic, like ts_device_input_stats: take the difference
 * around a call. */
int     ts_read_batch_stats(const ts_ctx *ctx, uint64_t out[4]);
/* Measurement aid (no counterpart in the reference): which way the per-side maxima of ts_terminal_ends and
 * ts_batch_terminal_ends were reduced since ts_create — out[0] segments reduced on the device by the tiled kernel's ENDS walk,
 * out[1] segments reduced on the device by the general kernels' ENDS walk (both calls count here), out[2] segments reduced on
 * the host from downloaded blocks (a tiled group whose scan overflowed a record region; a general group the walk does not take),
 * out[3] bytes of per-side maxima and flag words these calls copied device to host (what the blocks route downloads besides
 * is not in it: out[2] says how many segments took that route).  Cumulative, monotonic and atomic, like ts_device_input_stats:
 * take the difference around a call. */
int     ts_terminal_ends_stats(const ts_ctx *ctx, uint64_t out[4]);
/* The host entry points read a handful of measurement / test knobs from the environment (TS_TIMING, TS_PACKED_UPLOAD,
 * TS_PACKED_MIN_BYTES, TS_GEN_LIST, TS_REC32, TS_MATCH_SLICE_BYTES) ONCE, when the context is made — never per call.  This reads them again (tests and A/B scripts that flip one between two calls on one context).
 * No counterpart in the reference (its options are fixed by main, /root/reference/src/main.cpp:149-184). */
int     ts_refresh_env(ts_ctx *ctx);
/* HIP puts the streams of a process on a few hardware queues (four unless GPU_MAX_HW_QUEUES says otherwise) and does not say which;
 * kernels of two streams that share a queue run one after the other, whatever events allow.  Returns 1 when a kernel on stream_b
 * runs while one on stream_a is still running, 0 when the two streams share a queue (a caller that wants a pack beside the next
 * scan — ts_batch_pack_shard — makes streams until it holds a scan stream and pack streams that do not), negative on error.
 * Waits for the work both streams hold, then takes ~1 ms.  The library tries its own side stream (the terminal walks of
 * ts_batch_pack_shard) against every scan / pack stream it meets in the same way.  No counterpart in the reference (one thread
 * per path, /root/reference/src/input.cpp:719-733). */
int     ts_streams_concurrent(ts_ctx *ctx, void *stream_a, void *stream_b);
/* Restricts the CALLING thread (and the threads it starts from then on) to the CPUs of the NUMA node the context's
 * device is attached to; returns 1 if it did, 0 if the topology is unknown, the thread's mask holds none of those CPUs,
 * or TS_NO_NUMA_BIND is set.  The library's own pipeline threads do this by themselves; a front end calls it on the threads
 * that read, parse and format around the scan (the reference's ThreadPool workers, src/input.cpp:719-733): on a two-socket
 * host a buffer or a staging thread on the other socket costs 15-20 % of the PCIe-inclusive rate. */
int     ts_bind_thread_to_device(const ts_ctx *ctx);

/* ---- The packed upload's host half, as a utility (host only, no device needed): `n` bases at `src` -> 2-bit codes at
 *      `dst` ((n + 3) / 4 bytes; base i at bits 2 (i & 3) .. +1 of byte i >> 2; A 0, C 1, T 2, G 3 — the scan kernel's own
 *      code — and 0 for every byte that is not one of the four letters), and the runs of such bytes {start, length} in
 *      `runs` (up to run_cap; *n_runs = how many there are — more than run_cap: TS_ERR_INVALID_ARG, nothing usable).
 *      fold_case as in ts_params.  This is what the host entry points do to every chunk they upload (unless
 *      TS_PACKED_UPLOAD=0): a quarter of the bytes cross PCIe, and a kernel restores the byte layout in HBM. */
typedef struct ts_invalid_run { uint32_t start, len; } ts_invalid_run;
int     ts_pack_bases(const char *src, uint64_t n, int fold_case, uint8_t *dst, ts_invalid_run *runs, uint64_t run_cap,
                      uint64_t *n_runs);

/* ---- Teloscope::scanSegment, batched (src/teloscope.cpp:537-658).  out[i] receives the
 *      SegmentData of segs[i]; a one-element call equals one scanSegment() call.  Host
 *      buffers in, host results out (H2D, kernels, D2H and host block calling inside). */
int  ts_scan_segments(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, ts_segment_out *out);
void ts_free_segments(ts_segment_out *out, size_t n_segs);

/* ---- ReadTelomereFilter (src/read-filter.cpp:10-45).  ts_create_read_filter applies
 *      makeReadFilterInput's overrides (min_block_len 42 unless min_block_len_set,
 *      terminal_limit UINT32_MAX/2, all genome-wide outputs off); ts_filter_reads is
 *      matches() over a batch: trailing '\r' stripped, case folded, pass[i] = 1 iff the
 *      read has a terminal block. */
ts_ctx *ts_create_read_filter(const ts_params *params, int min_block_len_set,
                              const ts_pattern *patterns, size_t n_patterns);
int     ts_filter_reads(ts_ctx *ctx, const char *const *seqs, const uint64_t *lens,
                        size_t n_reads, uint8_t *pass);

/* ---- Teloscope::labelTerminalBlocks (src/teloscope.cpp:259-383): the step walkPath runs
 *      on the concatenated terminal blocks of a path (src/input.cpp:1031).  Sorts blocks in
 *      place, sets is_longest, writes the granular label (needs 2*n+1 bytes). */
int ts_label_terminal_blocks(ts_block *blocks, size_t n, uint16_t gaps, uint64_t path_size,
                             uint32_t terminal_limit, char *label_out, int *scaffold_type_out);

/* ---- window float metrics (include/teloscope.h:199-214), evaluated on the host from
 *      the integer counts exactly as the reference does. */
float ts_gc_content(const uint32_t counts[4], uint32_t window_size);
float ts_shannon_entropy(const uint32_t counts[4], uint32_t window_size);

/* ts_scan_segments for callers that do not read the match vectors (every reference run without -m:
 * writeBEDFile reads windows, blocks and canonicalMatches.size() only, src/teloscope.cpp:700-868).
 * Scan, terminal/interstitial block calling and the counts below all happen on the device; out[i] is
 * what ts_scan_segments returns with matches == NULL / n_matches == 0, and counts[i] (optional, may be
 * NULL) carries the sizes the match vectors would have had.  Free out with ts_free_segments(). */
typedef struct ts_segment_counts {
    uint64_t n_windows;         /* = windows.size() (0 for a tips-only segment) */
    uint64_t n_matches;         /* full scan: allMatches.size(); tips-only: fwdMatches.size() + revMatches.size() */
    uint64_t n_canonical;       /* canonicalMatches.size() of a full scan */
    uint64_t n_forward;         /* fwdMatches.size() */
} ts_segment_counts;
int ts_scan_segments_blocks(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, ts_segment_out *out,
                            ts_segment_counts *counts);

/* ---- The five window tracks as text, formatted on the device (no counterpart of its own in the reference: it stands in for the
 *      window loops of writeBEDFile, src/teloscope.cpp:785-812, whose lines BedWriter::format writes on host threads otherwise).
 *      A line is  name \t start \t end \t value \n  with value as operator<<(float) prints it (%g, precision 6).  Track order
 *      everywhere: repeat density, canonical ratio, strand ratio, GC, entropy.  The context decides which tracks exist: the
 *      first three with out_win_repeats, GC with out_gc, entropy with out_entropy; a track that does not exist comes back as
 *      text NULL, len 0.  The arrays are the library's until ts_free_track_text().
 *      A ts_track_text must be ZERO-INITIALISED before its first use.  Both calls REPLACE what the struct holds, they never
 *      append: a struct that still holds an earlier call's result is reused — its arrays are kept, grown if need be and filled
 *      again, so a caller that formats chunk after chunk allocates once — and nothing leaks; a struct holding anything else
 *      (uninitialised memory) is undefined.  After a failed call the struct is empty (freed).  ts_free_track_text() at the end.
 *      A column value the device formatter cannot print (anything but 0, -1 and the positive floats in [2^-32, 128]: no window
 *      of a scan has one) makes the call fail with TS_ERR_UNSUPPORTED and a message that names the window; it never yields
 *      wrong text.  One device: not part of ts_scan_segments_multi. */
#define TS_N_TRACKS 5
typedef struct ts_track_text {
    char    *text[TS_N_TRACKS];      /* not NUL-terminated */
    uint64_t len[TS_N_TRACKS];
    uint64_t n_lines;                /* lines per existing track (= windows formatted) */
    uint64_t capacity[TS_N_TRACKS];  /* the library's */
} ts_track_text;
/* One segment of the table ts_window_tracks_format reads: its windows are records [first_window, first_window + n_windows),
 * window k covers [abs_pos + k * step, abs_pos + k * step + min(window_size, len - k * step)) and carries the name
 * names[name_off, name_off + name_len).  Segments in ascending first_window order; one without windows is skipped. */
typedef struct ts_track_segment {
    uint64_t first_window, n_windows, abs_pos, len, name_off;
    uint32_t name_len, reserved;
} ts_track_segment;
/* The formatting stage by itself, host in, host out: `n` window records of eight uint32 {A, C, G, T, canonical, non-canonical,
 * forward, reverse covered} (what a scan leaves per window; ts_window's integer fields), the segment table and the names' bytes
 * -> the text of every track the context has.  Uploads the records and runs the kernels ts_scan_segments_tracks runs; exists so
 * that records no small scan produces can be formatted.  Stands in for src/teloscope.cpp:785-812. */
int  ts_window_tracks_format(ts_ctx *ctx, const uint32_t *records, uint64_t n, const ts_track_segment *segs, size_t n_segs,
                             const char *names, uint64_t names_len, ts_track_text *out);
void ts_free_track_text(ts_track_text *t);
/* ts_scan_segments_blocks plus the text: blocks and counts come back as there, but out[i].windows == NULL and
 * out[i].n_windows == 0 (counts[i].n_windows, if counts is given, carries the count), and `tracks` holds the lines of all
 * full-scan segments in input order, segs[i]'s under names[i] (NUL-terminated); tips-only segments contribute none.  Every
 * input format (TS_INPUT_DEVICE included), tiled and general kernels, any number of pipeline groups: each group's lines are
 * formatted where its window records lie and appended in order, in place of the download of the records and their expansion to
 * ts_window on host threads.  Calls of this kind are not coalesced with other callers'.  Stands in for scanSegment
 * (src/teloscope.cpp:537-658) followed by src/teloscope.cpp:785-812. */
int  ts_scan_segments_tracks(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, const char *const *names,
                             ts_segment_out *out, ts_segment_counts *counts, ts_track_text *tracks);

/* ---- The two match files (-m) as text, formatted on the device (no counterpart of its own in the reference: it stands in for
 *      scanSegment's matchSeq and its routing of a match into canonicalMatches / nonCanonicalMatches, src/teloscope.cpp:466-468,
 *      485-509, and for the two match loops of writeBEDFile that print those vectors, which BedWriter::format runs on host
 *      threads otherwise).  A line is  name \t position \t position + match_size \t matchSeq \n  with matchSeq the match's bases,
 *      a..z upper-cased.  File order everywhere: canonical matches, terminal non-canonical matches.  A full-scan record gives a
 *      canonical line if it is canonical, a non-canonical line if it is not and isTerminal (src/teloscope.cpp:451-459) holds for
 *      its position relative to its SEGMENT, and no line otherwise; tips-only segments give none.  Lines come in the order in
 *      which ts_scan_segments returns `matches`.
 *      A ts_match_text follows ts_track_text's rules: ZERO-INITIALISED before its first use; a call REPLACES what it holds and
 *      never appends; an earlier result's arrays are reused and grown; after a failed call the struct is empty (freed);
 *      ts_free_match_text() at the end.  A context without out_matches yields text NULL, len 0 for both files. */
#define TS_N_MATCH_FILES 2            /* canonical, terminal non-canonical */
typedef struct ts_match_text {
    char    *text[TS_N_MATCH_FILES];      /* not NUL-terminated */
    uint64_t len[TS_N_MATCH_FILES];
    uint64_t n_lines[TS_N_MATCH_FILES];
    uint64_t capacity[TS_N_MATCH_FILES];  /* the library's */
} ts_match_text;
void ts_free_match_text(ts_match_text *t);
/* One segment of the table ts_match_lines_format reads: its matches are records [first_record, first_record + n_records)
 * (ascending first_record; records between two segments are skipped), its bases are bases[base_off, base_off + len), base 0 at
 * absolute position abs_pos, its name names[name_off, name_off + name_len).  tips_only != 0: the segment gives no lines. */
typedef struct ts_match_line_segment {
    uint64_t first_record, n_records, abs_pos, len, base_off, name_off;
    uint32_t name_len, tips_only;
} ts_match_line_segment;
/* The formatting stage by itself, host in, host out: uploads the records, the table, the names and the bases and runs the
 * kernels ts_scan_segments_text runs; exists so that records no small scan produces can be formatted (sizes 1 and 63,
 * positions of ten and more digits).  Canonical is the record's TS_MATCH_CANONICAL flag; terminal is decided from its position
 * against the segment's len and the context's terminal_limit — the incoming TS_MATCH_TERMINAL bit is not trusted.  A record
 * outside its segment, or of size 0 or above 63, is TS_ERR_INVALID_ARG.  Stands in for src/teloscope.cpp:466-468, 485-509
 * and the two match loops of writeBEDFile. */
int  ts_match_lines_format(ts_ctx *ctx, const ts_match *records, uint64_t n, const ts_match_line_segment *segs, size_t n_segs,
                           const char *names, uint64_t names_len, const char *bases, uint64_t bases_len, ts_match_text *out);
/* ts_scan_segments_tracks plus the match lines of all full-scan segments in input order: `tracks` as there, `matches` the two
 * files' lines, segs[i]'s under names[i].  Either text argument may be NULL, not both.  out[i].matches == NULL and
 * out[i].windows == NULL; blocks and counts as from ts_scan_segments_blocks.  Every input format (TS_INPUT_DEVICE, text pieces
 * and packed included), tiled, general and wide kernels, any number of pipeline groups: each group's lines are formatted from
 * its match records and its input buffer where they lie, so neither a match record nor a base crosses to the host.  One
 * device: not part of ts_scan_segments_multi; not coalesced with other callers.  Stands in for scanSegment
 * (src/teloscope.cpp:537-658, its matchSeq and routing :466-468, 485-509) followed by the window loops (:785-812) and the two
 * match loops of writeBEDFile. */
int  ts_scan_segments_text(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, const char *const *names,
                           ts_segment_out *out, ts_segment_counts *counts, ts_track_text *tracks, ts_match_text *matches);
/* Measurement aid (no counterpart in the reference; it counts what stands in for src/teloscope.cpp:485-509 and the two match
 * loops of writeBEDFile): out[0] formatting calls (one per pipeline group, or per ts_match_lines_format), out[1] canonical
 * lines, out[2] non-canonical lines, out[3] text bytes the device formatted since ts_create.  Cumulative, monotonic, atomic. */
int  ts_match_text_stats(const ts_ctx *ctx, uint64_t out[4]);

/* ---- GFA annotation (src/input.cpp:625-716).  For every segment (tips_only must be 1), ends[2*i] / ends[2*i+1]: the
 *      longest terminal block (blockLen) at the start / end side of segs[i], 0 if none (walkSegment's distToStart <= distToEnd
 *      rule, src/input.cpp:835-881; positions relative to abs_pos).  Host in, host out, any context; the same numbers as
 *      ts_scan_segments_blocks' terminal blocks reduced per side, but only 8 bytes per segment leave the device — under
 *      every pattern set: the tiled kernel's records are reduced by the read predicate's walks, the general kernels' by the
 *      terminal walks of device block calling (ts_terminal_ends_stats says which way a call went). */
int ts_terminal_ends(ts_ctx *ctx, const ts_segment_in *segs, size_t n_segs, uint32_t *ends);

/* ---- device-resident batches: the same scan with inputs and outputs kept in HBM.
 *      Used by bench.py and the multi-GPU driver; ts_scan_segments is built on it. ----- */
typedef struct ts_batch_info {
    uint64_t n_segments;
    uint64_t total_bases;
    uint64_t input_bytes;       /* size of the device input buffer the batch expects */
    uint64_t n_windows;         /* window records produced */
    uint64_t n_tiles;
    uint64_t match_capacity;    /* match records the device buffer can hold */
    uint64_t n_matches;         /* valid after ts_batch_sync() */
    uint64_t algorithmic_bytes; /* window scan: 1 B/base + 32 B/window + 4 B/match (after sync); tips-only / read batch:
                                   1 B per scanned base + 1 bit per segment (its match stream is an intermediate) */
    double   last_kernel_ms;    /* HIP-event time of the last scan (after sync) */
    double   avg_kernel_ms;     /* mean HIP-event time of the scans enqueued since the previous sync
                                   (the latest 64 at most) */
    uint64_t kernel_launches;   /* how many scans avg_kernel_ms averages over */
} ts_batch_info;

/* Plans a batch of n_segs segments of the given lengths (all tips_only or all full scan).
 * match_capacity 0 = default (bases/4).
 *
 * GENERAL TIPS BATCHES.  With tips_only = 1 the call succeeds on every context for which ts_takes_text_input(ctx, 1) is 1.  On
 * a context whose tips-only scans go to the general kernels (mixed pattern lengths, patterns of 9 bases or more, up to 63 lengths
 * of up to 63 bases) it returns a general tips batch: the same input layout (ts_batch_segment_offset, TS_IN_PAD zero bytes
 * behind the last segment), so ts_batch_input_ptr, ts_batch_upload, ts_fastq_chunk_stage, ts_bam_chunk_decode and a caller's
 * own d_input fill it unchanged; ts_batch_scan enqueues the general kernels' fused tips pass, ts_batch_read_pass the read
 * predicate over its records (same stream), ts_batch_read_pass_status says whether a tile overflowed its record slot or a
 * candidate list spilled, and ts_batch_sync then regrows the slots (or changes the pass's form) and rescans — the protocol of a
 * tiled read batch.  The other tips-only results are served too: ts_batch_terminal_ends writes the longest terminal block
 * per side of every segment to device memory (same stream, same overflow protocol as the pass), ts_batch_download_blocks calls
 * the terminal blocks on the device over the records where they lie and returns them as ts_scan_segments_blocks returns the
 * same tips-only segments (no windows, no matches, no interstitial blocks; it syncs first when the batch is not synced), and
 * ts_batch_segment_summary writes {0, n_matches, n_canonical, n_forward} per segment, the numbers ts_scan_segments_blocks hands
 * back as ts_segment_counts (scan's stream; it syncs first likewise).  ts_batch_get_info fills the segments, bases, input
 * bytes, tiles and slot capacity (the rest is 0), and ts_batch_destroy frees it.  match_capacity is ignored.  EVERY OTHER
 * ts_batch_* call (restrict, partition, the shard calls, bind, export, adopt, ts_batch_download, get_tiles / range_info,
 * set_emit, set_record_bits, set_timing, wait_scan) and ts_shards_finalize answers TS_ERR_UNSUPPORTED with the call named in ts_last_error; the three pointer calls return NULL and
 * ts_batch_wire16_ok 0.  Full-scan batches (tips_only = 0) of such sets stay refused: the host entry points scan them.  The
 * reference has no batches at all (one job per read, src/input.cpp:753-812). */
ts_batch *ts_batch_create(ts_ctx *ctx, const uint64_t *seg_lens, const uint64_t *abs_pos,
                          size_t n_segs, int tips_only, uint64_t match_capacity);
void      ts_batch_destroy(ts_batch *b);
/* Byte offset of segment i inside the device input buffer (16-byte aligned). */
uint64_t  ts_batch_segment_offset(const ts_batch *b, size_t i);
/* Device pointer of the batch's own input buffer (input_bytes long). */
void     *ts_batch_input_ptr(ts_batch *b);
/* Copies one segment's bases host -> device input buffer. */
int       ts_batch_upload(ts_batch *b, size_t i, const char *seq);
/* Enqueues the scan on `stream` (a hipStream_t, NULL = default stream), reading bases from
 * d_input (NULL = the batch's own input buffer). Asynchronous. */
int       ts_batch_scan(ts_batch *b, const void *d_input, void *stream);
/* Makes `stream` wait for the batch's last scan (no-op when it is the scan's own stream): a stream wait on the event the library
 * records behind every scan anyway — a caller that records an event of its own behind the scan puts a second packet on the scan's
 * queue, 0.011-0.013 ms per scan that the next scan starts later (profiles/r05/shard_step_queues.txt).  What runs beside the next
 * scan (ts_batch_pack_shard, ts_batch_read_pass on a stream of their own) is ordered this way.  The reference orders the same two
 * steps by program order inside one job (scanSegment: scan, then block calling, /root/reference/src/teloscope.cpp:600-657). */
int       ts_batch_wait_scan(ts_batch *b, void *stream);
/* Width of the match records the batch's scans leave in their per-wave regions: 16 bits each — the kernel's own staged entries,
 * (tile-relative position << 2) | forward << 1 | canonical with positions below 2^14 — wherever the batch's tiles are that short
 * (every geometry the planner picks for windows up to 8 192 bases, and read batches), else 32.  Every reader inside the library
 * knows both (block calling, the read predicate, pack; export, downloads and the dense stream widen to 32 bits, so nothing that
 * leaves the device changes); the records are a tenth of the bytes a scan moves through HBM.  ts_batch_set_record_bits(b, 32)
 * before the first scan keeps 32-bit regions — what a caller that reads them raw through ts_batch_matches_ptr needs (that
 * pointer is NULL for 16-bit regions); 16 asks for 16 (TS_ERR_UNSUPPORTED when the tiles are too long).  TS_REC32=1 (read when the
 * context is made) makes 32 the default.  The reference has no such stream at all (it walks SegmentData in place,
 * /root/reference/src/teloscope.cpp:600-657, src/read-filter.cpp:10-45). */
int       ts_batch_set_record_bits(ts_batch *b, int bits);
/* Which of the batch's scans are timed: every `every`-th (1, the default: all; 0: none).  A timed scan has an event recorded in
 * front of it as well as the one behind every scan; ts_batch_info's kernel times are means over the timed scans since the last
 * ts_batch_sync.  An event is a packet on the scan's queue: a caller that enqueues scans back to back and does not need every
 * one's time (a rank's steps) saves 0.005 ms per untimed scan. */
int       ts_batch_set_timing(ts_batch *b, uint32_t every);
/* Waits for the last scan, reads back counters; grows the match buffer and rescans if it
 * overflowed. */
int       ts_batch_sync(ts_batch *b);
int       ts_batch_get_info(const ts_batch *b, ts_batch_info *info);
/* Device pointers to the raw result buffers (valid after sync): window records
 * (8 x uint32 each: A,C,G,T, canonical/nonCanonical/fwd/rev covered) and the stream of
 * packed 32-bit match records ((tile-relative position << 2) | fwd << 1 | canonical).  Records
 * of one tile are contiguous and position-ordered; tiles are placed in completion order and
 * located through the batch's tile directory (ts_batch_download does that).  ts_batch_matches_ptr is NULL
 * while the regions hold 16-bit records (ts_batch_set_record_bits). */
const void *ts_batch_windows_ptr(const ts_batch *b);
const void *ts_batch_matches_ptr(const ts_batch *b);
/* D2H + host post-processing (absolute positions, terminal flags, block calling):
 * fills out[0..n_segments). Free with ts_free_segments(). */
int       ts_batch_download(ts_batch *b, const char *const *host_seqs, ts_segment_out *out);
/* Block calling ON THE DEVICE (getTerminalBlocks / getInterstitialBlocks, src/teloscope.cpp:29-256)
 * from the resident match stream, for a synced batch: fills out[i].terminal_blocks /
 * interstitial_blocks (and windows for a full scan) exactly as ts_batch_download would, but
 * leaves out[i].matches empty — only the blocks (a few per segment) cross PCIe.  Free with
 * ts_free_segments(). */
int       ts_batch_download_blocks(ts_batch *b, ts_segment_out *out);
/* Per-segment summary (n_windows, n_matches, n_canonical, n_forward as 4 x uint64 per
 * segment) written to a device buffer of 32*n_segments bytes: the "hit buffer" ranks
 * gather over RCCL. */
int       ts_batch_segment_summary(ts_batch *b, void *d_out, void *stream);


/* ---- the tile directory and tile-range shards: multi-GPU form of the scan.
 *      The reference runs one thread-pool job per path (src/input.cpp:719-724) and merges the jobs' PathData
 *      in seqPos order (sortBySeqPos, include/teloscope.h:262-266).  Here the unit of work is a TILE of the
 *      batch's plan (a run of consecutive windows of one segment, plus its w-s halo); ranks scan disjoint tile
 *      ranges of the SAME plan and one rank adopts all their results, after which it holds exactly what a
 *      single-GPU scan of the whole batch holds.  Nothing here communicates: the exchange itself
 *      (RCCL through torch.distributed) belongs to the caller, teloscope_amd/distributed.py. ---------- */
typedef struct ts_tile_info {
    uint64_t seg_index;        /* segment the tile belongs to */
    uint64_t seg_offset;       /* segment-relative position of the tile's first owned base; the position field
                                  of a packed match record is relative to it */
    uint64_t first_window;     /* index of the tile's first window record in the batch's window array */
    uint32_t n_windows;        /* window records the tile owns (0 in a tips-only batch) */
    uint32_t owned_bases;
} ts_tile_info;
/* Fills out[0..n) with tiles first .. first+n-1 of the plan (host data; works on a planning-only context). */
int ts_batch_get_tiles(const ts_batch *b, uint64_t first, uint64_t n, ts_tile_info *out);

typedef struct ts_range_info {
    uint64_t tile_begin, tile_end;
    uint64_t window_begin, window_end;   /* window records the range owns */
    uint64_t input_begin, input_end;     /* bytes of the batch's input layout the range reads (halo and the kernel's
                                            over-read slack included; bytes past a segment's data may hold anything) */
    uint64_t bases;                      /* owned bases */
} ts_range_info;
int ts_batch_range_info(const ts_batch *b, uint64_t tile_begin, uint64_t tile_end, ts_range_info *out);
/* Deterministic split of the plan into n_parts consecutive tile ranges of equal owned bases (+-1 tile);
 * part p owns [*tile_begin, *tile_end).  Consecutive ranges make the gather a concatenation: window records,
 * the tile directory and the tile-ordered record stream of part p follow those of part p-1. */
int ts_batch_partition(const ts_batch *b, uint32_t n_parts, uint32_t part, uint64_t *tile_begin, uint64_t *tile_end);
/* Before the first scan: the batch will execute only tiles [tile_begin, tile_end) — device buffers are sized for
 * the range, ts_batch_scan expects d_input to point at byte input_begin of the input layout
 * (ts_batch_range_info), and ts_batch_upload copies only the part of a segment the range reads. */
int ts_batch_restrict(ts_batch *b, uint64_t tile_begin, uint64_t tile_end);
/* on != 0: the batch's scans (window scans only; a tips-only batch ignores it) also leave, in HBM, what the calls that
 * follow a scan would otherwise re-read the whole match stream for: the records a writer reads — canonicalMatches and
 * the terminal nonCanonicalMatches, /root/reference/src/teloscope.cpp:486-496 — as a second, sparse output, and per tile
 * a summary of its chains of matches (getInterstitialBlocks' grouping, src/teloscope.cpp:235-253).  Device block
 * calling (ts_batch_download*, the host entry points) then looks only at the tiles that can hold an interstitial block,
 * and ts_batch_pack_shard copies the visible records instead of filtering 4 bytes per match.  It costs the scan kernel
 * about a tenth of its time, so it is OFF for a batch that is only scanned (results left in HBM) and switched ON by
 * ts_batch_restrict_shard and by the host entry points, whose downloads always call blocks; results are identical
 * either way.  May be changed between scans; the fourth word of a tile's directory entry is its visible-record count
 * while on. */
int ts_batch_set_emit(ts_batch *b, int on);
/* Caller-owned result buffers (device): the scan writes the range's window records (32 B each, from
 * window_begin) to d_windows and its tile directory entries {matches, canonical, forward, 0 or visible} x uint32 (16 B per
 * tile, from tile_begin) to d_tile_stats.  Either may be NULL = the batch's own buffer.  Before the first scan. */
int ts_batch_bind_results(ts_batch *b, void *d_windows, void *d_tile_stats);
/* After a scan (asynchronous on `stream`): packs the range's match records into ONE stream in tile order
 * (= position order within each segment) at d_dense (capacity in records) and writes to d_total (2 x uint64 on
 * the device) {records the range produced, 1 if the stream is incomplete: a wave's region overflowed — call
 * ts_batch_sync, which grows it and rescans — or dense_capacity was too small}. */
int ts_batch_export(ts_batch *b, void *d_dense, uint64_t dense_capacity, void *d_total, void *stream);
/* On a whole (unrestricted) batch: take results produced elsewhere — window records, tile directory entries and
 * the tile-ordered record stream of ALL tiles, i.e. the concatenation over the parts of what ts_batch_bind_results
 * / ts_batch_export delivered — as this batch's results.  The buffers stay owned by the caller and must outlive
 * the batch's use.  Afterwards ts_batch_download, ts_batch_download_blocks and ts_batch_segment_summary work as
 * after a local scan + sync. */
int ts_batch_adopt(ts_batch *b, void *d_windows, void *d_tile_stats, const void *d_dense, uint64_t n_matches,
                   void *stream);
/* The exchange's wire format.  Every u32 of the three result arrays fits 16 bits when ts_batch_wire16_ok() says so
 * (packed match records always do: position < 2^14 plus two flag bits; tile counts too; window fields when
 * pattern length x window <= 65535), so ranks may send them as u16 — half the bytes over the link-bound gather — and
 * the destination widens them where they land: dst[i] = src[i] for n values, asynchronously on `stream`
 * (device pointers; ctx names the device). */
int ts_batch_wire16_ok(const ts_batch *b);
int ts_wire_widen_u16(ts_ctx *ctx, const void *d_src_u16, void *d_dst_u32, uint64_t n, void *stream);
/* Device pointer of the batch's tile directory entries (16 B per tile of the range). */
const void *ts_batch_tile_stats_ptr(const ts_batch *b);

/* ---- shard results: several devices share ONE scan and hand over what the reference's writers read ----------------
 *      The reference fans paths out to its thread-pool workers and merges their PathData in seqPos order
 *      (src/input.cpp:719-733, sortBySeqPos include/teloscope.h:262-266).  Of a path's results its writers read the
 *      windows, the blocks, canonicalMatches and the terminal nonCanonicalMatches (src/teloscope.cpp:486-496, :700-868;
 *      walkPath moves only those two match vectors into PathData, src/input.cpp:1000-1009) — about 3 % of the match
 *      records; allMatches / fwdMatches / revMatches feed block calling (:646-655) and nothing else.  A SHARD therefore
 *      calls its blocks on its own device and packs ONE message — bit-packed window records, the visible match records
 *      (16 bits each), its blocks — which is all that crosses xGMI (rank form, teloscope_amd/distributed.py) or PCIe
 *      (ts_scan_segments_multi): ~60 MB per 3 Gb scan at 8 devices instead of the 245 MB of the full exchange above.
 *
 *      A shard OWNS the p-th of n consecutive tile ranges (ts_batch_partition: equal bases; a boundary inside a segment
 *      keeps at least terminal zone + context tiles from both its ends) and also scans CONTEXT tiles either side where
 *      a segment continues on a neighbour, so that a chain of matches that starts in an owned tile can be followed.
 *      Terminal blocks belong to the shard that owns that end of the segment, an interstitial block to the shard that
 *      owns the tile it starts in.  What the shards assume about each other (the bounds of the interstitial search) is
 *      checked by ts_shards_finalize; when it does not hold — a telomere that reaches beyond the context tiles —
 *      ts_shards_finalize returns TS_SHARD_NEED_FULL and the caller takes the full path for that batch. ------------- */
typedef struct ts_shard_info {
    uint32_t n_parts, part;
    uint64_t own_begin, own_end;         /* tiles the shard owns */
    uint64_t ext_begin, ext_end;         /* tiles it scans: owned + context */
    uint64_t window_begin, window_end;   /* window records it owns */
    uint64_t input_begin, input_end;     /* bytes of the batch's input layout its scan reads (ts_batch_scan expects d_input
                                            to point at byte input_begin) */
    uint64_t bases;                      /* owned bases */
    uint64_t seg_begin, seg_end;         /* segments with an owned tile */
    uint64_t msg_bytes;                  /* size of its result message at this capacity scale */
    uint64_t visible_capacity;           /* visible match records / blocks the message has room for */
    uint32_t block_capacity;
    uint32_t window_bytes;               /* bytes per packed window record */
    uint32_t visible_bytes;              /* bytes per visible match record (2, or 4 when a tile-relative position needs more) */
    uint32_t context_tiles;
} ts_shard_info;
/* Host only (works on a planning-only context): sender and receiver compute the same numbers.  `scale` >= 1 multiplies
 * the capacities of the message's variable sections (visible records, blocks). */
int ts_batch_shard_info(const ts_batch *b, uint32_t n_parts, uint32_t part, uint32_t scale, ts_shard_info *out);
/* Before the first scan: the batch becomes shard `part` of `n_parts` (ts_batch_restrict to its scanned range). */
int ts_batch_restrict_shard(ts_batch *b, uint32_t n_parts, uint32_t part, uint32_t scale);
int ts_batch_set_shard_scale(ts_batch *b, uint32_t scale);
/* After ts_batch_scan, asynchronous on `stream`, no host synchronisation: block calling on the device and the packed
 * message at d_msg (device memory, msg_bytes >= ts_shard_info.msg_bytes). */
int ts_batch_pack_shard(ts_batch *b, void *d_msg, uint64_t msg_bytes, void *stream);
/* Optional, after ts_batch_restrict_shard: the message buffer (device memory, msg_bytes >= ts_shard_info.msg_bytes) the
 * shard's scans will be packed into.  Knowing it, an emitting scan writes the records of the windows it owns straight into the
 * message's window section in their bit-packed form (7 fields x bit_width(window) bits: what a writer reads of a WindowData,
 * /root/reference/src/teloscope.cpp:785-812, /root/reference/include/teloscope.h:119-137) instead of 8 x uint32 per window
 * that ts_batch_pack_shard then packs in a pass of its own: the pack has one kernel fewer and the scan stores a quarter of
 * the bytes.  The 8 x uint32 records of such a scan are NOT produced (ts_batch_windows_ptr / ts_batch_download see none), and
 * ts_batch_pack_shard must be given the same buffer (TS_ERR_STATE otherwise).  The message's bytes do not depend on it.
 * d_msg == NULL unbinds; ts_batch_set_shard_scale unbinds (the message's size changes with the scale).
 * Ordering: every scan of the batch writes the bound message, not only its pack.  A bound message must therefore not be in
 * flight — sent, copied, read by any stream — when the next scan of that batch is enqueued: make the scan's stream wait for
 * the reader first (an event recorded behind the send or copy).  An event recorded behind the pack is not enough: the next
 * scan would overwrite the window section of a message whose transfer has not finished, and the receiver would get the
 * window records of two different scans in one message (teloscope_amd/distributed.py: PackedShard.release). */
int ts_batch_bind_shard_message(ts_batch *b, void *d_msg, uint64_t msg_bytes);
#define TS_SHARD_OVERFLOW_VISIBLE 0x1u   /* ts_shard_status.flags */
#define TS_SHARD_OVERFLOW_BLOCKS  0x2u
#define TS_SHARD_OVERFLOW_SCAN    0x4u   /* a wave's record region overflowed in the scan: ts_batch_sync, then pack again */
#define TS_SHARD_OUT_OF_CONTEXT   0x8u   /* a chain or a terminal walk ran out of the context tiles */
typedef struct ts_shard_status {
    uint32_t part, n_parts, flags, n_blocks;
    uint64_t n_visible, visible_capacity;
    uint32_t block_capacity;
    uint32_t scale_factor_needed;        /* 1 when everything fitted, else the factor by which to raise the scale */
    uint64_t msg_bytes;
} ts_shard_status;
/* Reads a message's header (host memory). */
int ts_shard_peek(const void *msg, uint64_t msg_bytes, ts_shard_status *out);
/* positive returns of ts_shards_finalize: the messages could not be turned into results as they are */
#define TS_SHARD_RETRY_SYNC 1            /* a shard's scan overflowed: ts_batch_sync on it, pack again */
#define TS_SHARD_RETRY_GROW 2            /* a message overflowed: pack again with a larger scale (ts_shard_peek says which) */
#define TS_SHARD_NEED_FULL  3            /* the shards' assumptions about each other do not hold for this input */
/* Host: the messages of all n_parts shards of `plan` (a whole batch of the same plan; may sit on a planning-only
 * context) -> out[i] = SegmentData of segment i with windows, blocks and, as `matches`, the VISIBLE records only
 * (canonicalMatches + terminal nonCanonicalMatches, position order); counts[i] (optional) = the sizes the match
 * vectors had on the devices.  Free out with ts_free_segments(). */
int ts_shards_finalize(const ts_batch *plan, const void *const *msgs, const uint64_t *msg_bytes, uint32_t n_parts,
                       ts_segment_out *out, ts_segment_counts *counts);

/* ---- Teloscope::scanSegment over several devices (one host thread per context, as ts_filter_reads_multi): the batch's
 *      plan is split into one shard per context; every device uploads the bases its shard reads and downloads its
 *      shard's message over its OWN PCIe link; the host merges (ts_shards_finalize).  Replaces the reference's one job
 *      per path + merge under a mutex (src/input.cpp:719-733, :1036-1037).  out[i].matches holds the VISIBLE records
 *      only (see above); counts may be NULL.  Contexts must have been created with the same parameters and patterns and
 *      may share a device.  Parameter sets outside the tiled kernel have no shard results: their segments are dealt WHOLE to the
 *      contexts, in consecutive runs of equal bases (the reference's one job per path); inputs for which the shards' assumptions
 *      fail run on ctxs[0] alone (same results). */
int ts_scan_segments_multi(ts_ctx *const *ctxs, size_t n_ctx, const ts_segment_in *segs, size_t n_segs,
                           ts_segment_out *out, ts_segment_counts *counts);

/* ---- ReadTelomereFilter over several devices (the read shard of --fastq-subset / --bam-subset:
 *      the reference deals a batch's reads to its thread-pool workers in chunks and writes the chunk outputs in
 *      chunk order, src/input.cpp:753-812).  ctxs[0..n_ctx) are read-filter contexts (ts_create_read_filter),
 *      normally one per GPU; the batch is cut into n_ctx consecutive shards of equal bases, each filtered by one
 *      host thread on its context, and pass[] comes back in input order.  Contexts may share a device. */
/* ReadTelomereFilter::matches for reads that already are in HBM: on a tips-only batch made from a read-filter
 * context and scanned on `stream` (ts_batch_scan), writes pass[i] (one byte per read, device memory) asynchronously
 * on the same stream; the match stream never leaves the device. */
int ts_batch_read_pass(ts_batch *b, void *d_pass, void *stream);
/* The scan may have overflowed a wave's record region (tiles are taken on demand, so the per-wave fill differs from launch
 * to launch: a launch that fitted, even one ts_batch_sync vouched for, says nothing about the next).  ts_batch_read_pass
 * then judges NOTHING — d_pass keeps what it held — and raises a flag on the device that stays up until it is read here:
 * *overflowed = 1 if any pass since the last call was skipped for that reason (then: ts_batch_sync, which regrows and
 * rescans, and ts_batch_read_pass again).  Waits for the device. */
int ts_batch_read_pass_status(ts_batch *b, int *overflowed);
/* (On a general tips batch — see ts_batch_create — the pass is always enqueued; after an overflow or a spill its bytes mean
 * nothing, *overflowed says so on every call until ts_batch_sync has rescanned, and ts_batch_read_pass wants the stream of the
 * scan.) */
/* The GFA annotation's numbers for segment ends that already are in HBM: on a scanned tips-only batch, tiled or general, writes
 * d_ends[2*i] / d_ends[2*i+1] (uint32 each, device memory, 8 bytes per segment) = the longest terminal block at the start / end
 * side of segment i, 0 where there is none — what ts_terminal_ends returns for the same segments — asynchronously on `stream`.
 * Stands in for walkSegment / walkSegmentForPath's per-segment reduction (src/input.cpp:835-939) over scanSegment's terminal
 * blocks.  A full-scan batch answers TS_ERR_INVALID_ARG.  Overflow follows ts_batch_read_pass' protocol exactly:
 * ts_batch_read_pass_status reports it, the caller then calls ts_batch_sync and ts_batch_terminal_ends again; after an
 * overflow a tiled batch's d_ends keeps what it held and a general tips batch's holds memory-safe, meaningless numbers.  On a
 * general tips batch `stream` is the stream of the scan. */
int ts_batch_terminal_ends(ts_batch *b, void *d_ends, void *stream);
int ts_filter_reads_multi(ts_ctx *const *ctxs, size_t n_ctx, const char *const *seqs, const uint64_t *lens,
                          size_t n_reads, uint8_t *pass);

/* ---- the rank form's ONE exchange for a C++ host (one process per GPU): every rank's shard message
 *      (ts_batch_pack_shard) to rank `dst` in one grouped send / recv over RCCL — xGMI between the GPUs of a node.  The
 *      reference merges its per-path results in process, under a mutex (src/input.cpp:719-733, sortBySeqPos
 *      include/teloscope.h:262-266); this is that merge's transport when the paths were scanned by other processes.
 *      librccl is opened at run time: on a host without it these four calls fail with TS_ERR_UNSUPPORTED and nothing else
 *      changes.  Message sizes come from ts_batch_shard_info on both sides, so a step needs no size exchange and no host
 *      synchronisation.  (teloscope_amd/distributed.py's ShardExchange is the same exchange through torch.distributed.) */
typedef struct ts_exchange ts_exchange;
#define TS_EXCHANGE_ID_BYTES 128
/* One rank makes the id (ncclGetUniqueId) and hands its 128 bytes to the others by whatever the host has: MPI_Bcast, a
 * socket, a file.  On failure ts_exchange_last_error() says why. */
int          ts_exchange_unique_id(void *id_out);
const char  *ts_exchange_last_error(void);
/* Collective over the n_ranks processes (ncclCommInitRank on the context's device); NULL on failure (ts_last_error(ctx)). */
ts_exchange *ts_exchange_create(ts_ctx *ctx, const void *id, int rank, int n_ranks);
void         ts_exchange_destroy(ts_exchange *x);
/* Asynchronous on `stream` (the one the message was packed on, or one that waits for it).  A rank other than dst sends
 * d_msg[0, my_bytes); dst receives rank p's message into d_recv[p] (device memory, msg_bytes[p] bytes) for every p != dst —
 * its own message stays where it is (d_recv[dst] may be NULL; when it is given and differs from d_msg the message also goes
 * through RCCL to itself: the loop-back a one-GPU box rehearses the pattern with).  d_recv / msg_bytes are read on dst only. */
int          ts_exchange_gather(ts_exchange *x, int dst, const void *d_msg, uint64_t my_bytes, void *const *d_recv,
                                const uint64_t *msg_bytes, void *stream);

/* ---- BGZF members inflated and checksummed on the device (a wave per member): what the reference's BgzfReader::loadBlock
 *      does with zlib on one host thread, a member per call (src/bgzf.cpp:57-196: inflate(Z_FINISH), total_out == ISIZE,
 *      crc32 against the footer).  The caller locates the members (gzip header, BC subfield, footer: host work that reads no
 *      payload byte) and hands over the compressed bytes and one descriptor per member; only compressed bytes cross PCIe on
 *      the way in.  A member is accepted exactly when zlib accepts it there: the final deflate block ends in the payload's
 *      last byte, exactly isize bytes come out, and their CRC32 is crc.  Members without output (isize == 0: the EOF marker,
 *      legal in mid-stream) are checked like any other. */
typedef struct ts_bgzf_block {
    uint64_t src_off;            /* the deflate payload's first byte in `compressed` */
    uint32_t payload_len;        /* <= 65536 */
    uint32_t isize;              /* uncompressed size from the footer, <= 65536 */
    uint32_t crc;                /* CRC32 from the footer */
    uint32_t reserved;
    uint64_t dst_off;            /* where the member's bytes go in the output */
} ts_bgzf_block;
#define TS_BGZF_OK          0
#define TS_BGZF_BAD_DEFLATE 1    /* "invalid BGZF deflate payload" */
#define TS_BGZF_BAD_CRC     2    /* "BGZF checksum mismatch" */
typedef struct ts_bgzf_status {
    int32_t  code;               /* TS_BGZF_OK, or what is wrong with the LOWEST member that is not ok */
    uint32_t reserved;
    uint64_t block;              /* that member's index; n_blocks when all are ok */
} ts_bgzf_status;
/* Host in, host out.  compressed[0, n) holds the payloads, blocks[0, n_blocks) describe them (any order of dst_off; outputs
 * must not overlap), plain_out[0, plain_cap) receives the members' bytes; bytes of plain_out that no ok member covers are
 * zero.  Descriptors are checked on the host before anything is launched (src_off + payload_len <= n, payload_len and
 * isize <= 65536, dst_off + isize <= plain_cap, no overlap): TS_ERR_INVALID_ARG.  A damaged member is not an error of the
 * call: TS_OK, and *first_bad says which member and why; the other members' bytes are right all the same. */
int ts_bgzf_inflate(ts_ctx *ctx, const void *compressed, uint64_t n, const ts_bgzf_block *blocks, size_t n_blocks,
                    void *plain_out, uint64_t plain_cap, ts_bgzf_status *first_bad);

/* ---- the resident form, which the BAM route runs on (include/teloscope_mi355x_io.hpp: bamSubsetDevice): a chunk of a BAM's
 *      uncompressed stream that exists in HBM only.  Replaces, for --bam-subset, BgzfReader::loadBlock (src/bgzf.cpp:57-196)
 *      and the record loop of subsetBam with decodeSequence (src/bam.cpp:122-259): members are inflated and checksummed,
 *      records walked and validated, SEQ decoded from 4-bit codes into a read batch's input buffer and passing records
 *      gathered, all on the device; the record table and the passing records' bytes are what comes back. */
typedef struct ts_bam_chunk ts_bam_chunk;
typedef struct ts_bam_record {
    uint64_t off;                /* of the record's block_size field in the chunk */
    uint32_t block_size;
    uint32_t seq_at;             /* SEQ's first byte, relative to off */
    uint32_t l_seq;
    uint32_t reserved;
} ts_bam_record;
/* error of ts_bam_chunk_walk: the first record that is not valid, in the host route's order of checks */
#define TS_BAM_OK             0
#define TS_BAM_BAD_BLOCK_SIZE 1  /* "invalid BAM record block_size": not in 32 .. 256 MiB */
#define TS_BAM_BAD_LENGTHS    2  /* "invalid BAM record lengths": l_read_name == 0 or l_seq > 0x7fffffff */
#define TS_BAM_FIELDS_EXCEED  3  /* "BAM record fields exceed block_size" */
#define TS_BAM_NAME_NOT_NUL   4  /* "BAM read name is not NUL-terminated" */
/* Room for compressed_cap compressed and plain_cap uncompressed bytes on the context's device; NULL on failure. */
ts_bam_chunk *ts_bam_chunk_create(ts_ctx *ctx, uint64_t compressed_cap, uint64_t plain_cap);
void ts_bam_chunk_destroy(ts_bam_chunk *chunk);
/* The chunk's next contents: the tail [carry_from, size) of what it holds moves to its front (device to device: the head of a
 * record that continues), then the members are inflated behind it — blocks[i].dst_off counts from the chunk's first byte
 * and must not lie inside the carried tail.  Descriptors are checked as by ts_bgzf_inflate.  The kernel runs on `stream`;
 * the caller's buffers are free when the call returns. */
int ts_bam_chunk_inflate(ts_bam_chunk *chunk, const void *compressed, uint64_t n, const ts_bgzf_block *blocks, size_t n_blocks,
                         uint64_t carry_from, void *stream);
/* Waits for the device; the lowest member of the last inflate that is not ok (ts_bgzf_status as above). */
int ts_bam_chunk_status(ts_bam_chunk *chunk, ts_bgzf_status *first_bad);
/* Bytes the chunk holds. */
uint64_t ts_bam_chunk_size(const ts_bam_chunk *chunk);
/* chunk[off, off + n) to host memory (the BAM header, which the host parses; tests).  Waits for the device. */
int ts_bam_chunk_read(ts_bam_chunk *chunk, uint64_t off, uint64_t n, void *host);
/* Walks records from `from`: up to cap table entries to recs (host memory), *n of them; *next = the offset of the first
 * record that was not taken (it does not end inside the chunk: the carry; or the table was full); *error != TS_BAM_OK when
 * the walk stopped at a record that is not valid, at *error_off.  Waits for the device. */
int ts_bam_chunk_walk(ts_bam_chunk *chunk, uint64_t from, ts_bam_record *recs, uint64_t cap, uint64_t *n, uint64_t *next,
                      int *error, uint64_t *error_off);
/* The same table by a parallel index: the contract of ts_bam_chunk_walk, word for word (recs, *n, *next, *error and *error_off
 * are what that call gives for the same chunk, `from` and cap), for chunks of many short records, where the one-wave walk is
 * the slowest stage.  The chunk is cut at absolute multiples of a span size; a wave per span finds up to `candidates` offsets
 * from which the record rule survives to the span's end, the spans are chained from `from` (a span whose entry is no
 * candidate is settled by the serial rule), and a wave per span writes its records.  The result never depends on the
 * candidates, only the time does.  Replaces the record loop of subsetBam (src/bam.cpp:188-259), as ts_bam_chunk_walk does.
 * Waits for the device. */
int ts_bam_chunk_index(ts_bam_chunk *chunk, uint64_t from, ts_bam_record *recs, uint64_t cap, uint64_t *n, uint64_t *next,
                       int *error, uint64_t *error_off);
/* The index's span size (a power of two, 64 .. 2^30; 262144 unless set) and candidates kept per span (1 .. 8; 4 unless set), for
 * tests and A/B runs of the stage that replaces src/bam.cpp:188-259; anything else: TS_ERR_INVALID_ARG, nothing changes. */
int ts_bam_chunk_set_index_geometry(ts_bam_chunk *chunk, uint32_t span_bytes, uint32_t candidates);
/* Cumulative since ts_create, monotonic and atomic, like ts_device_input_stats: calls of ts_bam_chunk_index (the stage that
 * replaces src/bam.cpp:188-259), spans its chain entered, spans whose entry was a candidate row, spans settled by the serial
 * rule, records the index wrote, bytes of candidate rows copied device to host. */
int ts_bam_index_stats(const ts_ctx *ctx, uint64_t out[6]);
/* SEQ of recs[i] (l_seq > 0 each) as ASCII bases (=ACMGRSVTWYHKDBN) into segment i of `reads`: an unrestricted tips-only batch
 * of n segments of l_seq bases made by ts_batch_create on the chunk's context.  The judgement is then the existing
 * ts_batch_scan + ts_batch_read_pass (+ ts_batch_read_pass_status).  Asynchronous on `stream`. */
int ts_bam_chunk_decode(ts_bam_chunk *chunk, const ts_bam_record *recs, size_t n, ts_batch *reads, void *stream);
/* n bytes of device memory that belong to the chunk (valid until the next call of this function or ts_bam_chunk_destroy):
 * a place for ts_batch_read_pass to write to for callers that do not allocate device memory themselves.  NULL on failure. */
void *ts_bam_chunk_pass_buffer(ts_bam_chunk *chunk, uint64_t n);
/* The records whose pass byte (d_pass[i], device memory, as ts_batch_read_pass writes it) is set, whole (block_size field
 * included), in input order, to host_out; *bytes and *n_passed say how much.  When *bytes > cap nothing is copied and the
 * call answers TS_ERR_INVALID_ARG (call again with room for *bytes).  Ordered on `stream`; waits for it. */
int ts_bam_chunk_gather(ts_bam_chunk *chunk, const ts_bam_record *recs, size_t n, const void *d_pass, void *host_out,
                        uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream);

/* ---- BGZF members WRITTEN on the device (a wave per member): what the reference's BgzfWriter does with zlib on the host, a
 *      member per payload (src/bgzf.cpp:227-276: deflateInit2(Z_DEFAULT_COMPRESSION, -15), crc32, the footer).  A payload of at
 *      most 65 280 bytes becomes one raw deflate block — dynamic Huffman codes over greedy LZ77 matches, or stored where that is
 *      no shorter, so a payload never grows by more than five bytes — framed by the 18-byte BGZF header and the CRC32 / ISIZE
 *      footer.  zlib inflates every member to its payload; the compressed bytes are this encoder's, not zlib's, and are a
 *      function of the payload alone.  Nothing here is on by default: bamSubsetDevice writes through these calls only under
 *      BamOutputDeflate::Device (include/teloscope_mi355x_io.hpp). */
/* Host in, host out (tests and tools: blocks no BAM produces; the counterpart of ts_bgzf_inflate for src/bgzf.cpp:227-276).
 * plain[0, n) is cut into consecutive payloads of payload_bytes (1 .. 65280, else TS_ERR_INVALID_ARG; the last may be shorter),
 * each becomes one complete member, in order and contiguous in out; *bytes and *n_members say how much (n == 0: none).  No EOF
 * marker is appended.  When *bytes > cap nothing is copied and the call answers TS_ERR_INVALID_ARG (call again with room for
 * *bytes). */
int ts_bgzf_deflate(ts_ctx *ctx, const void *plain, uint64_t n, uint32_t payload_bytes, void *out, uint64_t cap, uint64_t *bytes,
                    uint64_t *n_members);
/* ts_bam_chunk_gather with the passing records gathered into a device buffer of the chunk's, deflated there in payloads of
 * payload_bytes and downloaded as BGZF members (replaces zlib in BgzfWriter::write / flush, src/bgzf.cpp:227-276): the same
 * records in the same order.  *bytes = the members' bytes in host_out, *plain_bytes = what ts_bam_chunk_gather would have
 * returned in *bytes; when nothing passes there is no member and *bytes == 0.  When *bytes > cap nothing is copied:
 * TS_ERR_INVALID_ARG.  Ordered on `stream`; waits for it. */
int ts_bam_chunk_gather_bgzf(ts_bam_chunk *chunk, const ts_bam_record *recs, size_t n, const void *d_pass, uint32_t payload_bytes,
                             void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_passed, uint64_t *plain_bytes, void *stream);
/* Cumulative since ts_create, monotonic and atomic, like ts_bam_index_stats: device deflate calls that passed their argument
 * checks (the stage that replaces zlib in src/bgzf.cpp:227-276; a gather with nothing passing makes none), members they
 * delivered, plain bytes that went in, member bytes that came out. */
int ts_bgzf_deflate_stats(const ts_ctx *ctx, uint64_t out[4]);

/* ---- FASTQ text in the same resident chunk (include/teloscope_mi355x_io.hpp: fastqSubsetDevice): replaces, for
 *      --fastq-subset, the line reader and record check of readFastqRecord (src/input.cpp:96-149) and the read / filter /
 *      echo loop of Input::readFastqSubset (src/input.cpp:737-832).  The text reaches the chunk as plain bytes
 *      (ts_chunk_upload) or as BGZF members (ts_bam_chunk_inflate); lines are indexed, records framed and validated,
 *      sequences staged into a read batch's input buffer and passing records gathered on the device.  The chunk object, its
 *      carry and its inflate are ts_bam_chunk's: ts_chunk is another name for it, and ts_bam_chunk_create / _destroy /
 *      _inflate / _status / _size / _read / _pass_buffer serve it as they are. */
typedef struct ts_bam_chunk ts_chunk;
typedef struct ts_fastq_record {
    uint64_t off;                /* of the header line's first byte in the chunk */
    uint32_t seq_at;             /* the sequence line's first byte, relative to off */
    uint32_t seq_len;            /* bytes of the sequence line without its '\n' (a trailing '\r' included: the filter strips it,
                                    as it does for the host route, src/input.cpp:113-138) */
    uint32_t size;               /* from off to the end of the quality line, without its '\n' */
    uint32_t seq_cr;             /* 1 when the sequence line ends in '\r': the filter judges seq_len - seq_cr bases
                                    (ReadTelomereFilter::matches drops it, src/read-filter.cpp:38-40) */
} ts_fastq_record;
/* error of ts_fastq_chunk_walk: what is wrong with the LOWEST record that is not valid, in the order readFastqRecord checks
 * (src/input.cpp:113-138) */
#define TS_FASTQ_OK            0
#define TS_FASTQ_TRUNCATED     1  /* "truncated FASTQ record": the input ended with fewer than four lines */
#define TS_FASTQ_BAD_HEADER    2  /* "expected header line starting with '@'" */
#define TS_FASTQ_BAD_SEPARATOR 3  /* "expected separator line starting with '+'" */
#define TS_FASTQ_BAD_LENGTHS   4  /* "sequence and quality length differ" */
/* Room for at least plain_cap uncompressed bytes: the chunk grows (what it holds is kept) — a record larger than the chunk it
 * was made for (std::getline, src/input.cpp:116-123, reads a line of any length).  Waits for the device. */
int ts_chunk_reserve(ts_chunk *chunk, uint64_t plain_cap);
/* The chunk's next contents, plain: the tail [carry_from, size) moves to the front as for ts_bam_chunk_inflate, then
 * bytes[0, n) (host memory) go behind it; the chunk grows when they do not fit.  What the reference's getline calls read
 * from the stream it opened (src/input.cpp:116-123, :739), a block at a time.  Ordered on `stream`; the caller's bytes are free
 * when the call returns. */
int ts_chunk_upload(ts_chunk *chunk, const void *bytes, uint64_t n, uint64_t carry_from, void *stream);
/* Lines and records of the whole chunk (at most 4 GiB - 1 bytes), which starts at a record boundary: readFastqRecord's rule
 * (src/input.cpp:113-138: blank lines in front of a header are skipped, then four lines whatever they hold) as a prefix
 * scan over the lines.  *n = whole records in the chunk, the first min(*n, cap) of them to recs (host memory); when
 * *n > cap the call answers TS_ERR_INVALID_ARG (call again with room for *n).  *next = the first byte that was not consumed:
 * the header of the record that does not end inside the chunk, or of the unfinished line behind the last record (the
 * carry); with at_end != 0 the input ends with the chunk, its last line may lack the '\n', and *next = size.  *error !=
 * TS_FASTQ_OK: record *error_record (counted from the chunk's first, the *n records before it are valid and in the table)
 * at *error_off is not valid.  Waits for the device. */
int ts_fastq_chunk_walk(ts_chunk *chunk, int at_end, ts_fastq_record *recs, uint64_t cap, uint64_t *n, uint64_t *next,
                        int *error, uint64_t *error_record, uint64_t *error_off);
/* The bases of recs[i] (seq_len - seq_cr > 0 each) into segment i of `reads`: an unrestricted tips-only batch of n segments
 * of seq_len - seq_cr bases made by ts_batch_create on the chunk's context; bytes behind a read stay zero.  What the reference hands
 * to ReadTelomereFilter::matches per record (src/input.cpp:786).  The judgement is then ts_batch_scan + ts_batch_read_pass
 * (+ ts_batch_read_pass_status).  Asynchronous on `stream`. */
int ts_fastq_chunk_stage(ts_chunk *chunk, const ts_fastq_record *recs, size_t n, ts_batch *reads, void *stream);
/* The records whose pass byte (d_pass[i], device memory) is set, their four lines as they are and a '\n' behind each
 * (appendFastqRecord, src/input.cpp:140-149, written at :798-801), in input order, to host_out; *bytes, *n_passed and cap as for
 * ts_bam_chunk_gather.  Ordered on `stream`; waits for it. */
int ts_fastq_chunk_gather(ts_chunk *chunk, const ts_fastq_record *recs, size_t n, const void *d_pass, void *host_out,
                          uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream);

/* ---- Interleaved paired FASTQ (include/teloscope_mi355x_io.hpp: fastqSubsetPaired, fastqSubsetPairedDevice): the read subset of
 *      an input whose records come in pairs, first mate then second, as `samtools fastq`, `seqtk mergepe` and the -p modes of the
 *      short-read mappers write and read them.  The reference has no paired mode; the rule is this project's own, stated here and
 *      nowhere else, and every route follows it:
 *        - Records are those of the FASTQ record rule above (blank lines in front of a header are skipped, a record is four
 *          lines), numbered from 0 over the whole input.  Records 2 j and 2 j + 1 are pair j: its first and its second mate.
 *        - A record's name is the read block report's FASTQ name: the bytes behind '@' up to the first space, tab or the line's
 *          end, a '\r' in front of the '\n' not counted.  Its mate name is that name without its last two bytes when they are
 *          "/1" or "/2", and the name itself otherwise.  The suffix is removed once, and whichever mate carries it: "/3", "/12"
 *          and "/1/" are no suffixes, and a name of exactly "/1" has the empty mate name.
 *        - A pair is well formed when its two mate names are byte-equal; two empty names are.
 *        - Every record with bases is judged exactly as the unpaired route judges it.  A pair is kept when at least one of its
 *          mates passes; both records of a kept pair are written verbatim, first mate first, by ts_fastq_chunk_gather's rule
 *          (the four lines as they are, a '\n' behind each).  A mate without bases is written with its pair.  Pair order is
 *          input order.
 *        - Errors; the lowest offending place of the input wins.  The record errors keep their texts and numbers, "FASTQ record
 *          <n>: ..." with n counted as the unpaired route counts it, and so do "FASTQ input is empty" and "FASTQ input must
 *          start with '@'".  "FASTQ records <2j+1> and <2j+2> do not have the same name" (1-based record numbers) is thrown for
 *          the lowest pair that is not well formed; "FASTQ input ends with an unpaired record" when the input is otherwise valid
 *          and holds an odd number of records.  A record error at record r wins over the name error of a pair that contains r
 *          or lies behind it; the name error of a pair wholly in front of r wins over the record error.
 *        - Before the exception every whole, well-formed pair in front of the offending place has been judged and, if kept,
 *          written; a single valid record in front of a bad record is never written.  The bytes written before a failure do not
 *          depend on chunk size, sub-batch size or the number of contexts.
 *        - Statistics: total = records read, kept = records written (an even number).  The block report keeps its rule; a record
 *          written only for its mate has no line. */
/* Whether recs[2 j] and recs[2 j + 1] (records of the chunk, as ts_fastq_chunk_walk gives them; n even, else TS_ERR_INVALID_ARG)
 * are mates, for every j, a lane per pair, the names read where the chunk holds them: *mismatch = the lowest j that is no well-
 * formed pair, or UINT64_MAX.  n == 0 is valid and launches nothing.  Waits for the device. */
int ts_fastq_chunk_mates(ts_chunk *chunk, const ts_fastq_record *recs, size_t n, uint64_t *mismatch);
/* The pair's verdict for both of its records: read_of[i] (host memory) is record i's index in d_pass (device memory, as
 * ts_batch_read_pass writes it), or 0xFFFFFFFF when the record had no bases and was not staged; d_pair_pass[2 j] and
 * d_pair_pass[2 j + 1] (device memory, n bytes, not aliasing d_pass: the two halves of one ts_bam_chunk_pass_buffer) both become
 * 1 when either mate's own pass byte is set, else 0 — a d_pass for ts_fastq_chunk_gather(chunk, recs, n, ...) over all n records.
 * n even, else TS_ERR_INVALID_ARG.  Asynchronous on `stream`. */
int ts_fastq_chunk_pair_pass(ts_chunk *chunk, size_t n, const uint32_t *read_of, const void *d_pass, void *d_pair_pass, void *stream);

/* ---- SAM text in the same resident chunk (include/teloscope_mi355x_io.hpp: samSubset, samSubsetDevice): the third front end of
 *      the read filter, which the reference names and does not have (docs/algorithm.md: "BAM I/O is isolated from scoring so a
 *      future SAM parser or optional CRAM backend can reuse the same filter").  The text reaches the chunk as for FASTQ
 *      (ts_chunk_upload, ts_bam_chunk_inflate, the staging calls).  The rule is this project's own, and every route follows it:
 *        - A line starts at byte 0 or right behind a '\n'.  Its content excludes the '\n' and one '\r' that is its last byte.
 *          The input's last line may lack the '\n'.
 *        - A line whose first byte is '@' is a header line.  Every other line, an empty one included, is an alignment line.
 *        - Header lines are allowed only before the first alignment line of the input.  They are written out verbatim and in
 *          order, line ends as read, before any record.
 *        - An alignment line is cut at its tabs.  Field 10 is SEQ.  Field 11 is QUAL: from tab 10 to tab 11, or to the
 *          content's end.
 *        - Checks, in this order; the lowest offending line of the input wins:
 *            TS_SAM_HEADER_AFTER_RECORD  a '@' line after an alignment line      "header line after the first alignment record"
 *            TS_SAM_TOO_FEW_FIELDS       fewer than 10 tabs inside the line      "fewer than 11 fields"
 *            TS_SAM_EMPTY_SEQ            SEQ has length 0                        "empty SEQ field"
 *            TS_SAM_BAD_LENGTHS          SEQ is not "*", QUAL is not "*", and
 *                                        their lengths differ                    "SEQ and QUAL length differ"
 *          A route throws "SAM line <n>: <message>", n counted from 1 over the whole input, after the valid records before
 *          the bad line have been judged and written.  An empty input is "SAM input is empty"; a header-only input is valid.
 *        - SEQ exactly "*": the record has no sequence, is never kept, and is counted as missing (what bamSubset does for
 *          l_seq == 0).  Every other record is judged on its SEQ bytes as they lie: the filter folds case, and '=', '.', 'N'
 *          and the IUPAC letters are not ACGT.
 *        - A passing record's line is written verbatim: content, its '\r' if any, and a '\n' (which the input's last line
 *          gets when it lacked one).  Order is kept. */
typedef struct ts_sam_record {
    uint64_t off;                /* of the alignment line's first byte in the chunk */
    uint32_t seq_at;             /* SEQ's first byte, relative to off */
    uint32_t seq_len;            /* bytes of SEQ */
    uint32_t size;               /* the content's length with a trailing '\r': what the gather copies in front of its '\n' */
    uint32_t flags;              /* bit 0: SEQ is "*" */
} ts_sam_record;
#define TS_SAM_OK                  0
#define TS_SAM_HEADER_AFTER_RECORD 1
#define TS_SAM_TOO_FEW_FIELDS      2
#define TS_SAM_EMPTY_SEQ           3
#define TS_SAM_BAD_LENGTHS         4
/* Lines and records of the whole chunk (at most 4 GiB - 1 bytes), which starts at a line's first byte.  in_header != 0: the
 * input's header may still go on, and header lines are accepted up to the chunk's first alignment line; *n_header_lines counts
 * them and *header_end is that alignment line's offset, or *next when every whole line is a header.  in_header == 0: both are
 * 0 and any '@' line is TS_SAM_HEADER_AFTER_RECORD.  *n = alignment lines among the whole lines, the first min(*n, cap) of them
 * to recs (host memory); when *n > cap the call answers TS_ERR_INVALID_ARG (call again with room for *n).  *n_lines = whole
 * lines consumed, headers included.  *next = the first byte that was not consumed: the unfinished last line (the carry); with
 * at_end != 0 the input ends with the chunk, its last line may lack the '\n', and *next = size.  *error != TS_SAM_OK: line
 * *error_line of the chunk (counted from 0) at *error_off fails that check; *n and *n_lines then count what lies before it, and
 * *next = *error_off.  Waits for the device. */
int ts_sam_chunk_walk(ts_chunk *chunk, int at_end, int in_header, ts_sam_record *recs, uint64_t cap, uint64_t *n,
                      uint64_t *n_header_lines, uint64_t *header_end, uint64_t *n_lines, uint64_t *next, int *error,
                      uint64_t *error_line, uint64_t *error_off);
/* ts_fastq_chunk_stage for SAM: the seq_len bytes of recs[i]'s SEQ (flags bit 0 clear, seq_len > 0 each) into segment i of
 * `reads`, an unrestricted tips-only batch of n segments of seq_len bases on the chunk's context; bytes behind a read stay
 * zero.  Asynchronous on `stream`. */
int ts_sam_chunk_stage(ts_chunk *chunk, const ts_sam_record *recs, size_t n, ts_batch *reads, void *stream);
/* ts_fastq_chunk_gather for SAM: the records whose pass byte (d_pass[i], device memory) is set, `size` bytes and a '\n'
 * behind each, in input order, to host_out; *bytes, *n_passed and cap as for ts_bam_chunk_gather.  Ordered on `stream`; waits
 * for it. */
int ts_sam_chunk_gather(ts_chunk *chunk, const ts_sam_record *recs, size_t n, const void *d_pass, void *host_out,
                        uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream);

/* ---- The read block report: the telomere blocks of the kept reads as text, a BED beside a read subset (--fastq-subset,
 *      --bam-subset, --sam-subset, the FASTA read subset; include/teloscope_mi355x_io.hpp: the trailing `blocks` stream of
 *      fastqSubset, bamSubset, samSubset, fastaSubset and their device forms), formatted where a sub-batch's reads were judged.  The reference has no such output; the
 *      rule is this project's own, stated here and nowhere else, and every caller follows it.  It mirrors the terminal loop of the
 *      reference's writeBEDFile (src/teloscope.cpp, the lines of _terminal_telomeres.bed) with pathSize replaced by the read's
 *      length and the scaffold / contig word dropped:
 *        - For every kept record, in output order, one line per terminal block of its read.  The blocks are those of the read
 *          scanned as ONE tips-only segment at abs_pos 0 under the read filter's parameters, in the order in which
 *          ts_scan_segments_blocks returns terminal_blocks (the forward list's walk from the start, then the reverse list's walk
 *          from the end, each in push order).
 *        - A line is
 *            name \t start \t end \t block_len \t label \t forward_count \t reverse_count \t canonical_count \t
 *            non_canonical_count \t read_len \n
 *          with end = start + block_len and label the block's block_label as that call returns it.  Always '\n', never '\r'.
 *        - read_len is the number of bases judged: seq_len - seq_cr for FASTQ, SEQ's length for SAM, l_seq for BAM, n_bases for
 *          FASTA reads.
 *        - name is, for FASTQ, the header line's bytes behind '@' up to the first space, tab or the line's end, a '\r' in front of
 *          the line's '\n' not counted to the line (the name may be empty); for FASTA reads the same with '>' in place of '@';
 *          for SAM the bytes in front of the first tab; for BAM read_name without its NUL.
 *        - A record that is not kept has no line; a kept record has at least one (matches() is !terminalBlocks.empty(),
 *          src/read-filter.cpp:37-45).  The one amendment: a record of an interleaved pair ("Interleaved paired FASTQ" above)
 *          that is written only for its mate has no blocks and no line.  Secondary and supplementary BAM records are records like any other. */
/* One row of a batch's ordered blocks: the segment (read) of the batch and its block, start relative to the segment's abs_pos. */
typedef struct ts_read_block {
    uint32_t segment;
    uint32_t reserved;
    ts_block block;
} ts_read_block;
/* On a scanned tips-only batch, tiled or general (a full-scan batch answers TS_ERR_INVALID_ARG): runs the terminal walks and
 * leaves, in device memory of the batch, the terminal blocks of all segments ordered by (segment, walk, push order) — the order
 * of ts_scan_segments_blocks' terminal_blocks — and the index of every segment's first block (n + 1 entries).  The walks run
 * twice: a counting form says how many blocks each walk closes, exchange.hip's sums turn the counts into places, and a placing
 * form writes every block at its walk's base plus its push order; nothing is sorted on the host, no block leaves the device, and
 * the rows are the same bytes from launch to launch.  Asynchronous on `stream` (a general tips batch: the stream of its scan).
 * Overflow follows ts_batch_read_pass' protocol exactly: ts_batch_read_pass_status reports it, the caller then calls
 * ts_batch_sync and ts_batch_call_read_blocks again; after an overflow a tiled batch holds no rows and a general tips batch's are
 * memory-safe and meaningless.  Stands in for getTerminalBlocks (src/teloscope.cpp:29-176) as scanSegment calls it per read. */
int ts_batch_call_read_blocks(ts_batch *b, void *stream);
/* The rows of the last ts_batch_call_read_blocks to host memory, for tests and tools: *n of them; when *n > cap nothing is copied
 * and the call answers TS_ERR_INVALID_ARG (call again with room for *n).  Waits for the device. */
int ts_batch_read_blocks(ts_batch *b, ts_read_block *out, uint64_t cap, uint64_t *n);
/* The report's lines of a sub-batch, formatted on the device from the rows where they lie and the names where the chunk holds
 * them.  recs / n are the arrays given to the matching stage / decode call (ts_fastq_chunk_stage, ts_sam_chunk_stage,
 * ts_bam_chunk_decode), `reads` that batch after ts_batch_call_read_blocks (and after ts_batch_read_pass_status said that nothing
 * overflowed).  The lines, in row order, to host_out; *bytes and *n_lines say how much; cap and *bytes behave as for
 * ts_fastq_chunk_gather (*bytes > cap: nothing is copied, TS_ERR_INVALID_ARG).  Ordered on `stream`; waits for it.
 * (ts_fasta_chunk_block_lines, for FASTA reads, is declared with that front end's stage and gather below.) */
int ts_fastq_chunk_block_lines(ts_chunk *chunk, const ts_fastq_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                               uint64_t *bytes, uint64_t *n_lines, void *stream);
int ts_sam_chunk_block_lines(ts_chunk *chunk, const ts_sam_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                             uint64_t *bytes, uint64_t *n_lines, void *stream);
int ts_bam_chunk_block_lines(ts_bam_chunk *chunk, const ts_bam_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                             uint64_t *bytes, uint64_t *n_lines, void *stream);
/* The formatting stage alone, host in, host out: rows[0, n_rows) (segment: an index into the three per-segment arrays, which
 * must cover it), segment s's name names[name_off[s], name_off[s] + name_len[s]) and read length read_len[s].  Uploads them and
 * runs the kernels the chunk calls run; exists so that values no small read produces can be formatted (positions of twenty
 * digits, names of hundreds of bytes).  cap and *bytes as above. */
int ts_read_block_lines_format(ts_ctx *ctx, const ts_read_block *rows, uint64_t n_rows, const uint64_t *name_off,
                               const uint32_t *name_len, const uint32_t *read_len, const char *names, uint64_t names_len, void *out,
                               uint64_t cap, uint64_t *bytes);
/* Measurement aid: out[0] formatting calls that reached the device (a *_block_lines call or ts_read_block_lines_format), out[1]
 * lines, out[2] text bytes the device formatted since ts_create.  Cumulative, monotonic, atomic, like ts_match_text_stats. */
int ts_read_block_text_stats(const ts_ctx *ctx, uint64_t out[3]);

/* ---- FASTQ out of the BAM and SAM subsets: the kept records of --bam-subset and --sam-subset as FASTQ text instead of the
 *      format they were read in (include/teloscope_mi355x_io.hpp: bamSubsetFastq, samSubsetFastq and their device forms), formatted
 *      where a sub-batch's reads were judged, in place of the verbatim gather (ts_bam_chunk_gather, ts_sam_chunk_gather).  The
 *      reference writes a subset in the format it read (subsetBam, src/bam.cpp:188-259) and FASTQ only from FASTQ
 *      (appendFastqRecord, src/input.cpp:140-149; docs/algorithm.md: "the output can be piped straight into a mapper"); it has
 *      no conversion.  The rule is this project's own, stated here and nowhere else, and every route follows it:
 *        - For every kept record, in output order, four lines that always end in '\n' and never in '\r':
 *            '@' name '\n'  bases '\n'  '+' '\n'  quals '\n'
 *        - name is the read block report's name for the same front end: for BAM read_name without its NUL, for SAM the bytes
 *          in front of the first tab.  It may be empty.  No /1 or /2 suffix is ever added.
 *        - L is the number of bases judged: l_seq for BAM, SEQ's length for SAM.  A kept record has L >= 1.
 *        - Stored bases b[0..L): for BAM "=ACMGRSVTWYHKDBN"[code]; for SAM SEQ's bytes as they lie, with no case folding.
 *        - Stored quals q[0..L): for BAM min(byte, 93) + 33, and QUAL is missing when its first byte is 0xFF; for SAM QUAL's
 *          bytes as they lie, and QUAL is missing when field 11 is exactly "*" (for L == 1 too).  Missing QUAL is written as
 *          L times '!'.
 *        - FLAG: for BAM the little-endian 16-bit word 18 bytes behind the record's block_size field; for SAM the decimal
 *          value of the leading digits of field 2, of which at most nine are read; no leading digit means 0.
 *        - reverse is true when the caller asked for the read's own strand (TS_FASTQ_OUT_RESTORE_STRAND) and FLAG & 0x10 is
 *          set.  Without reverse bases = b and quals = q; with it bases[j] = comp(b[L-1-j]) and quals[j] = q[L-1-j].
 *        - comp: for BAM the letter of the 4-bit code with its four bits reversed (A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D;
 *          '=', S, W and N stay); for SAM the same pairs on letters of either case, case kept, U and u go to A and a, and
 *          every other byte is unchanged.
 *        - The judgement does not change: the filter judges the stored SEQ, and a record is kept exactly when the verbatim
 *          subset keeps it.  Secondary and supplementary records are records like any other: a caller who wants primaries
 *          only filters upstream.
 *        - A read block report written beside this output stays in stored-SEQ coordinates, whatever the orientation of the text.
 *        - No BAM header, EOF member or SAM header line is written. */
#define TS_FASTQ_OUT_RESTORE_STRAND 1u
/* ts_bam_chunk_gather / ts_sam_chunk_gather with the text above in place of the records' own bytes: recs, n and d_pass are those
 * calls' arguments, `flags` is 0 or TS_FASTQ_OUT_RESTORE_STRAND (any other bit: TS_ERR_INVALID_ARG).  The text of the records
 * whose pass byte is set, in input order, to host_out; *bytes and *n_passed say how much.  When *bytes > cap nothing is copied
 * and the call answers TS_ERR_INVALID_ARG (call again with room for *bytes).  A lane per record sizes its text, prefix sums place
 * it and cut it into pieces, a wave per piece writes 16 bytes per lane and store.  Ordered on `stream`; waits for it. */
int ts_bam_chunk_gather_fastq(ts_bam_chunk *chunk, const ts_bam_record *recs, size_t n, const void *d_pass, uint32_t flags,
                              void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream);
int ts_sam_chunk_gather_fastq(ts_chunk *chunk, const ts_sam_record *recs, size_t n, const void *d_pass, uint32_t flags,
                              void *host_out, uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream);
/* Measurement aid: out[0] FASTQ-out gathers that formatted text on the device, out[1] records, out[2] text bytes since
 * ts_create.  Cumulative, monotonic, atomic, like ts_read_block_text_stats. */
int ts_read_fastq_text_stats(const ts_ctx *ctx, uint64_t out[3]);

/* ---- FASTA text in the same resident chunk: the device form of the assembly front end.  Replaces the reference's FASTA load
 *      (gfalibs' stream parser behind Input::read, src/input.cpp:655-716: header lines split off, body lines joined into one
 *      sequence per record) and the cut of a path into segments and gaps at its N-runs (the path components walkPath
 *      iterates, src/input.cpp:934-1037).  The text reaches the chunk as for FASTQ (ts_chunk_upload, ts_bam_chunk_inflate);
 *      lines are indexed, records framed, body lines joined into contiguous bases and the runs found, all on the device.
 *      What comes back is the record table, the header lines and the runs: a few entries per record.  The joined bases stay
 *      in HBM and are scanned from there (TS_INPUT_DEVICE).
 *      The rules, which are the host route's (include/teloscope_mi355x_io.hpp: readFasta, FastaGroupReader, splitPath):
 *        header line   a line whose first byte is '>'; a line starts at byte 0 of the input or right behind a '\n'; a '>'
 *                      anywhere else is a base.  Bytes in front of the first header line belong to no record.
 *        name          the header line without its '>', its '\n' and a '\r' right before that (the host cuts it at the first
 *                      space or tab).
 *        bases         every byte of the record's body lines except '\n', a '\r' right before a '\n', and a '\r' that is the
 *                      input's very last byte.  Blank lines give nothing; any other byte, a space included, is a base.  A
 *                      record may have no bases and still is a record.
 *        runs          maximal runs of N n X x are gaps, maximal runs of anything else segments; record-relative, never
 *                      joined across records. */
typedef struct ts_fasta_record {
    uint64_t off;                /* of the record's '>' in the chunk */
    uint32_t text_len;           /* from off to the next record's '>' (or the chunk's end) */
    uint32_t body_at;            /* the first body line's first byte, relative to off (== text_len: no body line) */
    uint32_t n_bases;
    uint32_t name_at;            /* where the record's header line (without '>' and line end) lies in `names` */
    uint32_t name_len;
    uint32_t reserved;
} ts_fasta_record;
typedef struct ts_fasta_run {
    uint32_t record;             /* index into the joined records */
    uint32_t is_gap;             /* 1: a run of N n X x */
    uint32_t start;              /* record-relative, in bases */
    uint32_t len;
} ts_fasta_run;
/* Lines and records of the whole chunk (at most 4 GiB - 2 bytes), which starts at a line's first byte.  *n = complete records,
 * the first min(*n, cap) of them to recs (host memory); their header lines, gathered on the device into one buffer, to
 * names[0, *names_bytes) in ONE copy.  When *n > cap or *names_bytes > names_cap nothing usable is copied and the call answers
 * TS_ERR_INVALID_ARG (call again with room for *n and *names_bytes).  Without at_end the chunk's last record is never complete
 * (the next chunk may continue it) and *next is its '>': the carry; a chunk that holds nothing but one unfinished record gives
 * *n = 0 and *next = 0 and the caller grows the chunk (ts_chunk_reserve), as for FASTQ.  A chunk without any header line holds
 * no record: *next is the first byte of its last, unfinished line.  With at_end != 0 the input ends with the chunk, the last
 * line may lack its '\n', every record is complete and *next = size.  Waits for the device. */
int ts_fasta_chunk_walk(ts_chunk *chunk, int at_end, ts_fasta_record *recs, uint64_t cap, uint64_t *n, uint64_t *next,
                        char *names, uint64_t names_cap, uint64_t *names_bytes);
/* The bases of recs[0, n) (entries of the last walk's table, with the same at_end) joined into a buffer the chunk owns: record
 * i's n_bases bases from byte offsets[i] (a multiple of 16; host memory, n entries) of *d_bases (device memory, valid until the
 * next join or ts_bam_chunk_destroy), zero bytes between records, *total_bytes in all; and the records' runs found,
 * *n_runs of them (ts_fasta_chunk_runs reads them).  A stream compaction: kept bytes counted per 16 KB of body text, the counts
 * summed, every byte read once and written once.  Ordered on `stream`; waits for it. */
int ts_fasta_chunk_join(ts_chunk *chunk, const ts_fasta_record *recs, size_t n, int at_end, const void **d_bases,
                        uint64_t *offsets, uint64_t *total_bytes, uint64_t *n_runs, void *stream);
/* The runs of the last join, per record in order, records ascending (a record without bases has none): *n_runs of them, to
 * runs (host memory) when they fit cap, else TS_ERR_INVALID_ARG (call again with room for *n_runs).  Waits for the device. */
int ts_fasta_chunk_runs(ts_chunk *chunk, ts_fasta_run *runs, uint64_t cap, uint64_t *n_runs);
/* joined[off, off + n) of the last join to host memory (tests; the match sequences of -m).  Waits for the device. */
int ts_fasta_chunk_bases(ts_chunk *chunk, uint64_t off, uint64_t n, void *host);

/* ---- FASTA reads in the same resident chunk (include/teloscope_mi355x_io.hpp: fastaSubset, fastaSubsetDevice): the fourth front
 *      end of the read filter, for reads that come without qualities (corrected reads, seqtk seq -A, samtools fasta, unitigs and
 *      contigs).  The reference has no such mode (its --fastq-subset answers "FASTQ input must start with '@'"); the rule is this
 *      project's own, stated here and nowhere else, and every route follows it:
 *        - Lines, header lines, names and bases are those of the FASTA section above ("header line", "name", "bases"), exactly.
 *        - An input of 0 bytes is "FASTA input is empty"; a first byte that is not '>' is "FASTA input must start with '>'".
 *          There is no other input error.
 *        - A record with 0 bases is never kept and is counted as missing (what samSubset does for SEQ "*").  Every other record
 *          is judged on its joined bases as one read: the filter folds case, and any byte that is not A, C, G or T matches nothing.
 *        - A kept record is written verbatim, in input order: every byte from its '>' up to the next record's '>', line ends and
 *          blank lines as read.  The input's last record gets a '\n' when its last byte is not one.
 *        - What the read block report names a read of this front end, and its read_len, are stated in that report's section above.
 *        - Limits are ts_fasta_record's: text_len and n_bases have 32 bits.  The device route refuses a larger record by naming
 *          the host route. */
/* ts_fastq_chunk_stage for FASTA reads: the bases of recs[i] (any n entries of the last walk's table with n_bases > 0, walked
 * with the same at_end) into segment i of `reads`, an unrestricted tips-only batch, tiled or general, of n segments of n_bases
 * bases on the chunk's context; segment i starts at ts_batch_segment_offset(reads, i), and bytes behind a read stay zero.  A
 * stream compaction of body text into the batch's layout with ts_fasta_chunk_join's keep rule (one source): body text is cut at
 * multiples of 16 KB, a record that lies in one piece is read once and written once, the pieces of a larger record are counted
 * and a segmented exclusive sum per record places them; aligned 16-byte stores.  No runs are searched.  Asynchronous on `stream`. */
int ts_fasta_chunk_stage(ts_chunk *chunk, const ts_fasta_record *recs, size_t n, int at_end, ts_batch *reads, void *stream);
/* ts_fastq_chunk_gather for FASTA reads: the records whose pass byte (d_pass[i], device memory) is set, their text_len bytes as
 * they are and a '\n' behind a text that does not end in one (only the input's last record can), in input order, to host_out;
 * *bytes, *n_passed and cap as for ts_bam_chunk_gather.  Ordered on `stream`; waits for it. */
int ts_fasta_chunk_gather(ts_chunk *chunk, const ts_fasta_record *recs, size_t n, const void *d_pass, void *host_out,
                          uint64_t cap, uint64_t *bytes, uint64_t *n_passed, void *stream);
/* ts_fastq_chunk_block_lines for FASTA reads: recs / n are the arrays given to ts_fasta_chunk_stage. */
int ts_fasta_chunk_block_lines(ts_chunk *chunk, const ts_fasta_record *recs, size_t n, ts_batch *reads, void *host_out, uint64_t cap,
                               uint64_t *bytes, uint64_t *n_lines, void *stream);

/* ---- GFA text in the same resident chunk: the device form of the graph front end (include/teloscope_mi355x_gfa.hpp:
 *      annotateGfaDevice).  Replaces the line loop of the reference's GFA load (src/input.cpp:625-716): which lines are S, P
 *      and H records and where an S line's first four tabs lie.  The text reaches the chunk as for FASTQ (ts_chunk_upload,
 *      ts_bam_chunk_inflate); lines and tabs are indexed on the device, and what comes back is one table entry per segment, one
 *      per P / H line, and the segments' names and those lines in one buffer.  The sequences stay in HBM and are scanned where
 *      they lie (TS_INPUT_DEVICE segments at ts_chunk_data + off + f2_at).
 *      The rules, which are readGfa's (include/teloscope_mi355x_gfa.hpp):
 *        line      starts at byte 0 of the input or right behind a '\n'; its content excludes the '\n' and one '\r' that is its
 *                  last byte, also when the input's last line has no '\n'.  A line with empty content is nothing.
 *        single    content length 1, or second byte '\t'; the type is the first byte.
 *        segment   a single S line whose content, cut at its first four tabs (at most five fields, the fifth is the rest), has
 *                  three fields or more.  Which field is the sequence is the caller's decision (the graph's version).
 *        P / H     every single P and every single H line, whole; the caller cuts their fields.
 *        foreign   a line with content whose type is not '#' and that is not a single H or S (so P, L, W ... lines are);
 *                  the lowest one of the chunk is reported by its offset and first field (up to the first tab or the content's
 *                  end): a GFA 2 input may hold none. */
typedef struct ts_gfa_segment {
    uint64_t off;                /* of the S line's first byte in the chunk */
    uint32_t len;                /* of its content */
    uint32_t n_fields;           /* 3..5 */
    uint32_t f1_at, f1_len;      /* fields 1, 2 and 3, relative to off */
    uint32_t f2_at, f2_len;
    uint32_t f3_at, f3_len;      /* 0, 0 when n_fields == 3 */
    uint32_t name_at;            /* where field 1 (f1_len bytes) lies in `text` */
    uint32_t star;               /* bit 0: field 2 is exactly "*"; bit 1: field 3 is */
} ts_gfa_segment;
typedef struct ts_gfa_line {
    uint64_t off;                /* of the line's first byte in the chunk */
    uint32_t len;                /* of its content */
    uint32_t kind;               /* 'P' or 'H' */
    uint32_t text_at;            /* where the content lies in `text` */
    uint32_t reserved;
} ts_gfa_line;
typedef struct ts_gfa_foreign {
    uint64_t off;                /* of the lowest foreign line's first byte in the chunk */
    uint32_t len;                /* of its first field */
    uint32_t found;              /* 0: the chunk's whole lines hold no foreign line */
} ts_gfa_foreign;
/* Lines, tabs and records of the whole chunk (at most 4 GiB - 2 bytes), which starts at a line's first byte.  The segments of
 * its whole lines in input order to segs, its P / H lines in input order to lines, the segments' names and those lines,
 * gathered on the device in input order, to text in ONE copy.  When *n_segs > seg_cap, *n_lines > line_cap or *text_bytes >
 * text_cap nothing is copied and the call answers TS_ERR_INVALID_ARG (call again with room for what the three say).  *next =
 * the first byte of the unfinished last line (the carry; the chunk's size when it ends in '\n'); with at_end != 0 the input ends
 * with the chunk, its last line may lack the '\n' and *next = size.  The chunk's bytes are not changed.  Waits for the device. */
int ts_gfa_chunk_walk(ts_chunk *chunk, int at_end, ts_gfa_segment *segs, uint64_t seg_cap, uint64_t *n_segs, ts_gfa_line *lines,
                      uint64_t line_cap, uint64_t *n_lines, char *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *next,
                      ts_gfa_foreign *foreign);
/* The device address of the chunk's first byte (valid until the chunk grows, is refilled or destroyed): what a TS_INPUT_DEVICE
 * segment that lies in the chunk is addressed from. */
const void *ts_chunk_data(const ts_chunk *chunk);
/* The tail [carry_from, size) of `from` becomes the whole contents of `to` (another chunk, which grows when it must); `from`
 * keeps every byte.  The two may belong to different contexts: device to device where both contexts are on one GPU, a peer copy
 * where the destination's GPU can reach the source's memory, through host memory otherwise (the caller sees to it that nothing
 * changes `from` meanwhile).  A following ts_chunk_upload(to, ..., 0, ...), ts_bam_chunk_inflate(to, ..., 0, ...) or
 * ts_chunk_commit(to, ...) appends behind the carried bytes: how an unfinished line or record moves on while the chunk it began
 * in stays resident.  Ordered on `stream` of the destination's context; waits for it. */
int ts_chunk_carry_over(ts_chunk *to, ts_chunk *from, uint64_t carry_from, void *stream);

/* ---- a chunk's staging region, for read routes that deal the chunks of one input to several contexts (include/
 *      teloscope_mi355x_io.hpp: fastqSubsetDevice and bamSubsetDevice on a ReadTelomereFilter of several contexts).  Chunk k + 1
 *      lives on another context than chunk k, and the front of its contents, the unfinished record of chunk k, is known only when
 *      chunk k has been walked; its new bytes need not wait for that.  They are staged beside the chunk's contents, and committed
 *      behind the carry once it is there: contents = carry ++ staged.  Stands in for the same reference loops as ts_chunk_upload
 *      and ts_bam_chunk_inflate (the getline calls of readFastqRecord, src/input.cpp:116-123; BgzfReader::loadBlock,
 *      src/bgzf.cpp:57-196), which read one stream front to back and have no such seam. */
/* bytes[0, n) (host memory) behind what is staged; the region grows when they do not fit.  The chunk's contents are not touched.
 * Ordered on `stream`; the caller's bytes are free when the call returns. */
int ts_chunk_stage_upload(ts_chunk *chunk, const void *bytes, uint64_t n, void *stream);
/* BGZF members inflated and checksummed into the staging region: ts_bam_chunk_inflate without a carry, blocks[i].dst_off
 * counting from the region's first byte and not below what is staged already; staged = the highest dst_off + isize.  The members
 * are judged by ts_bam_chunk_status, as after ts_bam_chunk_inflate.  The kernel runs on `stream`; the caller's buffers are free
 * when the call returns. */
int ts_chunk_stage_inflate(ts_chunk *chunk, const void *compressed, uint64_t n, const ts_bgzf_block *blocks, size_t n_blocks,
                           void *stream);
/* Bytes staged and not committed yet. */
uint64_t ts_chunk_staged(const ts_chunk *chunk);
/* The staged bytes go behind the chunk's contents (device to device; the chunk grows when it must) and the region is empty
 * again.  The contents before it are typically a carry placed by ts_chunk_carry_over, or nothing: the chunk's first byte stays
 * at the 16-byte aligned address every walk, stage and gather kernel reads from.  Ordered on `stream`; waits for it. */
int ts_chunk_commit(ts_chunk *chunk, void *stream);

/* ---- assembly record filters on the two device routes (include/teloscope_mi355x_filter.hpp; scanFastaToFilesDevice and
 *      annotateGfaDevice with a selector): the few facts the filtered loaders' rules ask about bytes that the host never sees.
 *      The host stays the judge: these calls say what the text holds, the routes turn that into the reference's messages. */
/* has_sequence[i] (host memory, n bytes) = 1 when the body lines of recs[i] (entries of the chunk's last walk, any subset) hold
 * a byte other than '\n' and '\r', else 0: the filtered FASTA loader's "has no sequence" (FastaGroupReader::checkStrict).  Not
 * n_bases > 0: a body of "\r\r\n" has one base and no sequence.  A wave per 16 KB of body text at most, which stops at the
 * first such byte it meets.  Ordered on `stream`; waits for it. */
int ts_fasta_chunk_strict(ts_chunk *chunk, const ts_fasta_record *recs, size_t n, unsigned char *has_sequence, void *stream);
/* The whole lines of a chunk that ts_gfa_chunk_walk walked last, with the same at_end, against the filtered GFA loader's rules
 * (validateFilteredGfa, include/teloscope_mi355x_gfa.hpp).  *n_lines = the whole lines in [0, *next) of that walk, blank and
 * '#' lines included.  flagged = the lines that break a rule, in input order; code = the first rule the line breaks, in the
 * loader's order:
 *     1  an "H\t" line that contains "\tVN:Z:2"            5  type C
 *     2  shorter than 2 bytes, or its second byte no tab   6  an S line whose third field is not empty, all digits and
 *     3  type O, U, E, G or F                                 followed by a tab
 *     4  type W                                            7  type not H, S, L, J or P
 * The loader drops every '\r' of a line before it judges it; the device does not: a line that holds a '\r' anywhere but as the
 * last byte of its content gets TS_GFA_CHECK_HOST_DECIDES and the caller reads that one line back (ts_bam_chunk_read) and
 * judges it on the host.  Lines without content and '#' lines are never flagged otherwise.  When *n_flagged > cap nothing is
 * copied and the call answers TS_ERR_INVALID_ARG (call again with room for *n_flagged).  Waits for the device. */
#define TS_GFA_CHECK_HOST_DECIDES 255
typedef struct ts_gfa_flagged {
    uint64_t off;                /* of the line's first byte in the chunk */
    uint32_t line;               /* its ordinal among the chunk's lines, from 0 */
    uint32_t len;                /* of its content (without '\n' and one '\r' in front of it) */
    uint32_t code;               /* 1..7, or TS_GFA_CHECK_HOST_DECIDES */
    uint32_t type;               /* the line's first byte */
} ts_gfa_flagged;
int ts_gfa_chunk_check(ts_chunk *chunk, int at_end, ts_gfa_flagged *flagged, uint64_t cap, uint64_t *n_flagged, uint64_t *n_lines);

/* ---- plain gzip (one long deflate stream per member, not BGZF) inflated on the device: replaces gzread in
 *      detail::ChunkFeed::read (include/teloscope_mi355x_io.hpp) for the text routes.  A window of a member's compressed bytes
 *      is cut into spans of span_bytes; a wave per span searches its first deflate block start (BFINAL = 0, BTYPE = 2, a
 *      header that builds three valid codes) and decodes from there without knowing the 32 KiB in front of it (16-bit
 *      symbols: a byte, or a marker for a byte of those 32 KiB); the host chains the spans whose start is the end of the
 *      one before (a false candidate is stepped over and its span dropped); the chained spans' last 32 KiB are resolved in
 *      order, then every symbol becomes a byte at its plain offset and the bytes' CRC32 is taken.  The caller parses member
 *      headers and trailers (host work that reads no payload byte) and keeps zlib for whatever the chain did not verify: a
 *      raw inflate primed at end_bit with the last 32 KiB as its dictionary continues at exactly that bit. */
typedef struct ts_gzip ts_gzip;
/* why the verified chain ended */
#define TS_GZIP_WINDOW_END    0  /* the window's bytes ended inside a block: end_bit is the last block boundary in front of it
                                    (start_bit: the block is larger than the window, which a larger window or zlib answers) */
#define TS_GZIP_FINAL_BLOCK   1  /* at the end of the member's final block: end_bit is the deflate stream's end */
#define TS_GZIP_NO_CANDIDATE  2  /* a window of four spans or more that does not begin with a dynamic block and has no candidate
                                    behind its start (stored blocks: a file that did not compress): nothing was decoded */
#define TS_GZIP_SPAN_OVERFLOW 3  /* a span's symbols did not fit its room (16 per compressed byte of a span, 512 Ki at least) */
#define TS_GZIP_BAD_DEFLATE   4  /* what follows end_bit is not deflate, or reaches in front of the member's first byte */
/* what lies in front of start_bit */
#define TS_GZIP_HISTORY_EMPTY 0  /* nothing: a member's first window */
#define TS_GZIP_HISTORY_KEPT  1  /* the bytes the object's last decode produced (and what lay in front of them) */
#define TS_GZIP_HISTORY_GIVEN 2  /* history[0, history_len), history_len <= 32768: the bytes right in front */
typedef struct ts_gzip_result {
    uint64_t end_bit;            /* in the window: where the verified chain ends, a block boundary; start_bit when nothing was verified */
    uint64_t plain_bytes;        /* produced by this call (they replace what the object held) */
    uint32_t crc32;              /* of those bytes */
    int32_t  status;             /* TS_GZIP_WINDOW_END ... TS_GZIP_BAD_DEFLATE */
    int32_t  member_ended;       /* 1 when status is TS_GZIP_FINAL_BLOCK */
    uint32_t spans_probed, spans_chained, spans_dropped;
} ts_gzip_result;
/* span_bytes: a multiple of 1024 in 1024 .. 1 MiB.  NULL on failure. */
ts_gzip *ts_gzip_create(ts_ctx *ctx, uint32_t span_bytes);
void ts_gzip_destroy(ts_gzip *gz);
/* Decodes compressed[0, n) (host memory, n <= 256 MiB, at most 65535 spans, and 2 bytes per symbol of the spans' room within
 * 4 GiB) from start_bit on (inside the first span).
 * Damaged input is not an error of the call: TS_OK, and res->status says where and why the chain ended.  Waits for the
 * device; the caller's buffers are free when the call returns. */
int ts_gzip_decode(ts_gzip *gz, const void *compressed, uint64_t n, uint64_t start_bit, int history_mode, const void *history,
                   uint64_t history_len, ts_gzip_result *res);
/* Up to `want` of the produced bytes that were not taken yet go behind the chunk's bytes from carry_from on (the tail moves to
 * the front as for ts_chunk_upload; device to device), *moved of them; what is left stays for the next call. */
int ts_gzip_take(ts_gzip *gz, ts_chunk *chunk, uint64_t carry_from, uint64_t want, uint64_t *moved);
/* produced[off, off + n) to host memory (tests).  Waits for the device. */
int ts_gzip_read(ts_gzip *gz, uint64_t off, uint64_t n, void *host);
/* The last *len <= 32768 bytes in front of the last decode's end_bit (the dictionary of the raw inflate that takes over there)
 * to host[0, *len). */
int ts_gzip_history(ts_gzip *gz, void *host, uint64_t *len);
/* The caller says that it handed `parts` stretches of the input to zlib (where a chain ended short and a larger window was
 * not the answer; a member too small to bother the device with): the library cannot see that, and the statistics should. */
int ts_gzip_note_fallback(ts_gzip *gz, uint64_t parts);
/* Cumulative since ts_create, like ts_device_input_stats: windows decoded, spans probed, spans chained, spans dropped (a
 * candidate that was stepped over), plain bytes produced on the device, parts handed to zlib (ts_gzip_note_fallback). */
int ts_gzip_stats(const ts_ctx *ctx, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* TELOSCAN_H */
