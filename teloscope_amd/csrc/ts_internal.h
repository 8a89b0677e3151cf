// ts_internal.h — structures shared by the host side of libteloscan and its HIP kernels.
#ifndef TS_INTERNAL_H
#define TS_INTERNAL_H

#include <stdint.h>

// Geometry of the tiled uniform-k scan kernel (kernels.hip: ts_scan_tiles).
//
// A segment (or tips-only region) is cut into tiles; ONE WAVEFRONT scans one tile.  A tile OWNS
// `nwin` consecutive windows (window k covers [k*s, k*s+w)) = the `nwin*s` bases where those
// windows start, and additionally reads a halo so that every owned window and every k-mer
// that starts in an owned base is complete.  Positions inside a tile are "plane coordinates":
// byte offset from the 16-byte-aligned address at or below the tile's first owned base.

#define TS_MAX_WG_THREADS 1024         // up to 16 wavefronts per workgroup, one workgroup per CU
#ifndef TS_LIST
#define TS_LIST         512            // entries of a wave's match queue (power of two >= 64; a denser chunk is appended in lane groups)
#endif
#define TS_CHUNK        2016           // positions a wave resolves per iteration (63 lanes x 32)
#define TS_BLK_COUNTERS 10             // 4 NB dwords of window nucleotide counts, then per step block: match head[3] rest[3]
#define TS_TICKET_STRIDE 64            // dwords between two ticket counters (each in its own 256 bytes)
#define TS_MAX_TICKET_GROUPS 64
#define TS_IN_PAD       4096           // bytes of zero padding after the last segment in the input buffer

struct TsTile {                 // 32 bytes
    uint64_t in_off;            // byte offset (input buffer) of the tile's first owned base
    uint64_t win_out;           // index of the first owned window record
    uint32_t nrel;              // bases from the first owned base to the end of the segment/region (clamped)
    uint32_t nwin;              // owned windows (tips mode: 1 pseudo block, no record written)
    uint32_t own_len;           // owned bases = min(nrel, nwin*s)
    uint32_t seg;               // segment index (host bookkeeping / summary kernel)
};

struct TsScanParams {
    const uint8_t  *in;
    const TsTile   *tiles;
    const uint32_t *table;      // pair table (table_rows dwords) followed by the flag table (fc_bytes)
    uint32_t       *windows_out;    // 8 x u32 per window
    uint32_t       *matches_out;    // packed records, one region of region_cap records per wave
    unsigned long long *tile_off;   // tile directory: first record of each tile (index into matches_out)
    uint32_t       *tile_stats;     // tile directory: {matches, canonical, forward, visible (with emit, else 0)} per tile
    uint32_t       *wave_fill;      // per wave: records it needed (> region_cap means overflow); with emit, behind them per wave: visible records it needed (> vis_cap)
    uint32_t       *tile_tickets;   // 2 x ticket_groups ticket counters, TS_TICKET_STRIDE dwords apart; set [ticket_slot] is zero at launch
    uint32_t        region_cap;     // records per wave region
    uint32_t        ntiles;
    uint32_t        waves_per_wg;
    uint32_t        table_rows;     // dwords of the pair table: 4^(k+1) / 16, or 4^(k+1) / 4 as a byte table
    uint32_t        pair_byte_table;// 1: one byte per (k+1)-mer (k <= 6); 0: 2 bits per (k+1)-mer
    uint32_t        fc_bytes;       // flag table size in bytes (16-byte multiple)
    uint32_t        fc_byte_table;  // 1: one byte {forward, canonical} per k-mer; 0: 2 bits per k-mer
    uint32_t        k;              // pattern length
    uint32_t        s, w;           // step and window (tips mode: s = w = tile size)
    uint32_t        s_inv;          // ceil(2^16 / s): 24-bit multiply division by s (tile-relative positions < 2^16)
    uint32_t        s_magic22;      // ceil(2^22 / s) and
    uint32_t        div_exact;      // 1: u x s_magic22 >> 22 == u / s for every tile position u (no correction step)
    uint32_t        halo_blocks;    // step blocks read beyond the owned ones: ceil(w / s) - 1
    uint32_t        nch;            // chunks of TS_CHUNK positions per tile
    uint32_t        max_windows;    // windows per tile (rows of the LDS record buffer)
    uint32_t        acc_copies;     // lane-interleaved copies of the window match accumulators (power of two)
    uint32_t        stage_cap;      // match records a wave can stage in LDS before it flushes them
    uint32_t        stage_u16;      // 1: the stage holds 16-bit entries (position << 2 | flags < 2^16: tiles of at most 16 k positions)
    uint32_t        fold_mask;      // 0xDFDFDFDF (fold case) or 0xFFFFFFFF
    uint32_t        straddle_fix;   // 1: w == s, drop matches that straddle a window end
    uint32_t        windows_on;     // 0 in tips-only mode
    uint32_t        nuc_on;         // nucleotide counts wanted (-g / -e)
    uint32_t        block_sums;     // 1: w is a multiple of s, nucleotide counts are summed per step block
    uint32_t        acc_blocks;     // 1: (w a multiple of s) the match fields of the window records accumulate per step block too
    uint32_t        dynamic_tiles;  // 1: a wave takes the next free tile (ticket counter); 0: tiles dealt round-robin
    uint32_t        ticket_slot;    // which of the two counter sets this launch counts on (it zeroes the other)
    uint32_t        ticket_groups;  // groups of workgroups with a counter each (<= 64; group g owns the tiles t = g mod groups)
    uint32_t        wgs_per_cu;     // host side: workgroups that share a CU (1, or 2 of 10 waves: selects the 80-VGPR build)
    // ---- what the scan hands to block calling and to a shard's message (window scans only; emit == 0: none of it)
    uint32_t        emit;           // 1: visible records + per-tile chain summaries are produced
    uint32_t        kdist;          // -k (maxMatchDistance): matches farther apart than this start a new chain
    uint32_t        vis_wide;       // 0: visible records are u16 (tile positions < 2^14), 1: u32
    uint32_t        vis_cap;        // visible records per wave region
    void           *vis_out;        // visible records, one region of vis_cap records per wave (u16 or u32 each)
    const uint32_t *tile_zone;      // per tile: {zlo, zhi} 16 bits each: a non-canonical record at tile position u is visible
                                    // (lies in its segment's terminal zone) iff u < zlo || u >= zhi
    uint32_t       *tile_chain;     // per tile: TsTileChain (4 dwords)
    // ---- a shard's scan that packs its window records itself (ts_batch_bind_shard_message; emit only).  nullptr: 8 x u32 per
    // window to windows_out.  Else the record of plan window i, win_pack_lo <= i < win_pack_hi (the owned windows), goes to
    // win_packed + i * win_pack_bytes in the message's bit-packed form (shard.hip: ts_shard_pack_windows) and windows_out is
    // not written at all.
    uint8_t        *win_packed;
    unsigned long long win_pack_lo, win_pack_hi;
    uint32_t        win_pack_bytes, win_field_bits;
    // ---- a read filter's batch (tips-only, 16-bit stage entries, every read terminal zone as a whole, no emit): the records leave as
    // 16 bits each — the stage's own entries: position (14 bits) << 2 | forward << 1 | canonical — into matches_out read as uint16_t
    // (regions of region_cap records as before).  Their only reader is the read predicate (predicate.hip), and the records are a
    // tenth of what the read step moves through HBM, a step that runs at what HBM gives (profiles/r05/reads_u16_records.txt).
    uint32_t        rec16;
};

// What ts_scan_tiles leaves per tile beside {matches, canonical, forward, visible} in tile_stats: the summary the
// interstitial screening needs instead of re-reading the tile's records, and where the tile's visible records are.
// A chain (getInterstitialBlocks, src/teloscope.cpp:235-253) links consecutive matches of any kind at most -k apart; an
// "internal head" is a record of the tile more than -k behind its predecessor IN the tile.
//   word 0   position of the tile's first record | position of its last record << 16      (tile-relative, < 2^16)
//   word 1   bits 0-14  canonical records ahead of the first internal head (all of them when there is none), saturating
//            bit  15    the tile holds an internal head
//            bits 16-30 canonical records from the last internal head on (all of them when there is none), saturating
//            bit  31    a chain between two internal heads of the tile holds four or more canonical records
//   word 2,3 index (u64) of the tile's first visible record in vis_out
#define TS_CHAIN_HEADS 0x8000u
#define TS_CHAIN_INNER 0x80000000u
#define TS_ZONE_NONE   0xFFFF0000u      // tile_zone word of a tile no position of which is terminal

// parameters of getTerminalBlocks for the device-side predicate (kernels.hip: ts_terminal_predicate)
struct TsPredParams {
    uint32_t terminal_limit;
    uint32_t max_match_dist, min_block_len, max_block_dist, min_block_counts;
    float    min_block_density;
    uint32_t k;                         // match length (uniform)
    uint32_t long_list;                 // least number of match records that makes a read "long" (walked by a whole wave, predicate.hip)
};

// ---- device block calling (blockcall.hip) ----
struct TsDevBlock {                     // ts_block (include/teloscan.h) + bookkeeping, 64 bytes
    unsigned long long start;
    uint32_t block_len, block_counts, forward_count, reverse_count, canonical_count, non_canonical_count;
    uint32_t total_covered, fwd_covered, can_covered;
    uint8_t  has_valid_or, is_longest;
    char     block_label;
    uint8_t  reserved;
    uint32_t seg;                       // segment index
    uint32_t kind;                      // 0/1 terminal (forward / reverse walk), 2 interstitial
    uint32_t seq;                       // push order among the segment's terminal blocks
    uint32_t pad;
};

// One row of a batch's ordered terminal blocks (ts_batch_call_read_blocks): ts_read_block of include/teloscan.h, 56 bytes — the
// segment, then the block as a TsDevBlock begins
struct TsReadBlockRow {
    uint32_t seg, reserved0;
    unsigned long long start;
    uint32_t block_len, block_counts, forward_count, reverse_count, canonical_count, non_canonical_count;
    uint32_t total_covered, fwd_covered, can_covered;
    uint8_t  has_valid_or, is_longest;
    char     block_label;
    uint8_t  reserved;
};

struct TsBlockCallParams {
    const TsTile *tiles;
    const unsigned long long *tile_off;
    const uint32_t *tile_stats;
    const uint32_t *matches;
    TsDevBlock *blocks;
    uint32_t *n_blocks;                 // atomic counter; > block_cap means overflow
    uint32_t block_cap;
    uint32_t *cand;                     // chains the interstitial screening lists for exact evaluation: {tile, record index} pairs
    uint32_t *n_cand;                   // atomic counter (zero at launch); > cand_cap: reported as a block overflow
    uint32_t cand_cap;
    uint32_t terminal_limit, max_match_dist, min_block_len, max_block_dist, min_block_counts;
    float    min_block_density;
    uint32_t k;                         // match length (uniform)
    uint32_t its_min_len;               // 2 * patterns.front().size()
    uint32_t rec16;                     // the tiled kernel's records at 16 bits each (TsScanParams.rec16): `matches` is then read as uint16_t
    unsigned long long gen_lens;        // 0: the tiled kernel's records (position << 2 | forward << 1 | canonical, length k);
                                        // else the general kernels' (position << 5 | length index << 2 | canonical << 1 | forward)
                                        // and the up to eight pattern lengths, six bits each, length index i at bits 6i..
    // the general path's other cases (blockcall.hip, MODE 1)
    uint32_t wide;                      // records of the wide form: position << 8 | length index (six bits) << 2 | canonical << 1 | forward
    uint32_t unordered;                 // the stream lies in the reference's PUSH order (generic.hip: ts_general_compact_push), not in position order
    const uint32_t *wide_len;           // wide: the lengths by index (device)
    unsigned long long *its_range;      // unordered: per segment {first, end} stream indices of the interstitial search (ts_its_range writes, the search reads)
};

// ---- shard results (shard.hip, shard.cpp): what one device contributes to a scan that several devices share ----
// A shard OWNS a run of consecutive tiles of the batch's plan and additionally scans a few CONTEXT tiles either side
// where a segment continues on a neighbour (blocks are chains of matches: a chain that begins in an owned tile is
// followed into the context).  After its scan it packs ONE message:
//
//   TsShardHeader | TsShardSeg x n_segs | packed window records | u16 visible-record count per owned tile |
//   visible records (u16 or u32 each, capacity) | TsDevBlock x capacity
//
// "visible" = the match records a writer reads: canonicalMatches, and nonCanonicalMatches of the terminal zone
// (src/teloscope.cpp:486-496, writers :700-868); everything else the match stream holds is consumed by block calling,
// which has happened on the device.  Section offsets are a pure function of the plan, the split and the capacity scale
// (shard_layout, tiled_plan_core.h), so sender and receiver agree on them without talking.
#define TS_SHARD_MAGIC   0x44485354u    // "TSHD"
#define TS_SHARD_VERSION 1u
#define TS_SHARD_F_VISIBLE_OVERFLOW 0x1u    // more visible records than the section holds (n_visible says how many)
#define TS_SHARD_F_BLOCK_OVERFLOW   0x2u    // more blocks than the section holds (n_blocks says how many)
#define TS_SHARD_F_SCAN_OVERFLOW    0x4u    // a wave's record region overflowed in the scan: ts_batch_sync, then pack again
#define TS_SHARD_F_CONTEXT          0x8u    // a chain or a terminal walk ran out of the context tiles: the segment needs the full path

struct TsShardHeader {                  // 128 bytes
    uint32_t magic, version;
    uint32_t part, n_parts;
    unsigned long long own_begin, own_end;      // tiles (plan indices)
    unsigned long long ext_begin, ext_end;
    unsigned long long seg_begin;               // first segment with an owned tile
    uint32_t n_segs;
    uint32_t flags;                             // TS_SHARD_F_*
    unsigned long long n_visible;               // visible records of the owned tiles (may exceed the capacity: overflow)
    uint32_t n_blocks;                          // blocks emitted (may exceed the capacity: overflow)
    uint32_t visible_bytes;                     // 2 or 4 per visible record
    unsigned long long visible_capacity;
    uint32_t block_capacity;
    uint32_t window_bytes;                      // bytes per packed window record
    unsigned long long n_windows;               // owned window records
    unsigned long long msg_bytes;
    unsigned long long reserved[2];             // [0]: scratch of the pack (candidate counter), 0 on the wire; [1]: the capacity scale
};
static_assert(sizeof(TsShardHeader) == 128, "TsShardHeader is 128 bytes on the wire");

#define TS_SEG_F_HAS_START   0x1u       // the shard owns the segment's first tile: it walked the forward list from the start
#define TS_SEG_F_HAS_END     0x2u       // ... its last tile: it walked the reverse list from the end
#define TS_SEG_F_FWD_WALKED  0x4u       // the forward walk ran (>= 2 forward matches among the tiles the shard sees)
#define TS_SEG_F_REV_WALKED  0x8u
#define TS_SEG_F_CONTEXT     0x10u      // a walk or a chain of this segment ran out of context
struct TsShardSeg {                     // 64 bytes, one per segment with an owned tile
    unsigned long long fwd_boundary, rev_boundary;  // segment-relative; what this shard used for its interstitial search
    unsigned long long n_matches, n_canonical, n_forward;   // over the OWNED tiles of the segment
    unsigned long long seen_matches, seen_forward;  // over all its tiles the shard scanned (owned + context)
    uint32_t flags;
    uint32_t reserved;
};
static_assert(sizeof(TsShardSeg) == 64, "TsShardSeg is 64 bytes on the wire");

struct TsShardSegIn {                   // per-segment table of the shard kernels, 64 bytes
    unsigned long long in_off, len, abs_pos;    // input layout offset, length, absolute position of the segment
    unsigned long long lo_rel, hi_rel;          // segment-relative position of the first base of tile t0 / behind the last base of
                                                // tile t1 - 1 (0 and len when the shard holds none of its tiles)
    uint32_t t0, t1;                            // its tiles the shard scanned, as indices into the batch's (range-local) arrays
    uint32_t o0, o1;                            // its OWNED tiles, same indexing (o0 == o1: none)
    uint32_t flags;                             // TS_SEG_F_HAS_START / HAS_END
    uint32_t seg;                               // plan index of the segment
};

struct TsVisibleOut {                   // the visible records of a shard's owned tiles, written by the interstitial pass
    const unsigned long long *off;      // per owned tile (+1): index of its first visible record; nullptr = not wanted
    void *dst;                          // the message's visible section
    unsigned long long capacity;        // records it holds (more in all: nothing is written, the header reports it)
    uint32_t own0, own1;                // owned tiles, range-local
    uint32_t rec_bytes;                 // 2 or 4
    uint32_t terminal_limit;
};

struct TsShardPackParams {
    const TsTile *tiles;                // range-local arrays of the batch (the range = owned + context tiles)
    const unsigned long long *tile_off;
    const uint32_t *tile_stats;
    const uint32_t *matches;      uint32_t rec16;      // (read as uint16_t when rec16: TsScanParams.rec16)
    const uint32_t *windows;            // 8 x u32 per window of the range, from win_lo
    const uint32_t *wave_fill;
    uint32_t region_cap, nwaves;
    uint32_t own0, own1;                // owned tiles, range-local
    unsigned long long win_lo;          // plan index of the range's first window record
    unsigned long long own_win0, own_win1;      // owned window records (plan indices)
    const TsShardSegIn *segs;
    uint32_t n_segs;
    uint32_t terminal_limit, k, nuc_on, field_bits;
    unsigned char *msg;
    unsigned long long off_segs, off_windows, off_tilevis, off_visible, off_blocks;   // byte offsets of the sections
    // what the scan left for the message (kp.emit; chain == nullptr: the visible records come out of the match stream)
    const uint32_t *chain;              // TsTileChain per tile (words 2, 3: where the tile's visible records are in vis_src)
    const void *vis_src;                // the scan's visible records, per-wave regions
    uint32_t vis_src_wide;              // 1: u32 each, 0: u16
    uint32_t vis_cap;                   // records per wave region (wave_fill[nwaves + w] > vis_cap: that wave's region overflowed)
};

// ---- general kernels (generic.hip) ----
struct TsGenericPatterns {
    const unsigned long long *codes;    // per length: ascending 2-bit codes (base i at bits 2i..2i+1)
    const uint8_t *flags;               // bit0 forward, bit1 canonical (parallel to codes)
    uint32_t nlen;                      // distinct pattern lengths, ascending
    uint32_t len[8];
    uint32_t first[9];                  // codes[first[i] .. first[i+1]) have length len[i]
};

// The WIDE form's tables (generic.hip: ts_general_wide): pattern sets beyond the table forms above — up to 63 distinct lengths of
// up to 63 bases, what a ts_pattern can hold.  Codes are 128 bits (lo: bases 0..31, hi: bases 32..62), per length ascending by
// (lo, hi); everything lives in device memory.
struct TsWidePatterns {
    const unsigned long long *lo, *hi;
    const uint8_t *flags;               // bit0 forward, bit1 canonical (parallel to lo / hi)
    const uint32_t *len;                // nlen lengths, ascending
    const uint32_t *first;              // nlen + 1: patterns [first[i], first[i + 1]) have length len[i]
    uint32_t nlen, npat;
};
#define TS_WIDE_HALO 64                 // bases staged beyond a tile for the wide form (the other forms: 32)

struct TsGenericGeom {
    uint32_t s, w, longest;
    uint32_t nuc_on, fold;
    uint32_t s_magic;                   // floor(2^32 / s) + 1 (s >= 2): x / s == umulhi(x, s_magic) for x < 2^32 / s (the list form, s <= 8192)
    uint32_t cw, rw;                    // w / s and w - cw s
};

#define TS_GENERAL_TILE 4096            // positions per tile of the general kernels (generic.hip)
struct TsGeneralTile {                  // 40 bytes
    unsigned long long in_off;          // byte offset (input layout) of the tile's first base; the match mask is indexed alike
    unsigned long long seg_rel;         // segment-relative position of that base (P0)
    unsigned long long k_p0;            // P0 / step and
    uint32_t n;                         // positions of the tile (<= TS_GENERAL_TILE)
    uint32_t avail;                     // bases from the tile's first base to the end of its region (clamped to n + 32)
    uint32_t seg;                       // segment index within the group
    uint32_t r_p0;                      // P0 - k_p0 step: the host walks them from tile to tile, so that the list kernel never
                                        // divides 64-bit numbers (five such divisions per tile and wave were a third of its
                                        // vector instructions)
};

struct TsLaunchInfo {
    uint32_t grid;
    uint32_t lds_bytes;
};

#ifdef __cplusplus
extern "C++" {
// Implemented in kernels.hip (compiled by hipcc).  All return a hipError_t as int.
int  ts_k_prepare(uint32_t lds_bytes);                       // raises the dynamic-LDS limit
int  ts_k_launch_scan(const TsScanParams *p, uint32_t grid, uint32_t lds_bytes, void *stream);
int  ts_k_launch_summary(const uint32_t *tile_stats, const uint32_t *seg_first_tile,
                         const uint64_t *seg_nwin, uint32_t nseg, unsigned long long *out, void *stream);
unsigned long long ts_k_general_lds_bytes(const TsGenericPatterns *G, uint32_t *lds_patterns);
int  ts_k_launch_general_fused(const unsigned char *in, const TsGeneralTile *tiles, uint32_t ntiles,
                               const unsigned long long *seg_len, const unsigned long long *seg_win_base, const unsigned long long *seg_nwin,
                               const TsGenericPatterns *G, const TsGenericGeom *Q, int tips, uint32_t slot_cap,
                               uint32_t *tile_stats, uint32_t *records, uint32_t *win_out, uint32_t *overflow, int list, int num_cu, void *stream);
uint32_t ts_k_general_list_max_records(void);
// the wide form of the same pass: any set a ts_pattern[] can express; records are (tile position << 8) | (length index << 2) |
// canonical << 1 | forward; tiles' avail is clamped to n + TS_WIDE_HALO; *overflow bit 0 as above
int  ts_k_launch_general_wide(const unsigned char *in, const TsGeneralTile *tiles, uint32_t ntiles,
                              const unsigned long long *seg_len, const unsigned long long *seg_win_base, const unsigned long long *seg_nwin,
                              const TsWidePatterns *W, const TsGenericGeom *Q, int tips, uint32_t slot_cap,
                              uint32_t *tile_stats, uint32_t *records, uint32_t *win_out, uint32_t *overflow, void *stream);
                               // (records: ntiles x slot_cap entries; win_out zeroed by the caller; *overflow raised when a tile
                               //  holds more than slot_cap records — its count is still written; list != 0: the list form of
                               //  the pass — for parameter sets whose tiles add to at most ts_k_general_list_max_records()
                               //  window records and whose pattern lists fit LDS; *overflow bit 1: run again with list = 0)
// after the compaction: what device block calling needs of the group (TsTile per tile with in_off = seg_base[seg] + the tile's
// segment-relative position; canonical / forward counts into words 1, 2 of the tile directory)
int  ts_k_launch_general_block_inputs(const TsGeneralTile *gtiles, const unsigned long long *tile_off, const uint32_t *dense,
                                      const unsigned long long *seg_base, uint32_t ntiles, TsTile *tiles, uint32_t *tile_stats,
                                      int count_from_offsets, void *stream);
int  ts_k_launch_general_slot_offsets(unsigned long long *tile_off, uint32_t ntiles, uint32_t slot_cap, void *stream);
int  ts_k_launch_general_compact_push(const TsGeneralTile *gtiles, const uint32_t *tile_stats, unsigned long long *tile_off,
                                      const uint32_t *records, uint32_t slot_cap, uint32_t ntiles, const unsigned long long *seg_len,
                                      uint32_t w, uint32_t s, uint32_t spread, int wide, unsigned long long gen_lens,
                                      const uint32_t *wide_len, uint32_t *dense, void *stream);
int  ts_k_launch_general_compact(const uint32_t *tile_stats, const unsigned long long *tile_off, const uint32_t *records,
                                 uint32_t slot_cap, uint32_t ntiles, uint32_t *dense, void *stream);
int  ts_k_launch_predicate(const TsTile *tiles, const unsigned long long *tile_off, const uint32_t *tile_stats,
                           const uint32_t *matches, unsigned long long nrec_limit, const uint32_t *seg_first_tile,
                           const unsigned long long *seg_in_off, const unsigned long long *seg_len,
                           uint32_t nseg, const TsPredParams *Q, unsigned char *pass, uint32_t *long_list,
                           uint32_t *long_count, int all_terminal, const uint32_t *wave_fill, uint32_t region_cap,
                           uint32_t nwaves, uint32_t *overflow, int rec16, void *stream);
                           // (nrec_limit: records that may be READ behind `matches` — the predicate fetches aligned 16-byte blocks;
                           //  long_list: nseg entries of scratch + long_count: one counter, for the reads a whole wave walks;
                           //  all_terminal: no segment is longer than the terminal limit — every read batch — the lean kernel;
                           //  wave_fill / region_cap / nwaves -> *overflow: raised, and nothing judged, when the scan overflowed a wave's region)
int  ts_k_launch_terminal_ends(const TsTile *tiles, const unsigned long long *tile_off, const uint32_t *tile_stats,
                               const uint32_t *matches, unsigned long long nrec_limit, const uint32_t *seg_first_tile,
                               const unsigned long long *seg_in_off, const unsigned long long *seg_len, uint32_t nseg,
                               const TsPredParams *Q, uint32_t *ends, uint32_t *long_list, uint32_t *long_count, int all_terminal,
                               const uint32_t *wave_fill, uint32_t region_cap, uint32_t nwaves, uint32_t *overflow, int rec16,
                               void *stream);
                           // the predicate's walks reduced to the longest terminal block per side: ends[2 i] start side, ends[2 i + 1]
                           // end side of segment i (predicate.hip, ENDS); arguments as above
// blockcall.hip: terminal walks per segment of `segs` (nseg entries; bounds: 2 x u64 per segment), then the interstitial
// search over the batch's ntiles (range-local) tiles; seg_base = plan index of segs[0]'s segment; seg_out (nullable):
// what a shard reports per segment
// vis (nullable): where the interstitial pass leaves the visible records of the owned tiles (a shard's message)
// sums (nullable): 5 x u64 per segment, the per-segment totals for a caller that wants them
// chain + work (both or neither): the scan's per-tile chain summaries (TsTileChain) and scratch of (ntiles + 1) dwords — the
// interstitial search then screens the tiles by their summaries and walks only the listed ones (ignored when vis asks for
// the visible records out of the match stream)
int  ts_k_launch_block_call(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, uint32_t seg_base,
                            uint32_t ntiles, unsigned long long *bounds, TsShardSeg *seg_out, int with_its,
                            const TsVisibleOut *vis, unsigned long long *sums, const uint32_t *chain, uint32_t *work, void *stream);
// the terminal walks alone (they answer scanSegment's ">= 2 matches" gates from the tile directory themselves)
int  ts_k_launch_terminal(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, uint32_t seg_base, uint32_t ntiles,
                          unsigned long long *bounds, TsShardSeg *seg_out, void *stream);
// the read predicate over the general kernels' records where the fused pass left them (a general tips batch): Q->matches = the
// slots (ntiles x slot_cap records), Q->tile_off[t] = t * slot_cap, tile_stats = the pass's directory (counts cut to the slot,
// canonical / forward counts added); pass[i] = 1 where segment i has a terminal block, else 0
int  ts_k_launch_read_pass_general(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, uint32_t ntiles, uint32_t slot_cap,
                                   uint32_t *tile_stats, unsigned char *pass, void *stream);
// the same walks in their ENDS form (ts_terminal_ends_walk): ends[2 i] / ends[2 i + 1] = the longest terminal block at the start /
// end side of segment i (zeroed here).  tile_stats == nullptr: the directory's canonical / forward counts are already there
int  ts_k_launch_terminal_ends_general(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, uint32_t ntiles, uint32_t slot_cap,
                                       uint32_t *tile_stats, uint32_t *ends, void *stream);
// The same walks in their counting and placing forms (ts_batch_call_read_blocks): the terminal blocks of every segment as rows in
// device memory, ordered by (segment, walk, push order).  tab: 2 nseg x 16 bytes of counts (word 0 of entry 2 i + w: the blocks
// walk w of segment i closes), places: 2 nseg + 1 x u64 (their exclusive sums, the total behind them), first: nseg + 1 x u64 (the
// index of every segment's first row, the total behind them), tmp: ts_k_scan_tmp_bytes(2 nseg) bytes.  rows: room for row_cap rows;
// a row beyond it is not written (first[nseg] > row_cap says so: ts_k_launch_read_blocks_place places again into a larger
// buffer from the same places).  wave_fill != nullptr (a tiled batch): *overflow is raised when a wave's region overflowed in the
// scan, and then no walk runs and there are no rows; slot_cap != 0 (a general tips batch): the directory's counts are completed
// first, as for the read pass.
int  ts_k_launch_read_blocks(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, uint32_t ntiles, uint32_t slot_cap,
                             uint32_t *tile_stats, const uint32_t *wave_fill, uint32_t region_cap, uint32_t nwaves, uint32_t *overflow,
                             uint32_t *counts, unsigned long long *places, unsigned long long *first, void *tmp, TsReadBlockRow *rows,
                             unsigned long long row_cap, void *stream);
int  ts_k_launch_read_blocks_place(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, const uint32_t *overflow,
                                   const unsigned long long *places, TsReadBlockRow *rows, unsigned long long row_cap, void *stream);
// the directory's counts alone (ts_slot_counts), for block calling over a general tips batch's slots
int  ts_k_launch_slot_counts(const uint32_t *records, uint32_t slot_cap, uint32_t ntiles, uint32_t *tile_stats, void *stream);
// per-segment totals into sums (5 x u64 per segment) or into the segments' entries of a shard's message (seg_out)
int  ts_k_launch_segment_sums(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, uint32_t seg_base, uint32_t ntiles,
                              unsigned long long *sums, TsShardSeg *seg_out, int prezeroed, void *stream);
int  ts_k_launch_zero(void *p0, unsigned long long n0, void *p1, unsigned long long n1, void *p2, unsigned long long n2,
                      void *p3, unsigned long long n3, void *stream);
int  ts_k_launch_interstitial(const TsBlockCallParams *Q, const TsShardSegIn *segs, uint32_t nseg, uint32_t seg_base, uint32_t ntiles,
                              const unsigned long long *bounds, TsShardSeg *seg_out, const TsVisibleOut *vis,
                              const uint32_t *chain, uint32_t *work, int prezeroed, void *stream);
// shard.hip: packed window records, visible records + per-tile counts, and the header of a shard's message
int  ts_k_launch_shard_count(const TsShardPackParams *P, const TsShardHeader *H, void *tmp, int with_visible, TsVisibleOut *vis, void *stream);
// the same from the scan's own visible records (P->chain != nullptr): per-tile counts out of tile_stats, prefix sum, then the
// records copied into the message in tile order — nothing is left for the interstitial pass to write
int  ts_k_launch_shard_visible(const TsShardPackParams *P, const TsShardHeader *H, void *tmp, int prezeroed, void *stream);
void *ts_k_shard_big_counter(void *tmp, uint32_t own_tiles);      // the 4 bytes ts_k_launch_shard_visible wants zero
int  ts_k_launch_shard_windows(const TsShardPackParams *P, const TsShardHeader *H, void *stream);
// 1 in *concurrent when a kernel on stream b runs while one on stream a is still running (the streams sit on different hardware
// queues); both streams are synchronised first; ~1 ms.
int  ts_k_streams_concurrent(void *a, void *b, int *concurrent);
int  ts_k_launch_shard_overflow(const TsShardPackParams *P, void *stream);     // after the header's memset, before ts_k_launch_shard_pack
int  ts_k_launch_shard_pack(const TsShardPackParams *P, const TsShardHeader *H, void *tmp, int with_visible, void *stream);
unsigned long long ts_k_shard_tmp_bytes(uint32_t own_tiles);
// exchange.hip: tile directory of a dense tile-ordered stream, and the export of a scan's records into one
unsigned long long ts_k_scan_tmp_bytes(uint32_t ntiles);
int  ts_k_launch_tile_offsets(const uint32_t *tile_stats, uint32_t ntiles, unsigned long long *tile_off, void *tmp,
                              void *stream);
int  ts_k_launch_tile_order_export(const uint32_t *tile_stats, const unsigned long long *region_off,
                                   const uint32_t *regions, const uint32_t *wave_fill, uint32_t region_cap,
                                   uint32_t nwaves, uint32_t ntiles, unsigned long long *dense_off, void *tmp,
                                   uint32_t *dense, unsigned long long capacity, unsigned long long *total_out,
                                   int rec16, void *stream);
// unpack.hip: a staged chunk of 2-bit codes (pack.cpp) -> the byte layout: chunk positions [first, first + n) to dst, then
// 'N' over the chunk's invalid runs ({start, len} pairs, device memory; run position x lies at runs_base + x).
// packed: 4-byte aligned, 8 readable bytes behind the last code.
int  ts_k_launch_unpack(const void *packed, uint32_t first, void *dst, unsigned long long n, const void *runs, uint32_t nruns,
                        void *runs_base, void *stream);
// gather.hip: device-resident pieces into the input layout, a wave per job (jobs: tsgather::Job of gather_core.h, device memory;
// a job's bytes go to base + its dst)
int  ts_k_launch_gather_pieces(const void *jobs, uint32_t n_jobs, void *base, void *stream);
// tracks.hip: the five window tracks as text (track_format_core.h: tstrack::Segment, tstrack::Patch).  A workgroup formats
// TS_TRACK_BLOCK windows; block_sums holds 5 x (n_blocks + 1) values — per track the workgroups' bytes, after
// ts_k_launch_track_count their exclusive prefix sums with the track's total behind them; *bad_window (preset to ~0) the
// lowest window with a value the formatter cannot print.  ts_k_launch_track_write needs out[t] of block_sums[t][n_blocks]
// bytes for every track of on_mask; it writes nothing when *bad_window is set.
#define TS_TRACK_BLOCK 256u
#define TS_TRACK_MAX_NAME (1u << 24)     // bytes of a segment name: 64 lines of a wave stay far below 2^32 bytes
struct TsTrackParams {
    const uint32_t *records;                // eight u32 per window, 16-byte aligned
    unsigned long long first, n;            // the call formats windows [first, n) of the records, workgroup b those from first + b * TS_TRACK_BLOCK
    const void *segs;                       // tstrack::Segment[n_segs]: the segments that have windows, first_window ascending
    const void *names;                      // the bytes the segments' name_off / name_len point into
    const float *term;                      // ts::entropy_terms(w), or null: every window's entropy is in the patch list
    const void *patches;                    // tstrack::Patch[n_patches], sorted by window
    unsigned long long n_patches;
    unsigned long long *block_sums;
    unsigned long long *bad_window;
    void *out[5];
    uint32_t n_segs, n_blocks, w, step, on_mask;
};
int  ts_k_launch_track_count(const TsTrackParams *P, void *stream);
int  ts_k_launch_track_write(const TsTrackParams *P, void *stream);
// out[j] = the record of window idx[j] (device memory, all three)
int  ts_k_launch_track_pick(const uint32_t *records, const unsigned long long *idx, unsigned long long n, uint32_t *out, void *stream);
// ts_track_scan_blocks by itself: n_columns columns of n_blocks + 1 values each — a column's n_blocks sums become their exclusive
// 64-bit prefix sums, its last entry their total
int  ts_k_launch_scan_columns(unsigned long long *sums, uint32_t n_columns, uint32_t n_blocks, void *stream);
// read_blocks.hip: the read block report as text (read_block_format_core.h).  A segment's entry says where its read's name lies in
// `names` (the chunk, or an uploaded buffer) and how many bases were judged; a workgroup of one wave formats 64 rows.  sums holds
// two columns of n_blocks + 1 values: after ts_k_launch_read_block_count the exclusive prefix sums of the workgroups' bytes and of
// their line counts, each column's total behind it.
struct TsReadBlockSeg { unsigned long long name_off; uint32_t name_len, read_len; };
struct TsReadBlockTextParams {
    const TsReadBlockRow *rows;
    const TsReadBlockSeg *segs;
    const void *names;
    unsigned long long *sums;
    void *out;
    unsigned long long n_rows;
    uint32_t n_segs;
};
#define TS_READ_BLOCK_FASTQ 0u
#define TS_READ_BLOCK_SAM   1u
#define TS_READ_BLOCK_BAM   2u
#define TS_READ_BLOCK_FASTA 3u
// segs[i] from entry i of a chunk's record table (ts_fastq_record / ts_sam_record / ts_bam_record by `kind`, device memory)
int  ts_k_launch_read_block_names(const void *recs, uint32_t n, uint32_t kind, const void *chunk, TsReadBlockSeg *segs, void *stream);
int  ts_k_launch_read_block_count(const TsReadBlockTextParams *P, uint32_t n_blocks, void *stream);
int  ts_k_launch_read_block_write(const TsReadBlockTextParams *P, uint32_t n_blocks, void *stream);
// match_text.hip: the two match files as text (match_format_core.h: tsmatch::Segment).  A workgroup of one wave formats one tile
// of the record stream's directory.  sums holds 4 x (n_tiles + 1) values — per tile the bytes of the canonical and of the
// non-canonical file and their line counts; after ts_k_launch_match_count their exclusive prefix sums with the totals behind
// them.  ts_k_launch_match_write(P, n) formats tiles [tile_first, tile_first + n): file f's lines of tile t start at
// out[f] + sums[f][t] - slice_base[f].
#define TS_MATCH_FORM_TILED16 0u        // the tiled kernel's regions, 16-bit records: tiles = TsTile[], {tile_off, tile_stats} the batch's directory
#define TS_MATCH_FORM_TILED32 1u        // ... 32-bit records
#define TS_MATCH_FORM_GENERAL 2u        // the general kernels' stream (shift 5, 3-bit length index into gen_lens): tiles = TsGeneralTile[]
#define TS_MATCH_FORM_WIDE    3u        // the wide form's (shift 8, 6-bit index into wide_len)
#define TS_MATCH_FORM_ARRAY   4u        // ts_match[]: tiles = TsMatchTile[], no directory
struct TsMatchTile { unsigned long long first; uint32_t count, seg; };   // records [first, first + count) belong to segment seg
struct TsMatchTextParams {
    const void *records;
    const void *tiles;
    const unsigned long long *tile_off;     // per tile: index of its first record
    const uint32_t *tile_stats;             // per tile four words, the first its record count
    const void *segs;                       // tsmatch::Segment[n_segs]; a tiled segment's base_off is its in_off of the input layout
    const void *names;
    const void *bases;                      // the input layout (or the caller's bases): base_off + segment-relative position
    const uint32_t *wide_len;
    unsigned long long gen_lens;
    unsigned long long *sums;
    void *out[2];
    unsigned long long slice_base[2];
    uint32_t form, n_tiles, tile_first, n_segs, k, terminal_limit;
};
int  ts_k_launch_match_count(const TsMatchTextParams *P, void *stream);
int  ts_k_launch_match_write(const TsMatchTextParams *P, uint32_t n, void *stream);
// exchange.hip: box calibration (see there)
int  ts_k_box_probe(void *scratch, unsigned long long bytes, int num_cu, double *issue_per_ns, double *copy_bytes_per_ns, void *stream);
int  ts_k_launch_widen_u16(const uint16_t *src, uint32_t *dst, unsigned long long n, void *stream);
int  ts_k_launch_compact(const uint32_t *regions, const uint32_t *wave_fill,
                         const unsigned long long *wave_dense_base, uint32_t region_cap,
                         uint32_t nwaves, uint32_t *dense, int rec16, void *stream);
// bgzf.hip: a wave per BGZF member (blocks: ts_bgzf_block descriptors in device memory, checked by the caller; compressed:
// 4-byte aligned with 4 readable bytes behind the last payload); result[i] = TS_BGZF_OK / _BAD_DEFLATE / _BAD_CRC
int  ts_k_launch_bgzf_inflate(const void *compressed, const void *blocks, uint32_t n_blocks, void *plain, uint32_t *result,
                              void *stream);
// ... the record walk over an inflated chunk (one wave; out4 = {records, next offset, error code, error offset}; plain is
// readable 16 bytes beyond plain_n), SEQ -> ASCII (jobs: {src, dst, n, pad} of 24 bytes, a wave each, dst 16-byte aligned,
// n <= 2048), and the copy of passing records to the places chunk.hip's gather plan gave them
int  ts_k_launch_bam_walk(const void *plain, unsigned long long plain_n, unsigned long long from, unsigned long long cap,
                          void *recs, void *out4, void *stream);
// ... the parallel record index (bam_walk_core.h): a wave per span [first_span, first_span + n_spans) writes its K candidate rows
// (tsbam::Row); one wave settles a span by the serial rule (out3 = {exit, records, stop}); a wave per task (tsbam::Task) walks
// its span from the verified entry and stores records below cap (out1[0] = the offset of record `cap` where a span holds it)
int  ts_k_launch_bam_index_candidates(const void *plain, unsigned long long plain_n, unsigned long long from, uint32_t span_log2,
                                      uint32_t K, unsigned long long first_span, uint32_t n_spans, void *rows, void *stream);
int  ts_k_launch_bam_index_settle(const void *plain, unsigned long long plain_n, unsigned long long entry, unsigned long long span_end,
                                  void *out3, void *stream);
int  ts_k_launch_bam_index_write(const void *plain, unsigned long long plain_n, const void *tasks, uint32_t n_tasks, uint32_t span_log2,
                                 unsigned long long cap, void *recs, void *out1, void *stream);
int  ts_k_launch_bam_decode(const void *plain, const void *jobs, uint32_t n_jobs, void *in, void *stream);
int  ts_k_launch_bam_gather(const void *plain, const void *recs, const void *dst_off, unsigned long long n, unsigned long long cap,
                            void *out, void *stream);
// deflate.hip: a wave per BGZF member written — plain[0, n) (device memory) cut into payloads of payload_bytes (1 .. 0xff00), member
// i framed in slots + i * stride (zeroed by the caller; stride >= payload_bytes + 33, a multiple of 4; header at byte 2), sizes[i]
// = its length (zeroed by the caller); then offs[i] = the exclusive sums of the sizes, total[0] their sum and total[1] the count of zero sizes (one wave) ...
int  ts_k_launch_bgzf_deflate(const void *plain, unsigned long long n, uint32_t payload_bytes, uint32_t n_members, void *slots,
                              uint32_t stride, uint32_t *sizes, unsigned long long *offs, unsigned long long *total, void *stream);
// ... and the members copied to packed + offs[i] (packed: 16-byte aligned, cap bytes; slots readable 64 bytes beyond the last)
int  ts_k_launch_deflate_pack(const void *slots, uint32_t stride, const uint32_t *sizes, const unsigned long long *offs,
                              uint32_t n_members, unsigned long long cap, void *packed, void *stream);
// gzip.hip: a window of one gzip member's deflate stream (window: 16-byte aligned, zero from window_len to the next dword).
// cand[n_spans] = each span's first candidate block start (span 0: start_bit); then a wave per span decodes 16-bit symbols to
// sym[s * cap ...] and writes table[s] (24 bytes: start_bit, end_bit, n_out, status, final_seen, reserved; status 0xff = no
// candidate); then, for the chain the host picked (chain[k]: 24 bytes {span, n_out, hist_avail, reserved, u64 plain_off};
// hist: (n_chain + 1) * 32 KiB, the first the history in front of the window), the histories, the plain bytes and
// *bad_span = min(k whose markers reach in front of hist_avail); then CRC32 per slice (16 bytes {u64 off, u32 len, u32 crc})
int  ts_k_launch_gzip_probe(const void *window, uint32_t window_len, uint32_t start_bit, uint32_t span_bytes, uint32_t n_spans,
                            uint32_t *cand, void *stream);
int  ts_k_launch_gzip_decode(const void *window, uint32_t window_len, uint32_t n_spans, const uint32_t *cand, uint32_t cap,
                             uint32_t hist0_len, void *sym, void *table, void *stream);
int  ts_k_launch_gzip_resolve(const void *sym, uint32_t cap, const void *chain, uint32_t n_chain, uint32_t max_out, void *hist,
                              void *plain, unsigned long long plain_n, uint32_t *bad_span, void *stream);
int  ts_k_launch_gzip_crc(const void *plain, unsigned long long plain_n, void *slices, uint32_t n_slices, void *stream);
}
#endif

#endif
