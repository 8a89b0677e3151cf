// bgzf.hip — BGZF members inflated and checksummed on the device: one wave per member (a BAM chunk of 256 MB is ~4 000
// independent members of <= 64 KB).  The decoder itself is inflate_core.h, the source a host test program compiles too; this
// file is its device policy — where the payload's bits come from and how a batch of decoded symbols becomes bytes — and the
// CRC32 behind it.
//
// Shape of a wave's work:
//   * payload bits: a 1 KB window of the payload in LDS, refilled by the wave with coalesced dword loads; the bit buffer and
//     the decoder's control flow are wave-uniform (the compiler keeps them on the scalar unit);
//   * Huffman tables (first-level lookup + canonical counts / sorted symbols) in LDS, the lookups filled a symbol per lane;
//   * symbols are decoded one after the other into a batch of 64 held a symbol per lane, then WRITTEN by all lanes: a prefix
//     sum of the symbols' lengths places them, and the batch's bytes go out 64 at a time, a byte per lane — a literal is its
//     lane's byte, a match byte reads out[p - dist + (j mod dist)]; sources inside the 64 bytes being written are resolved
//     between lanes by pointer jumping (<= 6 rounds), sources before them are read back from global memory (the wave waits for
//     its own earlier stores only when a source lies behind the last wait);
//   * output goes straight to global memory: no 32 KB window in LDS, so the LDS footprint (tables + window, ~6 KB) and not the
//     window decides how many members a CU decodes at once;
//   * CRC32 of the member's bytes: lanes take consecutive 16-byte-aligned slices (table in LDS), partial CRCs are joined by
//     x^(8n) mod P in a log-step reduction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teloscan.h"
#include "bam_walk_core.h"
#include "chunk_device.h"
#include "inflate_core.h"
#include "ts_device.h"
#include "ts_internal.h"

namespace {

constexpr uint32_t kWindowWords = 256;      // payload dwords per window (+ 1: a payload dword straddles two aligned ones)

struct DevicePolicy {
    const uint32_t *gw;             // the aligned dword that holds the payload's first byte
    uint32_t shift;                 // bits between that dword's start and the payload's
    uint32_t gwords;                // aligned dwords that hold payload bytes
    const unsigned char *payload;
    unsigned char *out;
    uint32_t *win;                  // LDS: kWindowWords + 1 aligned dwords from wbase on
    uint32_t *mark;                 // LDS: 64 words
    uint32_t wbase;
    uint32_t entry;                 // this lane's symbol of the batch
    uint32_t waited;                // out[0, waited) is known to have reached memory

    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ uint32_t nlanes() const { return 64u; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

    __device__ __forceinline__ uint32_t word(uint32_t i) {
        if (i - wbase >= kWindowWords) {                        // (wave-uniform)
            __syncthreads();
            wbase = i;
            for (uint32_t k = threadIdx.x; k <= kWindowWords; k += 64u) {
                const uint32_t g = i + k;
                win[k] = g < gwords ? gw[g] : 0u;
            }
            __syncthreads();
        }
        const uint32_t a = win[i - wbase], b = win[i - wbase + 1u];
        return uni(shift ? (a >> shift) | (b << (32u - shift)) : a);
    }

    __device__ __forceinline__ void put(uint32_t k, uint32_t e) { if (threadIdx.x == k) entry = e; }

    __device__ __forceinline__ void wait_stores(uint32_t upto) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        waited = upto;
    }

    __device__ __forceinline__ void copy_stored(uint32_t from, uint32_t n, uint32_t pos) {
        for (uint32_t j = threadIdx.x; j < n; j += 64u) out[pos + j] = payload[from + j];
    }

    __device__ void flush(uint32_t n, uint32_t pos) {
        const uint32_t lane = threadIdx.x;
        const bool have = lane < n;
        const uint32_t e = have ? entry : 0u;
        const uint32_t len = !have ? 0u : (e & tsinf::kLiteral) ? 1u : (e & 511u);
        const uint32_t incl = wave_scan_add(len);
        const uint32_t start = incl - len;
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        uint32_t carry = 1u;                                    // 1 + the symbol that owns the byte before the 64 at hand
        for (uint32_t c0 = 0; c0 < total; c0 += 64u) {
            // which symbol owns byte c0 + lane: the symbols that start in these 64 bytes mark their first byte, a prefix
            // maximum spreads the marks
            __syncthreads();
            mark[lane] = 0u;
            __syncthreads();
            if (have && start - c0 < 64u) mark[start - c0] = lane + 1u;
            __syncthreads();
            uint32_t own = wave_scan_max(mark[lane]);
            if (own == 0u) own = carry;
            carry = (uint32_t)__builtin_amdgcn_readlane((int)own, 63);
            own -= 1u;
            const uint32_t oe = (uint32_t)__shfl((int)e, (int)own), ostart = (uint32_t)__shfl((int)start, (int)own);
            const uint32_t b = c0 + lane;
            const bool valid = b < total;
            const bool olit = (oe & tsinf::kLiteral) != 0u;
            const uint32_t odist = olit ? 1u : (oe >> 9) ? (oe >> 9) : 1u;
            const uint32_t j = b - ostart;
            bool resolved = olit || !valid;
            uint32_t val = oe & 255u;
            uint32_t src = pos + ostart - odist + (j < odist ? j : j % odist);     // (meaningful where !resolved)
            const uint32_t base = pos + c0;
            for (int round = 0; round < 64; ++round) {          // (a source chain inside 64 bytes halves per round: <= 6 rounds)
                const bool need = !resolved && src >= base;
                if (ballot64(need) == 0ull) break;
                const int from = need ? (int)(src - base) : (int)lane;
                const uint32_t tv = (uint32_t)__shfl((int)val, from), ts = (uint32_t)__shfl((int)src, from);
                const bool tr = __shfl((int)resolved, from) != 0;
                if (need) { if (tr) { val = tv; resolved = true; } else src = ts; }
            }
            const bool fetch = valid && !resolved;
            if (ballot64(fetch && src >= waited) != 0ull) wait_stores(base);
            if (fetch) val = out[src];
            if (valid) out[pos + b] = (unsigned char)val;
        }
    }
};

// CRC32 of p[0, n) by the wave: lane l takes the bytes of the l-th aligned slice
__device__ uint32_t wave_crc32(const unsigned char *p, uint32_t n, const uint32_t *table) {
    const uintptr_t a = (uintptr_t)p, lo = a, hi = a + n, s0 = a & ~(uintptr_t)15;
    const uint32_t slice = (((uint32_t)(hi - s0) + 63u) / 64u + 15u) & ~15u;       // bytes per lane, a multiple of 16
    uintptr_t from = s0 + (uintptr_t)threadIdx.x * slice, to = from + slice;
    if (from < lo) from = lo;
    if (to > hi) to = hi;
    uint32_t c = 0xffffffffu, mine = 0;
    if (from < to) {
        mine = (uint32_t)(to - from);
        uintptr_t at = from;
        for (; at < to && (at & 15u); ++at) c = table[(c ^ *(const unsigned char *)at) & 255u] ^ (c >> 8);
        for (; at + 16u <= to; at += 16u) {
            const uint4 q = *(const uint4 *)at;
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c ^= w[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) c = table[c & 255u] ^ (c >> 8);
            }
        }
        for (; at < to; ++at) c = table[(c ^ *(const unsigned char *)at) & 255u] ^ (c >> 8);
    }
    uint32_t crc = c ^ 0xffffffffu;                             // (an empty slice: 0, the CRC of nothing)
    uint32_t len = mine;
    for (int s = 1; s < 64; s *= 2) {
        const uint32_t pc = (uint32_t)__shfl_down((int)crc, s), pl = (uint32_t)__shfl_down((int)len, s);
        if (threadIdx.x + (uint32_t)s < 64u) { crc = tsinf::crc_combine(crc, pc, pl); len += pl; }
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)crc);
}

__global__ __launch_bounds__(64)
void ts_bgzf_inflate_kernel(const unsigned char *compressed, const ts_bgzf_block *blocks, uint32_t n_blocks,
                            unsigned char *plain, uint32_t *result) {
    __shared__ tsinf::Tables tables;
    __shared__ uint32_t win[kWindowWords + 4];
    __shared__ uint32_t mark[64];
    __shared__ uint32_t crc_table[256];
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const ts_bgzf_block blk = blocks[b];
    const unsigned char *payload = compressed + blk.src_off;
    unsigned char *out = plain + blk.dst_off;
    const uintptr_t pa = (uintptr_t)payload;
    DevicePolicy pol;
    pol.gw = (const uint32_t *)(pa & ~(uintptr_t)3);
    pol.shift = 8u * (uint32_t)(pa & 3u);
    pol.gwords = ((uint32_t)(pa & 3u) + blk.payload_len + 3u) / 4u;
    pol.payload = payload;
    pol.out = out;
    pol.win = win;
    pol.mark = mark;
    pol.wbase = 0x80000000u;
    pol.entry = 0u;
    pol.waited = 0u;
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u) crc_table[i] = tsinf::crc_table_entry(i);
    __syncthreads();
    int verdict = tsinf::inflate(pol, &tables, blk.payload_len, blk.isize);
    verdict = __builtin_amdgcn_readfirstlane(verdict);
    if (verdict == tsinf::kOk) {
        pol.wait_stores(blk.isize);
        if (wave_crc32(out, blk.isize, crc_table) != blk.crc) verdict = tsinf::kBadCrc;
    }
    if (threadIdx.x == 0) result[b] = (uint32_t)verdict;
}

// ---- the record walk over an inflated chunk: a dependent chain, one wave.  The bytes it looks at are staged in LDS — 16 KB
// at a time where records are short (a short-read BAM pays an LDS latency per record, not a memory one), 1 KB where the
// record before was long and the walk simply jumped.  Validation is the host route's, in its order (bamSubset in
// include/teloscope_mi355x_io.hpp); out = {records, next offset, error code, error offset}.
constexpr uint32_t kWalkWindow = 16384, kWalkHeader = 4 + 32 + 256;

__global__ __launch_bounds__(64)
void ts_bam_walk_kernel(const unsigned char *plain, unsigned long long plain_n, unsigned long long from, unsigned long long cap,
                        ts_bam_record *recs, unsigned long long *out) {
    __shared__ uint4 win4[kWalkWindow / 16];
    const unsigned char *win = (const unsigned char *)win4;
    unsigned long long wlo = 0, whi = 0, pos = from, n = 0;
    uint32_t err = 0, last_size = 0;
    auto byte_at = [&](unsigned long long p) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)win[p - wlo]); };
    auto le32 = [&](unsigned long long p) -> uint32_t {
        return byte_at(p) | byte_at(p + 1) << 8 | byte_at(p + 2) << 16 | byte_at(p + 3) << 24;
    };
    while (n < cap && plain_n - pos >= 4ull) {
        const unsigned long long want = plain_n - pos < kWalkHeader ? plain_n : pos + kWalkHeader;
        if (pos < wlo || want > whi) {                          // (wave-uniform)
            const uint32_t bytes = last_size > kWalkWindow / 2 ? 1024u : kWalkWindow;
            __syncthreads();
            wlo = pos & ~15ull;
            whi = wlo + bytes;
            for (uint32_t k = threadIdx.x; k < bytes / 16u; k += 64u) {
                const unsigned long long a = wlo + 16ull * k;   // (the chunk's buffer is readable 16 bytes beyond plain_n)
                win4[k] = a < plain_n ? *(const uint4 *)(plain + a) : make_uint4(0u, 0u, 0u, 0u);
            }
            __syncthreads();
        }
        const uint32_t bs = le32(pos);
        if ((int32_t)bs < 32 || bs > (256u << 20)) { err = 1; break; }
        if (plain_n - pos < 4ull + bs) break;
        const unsigned long long core = pos + 4ull;
        const uint32_t lname = byte_at(core + 8), ncigar = byte_at(core + 12) | byte_at(core + 13) << 8, lseq = le32(core + 16);
        const unsigned long long seq_at = 32ull + lname + 4ull * ncigar;
        if (lname == 0u || lseq > 0x7fffffffu) { err = 2; break; }
        if (seq_at + ((unsigned long long)lseq + 1ull) / 2ull + lseq > (unsigned long long)bs) { err = 3; break; }
        if (byte_at(core + 32ull + lname - 1ull) != 0u) { err = 4; break; }
        if (threadIdx.x == 0) {
            ts_bam_record r;
            r.off = pos; r.block_size = bs; r.seq_at = 4u + (uint32_t)seq_at; r.l_seq = lseq; r.reserved = 0u;
            recs[n] = r;
        }
        ++n;
        last_size = bs;
        pos += 4ull + bs;
    }
    if (threadIdx.x == 0) { out[0] = n; out[1] = pos; out[2] = err; out[3] = err ? pos : 0ull; }
}

// ---- the parallel record index (ts_bam_chunk_index; the scheme and its rule: bam_walk_core.h).  The chunk is cut into spans;
// a wave per span finds the span's candidates, the host chains them from `from` (bgzf.cpp; a span it cannot chain is settled
// by ts_bam_index_settle_kernel), and a wave per entered span walks it again from its verified entry and stores the table.
// Three ways to the bytes: per-lane reads of an LDS window (the candidate test's first record: 64 offsets side by side),
// per-lane reads of memory (the rest of a candidate's walk: each lane is somewhere else), and the serial walk's wave-uniform
// LDS window (settle and write).  Every read is bounded by plain_n inside tsbam::record_at; the staging loads are whole aligned
// 16-byte words that begin below plain_n (the chunk's buffer is readable 16 bytes beyond it).
constexpr uint32_t kCandWindow = 4096, kCandStage = kCandWindow + 304;      // offsets per staged window; its bytes (+ a header region)

struct LdsBytes {                                               // [wlo, ...) staged in LDS, read per lane
    const unsigned char *win;
    unsigned long long wlo;
    __device__ __forceinline__ uint32_t byte(unsigned long long p) const { return win[p - wlo]; }
    __device__ __forceinline__ uint32_t le32(unsigned long long p) const { return byte(p) | byte(p + 1) << 8 | byte(p + 2) << 16 | byte(p + 3) << 24; }
    __device__ __forceinline__ void stage(unsigned long long, unsigned long long) const {}
};

struct GlobalBytes {                                            // the chunk in memory, read per lane
    const unsigned char *plain;
    __device__ __forceinline__ uint32_t byte(unsigned long long p) const { return plain[p]; }
    __device__ __forceinline__ uint32_t le32(unsigned long long p) const { uint32_t v; __builtin_memcpy(&v, plain + p, 4); return v; }
    __device__ __forceinline__ void stage(unsigned long long, unsigned long long) const {}
};

// The serial walk's staging for a wave that walks one span: 16 KB windows, 1 KB behind a jump of more than 8 KB, and never
// beyond the header region of the span's last possible record.  All lanes run the walk; every value read is wave-uniform.
struct WaveWindow {
    uint4 *win4;
    const unsigned char *plain;
    unsigned long long span_end, wlo, whi, prev;
    __device__ __forceinline__ uint32_t byte(unsigned long long p) const {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)((const unsigned char *)win4)[p - wlo]);
    }
    __device__ __forceinline__ uint32_t le32(unsigned long long p) const { return byte(p) | byte(p + 1) << 8 | byte(p + 2) << 16 | byte(p + 3) << 24; }
    __device__ __forceinline__ void stage(unsigned long long pos, unsigned long long n) {
        const unsigned long long want = n - pos < tsbam::kHeader ? n : pos + tsbam::kHeader;
        if (pos < wlo || want > whi) {                          // (wave-uniform)
            uint32_t bytes = whi != 0ull && pos - prev > kWalkWindow / 2 ? 1024u : kWalkWindow;
            __syncthreads();
            wlo = pos & ~15ull;
            const unsigned long long need = (span_end + tsbam::kHeader - wlo + 15ull) & ~15ull;     // (pos < span_end)
            if (need < bytes) bytes = (uint32_t)need;
            whi = wlo + bytes;
            for (uint32_t k = threadIdx.x; k < bytes / 16u; k += 64u) {
                const unsigned long long a = wlo + 16ull * k;
                win4[k] = a < n ? *(const uint4 *)(plain + a) : make_uint4(0u, 0u, 0u, 0u);
            }
            __syncthreads();
        }
        prev = pos;
    }
};

__global__ __launch_bounds__(64)
void ts_bam_index_candidates_kernel(const unsigned char *plain, unsigned long long plain_n, unsigned long long from, uint32_t span_log2,
                                    uint32_t K, unsigned long long first_span, tsbam::Row *rows) {
    __shared__ uint4 win4[kCandStage / 16];
    const unsigned long long k = first_span + blockIdx.x, span_lo = k << span_log2, span_end = span_lo + (1ull << span_log2);
    tsbam::Row *mine = rows + (unsigned long long)blockIdx.x * K;
    uint64_t lo, hi;
    tsbam::scan_range(plain_n, from, span_log2, k, lo, hi);
    uint32_t found = 0;
    GlobalBytes g{plain};
    for (unsigned long long w = lo & ~15ull; w < hi && found < K; w += kCandWindow) {
        const unsigned long long wend = w + kCandWindow < hi ? w + kCandWindow : hi;
        const uint32_t bytes = (uint32_t)((wend - w + tsbam::kHeader + 15ull) & ~15ull);            // <= kCandStage
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < bytes / 16u; i += 64u) {
            const unsigned long long a = w + 16ull * i;
            win4[i] = a < plain_n ? *(const uint4 *)(plain + a) : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        LdsBytes l{(const unsigned char *)win4, w};
        for (unsigned long long b = w; b < wend && found < K; b += 64ull) {     // 64 offsets, ascending with the lane
            const unsigned long long p = b + threadIdx.x;
            tsbam::Row row;
            bool ok = false;
            if (p >= lo && p < wend) ok = tsbam::candidate(l, g, plain_n, p, span_lo, span_end, row);
            const unsigned long long mask = ballot64(ok);
            const uint32_t slot = found + (uint32_t)__popcll(mask & ((1ull << threadIdx.x) - 1ull));
            if (ok && slot < K) mine[slot] = row;
            found += (uint32_t)__popcll(mask);
        }
    }
    if (threadIdx.x >= found && threadIdx.x < K) {
        tsbam::Row none;
        none.entry = tsbam::kNoRow; none.exit = 0u; none.records = 0u; none.stop = 0u;
        mine[threadIdx.x] = none;
    }
}

__global__ __launch_bounds__(64)
void ts_bam_index_settle_kernel(const unsigned char *plain, unsigned long long plain_n, unsigned long long entry,
                                unsigned long long span_end, unsigned long long *out) {
    __shared__ uint4 win4[kWalkWindow / 16];
    WaveWindow a{win4, plain, span_end, 0ull, 0ull, 0ull};
    const tsbam::SpanResult s = tsbam::span_walk(a, plain_n, entry, span_end, ~0ull, tsbam::NoEmit());
    if (threadIdx.x == 0) { out[0] = s.exit; out[1] = s.records; out[2] = s.stop; }
}

__global__ __launch_bounds__(64)
void ts_bam_index_write_kernel(const unsigned char *plain, unsigned long long plain_n, const tsbam::Task *tasks, uint32_t n_tasks,
                               uint32_t span_log2, unsigned long long cap, ts_bam_record *recs, unsigned long long *out) {
    __shared__ uint4 win4[kWalkWindow / 16];
    if (blockIdx.x >= n_tasks) return;
    const unsigned long long entry = tasks[blockIdx.x].entry, base = tasks[blockIdx.x].base;
    if (base >= cap) return;
    const unsigned long long span_end = ((entry >> span_log2) + 1ull) << span_log2;
    WaveWindow a{win4, plain, span_end, 0ull, 0ull, 0ull};
    const tsbam::SpanResult s = tsbam::span_walk(a, plain_n, entry, span_end, cap - base,
                                                 [&](unsigned long long i, unsigned long long pos, const tsbam::Record &r) {
        if (threadIdx.x == 0) {
            ts_bam_record o;
            o.off = pos; o.block_size = r.block_size; o.seq_at = r.seq_at; o.l_seq = r.l_seq; o.reserved = 0u;
            recs[base + i] = o;
        }
    });
    if (s.stop == tsbam::kTableFull && threadIdx.x == 0) out[0] = s.exit;      // the offset of record `cap`
}

// ---- SEQ nibbles -> ASCII bases into a read batch's input buffer: a wave per <= 2 KB of a read, 16 output bytes per lane per
// store.  The 16 letters sit in four registers; v_perm_b32 picks from eight bytes at a time.
struct DecodeJob { unsigned long long src, dst; uint32_t n, pad; };         // packed bytes at plain + src -> n bases at in + dst

__device__ __forceinline__ uint32_t nibbles_to_letters(uint32_t x) {         // four codes 0..15, one per byte
    const uint32_t t0 = 0x4d43413du, t1 = 0x56535247u, t2 = 0x48595754u, t3 = 0x4e42444bu;      // "=ACM" "GRSV" "TWYH" "KDBN"
    const uint32_t sel = x & 0x07070707u;
    const uint32_t a = __builtin_amdgcn_perm(t1, t0, sel), b = __builtin_amdgcn_perm(t3, t2, sel);
    const uint32_t m = ((x >> 3) & 0x01010101u) * 0xffu;
    return (a & ~m) | (b & m);
}

__global__ __launch_bounds__(64)
void ts_bam_decode_seq_kernel(const unsigned char *plain, const DecodeJob *jobs, uint32_t n_jobs, unsigned char *in) {
    if (blockIdx.x >= n_jobs) return;
    const DecodeJob job = jobs[blockIdx.x];
    const unsigned char *src = plain + job.src;
    unsigned char *dst = in + job.dst;                          // 16-byte aligned
    for (uint32_t i = threadIdx.x * 16u; i < job.n; i += 1024u) {
        const uint32_t bases = job.n - i < 16u ? job.n - i : 16u, bytes = (bases + 1u) / 2u;
        uint32_t w[2] = {0u, 0u};
        if (bytes == 8u) __builtin_memcpy(w, src + i / 2u, 8);
        else for (uint32_t k = 0; k < bytes; ++k) w[k >> 2] |= (uint32_t)src[i / 2u + k] << (8u * (k & 3u));
        uint32_t o[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t hi = (w[h] >> 4) & 0x0f0f0f0fu, lo = w[h] & 0x0f0f0f0fu;
            o[2 * h] = nibbles_to_letters(__builtin_amdgcn_perm(lo, hi, 0x05010400u));
            o[2 * h + 1] = nibbles_to_letters(__builtin_amdgcn_perm(lo, hi, 0x07030602u));
        }
        if (bases < 16u) zero_tail16(o, bases);                 // the bytes behind the read stay zero, as an upload leaves them
        *(uint4 *)(dst + i) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// ---- passing records, in input order, into one contiguous buffer, at the places chunk.hip's plan gave them: a wave per passing
// record copies it as the FASTQ gather does (chunk_device.h: copy_record16).  The copy reads up to 19 bytes beyond a record's
// last byte (load16_any's five aligned dwords) and stores none: they lie inside the 64 readable bytes every chunk's plain buffer
// has behind its capacity (chunk.cpp: ts_bam_chunk_create, ts_chunk_reserve), and `out` is written in [to, to + size) only.
__global__ __launch_bounds__(64)
void ts_bam_gather_kernel(const unsigned char *plain, const ts_bam_record *recs, const unsigned long long *dst_off,
                          unsigned long long n, unsigned long long cap, unsigned char *out) {
    const unsigned long long i = blockIdx.x;
    if (i >= n) return;
    const unsigned long long to = dst_off[i];
    if (to == ~0ull) return;
    const uint32_t size = 4u + recs[i].block_size;              // (block_size <= 256 MiB: the host checked the table)
    if (to > cap || size > cap - to) return;                    // (the caller has compared the total with cap already)
    copy_record16(out + to, plain + recs[i].off, size, to);
}

}  // namespace

int ts_k_launch_bam_walk(const void *plain, unsigned long long plain_n, unsigned long long from, unsigned long long cap,
                         void *recs, void *out4, void *stream) {
    hipLaunchKernelGGL(ts_bam_walk_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, plain_n, from,
                       cap, (ts_bam_record *)recs, (unsigned long long *)out4);
    return (int)hipGetLastError();
}

int ts_k_launch_bam_index_candidates(const void *plain, unsigned long long plain_n, unsigned long long from, uint32_t span_log2,
                                     uint32_t K, unsigned long long first_span, uint32_t n_spans, void *rows, void *stream) {
    if (n_spans == 0) return 0;
    hipLaunchKernelGGL(ts_bam_index_candidates_kernel, dim3(n_spans), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain,
                       plain_n, from, span_log2, K, first_span, (tsbam::Row *)rows);
    return (int)hipGetLastError();
}

int ts_k_launch_bam_index_settle(const void *plain, unsigned long long plain_n, unsigned long long entry, unsigned long long span_end,
                                 void *out3, void *stream) {
    hipLaunchKernelGGL(ts_bam_index_settle_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, plain_n,
                       entry, span_end, (unsigned long long *)out3);
    return (int)hipGetLastError();
}

int ts_k_launch_bam_index_write(const void *plain, unsigned long long plain_n, const void *tasks, uint32_t n_tasks, uint32_t span_log2,
                                unsigned long long cap, void *recs, void *out1, void *stream) {
    if (n_tasks == 0) return 0;
    hipLaunchKernelGGL(ts_bam_index_write_kernel, dim3(n_tasks), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, plain_n,
                       (const tsbam::Task *)tasks, n_tasks, span_log2, cap, (ts_bam_record *)recs, (unsigned long long *)out1);
    return (int)hipGetLastError();
}

int ts_k_launch_bam_decode(const void *plain, const void *jobs, uint32_t n_jobs, void *in, void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_bam_decode_seq_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain,
                       (const DecodeJob *)jobs, n_jobs, (unsigned char *)in);
    return (int)hipGetLastError();
}

int ts_k_launch_bam_gather(const void *plain, const void *recs, const void *dst_off, unsigned long long n, unsigned long long cap,
                           void *out, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(ts_bam_gather_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain,
                       (const ts_bam_record *)recs, (const unsigned long long *)dst_off, n, cap, (unsigned char *)out);
    return (int)hipGetLastError();
}

int ts_k_launch_bgzf_inflate(const void *compressed, const void *blocks, uint32_t n_blocks, void *plain, uint32_t *result,
                             void *stream) {
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(ts_bgzf_inflate_kernel, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream,
                       (const unsigned char *)compressed, (const ts_bgzf_block *)blocks, n_blocks, (unsigned char *)plain, result);
    return (int)hipGetLastError();
}
