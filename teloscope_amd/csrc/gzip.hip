// gzip.hip — one plain gzip member's deflate stream decoded by many waves (include/teloscan.h: ts_gzip_decode).  The search and
// the decoder are gzip_core.h, the source a host test program compiles too; this file is their device policy and the passes
// around them.  A window of compressed bytes is cut into spans of span_bytes:
//   probe    a wave per span: the span's first bit offset that passes the candidate test (64 offsets at a time through the
//            cheap filters, a lane each; the survivors one after the other through the serial part);
//   decode   a wave per span that has a candidate, built like the BGZF kernel (bgzf.hip): bit buffer and control flow on the
//            scalar unit, tables in LDS, batches of 64 symbols written by all lanes — here as 16-bit symbols, a byte or a
//            marker for a byte of the 32 KiB in front of the span; it decodes up to the next span's candidate and, where it
//            steps over that one, on to the one after;
//   tails    the chained spans' last 32 KiB resolved one span after the other (the only serial step);
//   resolve  every symbol of every chained span to its byte at its plain offset;
//   crc      CRC32 of slices of the plain bytes (the host joins them with crc_combine).
// Everything a kernel writes is bounded by what the host sized: a span's symbols by `cap`, the plain bytes by the chain's sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gzip_core.h"
#include "ts_device.h"
#include "ts_internal.h"

namespace {

constexpr uint32_t kWindowWords = 256;      // window dwords staged in LDS at a time

struct GzPolicy {
    const uint32_t *gw;             // the window (16-byte aligned, zero behind its last byte up to a dword boundary)
    uint32_t gwords;                // dwords that hold window bytes
    uint16_t *out;                  // the span's symbols
    uint32_t *win;                  // LDS: kWindowWords + 1 dwords from wbase on
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
            for (uint32_t k = threadIdx.x; k < kWindowWords; k += 64u) {
                const uint32_t g = i + k;
                win[k] = (g >= i && g < gwords) ? gw[g] : 0u;
            }
            __syncthreads();
        }
        return uni(win[i - wbase]);
    }

    __device__ __forceinline__ void put(uint32_t k, uint32_t e) { if (threadIdx.x == k) entry = e; }

    __device__ __forceinline__ void wait_stores(uint32_t upto) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        waited = upto;
    }

    __device__ __forceinline__ void copy_stored(uint32_t from, uint32_t n, uint32_t pos) {
        const unsigned char *bytes = (const unsigned char *)gw;
        for (uint32_t j = threadIdx.x; j < n; j += 64u) out[pos + j] = (uint16_t)bytes[from + j];
    }

    // bgzf.hip's flush with 16-bit symbols: a source in front of the span becomes a marker, a source inside it is copied as the
    // symbol it is
    __device__ void flush(uint32_t n, uint32_t pos) {
        const uint32_t lane = threadIdx.x;
        const bool have = lane < n;
        const uint32_t e = have ? entry : 0u;
        const uint32_t len = !have ? 0u : (e & tsinf::kLiteral) ? 1u : (e & 511u);
        const uint32_t incl = wave_scan_add(len);
        const uint32_t start = incl - len;
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        uint32_t carry = 1u;                                    // 1 + the symbol that owns the position before the 64 at hand
        for (uint32_t c0 = 0; c0 < total; c0 += 64u) {
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
            const int32_t from = (int32_t)(pos + ostart) - (int32_t)odist + (int32_t)(j < odist ? j : j % odist);
            if (!resolved && from < 0) { val = tsgz::kMarker | (uint32_t)(32768 + from); resolved = true; }
            uint32_t src = from < 0 ? 0u : (uint32_t)from;      // (meaningful where !resolved)
            const uint32_t base = pos + c0;
            for (int round = 0; round < 64; ++round) {          // (a source chain inside 64 positions halves per round)
                const bool need = !resolved && src >= base;
                if (ballot64(need) == 0ull) break;
                const int at = need ? (int)(src - base) : (int)lane;
                const uint32_t tv = (uint32_t)__shfl((int)val, at), ts = (uint32_t)__shfl((int)src, at);
                const bool tr = __shfl((int)resolved, at) != 0;
                if (need) { if (tr) { val = tv; resolved = true; } else src = ts; }
            }
            const bool fetch = valid && !resolved;
            if (ballot64(fetch && src >= waited) != 0ull) wait_stores(base);
            if (fetch) val = out[src];
            if (valid) out[pos + b] = (uint16_t)val;
        }
    }
};

// cand[s] = the first bit offset in span s (window bits [s * span_bits, (s + 1) * span_bits)) that passes the candidate test,
// or kNoCandidate; span 0's is the known start bit
__global__ __launch_bounds__(64)
void ts_gzip_probe_kernel(const uint32_t *window, uint32_t window_len, uint32_t start_bit, uint32_t span_bits, uint32_t n_spans,
                          uint32_t *cand) {
    __shared__ tsinf::Tables tables;
    __shared__ uint32_t win[kWindowWords + 4];
    __shared__ uint32_t mark[64];
    const uint32_t s = blockIdx.x;
    if (s >= n_spans) return;
    if (s == 0) { if (threadIdx.x == 0) cand[0] = start_bit; return; }
    GzPolicy pol;
    pol.gw = window; pol.gwords = (window_len + 3u) / 4u; pol.out = nullptr; pol.win = win; pol.mark = mark;
    pol.wbase = 0x80000000u; pol.entry = 0u; pol.waited = 0u;
    const uint32_t total_bits = 8u * window_len;
    const uint32_t from = s * span_bits, to = from + span_bits < total_bits ? from + span_bits : total_bits;
    uint32_t found = tsgz::kNoCandidate;
    for (uint32_t base = from; base < to && found == tsgz::kNoCandidate; base += 64u) {
        const uint32_t at = base + threadIdx.x;
        const uint32_t w = at / 32u, sh = at & 31u;
        uint32_t d[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) d[k] = w + k < pol.gwords ? window[w + k] : 0u;
        const uint64_t q0 = (uint64_t)d[0] | (uint64_t)d[1] << 32, q1 = (uint64_t)d[2] | (uint64_t)d[3] << 32;
        const uint64_t lo = sh ? (q0 >> sh) | (q1 << (64u - sh)) : q0;
        const uint32_t hi = (uint32_t)(q1 >> sh);
        unsigned long long pass = ballot64(at > start_bit && at < to && tsgz::probe_cheap(lo, hi));
        while (pass != 0ull) {                                  // (wave-uniform: the survivors, lowest offset first)
            const uint32_t b = (uint32_t)__builtin_ctzll(pass);
            pass &= pass - 1ull;
            if (tsgz::probe_codes(pol, &tables, window_len, base + b)) { found = base + b; break; }
        }
    }
    if (threadIdx.x == 0) cand[s] = found;
}

struct SpanEntry { uint32_t start_bit, end_bit, n_out, status, final_seen, reserved; };
constexpr uint32_t kSpanEmpty = 0xffu;      // status of a span without a candidate

// a wave per span: symbols to sym[s * cap ...], the span's fate to table[s]
__global__ __launch_bounds__(64)
void ts_gzip_decode_kernel(const uint32_t *window, uint32_t window_len, uint32_t n_spans, const uint32_t *cand, uint32_t cap,
                           uint32_t hist0_len, uint16_t *sym, SpanEntry *table) {
    __shared__ tsinf::Tables tables;
    __shared__ uint32_t win[kWindowWords + 4];
    __shared__ uint32_t mark[64];
    const uint32_t s = blockIdx.x;
    if (s >= n_spans) return;
    GzPolicy pol;
    pol.gw = window; pol.gwords = (window_len + 3u) / 4u; pol.out = sym + (size_t)s * cap; pol.win = win; pol.mark = mark;
    pol.wbase = 0x80000000u; pol.entry = 0u; pol.waited = 0u;
    const uint32_t c = pol.uni(cand[s]);
    SpanEntry e{c, c, 0u, kSpanEmpty, 0u, 0u};
    if (c != tsgz::kNoCandidate) {
        uint32_t next = s + 1u;
        tsgz::SpanResult r{c, 0u, 0u, tsgz::kSpanStop};
        for (;;) {                                              // (a round passes one span's candidate at least)
            uint32_t stop = 0xffffffffu;
            for (; next < n_spans; ++next) {
                const uint32_t cn = pol.uni(cand[next]);
                if (cn != tsgz::kNoCandidate && cn >= r.end_bit) { stop = cn; break; }
            }
            r = tsgz::inflate_span(pol, &tables, window_len, r.end_bit, stop, r.n_out, cap, s == 0u ? hist0_len : tsgz::kHistory);
            r.end_bit = pol.uni(r.end_bit); r.n_out = pol.uni(r.n_out); r.status = pol.uni(r.status); r.final_seen = pol.uni(r.final_seen);
            if (r.status != tsgz::kSpanStop || r.end_bit == stop || next >= n_spans) break;
            ++next;                                             // stepped over that candidate: on to the one after
        }
        e.end_bit = r.end_bit; e.n_out = r.n_out; e.status = r.status; e.final_seen = r.final_seen;
    }
    if (threadIdx.x == 0) table[s] = e;
}

struct ChainEntry { uint32_t span, n_out, hist_avail, reserved; unsigned long long plain_off; };

// hist[k + 1] = the last 32 KiB of hist[k] ++ bytes of chained span k, k = 0 .. n_chain - 1, one after the other
__global__ __launch_bounds__(1024)
void ts_gzip_tails_kernel(const uint16_t *sym, uint32_t cap, const ChainEntry *chain, uint32_t n_chain, unsigned char *hist) {
    for (uint32_t k = 0; k < n_chain; ++k) {
        const ChainEntry ce = chain[k];
        const unsigned char *hin = hist + (size_t)k * tsgz::kHistory;
        unsigned char *hout = hist + (size_t)(k + 1u) * tsgz::kHistory;
        const uint16_t *sk = sym + (size_t)ce.span * cap;
        const uint32_t n = ce.n_out < cap ? ce.n_out : cap;
        for (uint32_t j = threadIdx.x; j < tsgz::kHistory; j += 1024u) {
            // position j of the new history is position n - 32768 + j of the span's output
            hout[j] = j + n < tsgz::kHistory ? hin[j + n] : (unsigned char)tsgz::resolve(sk[j + n - tsgz::kHistory], hin);
        }
        __threadfence();
        __syncthreads();
    }
}

// plain[plain_off + q] = byte of symbol q of chained span blockIdx.y; a marker that reaches in front of the member's first byte
// (hist_avail < 32768) lowers *bad_span to the span's place in the chain
constexpr uint32_t kResolveTile = 4096;
__global__ __launch_bounds__(256)
void ts_gzip_resolve_kernel(const uint16_t *sym, uint32_t cap, const ChainEntry *chain, uint32_t n_chain, const unsigned char *hist,
                            unsigned char *plain, unsigned long long plain_n, uint32_t *bad_span) {
    const uint32_t k = blockIdx.y;
    if (k >= n_chain) return;
    const ChainEntry ce = chain[k];
    const uint32_t n = ce.n_out < cap ? ce.n_out : cap;
    const uint32_t q0 = blockIdx.x * kResolveTile;
    if (q0 >= n) return;
    const unsigned char *h = hist + (size_t)k * tsgz::kHistory;
    const uint16_t *sk = sym + (size_t)ce.span * cap;
    const uint32_t floor_i = tsgz::kHistory - (ce.hist_avail < tsgz::kHistory ? ce.hist_avail : tsgz::kHistory);
    bool bad = false;
    for (uint32_t q = q0 + threadIdx.x; q < q0 + kResolveTile && q < n; q += 256u) {
        const uint32_t v = sk[q];
        if ((v & tsgz::kMarker) && (v & 0x7fffu) < floor_i) bad = true;
        const unsigned long long at = ce.plain_off + q;
        if (at < plain_n) plain[at] = (unsigned char)tsgz::resolve(v, h);
    }
    if (bad) atomicMin(bad_span, k);
}

// CRC32 of plain[off, off + len) per slice (len <= 65536): lanes take consecutive pieces, joined by x^(8n) mod P
struct CrcSlice { unsigned long long off; uint32_t len, crc; };
__global__ __launch_bounds__(64)
void ts_gzip_crc_kernel(const unsigned char *plain, unsigned long long plain_n, CrcSlice *slices, uint32_t n_slices) {
    __shared__ uint32_t table[256];
    const uint32_t s = blockIdx.x;
    if (s >= n_slices) return;
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u) table[i] = tsinf::crc_table_entry(i);
    __syncthreads();
    const unsigned long long off = slices[s].off;
    uint32_t len = slices[s].len;
    if (len > 65536u || off > plain_n || len > plain_n - off) len = 0u;
    const uint32_t per = (len + 63u) / 64u;
    const uint32_t a = threadIdx.x * per < len ? threadIdx.x * per : len, b = a + per < len ? a + per : len;
    uint32_t c = 0xffffffffu;
    for (uint32_t i = a; i < b; ++i) c = table[(c ^ plain[off + i]) & 255u] ^ (c >> 8);
    uint32_t crc = c ^ 0xffffffffu, n = b - a;
    for (int st = 1; st < 64; st *= 2) {
        const uint32_t pc = (uint32_t)__shfl_down((int)crc, st), pl = (uint32_t)__shfl_down((int)n, st);
        if (threadIdx.x + (uint32_t)st < 64u) { crc = tsinf::crc_combine(crc, pc, pl); n += pl; }
    }
    if (threadIdx.x == 0) slices[s].crc = crc;
}

}  // namespace

int ts_k_launch_gzip_probe(const void *window, uint32_t window_len, uint32_t start_bit, uint32_t span_bytes, uint32_t n_spans,
                           uint32_t *cand, void *stream) {
    if (n_spans == 0) return 0;
    hipLaunchKernelGGL(ts_gzip_probe_kernel, dim3(n_spans), dim3(64), 0, (hipStream_t)stream, (const uint32_t *)window, window_len,
                       start_bit, 8u * span_bytes, n_spans, cand);
    return (int)hipGetLastError();
}

int ts_k_launch_gzip_decode(const void *window, uint32_t window_len, uint32_t n_spans, const uint32_t *cand, uint32_t cap,
                            uint32_t hist0_len, void *sym, void *table, void *stream) {
    if (n_spans == 0) return 0;
    hipLaunchKernelGGL(ts_gzip_decode_kernel, dim3(n_spans), dim3(64), 0, (hipStream_t)stream, (const uint32_t *)window, window_len,
                       n_spans, cand, cap, hist0_len, (uint16_t *)sym, (SpanEntry *)table);
    return (int)hipGetLastError();
}

int ts_k_launch_gzip_resolve(const void *sym, uint32_t cap, const void *chain, uint32_t n_chain, uint32_t max_out, void *hist,
                             void *plain, unsigned long long plain_n, uint32_t *bad_span, void *stream) {
    if (n_chain == 0) return 0;
    hipLaunchKernelGGL(ts_gzip_tails_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const uint16_t *)sym, cap,
                       (const ChainEntry *)chain, n_chain, (unsigned char *)hist);
    if (max_out) {
        hipLaunchKernelGGL(ts_gzip_resolve_kernel, dim3((max_out + kResolveTile - 1u) / kResolveTile, n_chain), dim3(256), 0,
                           (hipStream_t)stream, (const uint16_t *)sym, cap, (const ChainEntry *)chain, n_chain,
                           (const unsigned char *)hist, (unsigned char *)plain, plain_n, bad_span);
    }
    return (int)hipGetLastError();
}

int ts_k_launch_gzip_crc(const void *plain, unsigned long long plain_n, void *slices, uint32_t n_slices, void *stream) {
    if (n_slices == 0) return 0;
    hipLaunchKernelGGL(ts_gzip_crc_kernel, dim3(n_slices), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, plain_n,
                       (CrcSlice *)slices, n_slices);
    return (int)hipGetLastError();
}
