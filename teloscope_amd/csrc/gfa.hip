// gfa.hip — GFA text of a resident chunk (chunk_internal.h) turned into a segment table, a table of its P and H lines and one
// buffer of the segments' names and those lines, on the device.  One-wave workgroups throughout, like fasta.hip's.  The chunk
// layer's line index and tab index (chunk.hip: the byte count, the scan and the byte index for '\n' and for '\t') run in front of
// everything here: the one step that touches every byte is spread over the bytes, so an S line of hundreds of megabases costs
// what its bytes cost, and no thread walks it.
//
//   * line kinds: a lane per line.  Kind, second byte and content length come from the line index; an S line finds its first tabs
//     by a lower bound of its start in the tab offsets (a binary search of ~25 steps, whatever the line's length).  A wave per
//     2 048 lines counts segments, P / H lines and the bytes to gather; one wave sums the counts; a second pass gives every kept
//     line its index and its place in the gathered text.  The lowest foreign line is taken by a 64-bit atomic minimum.
//   * gather: a wave per item copies a segment's name or a P / H line into the text buffer.  Sequences are never copied.
//   * check (assembly record filters): a lane per line judges it by the filtered loader's rules over the same line and tab
//     indexes; the one thing the indexes do not say, whether a line holds a '\r' that is not its last byte, comes from a pass
//     over the bytes in the tab count's shape that marks such lines for the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teloscan.h"
#include "chunk_device.h"
#include "gfa_internal.h"
#include "ts_device.h"

namespace {

// the first tab at or behind byte pos, as an index into tabs (n_tabs: there is none)
__device__ __forceinline__ uint32_t tab_lower_bound(const uint32_t *tabs, uint32_t n_tabs, uint32_t pos) {
    uint32_t lo = 0, hi = n_tabs;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tabs[mid] < pos) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// line i of n_lines by readGfa's rules: its kind byte and the bytes it gathers (a segment's name, a P / H line whole)
__device__ __forceinline__ void line_facts(const unsigned char *plain, const uint32_t *lstart, const unsigned char *first,
                                           const unsigned char *cr, const uint32_t *tabs, uint32_t n_tabs, uint32_t i,
                                           uint32_t n_lines, uint32_t &kind, uint32_t &bytes) {
    kind = kGfaNothing; bytes = 0u;
    if (i >= n_lines) return;
    const uint32_t ls = lstart[i], len = lstart[i + 1] - 1u - ls - (uint32_t)cr[i];    // without '\n' and the '\r' in front of it
    if (len == 0u) return;
    const unsigned char type = first[i];
    const bool single = len == 1u || plain[ls + 1u] == '\t';
    if (type != '#' && !(single && (type == 'H' || type == 'S'))) kind = kGfaForeign;
    if (!single) return;
    if (type == 'H') { kind |= kGfaHeader; bytes = len; }
    else if (type == 'P') { kind |= kGfaPath; bytes = len; }
    else if (type == 'S') {
        // three fields or more: two tabs inside the content
        const uint32_t k = tab_lower_bound(tabs, n_tabs, ls), end = ls + len;
        if (k + 1u < n_tabs && tabs[k + 1u] < end) { kind |= kGfaSegment; bytes = tabs[k + 1u] - tabs[k] - 1u; }
    }
}

__global__ __launch_bounds__(64)
void ts_gfa_kinds_kernel(const unsigned char *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                         uint32_t n_lines, const uint32_t *tabs, uint32_t n_tabs, unsigned char *kinds, GfaFrame *frames,
                         unsigned long long *out) {
    uint32_t segs = 0, lines = 0, text = 0;
    for (uint32_t s = 0; s < kGfaSliceLines; s += 64u) {
        // (in 64 bits: the last slice of a chunk of nearly 2^32 lines would wrap)
        const unsigned long long at = (unsigned long long)blockIdx.x * kGfaSliceLines + s + threadIdx.x;
        const uint32_t i = at < n_lines ? (uint32_t)at : n_lines;
        uint32_t kind, bytes;
        line_facts(plain, lstart, first, cr, tabs, n_tabs, i, n_lines, kind, bytes);
        if (i < n_lines) kinds[i] = (unsigned char)kind;
        const uint32_t what = kind & 3u;
        segs += what == kGfaSegment ? 1u : 0u;
        lines += what == kGfaPath || what == kGfaHeader ? 1u : 0u;
        text += bytes;
        const unsigned long long foreign = ballot64((kind & kGfaForeign) != 0u);
        // (lines ascend with the lanes: the lowest lane's is the step's lowest)
        if (foreign && threadIdx.x == (uint32_t)__builtin_ctzll(foreign)) atomicMin(&out[kGfForeignLine], (unsigned long long)i);
    }
    segs = wave_total(segs); lines = wave_total(lines); text = wave_total(text);
    if (threadIdx.x == 0) { GfaFrame f; f.segs = segs; f.lines = lines; f.text_bytes = text; f.pad = 0u; frames[blockIdx.x] = f; }
}

// the slices' sums -> the sums before every slice, in place (one wave, 64 slices per step); the totals; the lowest foreign line
__global__ __launch_bounds__(64)
void ts_gfa_frame_scan_kernel(GfaFrame *frames, uint32_t n_frames, const uint32_t *lstart, const unsigned char *cr, uint32_t newlines,
                              const uint32_t *tabs, uint32_t n_tabs, unsigned long long *out) {
    uint32_t segs = 0, lines = 0, text = 0;
    for (uint32_t b = 0; b < n_frames; b += 64u) {
        const uint32_t i = b + threadIdx.x;
        GfaFrame f; f.segs = f.lines = f.text_bytes = f.pad = 0u;
        if (i < n_frames) f = frames[i];
        const uint32_t is = wave_scan_add(f.segs), il = wave_scan_add(f.lines), it = wave_scan_add(f.text_bytes);
        if (i < n_frames) {
            GfaFrame g; g.segs = segs + is - f.segs; g.lines = lines + il - f.lines; g.text_bytes = text + it - f.text_bytes; g.pad = 0u;
            frames[i] = g;
        }
        segs += (uint32_t)__builtin_amdgcn_readlane((int)is, 63);
        lines += (uint32_t)__builtin_amdgcn_readlane((int)il, 63);
        text += (uint32_t)__builtin_amdgcn_readlane((int)it, 63);
    }
    if (threadIdx.x == 0) {
        out[kGfSegs] = segs; out[kGfLines] = lines; out[kGfTextBytes] = text; out[kGfLastLine] = lstart[newlines];
        const unsigned long long fl = out[kGfForeignLine];
        unsigned long long off = 0ull, flen = 0ull;
        if (fl != ~0ull) {                                      // its first field: up to the first tab or the content's end
            const uint32_t i = (uint32_t)fl, ls = lstart[i], end = lstart[i + 1] - 1u - (uint32_t)cr[i];
            const uint32_t k = tab_lower_bound(tabs, n_tabs, ls);
            off = ls;
            flen = (k < n_tabs && tabs[k] < end ? tabs[k] : end) - ls;
        }
        out[kGfForeignOff] = off; out[kGfForeignLen] = flen;
    }
}

__global__ __launch_bounds__(64)
void ts_gfa_tables_kernel(const unsigned char *plain, const uint32_t *lstart, const unsigned char *cr, uint32_t n_lines,
                          const uint32_t *tabs, uint32_t n_tabs, const unsigned char *kinds, const GfaFrame *frames,
                          ts_gfa_segment *segs, uint32_t n_segs, ts_gfa_line *lines, uint32_t n_kept) {
    const GfaFrame f = frames[blockIdx.x];
    uint32_t s0 = f.segs, l0 = f.lines, t0 = f.text_bytes;
    for (uint32_t s = 0; s < kGfaSliceLines; s += 64u) {
        const unsigned long long at = (unsigned long long)blockIdx.x * kGfaSliceLines + s + threadIdx.x;
        const uint32_t i = at < n_lines ? (uint32_t)at : n_lines;
        const uint32_t what = i < n_lines ? (uint32_t)kinds[i] & 3u : kGfaNothing;
        uint32_t ls = 0, len = 0, bytes = 0, k = 0;
        if (what != kGfaNothing) {
            ls = lstart[i]; len = lstart[i + 1] - 1u - ls - (uint32_t)cr[i];
            bytes = len;
            if (what == kGfaSegment) { k = tab_lower_bound(tabs, n_tabs, ls); bytes = tabs[k + 1u] - tabs[k] - 1u; }
        }
        const uint32_t is_seg = what == kGfaSegment ? 1u : 0u, is_line = what == kGfaPath || what == kGfaHeader ? 1u : 0u;
        const uint32_t is = wave_scan_add(is_seg), il = wave_scan_add(is_line), it = wave_scan_add(bytes);
        const uint32_t place = t0 + it - bytes;
        if (is_seg) {
            const uint32_t r = s0 + is - 1u, end = ls + len;
            if (r < n_segs) {                                   // (always: the count pass saw the same lines)
                // the content is cut at its first four tabs: tabs k .. k + 3, those before its end
                const uint32_t ta = tabs[k], tb = tabs[k + 1u];
                const uint32_t tc = k + 2u < n_tabs && tabs[k + 2u] < end ? tabs[k + 2u] : end;
                const uint32_t td = tc < end && k + 3u < n_tabs && tabs[k + 3u] < end ? tabs[k + 3u] : end;
                ts_gfa_segment e;
                e.off = ls; e.len = len;
                e.n_fields = 3u + (tc < end ? 1u : 0u) + (td < end ? 1u : 0u);
                e.f1_at = ta + 1u - ls; e.f1_len = tb - ta - 1u;
                e.f2_at = tb + 1u - ls; e.f2_len = tc - tb - 1u;
                e.f3_at = tc < end ? tc + 1u - ls : 0u; e.f3_len = tc < end ? td - tc - 1u : 0u;
                e.name_at = place;
                e.star = (e.f2_len == 1u && plain[tb + 1u] == '*' ? 1u : 0u) | (e.f3_len == 1u && plain[tc + 1u] == '*' ? 2u : 0u);
                segs[r] = e;
            }
        }
        if (is_line) {
            const uint32_t r = l0 + il - 1u;
            if (r < n_kept) {
                ts_gfa_line e;
                e.off = ls; e.len = len; e.kind = what == kGfaPath ? 'P' : 'H'; e.text_at = place; e.reserved = 0u;
                lines[r] = e;
            }
        }
        s0 += (uint32_t)__builtin_amdgcn_readlane((int)is, 63);
        l0 += (uint32_t)__builtin_amdgcn_readlane((int)il, 63);
        t0 += (uint32_t)__builtin_amdgcn_readlane((int)it, 63);
    }
}

// a wave per item: a segment's name, or a P / H line without its line end
__global__ __launch_bounds__(64)
void ts_gfa_gather_kernel(const unsigned char *plain, unsigned long long size, const ts_gfa_segment *segs, uint32_t n_segs,
                          const ts_gfa_line *lines, uint32_t n_kept, unsigned char *text, unsigned long long text_bytes) {
    unsigned long long from, to;
    uint32_t n;
    if (blockIdx.x < n_segs) { const ts_gfa_segment e = segs[blockIdx.x]; from = e.off + e.f1_at; to = e.name_at; n = e.f1_len; }
    else if (blockIdx.x - n_segs < n_kept) { const ts_gfa_line e = lines[blockIdx.x - n_segs]; from = e.off; to = e.text_at; n = e.len; }
    else return;
    for (uint32_t i = threadIdx.x; i < n; i += 64u)
        if (from + i < size && to + i < text_bytes) text[to + i] = plain[from + i];
}

// ---- the filtered loader's check
// A stray '\r': one that is not the last byte of its line's content, i.e. whose next byte is no '\n' and that is not the input's
// last byte.  A wave per slice, 16 bytes per lane per step; a step without one is skipped.  The line of a stray '\r' at p is the
// last one that starts at or before p: a search of lstart[0, n_lines] (lstart[n_lines] is the end of the whole lines), and a
// '\r' of the unfinished last line finds none.
__global__ __launch_bounds__(64)
void ts_gfa_stray_cr_kernel(const unsigned char *plain, unsigned long long n, int at_end, const uint32_t *lstart, uint32_t n_lines,
                            unsigned char *stray) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kChunkSliceBytes + threadIdx.x * 16u;
    for (uint32_t s = 0; s < kChunkSliceBytes / 1024u; ++s) {
        const unsigned long long a = base + 1024ull * s;
        uint32_t m = 0u;
        if (a < n) {
            const uint4 q = *(const uint4 *)(plain + a);        // (the chunk's buffer is readable 64 bytes beyond its capacity)
            const uint32_t in_chunk = n - a >= 16ull ? 0xffffu : (1u << (uint32_t)(n - a)) - 1u;
            const uint32_t lf = byte_eq_mask16(q, 0x0a0a0a0au) & in_chunk, cr = byte_eq_mask16(q, 0x0d0d0d0du) & in_chunk;
            const uint32_t lf_next = (lf >> 1) | (a + 16ull < n && plain[a + 16ull] == '\n' ? 0x8000u : 0u);
            m = cr & ~lf_next;
            if (at_end && n - 1ull >= a && n - 1ull < a + 16ull) m &= ~(1u << (uint32_t)(n - 1ull - a));
        }
        if (ballot64(m != 0u) == 0ull) continue;                // (wave-uniform)
        while (m) {
            const uint32_t p = (uint32_t)a + (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            uint32_t lo = 0u, hi = n_lines + 1u;                // the first entry of lstart[0, n_lines] beyond p
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (lstart[mid] <= p) lo = mid + 1u; else hi = mid;
            }
            if (lo >= 1u && lo <= n_lines) stray[lo - 1u] = 1;
        }
    }
}

// line i (< n_lines) by validateFilteredGfa's rules: 0, the first rule it breaks (1..7), or 255 where the host decides
__device__ __forceinline__ uint32_t check_line(const unsigned char *plain, const uint32_t *lstart, const unsigned char *first,
                                               const unsigned char *cr, const uint32_t *tabs, uint32_t n_tabs,
                                               const unsigned char *stray, uint32_t i) {
    if (stray[i]) return TS_GFA_CHECK_HOST_DECIDES;
    const uint32_t ls = lstart[i], len = lstart[i + 1] - 1u - ls - (uint32_t)cr[i], end = ls + len;
    const unsigned char type = first[i];
    if (len == 0u || type == '#') return 0u;
    const bool tabbed = len >= 2u && plain[ls + 1u] == '\t';
    if (tabbed && type == 'H') {                                // "\tVN:Z:2" behind any of the line's tabs
        for (uint32_t k = tab_lower_bound(tabs, n_tabs, ls); k < n_tabs && tabs[k] + 7ull <= end; ++k) {
            const unsigned char *p = plain + tabs[k];
            if (p[1] == 'V' && p[2] == 'N' && p[3] == ':' && p[4] == 'Z' && p[5] == ':' && p[6] == '2') return 1u;
        }
    }
    if (!tabbed) return 2u;
    if (type == 'O' || type == 'U' || type == 'E' || type == 'G' || type == 'F') return 3u;
    if (type == 'W') return 4u;
    if (type == 'C') return 5u;
    if (type == 'S') {                                          // S name LEN seq: the tabs behind the name and behind the third field
        const uint32_t k = tab_lower_bound(tabs, n_tabs, ls + 2u);
        if (k + 1u < n_tabs && tabs[k + 1u] < end && tabs[k + 1u] > tabs[k] + 1u) {
            uint32_t p = tabs[k] + 1u;
            while (p < tabs[k + 1u] && plain[p] >= '0' && plain[p] <= '9') ++p;
            if (p == tabs[k + 1u]) return 6u;
        }
    }
    if (type != 'H' && type != 'S' && type != 'L' && type != 'J' && type != 'P') return 7u;
    return 0u;
}

__global__ __launch_bounds__(64)
void ts_gfa_check_kernel(const unsigned char *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                         uint32_t n_lines, const uint32_t *tabs, uint32_t n_tabs, const unsigned char *stray, unsigned char *codes,
                         uint32_t *counts) {
    uint32_t flagged = 0;
    for (uint32_t s = 0; s < kGfaSliceLines; s += 64u) {
        const unsigned long long at = (unsigned long long)blockIdx.x * kGfaSliceLines + s + threadIdx.x;
        if (at >= n_lines) continue;
        const uint32_t code = check_line(plain, lstart, first, cr, tabs, n_tabs, stray, (uint32_t)at);
        codes[at] = (unsigned char)code;
        flagged += code ? 1u : 0u;
    }
    flagged = wave_total(flagged);
    if (threadIdx.x == 0) counts[blockIdx.x] = flagged;
}

__global__ __launch_bounds__(64)
void ts_gfa_flagged_kernel(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                           const unsigned char *codes, const uint32_t *sums, ts_gfa_flagged *flagged, uint32_t n_flagged) {
    uint32_t f0 = sums[blockIdx.x];
    for (uint32_t s = 0; s < kGfaSliceLines; s += 64u) {
        const unsigned long long at = (unsigned long long)blockIdx.x * kGfaSliceLines + s + threadIdx.x;
        const uint32_t i = at < n_lines ? (uint32_t)at : n_lines;
        const uint32_t code = i < n_lines ? (uint32_t)codes[i] : 0u;
        const uint32_t is = code ? 1u : 0u, incl = wave_scan_add(is);
        const uint32_t r = f0 + incl - 1u;
        if (is && r < n_flagged) {                              // (always: the count pass wrote these codes)
            ts_gfa_flagged e;
            e.off = lstart[i]; e.line = i; e.len = lstart[i + 1] - 1u - lstart[i] - (uint32_t)cr[i]; e.code = code; e.type = first[i];
            flagged[r] = e;
        }
        f0 += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
}

}  // namespace

extern "C" {

int ts_k_launch_gfa_stray_cr(const void *plain, unsigned long long n, int at_end, const uint32_t *lstart, uint32_t n_lines,
                             unsigned char *stray, void *stream) {
    const uint32_t slices = (uint32_t)((n + kChunkSliceBytes - 1) / kChunkSliceBytes);
    if (slices == 0 || n_lines == 0) return 0;
    hipLaunchKernelGGL(ts_gfa_stray_cr_kernel, dim3(slices), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, n, at_end,
                       lstart, n_lines, stray);
    return (int)hipGetLastError();
}

int ts_k_launch_gfa_check(const void *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                          uint32_t n_lines, const uint32_t *tabs, uint32_t n_tabs, const unsigned char *stray, unsigned char *codes,
                          uint32_t *counts, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kGfaSliceLines - 1) / kGfaSliceLines);
    if (nf == 0) return 0;
    hipLaunchKernelGGL(ts_gfa_check_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, lstart, first, cr,
                       n_lines, tabs, n_tabs, stray, codes, counts);
    return (int)hipGetLastError();
}

int ts_k_launch_gfa_flagged(const uint32_t *lstart, const unsigned char *first, const unsigned char *cr, uint32_t n_lines,
                            const unsigned char *codes, const uint32_t *sums, void *flagged, uint32_t n_flagged, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kGfaSliceLines - 1) / kGfaSliceLines);
    if (nf == 0 || n_flagged == 0) return 0;
    hipLaunchKernelGGL(ts_gfa_flagged_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, lstart, first, cr, n_lines, codes, sums,
                       (ts_gfa_flagged *)flagged, n_flagged);
    return (int)hipGetLastError();
}

int ts_k_launch_gfa_kinds(const void *plain, const uint32_t *lstart, const unsigned char *first, const unsigned char *cr,
                          uint32_t n_lines, uint32_t newlines, const uint32_t *tabs, uint32_t n_tabs, unsigned char *kinds,
                          void *frames, unsigned long long *out, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kGfaSliceLines - 1) / kGfaSliceLines);
    if (nf) hipLaunchKernelGGL(ts_gfa_kinds_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, lstart,
                               first, cr, n_lines, tabs, n_tabs, kinds, (GfaFrame *)frames, out);
    hipLaunchKernelGGL(ts_gfa_frame_scan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (GfaFrame *)frames, nf, lstart, cr, newlines,
                       tabs, n_tabs, out);
    return (int)hipGetLastError();
}

int ts_k_launch_gfa_tables(const void *plain, const uint32_t *lstart, const unsigned char *cr, uint32_t n_lines,
                           const uint32_t *tabs, uint32_t n_tabs, const unsigned char *kinds, const void *frames, void *segs,
                           uint32_t n_segs, void *lines, uint32_t n_kept, void *stream) {
    const uint32_t nf = (uint32_t)(((unsigned long long)n_lines + kGfaSliceLines - 1) / kGfaSliceLines);
    if (nf == 0) return 0;
    hipLaunchKernelGGL(ts_gfa_tables_kernel, dim3(nf), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, lstart, cr,
                       n_lines, tabs, n_tabs, kinds, (const GfaFrame *)frames, (ts_gfa_segment *)segs, n_segs, (ts_gfa_line *)lines, n_kept);
    return (int)hipGetLastError();
}

int ts_k_launch_gfa_gather(const void *plain, unsigned long long size, const void *segs, uint32_t n_segs, const void *lines,
                           uint32_t n_kept, void *text, unsigned long long text_bytes, void *stream) {
    const unsigned long long items = (unsigned long long)n_segs + n_kept;
    if (items == 0 || items > 0x7fffffffull) return 0;
    hipLaunchKernelGGL(ts_gfa_gather_kernel, dim3((unsigned)items), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, size,
                       (const ts_gfa_segment *)segs, n_segs, (const ts_gfa_line *)lines, n_kept, (unsigned char *)text, text_bytes);
    return (int)hipGetLastError();
}

}  // extern "C"
