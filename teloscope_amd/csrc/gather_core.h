// gather_core.h — the copy of one device-resident piece into the scan's input layout, one source for the gfx950 kernel
// (gather.hip: ts_gather_pieces_kernel) and for a host test program (tests/cpp/device_gather_host.cpp, built by g++ under
// ASan + UBSan), and the host splitter that turns pieces into the kernel's jobs.  No allocation, no library calls.
//
// A job is {source address, destination, byte count}; 64 callers ("lanes") share it.  Source and destination may be ANY
// addresses, and both have neighbours the copy must leave alone:
//
//   reads    the caller's allocation may end with the piece's last byte (include/teloscan.h: "any address will do"), so the only
//            loads are of 4-byte aligned words that hold at least one byte of [src, src + n): such a word shares its page with a
//            byte of the piece.  Sixteen bytes from an unaligned address are the four aligned words that hold its first
//            thirteen bytes — every one of them holds a byte of the vector — plus a fifth word that is loaded only when the
//            address is off a word boundary (on one, that word lies wholly behind the vector and perhaps behind the piece);
//   writes   other jobs, and host pieces' uploads, write the bytes either side of [dst, dst + n), possibly within the same
//            16-byte line and at the same time: no read-modify-write, every byte of the job is stored exactly once — single
//            bytes up to the destination's next 16-byte boundary, aligned 16-byte stores for the body, single bytes for the rest.
//
// Memory is reached through an accessor A, which is what differs between the two builds:
//   uint32_t word(uint64_t a)                          the aligned word at address a (a % 4 == 0)
//   void     words4(uint64_t a, uint32_t w[4])         the four aligned words at a, a + 4, a + 8, a + 12 (a % 4 == 0)
//   void     store_byte(uint64_t a, uint32_t v)        the low byte of v to address a
//   void     store16(uint64_t a, const uint32_t v[4])  sixteen bytes to address a (a % 16 == 0)
#ifndef TS_GATHER_CORE_H
#define TS_GATHER_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TS_GHD __host__ __device__ __forceinline__
#else
#define TS_GHD inline
#endif

namespace tsgather {

constexpr uint32_t kLanes = 64;                     // callers per job (one wave)
constexpr uint32_t kSliceBytes = 16384;             // the most one job copies (the slice of fastq.hip's and fasta.hip's kernels)

struct Job {                                        // 24 bytes
    unsigned long long src;                         // device address of the first byte
    unsigned long long dst;                         // byte offset of its place from the base the kernel is given
    uint32_t n;                                     // bytes, at most kSliceBytes
    uint32_t reserved;
};

// bytes sh .. sh + 3 of the eight bytes lo (0..3), hi (4..7): what __builtin_amdgcn_alignbyte(hi, lo, sh) gives for sh < 4
TS_GHD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return sh ? (lo >> (8u * sh)) | (hi << (32u - 8u * sh)) : lo;
#endif
}

// the byte at address a, out of the aligned word that holds it
template <class A>
TS_GHD uint32_t load_byte(A &m, uint64_t a) {
    return (m.word(a & ~(uint64_t)3) >> (8u * (uint32_t)(a & 3u))) & 0xffu;
}

// sixteen bytes from address a, all of them bytes of the piece
template <class A>
TS_GHD void load16(A &m, uint64_t a, uint32_t v[4]) {
    const uint64_t q = a & ~(uint64_t)3;
    const uint32_t sh = (uint32_t)(a & 3u);
    uint32_t w[4];
    m.words4(q, w);
    const uint32_t w4 = sh ? m.word(q + 16) : 0u;   // (sh == 0: that word holds no byte of the vector)
    v[0] = align_bytes(w[1], w[0], sh);
    v[1] = align_bytes(w[2], w[1], sh);
    v[2] = align_bytes(w[3], w[2], sh);
    v[3] = align_bytes(w4, w[3], sh);
}

// Lane `lane` of kLanes' share of the copy of n bytes from address src to address dst.  Lanes 0..15 store the bytes in front
// of the destination's first 16-byte boundary, lanes 16..31 those behind its last one, and all lanes the 16-byte vectors in
// between, lane l the l-th, (l + 64)-th, ... of them.
template <class A>
TS_GHD void copy_lane(A &m, uint64_t src, uint64_t dst, uint32_t n, uint32_t lane) {
    uint32_t head = (16u - (uint32_t)(dst & 15u)) & 15u;
    if (head > n) head = n;
    const uint32_t body = (n - head) & ~15u, rest = n - head - body;
    if (lane < head) m.store_byte(dst + lane, load_byte(m, src + lane));
    if (lane >= 16u && lane - 16u < rest) {
        const uint32_t at = head + body + (lane - 16u);
        m.store_byte(dst + at, load_byte(m, src + at));
    }
    for (uint32_t i = lane * 16u; i < body; i += kLanes * 16u) {
        uint32_t v[4];
        load16(m, src + head + i, v);
        m.store16(dst + head + i, v);
    }
}

// Host side: the jobs of one piece of len bytes from address src to place dst, where dst is any number congruent, modulo 16,
// to the ADDRESS the piece's first byte goes to (the offset in the layout when the layout's base is 16-byte aligned).  The
// first job ends at the destination's 16-byte boundary at most `slice` bytes on (slice: a multiple of 16), the others begin on
// one and hold `slice` bytes, the last what is left: in order, without gaps or overlap, none longer than a slice, and every job
// but the first stores whole vectors from its first byte on.  emit(src, dst, n) is called per job; a piece of no bytes has none.
template <class F>
inline void split_piece(uint64_t src, uint64_t dst, uint64_t len, uint32_t slice, F &&emit) {
    uint64_t at = 0;
    while (at < len) {
        const uint64_t room = slice - ((dst + at) & 15u);
        const uint64_t n = len - at < room ? len - at : room;
        emit(src + at, dst + at, (uint32_t)n);
        at += n;
    }
}

// ... and how many there are
inline uint64_t split_count(uint64_t dst, uint64_t len, uint32_t slice) {
    if (!len) return 0;
    const uint64_t first = slice - (dst & 15u);
    return len <= first ? 1 : 1 + (len - first + slice - 1) / slice;
}

}  // namespace tsgather

#endif
