// text_store_core.h — how a wave's text leaves its staging area, one source for the gfx950 kernels (ts_text_emit.h, used by
// tracks.hip and match_text.hip) and for a host test program (tests/cpp/text_store_host.cpp, built by g++ under ASan + UBSan)
// that plays the 64 lanes.  No allocation, no library calls.
//
// A wave has n bytes of text for the file position dst.  It stages them in LDS at offset shift = dst & 15, so that 16-byte
// pieces of the staging area are 16-byte pieces of the file, and copies them out as
//   head   the bytes in front of the first 16-byte boundary of the file (at most 15: lane l < head stores byte l),
//   body   whole 16-byte pieces (lane l stores the l-th, (l + 64)-th, ... of them, piece v from staging vector v0 + v),
//   rest   the bytes behind the last boundary (at most 15: lane 16 + j stores byte head + body + j).
#ifndef TS_TEXT_STORE_CORE_H
#define TS_TEXT_STORE_CORE_H

#include <stdint.h>

#if !defined(TS_THD) && defined(__HIPCC__)
#define TS_THD __host__ __device__ __forceinline__
#elif !defined(TS_THD)
#define TS_THD inline
#endif

namespace tsstore {

constexpr uint32_t kStageBytes = 8192u;             // staged text per wave and file; the area holds 15 bytes more (the shift)

struct Plan { uint32_t head, body, rest, v0; };

// these n bytes go through a staging area of `capacity` bytes (else the lanes write their lines bytewise)
TS_THD bool staged(uint32_t n, uint32_t capacity) { return n <= capacity; }

TS_THD Plan plan(uint32_t shift, uint32_t n) {      // shift: 0..15
    uint32_t head = (16u - shift) & 15u;
    if (head > n) head = n;
    const uint32_t body = (n - head) & ~15u;
    return Plan{head, body, n - head - body, (shift + head) / 16u};     // (shift + head is 0 or 16 when there is a body)
}

}  // namespace tsstore

#endif
