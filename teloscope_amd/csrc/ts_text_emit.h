// ts_text_emit.h — how the device text formatters (tracks.hip, match_text.hip) get a wave's lines into a file (device code only).
//
// Stores.  A lane's line starts at whatever byte the lines before it end on, so lanes that stored their own lines would issue
// byte stores at unaligned addresses, ~70 per line.  Instead a wave stages the text of its 64 lines of one file in LDS — shifted
// by the destination's offset within a 16-byte line, so that 16-byte pieces of the staging area are 16-byte pieces of the file —
// and copies it out with aligned 16-byte stores, lane l the l-th, (l + 64)-th, ... of them; only the bytes in front of the first
// and behind the last 16-byte boundary go out singly (the neighbouring waves store the rest of those lines at the same time: no
// read-modify-write).  A wave whose 64 lines exceed the staging area writes them bytewise.  What is staged and which lane stores
// what is text_store_core.h, which a host program checks lane by lane.  Neither function here holds a barrier: the CALLER puts one
// between wave_put and wave_copy_out (the staged text is read by other lanes) and one behind (the staging area is used again).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "text_store_core.h"

#define TS_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kStageVecs = tsstore::kStageBytes / 16u + 1u;    // a wave's staging area, u32x4 (+ the shift of up to 15 bytes)

struct GlobalBytes {                                        // names, bases
    const TS_GLOBAL unsigned char *p;
    __device__ __forceinline__ uint32_t byte(unsigned long long i) const { return p[i]; }
};
struct StageSink {                                          // a wave's staging area (the pointer comes straight from a __shared__ array)
    unsigned char *p;
    __device__ __forceinline__ void put(uint32_t at, uint32_t byte) const { p[at] = (unsigned char)byte; }
};
struct GlobalSink {
    TS_GLOBAL unsigned char *p;
    __device__ __forceinline__ void put(uint32_t at, uint32_t byte) const { p[at] = (unsigned char)byte; }
};

// A lane's line, which starts `excl` bytes into the wave's n bytes for dst: put(sink, at) writes it into the staging area, or,
// when the n bytes are not staged, straight into the file.
template <class Put>
__device__ __forceinline__ void wave_put(u32x4 *stage, TS_GLOBAL unsigned char *dst, uint32_t n, uint32_t excl, const Put &put) {
    if (tsstore::staged(n, tsstore::kStageBytes)) put(StageSink{(unsigned char *)stage}, (uint32_t)((uintptr_t)dst & 15u) + excl);
    else put(GlobalSink{dst}, excl);
}

// The wave's n staged bytes to dst (n: uniform over the wave; nothing to do when they were written bytewise).
__device__ __forceinline__ void wave_copy_out(const u32x4 *stage, TS_GLOBAL unsigned char *dst, uint32_t n, uint32_t lane) {
    if (!n || !tsstore::staged(n, tsstore::kStageBytes)) return;
    const unsigned char *lds = (const unsigned char *)stage;
    const uint32_t shift = (uint32_t)((uintptr_t)dst & 15u);
    const tsstore::Plan p = tsstore::plan(shift, n);
    if (lane < p.head) dst[lane] = lds[shift + lane];
    if (lane >= 16u && lane - 16u < p.rest) dst[p.head + p.body + lane - 16u] = lds[shift + p.head + p.body + lane - 16u];
    for (uint32_t v = lane; v < p.body / 16u; v += 64u) *(TS_GLOBAL u32x4 *)(dst + p.head + 16u * v) = stage[p.v0 + v];
}
