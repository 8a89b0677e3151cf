// chunk_device.h — what the kernels over a resident chunk's bytes share (device code only; the wave primitives are ts_device.h's):
// the per-word byte test, 16 bytes from any address, the record copy of the two gathers and the tail mask of the two stages.
// Every chunk buffer is readable 64 bytes beyond its capacity (chunk.cpp), which is what the loads here rely on.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// the bytes of w that equal the byte repeated in c4, a bit per byte (bits 0..3).  t has bit 7 of every byte that is zero in x
// (exact per byte: no carry leaves a byte); the multiply moves bit 8 i + 7 to bit 24 + i (the sixteen partial products land on
// distinct bits)
__device__ __forceinline__ uint32_t byte_eq_bits(uint32_t w, uint32_t c4) {
    const uint32_t x = w ^ c4;
    const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
    return (((t >> 7) * 0x01020408u) >> 24) & 15u;
}
__device__ __forceinline__ uint32_t byte_eq_mask16(uint4 q, uint32_t c4) {
    return byte_eq_bits(q.x, c4) | byte_eq_bits(q.y, c4) << 4 | byte_eq_bits(q.z, c4) << 8 | byte_eq_bits(q.w, c4) << 12;
}

// the bytes equal to C among the 16 at plain + a (a: a multiple of 16), those at or beyond n left out
template <unsigned char C>
__device__ __forceinline__ uint32_t byte_mask16(const unsigned char *plain, unsigned long long a, unsigned long long n) {
    if (a >= n) return 0u;
    const uint32_t m = byte_eq_mask16(*(const uint4 *)(plain + a), C * 0x01010101u);
    return n - a >= 16ull ? m : m & ((1u << (uint32_t)(n - a)) - 1u);
}

// 16 bytes from any address: the five aligned dwords that hold them, shifted into place (reads up to 19 bytes beyond p + 16
// rounded down to a dword: inside the 64 readable bytes behind the chunk)
__device__ __forceinline__ uint4 load16_any(const unsigned char *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t *q = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3u);
    uint32_t w[5];
    __builtin_memcpy(w, __builtin_assume_aligned(q, 4), 20);
    return make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], sh), __builtin_amdgcn_alignbyte(w[2], w[1], sh),
                      __builtin_amdgcn_alignbyte(w[3], w[2], sh), __builtin_amdgcn_alignbyte(w[4], w[3], sh));
}

// a record of `size` bytes at src to dst = out + to, by one wave: bytes up to the destination's next 16-byte boundary, whole
// 16-byte stores, the rest.  Nothing is stored outside dst[0, size); the source is read through load16_any.
__device__ __forceinline__ void copy_record16(unsigned char *dst, const unsigned char *src, uint32_t size, unsigned long long to) {
    uint32_t head = (16u - (uint32_t)(to & 15ull)) & 15u;
    if (head > size) head = size;
    const uint32_t body = (size - head) & ~15u, rest = size - head - body;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t i = threadIdx.x * 16u; i < body; i += 1024u) *(uint4 *)(dst + head + i) = load16_any(src + head + i);
    if (threadIdx.x < rest) dst[head + body + threadIdx.x] = src[head + body + threadIdx.x];
}

// the 16 output bytes of a stage in o[0..3], of which `left` (< 16) belong to the read: the bytes behind it become zero, as an
// upload leaves them
__device__ __forceinline__ void zero_tail16(uint32_t o[4], uint32_t left) {
    __builtin_assume(left < 16u);
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t have = left > 4u * q ? left - 4u * q : 0u;
        o[q] &= have >= 4u ? 0xffffffffu : have == 0u ? 0u : (1u << (8u * have)) - 1u;
    }
}
