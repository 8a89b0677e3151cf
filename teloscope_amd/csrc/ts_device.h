// ts_device.h — wave primitives and uncounted global stores shared by the gfx950 kernels of libteloscan (device code only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Wave-wide inclusive prefix sum in 6 DPP adds (row_shr 1/2/4/8 inside each row of 16, then row_bcast:15 into rows 1,3 and
// row_bcast:31 into rows 2,3; lanes outside a shift read 0); no LDS traffic.  Lane 63 holds the total.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    return v;
}
// sum of v over the wave's lanes (wave-uniform)
__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_add(v), 63);
}

// Wave-wide exclusive prefix sum of one 64-bit value per lane (callers: one wave per workgroup, or the lanes of one wave);
// returns the lane's exclusive prefix, *total = the wave's sum.
__device__ __forceinline__ unsigned long long wave_excl_scan_u64(unsigned long long v, unsigned long long *total) {
    unsigned long long incl = v;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, (int)o), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), (int)o);
        if (lane >= o) incl += ((unsigned long long)hi << 32) | lo;
    }
    const uint32_t tlo = (uint32_t)__shfl((int)(uint32_t)incl, 63), thi = (uint32_t)__shfl((int)(uint32_t)(incl >> 32), 63);
    *total = ((unsigned long long)thi << 32) | tlo;
    return incl - v;
}

// Wave-wide inclusive prefix maximum, the same six DPP steps.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
    return v > o ? v : o;
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
    v = dpp_max<0x111, 0xf>(v);
    v = dpp_max<0x112, 0xf>(v);
    v = dpp_max<0x114, 0xf>(v);
    v = dpp_max<0x118, 0xf>(v);
    v = dpp_max<0x142, 0xa>(v);
    v = dpp_max<0x143, 0xc>(v);
    return v;
}

// The value of the lane below (lane 0: fill) by DPP wave_shr:1.  The empty asm keeps it a v_mov_b32_dpp: folded into the
// subtraction that follows (v_subrev_u32_dpp v, x, x wave_shr:1, what the DPP combiner makes of it) it came back wrong on gfx950.
__device__ __forceinline__ uint32_t lane_below(uint32_t v, uint32_t fill = 0u) {
    uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xf, 0xf, false);
    asm volatile("" : "+v"(r));
    return r;
}

// the lowest n bits of a lane mask (n >= 64: all)
__device__ __forceinline__ unsigned long long low_bits(uint32_t n) { return n >= 64u ? ~0ull : ((1ull << n) - 1ull); }

// the lanes for which `p` holds, as a mask: on a bool this is one scalar AND of the compare's result with exec (__ballot takes
// an int: the bool is first materialised per lane and compared again, two vector instructions per ballot)
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// sixteen 2-bit codes, held doubled (2 * code = ASCII & 6) one per byte of t[0..3] -> one dword, base i at
// bits 2i..2i+1; four independent v_dot4_u32_u8 (weights 1,4,16,64: twice the packed byte, 9 bits) and four
// shift/or, no dependent dot chain
__device__ __forceinline__ uint32_t pack16(const uint32_t t[4]) {
    const uint32_t b0 = __builtin_amdgcn_udot4(t[0], 0x40100401u, 0u, false);
    const uint32_t b1 = __builtin_amdgcn_udot4(t[1], 0x40100401u, 0u, false);
    const uint32_t b2 = __builtin_amdgcn_udot4(t[2], 0x40100401u, 0u, false);
    const uint32_t b3 = __builtin_amdgcn_udot4(t[3], 0x40100401u, 0u, false);
    return ((b0 | (b1 << 8)) >> 1) | ((b2 | (b3 << 8)) << 15);
}

// Global stores and return-less atomics the compiler does not see.  On gfx9 loads and stores share one counter (vmcnt) and may
// retire out of order with respect to each other, so once a store is pending the compiler can only wait for a LOAD with vmcnt(0) —
// and it does so early: in front of every loop that holds a store and no load it empties the counter ("flush in the preheader").
// In the tiled kernel that meant an s_waitcnt vmcnt(0) right behind the request of the next tile's first chunk (the last drain of
// the match queue is such a loop: its overflow path stores), i.e. the prefetch was waited for on the spot, and two more in phase 2;
// in the general list kernel the wait for the next tile's prefetch came a few instructions behind its issue.
// The stores never feed a load of the kernel that issues them (the one place that reads records back waits for vmcnt(0) itself), so
// they are issued by inline asm: the compiler counts only its loads, whose waits stay counted, and a pending store can only make
// such a wait longer, never too short (loads retire in order among themselves).  Measurements: profiles/r05/asm_stores.txt.
__device__ __forceinline__ void gstore(uint32_t *p, uint32_t v) {
    asm volatile("global_store_dword %0, %1, off" :: "v"(p), "v"(v));
}
__device__ __forceinline__ void gstore(uint16_t *p, uint16_t v) {
    asm volatile("global_store_short %0, %1, off" :: "v"(p), "v"((uint32_t)v));
}
// (the low 16 bits of v: the store takes them itself)
__device__ __forceinline__ void gstore_lo16(uint16_t *p, uint32_t v) {
    asm volatile("global_store_short %0, %1, off" :: "v"(p), "v"(v));
}
__device__ __forceinline__ void gstore(unsigned char *p, unsigned char v) {
    asm volatile("global_store_byte %0, %1, off" :: "v"(p), "v"((uint32_t)v));
}
__device__ __forceinline__ void gstore(unsigned long long *p, unsigned long long v) {
    asm volatile("global_store_dwordx2 %0, %1, off" :: "v"(p), "v"(v));
}
__device__ __forceinline__ void gstore(uint4 *p, uint4 v) {
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    const u32x4_t d = {v.x, v.y, v.z, v.w};
    // (s_nop: a store of more than 8 bytes reads its data a cycle late, and the hazard recogniser does not look into asm)
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 0" :: "v"(p), "v"(d));
}
// (possibly unaligned: the bit-packed window records)
__device__ __forceinline__ void gstore_unaligned(unsigned char *p, unsigned long long v) {
    asm volatile("global_store_dwordx2 %0, %1, off" :: "v"(p), "v"(v));
}
__device__ __forceinline__ void gstore_unaligned(unsigned char *p, uint32_t v) {
    asm volatile("global_store_dword %0, %1, off" :: "v"(p), "v"(v));
}
__device__ __forceinline__ void gatomic_add(uint32_t *p, uint32_t v) { asm volatile("global_atomic_add %0, %1, off" :: "v"(p), "v"(v)); }
__device__ __forceinline__ void gatomic_or(uint32_t *p, uint32_t v) { asm volatile("global_atomic_or %0, %1, off" :: "v"(p), "v"(v)); }
