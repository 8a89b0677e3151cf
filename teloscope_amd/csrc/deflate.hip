// deflate.hip — BGZF members written on the device: one wave per member deflates its payload, checksums it and frames it
// (what zlib behind the reference's BgzfWriter does on a host thread, src/bgzf.cpp:227-276).  The encoder itself is
// deflate_core.h, the source a host test program compiles too; this file is its device policy — where the plain bytes come from
// and where the payload's bits go — the member's 18-byte header and 8-byte footer, and the copy that packs the members.
//
// Shape of a wave's work:
//   * plain bytes are read through the cache (dword loads at any byte address), not staged: a block is up to 65 280 bytes, more
//     than a workgroup may hold in LDS beside its tables, and the encoder reads each byte a few times only;
//   * LDS holds deflate_core.h's tables: the hash table of 8 192 16-bit positions (16 KB), symbol counts, code tables, the tree
//     scratch and the batch's match and bit-length words — 27 KB in all, so five waves share a CU's 160 KB;
//   * symbol counts are LDS atomics; the token bits are ORed into the member's slot with global atomics (the slots are zeroed on
//     the stream before the launch), a prefix sum over the batch's bit lengths having placed them;
//   * a member's slot is `stride` bytes: two bytes of padding, the header at 2, the payload at 20 (dword aligned), the footer
//     behind it; sizes[i] = the member's length.  ts_deflate_pack_kernel copies the members to their places in one buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teloscan.h"
#include "chunk_device.h"
#include "deflate_core.h"
#include "ts_device.h"
#include "ts_internal.h"

namespace {

struct DeflatePolicy {
    const unsigned char *plain;
    uint32_t *out;                  // the payload's first dword

    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ uint32_t nlanes() const { return 64u; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ uint32_t byte(uint32_t i) const { return plain[i]; }
    __device__ __forceinline__ uint32_t load32(uint32_t i) const { uint32_t v; __builtin_memcpy(&v, plain + i, 4); return v; }
    __device__ __forceinline__ void tab_add(uint32_t *at, uint32_t v) const {
        (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ void tab_or(uint32_t *at, uint32_t v) const {
        (void)__hip_atomic_fetch_or(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ uint32_t prefix64(uint32_t *a) const {
        const uint32_t v = a[threadIdx.x], incl = wave_scan_add(v);
        __syncthreads();
        a[threadIdx.x] = incl - v;
        __syncthreads();
        return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    __device__ __forceinline__ void out_or(uint32_t w, uint32_t v) const {
        (void)__hip_atomic_fetch_or(out + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void out_byte(uint32_t i, uint32_t v) const { ((unsigned char *)out)[i] = (unsigned char)v; }
};

constexpr uint32_t kHeaderAt = 2, kPayloadAt = 20;

// member i: plain[i * payload_bytes, + min(payload_bytes, n - i * payload_bytes)) -> slots + i * stride
__global__ __launch_bounds__(64)
void ts_bgzf_deflate_kernel(const unsigned char *plain, unsigned long long n, uint32_t payload_bytes, uint32_t n_members,
                            unsigned char *slots, uint32_t stride, uint32_t *sizes) {
    __shared__ tsdef::Work work;
    const uint32_t b = blockIdx.x;
    if (b >= n_members) return;
    const unsigned long long from = (unsigned long long)b * payload_bytes;
    if (from >= n) return;
    const uint32_t len = n - from < payload_bytes ? (uint32_t)(n - from) : payload_bytes;
    if (len > tsdef::kMaxBlock || len + 5u + 28u > stride) return;          // (the launcher has checked both)
    unsigned char *slot = slots + (unsigned long long)b * stride;
    DeflatePolicy pol{plain + from, (uint32_t *)(slot + kPayloadAt)};
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)tsdef::deflate(pol, &work, len));
    const uint32_t crc = tsdef::crc32(pol, &work, len);
    const uint32_t total = 18u + m + 8u;
    const uint32_t t = threadIdx.x;
    if (t < 16u) {
        const uint32_t w = t < 4u ? 0x04088b1fu : t < 8u ? 0u : t < 12u ? 0x0006ff00u : 0x00024342u;
        slot[kHeaderAt + t] = (unsigned char)(w >> (8u * (t & 3u)));
    } else if (t < 18u) slot[kHeaderAt + t] = (unsigned char)((total - 1u) >> (8u * (t - 16u)));
    else if (t < 22u) slot[kPayloadAt + m + (t - 18u)] = (unsigned char)(crc >> (8u * (t - 18u)));
    else if (t < 26u) slot[kPayloadAt + m + (t - 18u)] = (unsigned char)(len >> (8u * (t - 22u)));
    if (t == 0) sizes[b] = total;
}

// member i from its slot to packed + offs[i] (offs: the exclusive sums of the sizes); a wave per member.  The copy reads up to
// 19 bytes beyond a member's last byte (load16_any): inside the slot's padding or the 64 readable bytes behind the last slot.
__global__ __launch_bounds__(64)
void ts_deflate_pack_kernel(const unsigned char *slots, uint32_t stride, const uint32_t *sizes, const unsigned long long *offs,
                            uint32_t n_members, unsigned long long cap, unsigned char *packed) {
    const uint32_t b = blockIdx.x;
    if (b >= n_members) return;
    const unsigned long long to = offs[b];
    const uint32_t size = sizes[b];
    if (size > stride - kHeaderAt || to > cap || size > cap - to) return;
    copy_record16(packed + to, slots + (unsigned long long)b * stride + kHeaderAt, size, to);
}

// sizes[n] -> offs[n] (exclusive sums), total[0] = their sum and total[1] = how many of them are zero (a member that was not
// written), one wave
__global__ __launch_bounds__(64)
void ts_deflate_offsets_kernel(const uint32_t *sizes, uint32_t n, unsigned long long *offs, unsigned long long *total) {
    unsigned long long base = 0, zeros = 0;
    for (uint32_t i = 0; i < n; i += 64u) {
        const uint32_t k = i + threadIdx.x;
        const unsigned long long v = k < n ? sizes[k] : 0ull;
        unsigned long long sum;
        const unsigned long long ex = wave_excl_scan_u64(v, &sum);
        if (k < n) offs[k] = base + ex;
        base += sum;
        zeros += (unsigned long long)__popcll(ballot64(k < n && v == 0ull));
    }
    if (threadIdx.x == 0) { total[0] = base; total[1] = zeros; }
}

}  // namespace

int ts_k_launch_bgzf_deflate(const void *plain, unsigned long long n, uint32_t payload_bytes, uint32_t n_members, void *slots,
                             uint32_t stride, uint32_t *sizes, unsigned long long *offs, unsigned long long *total, void *stream) {
    if (n_members == 0) return 0;
    if (payload_bytes == 0 || payload_bytes > tsdef::kMaxBlock || payload_bytes + 5u + 28u > stride) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(ts_bgzf_deflate_kernel, dim3(n_members), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)plain, n,
                       payload_bytes, n_members, (unsigned char *)slots, stride, sizes);
    hipLaunchKernelGGL(ts_deflate_offsets_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint32_t *)sizes, n_members, offs,
                       total);
    return (int)hipGetLastError();
}

int ts_k_launch_deflate_pack(const void *slots, uint32_t stride, const uint32_t *sizes, const unsigned long long *offs,
                             uint32_t n_members, unsigned long long cap, void *packed, void *stream) {
    if (n_members == 0) return 0;
    hipLaunchKernelGGL(ts_deflate_pack_kernel, dim3(n_members), dim3(64), 0, (hipStream_t)stream, (const unsigned char *)slots, stride,
                       sizes, offs, n_members, cap, (unsigned char *)packed);
    return (int)hipGetLastError();
}
