// gather.hip — device-resident pieces (TS_INPUT_DEVICE) into the scan's input layout: ONE launch per upload_pieces call over a
// job list (pipeline.cpp builds it), a wave per job, instead of one device-to-device copy per piece (~3 us each: 400 000 GFA
// segments spent 1.2 s there).  The sibling of ts_fastq_stage_kernel / ts_fastq_gather_kernel (fastq.hip), with one difference:
// those read inside a chunk that has 64 readable bytes behind it, these pieces lie anywhere and nothing behind one may be read.
// What a lane loads and stores is gather_core.h, shared with the host program that checks exactly that.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gather_core.h"
#include "ts_internal.h"

namespace {

// gather_core.h's accessor over global memory: plain loads and vector stores (the addresses arrive as numbers: the address
// space says they are global memory, not LDS or scratch)
#define TS_GLOBAL __attribute__((address_space(1)))
struct DeviceMemory {
    __device__ __forceinline__ uint32_t word(uint64_t a) const { return *(const TS_GLOBAL uint32_t *)a; }
    __device__ __forceinline__ void words4(uint64_t a, uint32_t w[4]) const {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
        const u32x4 v = *(const TS_GLOBAL u32x4 *)a;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ __forceinline__ void store_byte(uint64_t a, uint32_t v) const { *(TS_GLOBAL unsigned char *)a = (unsigned char)v; }
    __device__ __forceinline__ void store16(uint64_t a, const uint32_t v[4]) const {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        *(TS_GLOBAL u32x4 *)a = u32x4{v[0], v[1], v[2], v[3]};
    }
};

__global__ __launch_bounds__(64)
void ts_gather_pieces_kernel(const tsgather::Job *jobs, uint32_t n_jobs, unsigned char *base) {
    if (blockIdx.x >= n_jobs) return;
    const tsgather::Job job = jobs[blockIdx.x];
    if (job.n > tsgather::kSliceBytes) return;                   // (the splitter never makes one: no wave's work is unbounded)
    DeviceMemory m;
    tsgather::copy_lane(m, job.src, (uint64_t)(uintptr_t)base + job.dst, job.n, threadIdx.x);
}

}  // namespace

int ts_k_launch_gather_pieces(const void *jobs, uint32_t n_jobs, void *base, void *stream) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ts_gather_pieces_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const tsgather::Job *)jobs, n_jobs,
                       (unsigned char *)base);
    return (int)hipGetLastError();
}
