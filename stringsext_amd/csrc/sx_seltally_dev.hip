// sx_seltally_dev.hip — the keyword tally over a segment in HBM (sx_result_tally_device): seltally_kernel walks the set's automaton
// (sx_seltally_build.hpp) over the strings of 64 consecutive records per wavefront, a record per lane, every string to its end, and
// counts every keyword that ends at a step (sx_seltally_core.hpp).  As in selset_match_kernel the class map and the rows of the first
// lds_states states are copied into LDS once per workgroup, so a workgroup takes many wavefronts' worth of records: the grid is as
// large as the device holds at once and strides over the segment.  Next to the rows lie the workgroup's counters of the unique ids
// below lds_ids, flushed into hits[] when its wavefronts are done.  LDS per workgroup: 256 + 32 KiB + 16 KiB = 49 408 bytes.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"

#define SXD __device__ __forceinline__
#include "sx_seltally_build.hpp"
#include "sx_seltally_core.hpp"

namespace sx {

constexpr uint32_t kSeltallyWaves = 8;          // wavefronts per workgroup, which share the rows and the counters in LDS
constexpr uint32_t kSeltallyGroupsPerCu = 3;    // 3 x 49 408 bytes <= 160 KiB; 24 wavefronts per CU

struct alignas(16) Seltally16 { uint32_t w[4]; };

// wavefronts [0, waves): waves = ceil(n / 64)
template <class E>
__global__ __launch_bounds__(64 * kSeltallyWaves) void seltally_kernel(SeltallyParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Seltally16 rows16[kSeltallyLdsBytes / 16];
    __shared__ uint32_t counts[kSeltallyLdsIds];
    if (threadIdx.x < 256 / 4) ((uint32_t*)map)[threadIdx.x] = ((const uint32_t*)P.set.map)[threadIdx.x];
    // (the table's allocation is a multiple of 16 bytes)
    const uint32_t chunks = (P.set.lds_states * P.set.classes * (uint32_t)sizeof(E) + 15u) / 16u;
    for (uint32_t c = threadIdx.x; c < chunks; c += 64 * kSeltallyWaves) rows16[c] = ((const Seltally16*)P.set.next)[c];
    for (uint32_t c = threadIdx.x; c < P.set.lds_ids; c += 64 * kSeltallyWaves) counts[c] = 0;
    __syncthreads();
    const E* rows = (const E*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kSeltallyWaves + wv; w < waves; w += (uint64_t)gridDim.x * kSeltallyWaves) {
        SeltallyLane L = seltally_begin_lane(P, w, lane);
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) seltally_step_lane<E>(P, map, rows, counts, L);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < P.set.lds_ids; c += 64 * kSeltallyWaves) seltally_flush_lane(P, counts, c);
}

// The tally of one segment: P = the segment, its first record's ordinal and the set.
hipError_t seltally_launch(const SeltallyParams& P, hipStream_t stream) {
    const SeltallyDevice& set = P.set;
    if (set.entry_bytes != 2 && set.entry_bytes != 4) return hipErrorInvalidValue;
    if ((uint64_t)set.lds_states * set.classes * set.entry_bytes > kSeltallyLdsBytes || set.lds_states > set.states) return hipErrorInvalidValue;
    if (set.lds_ids > kSeltallyLdsIds || set.lds_ids > set.unique) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    const uint64_t groups = (waves + kSeltallyWaves - 1) / kSeltallyWaves, most = (uint64_t)(cus > 0 ? cus : 1) * kSeltallyGroupsPerCu;
    const dim3 grid((unsigned)(groups < most ? groups : most)), block(64 * kSeltallyWaves);
    if (set.entry_bytes == 2) hipLaunchKernelGGL(seltally_kernel<uint16_t>, grid, block, 0, stream, P, waves);
    else hipLaunchKernelGGL(seltally_kernel<uint32_t>, grid, block, 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
