// sx_selset_dev.hip — pass 1 of the selection by a compiled keyword list (sx_result_select_set_device): selset_match_kernel walks the
// set's automaton (sx_selset_build.hpp) over the strings of 64 consecutive records per wavefront, a record per lane
// (sx_selset_core.hpp), and leaves what select_match_kernel leaves.  The class map and the rows of the first lds_states states are
// copied into LDS once per workgroup, so a workgroup takes many wavefronts' worth of records: the grid is as large as the device
// holds at once and strides over the segment.  select_measure (sx_select_dev.hip) launches it in select_match_kernel's place.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"

#define SXD __device__ __forceinline__
#include "sx_selset_build.hpp"
#include "sx_selset_core.hpp"

namespace sx {

constexpr uint32_t kSelsetWaves = 8;          // wavefronts per workgroup, which share the rows in LDS
constexpr uint32_t kSelsetGroupsPerCu = 3;    // 3 x (48 KiB of rows + the map) <= 160 KiB; 24 wavefronts per CU

struct alignas(16) Selset16 { uint32_t w[4]; };

// wavefronts [0, waves]: the last one (behind the last record) selects nothing, as in select_match_kernel
template <class E>
__global__ __launch_bounds__(64 * kSelsetWaves) void selset_match_kernel(SelsetParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Selset16 rows16[kSelsetLdsBytes / 16];
    if (threadIdx.x < 256 / 4) ((uint32_t*)map)[threadIdx.x] = ((const uint32_t*)P.set.map)[threadIdx.x];
    // (the table's allocation is a multiple of 16 bytes)
    const uint32_t chunks = (P.set.lds_states * P.set.classes * (uint32_t)sizeof(E) + 15u) / 16u;
    for (uint32_t c = threadIdx.x; c < chunks; c += 64 * kSelsetWaves) rows16[c] = ((const Selset16*)P.set.next)[c];
    __syncthreads();
    const E* rows = (const E*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kSelsetWaves + wv; w <= waves; w += (uint64_t)gridDim.x * kSelsetWaves) {
        SelsetLane L = selset_begin_lane(P, w, lane);
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) selset_step_lane<E>(P, map, rows, L);
        const bool sel = selset_lane_selected(P, w, lane, L);
        const uint64_t mask = __ballot(sel ? 1 : 0);
        uint64_t bytes = sel ? L.len : 0u;
#pragma unroll
        for (int d = 32; d; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
        if (lane == 0) { P.wmask[w] = mask; P.wcount[w] = (uint32_t)__popcll(mask); P.wbytes[w] = bytes; }
    }
}

// Pass 1 of a segment with a set: S = the segment and the per-wavefront tables of a SelectParams that select_measure has laid out.
hipError_t selset_launch_match(const SelectParams& S, const SelsetDevice& set, uint64_t waves, hipStream_t stream) {
    if (set.entry_bytes != 2 && set.entry_bytes != 4) return hipErrorInvalidValue;
    if ((uint64_t)set.lds_states * set.classes * set.entry_bytes > kSelsetLdsBytes || set.lds_states > set.states) return hipErrorInvalidValue;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    SelsetParams P{};
    P.recs = S.recs; P.arena = S.arena; P.n = S.n; P.packed = S.packed; P.invert = S.pat.invert;
    P.wmask = S.wmask; P.wcount = S.wcount; P.wbytes = S.wbytes;
    P.set = set;
    const uint64_t groups = (waves + 1 + kSelsetWaves - 1) / kSelsetWaves, most = (uint64_t)(cus > 0 ? cus : 1) * kSelsetGroupsPerCu;
    const dim3 grid((unsigned)(groups < most ? groups : most)), block(64 * kSelsetWaves);
    if (set.entry_bytes == 2) hipLaunchKernelGGL(selset_match_kernel<uint16_t>, grid, block, 0, stream, P, waves);
    else hipLaunchKernelGGL(selset_match_kernel<uint32_t>, grid, block, 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
