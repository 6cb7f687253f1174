// sx_seltally_dev.hip — the keyword tally over a segment in HBM (sx_result_tally_device): seltally_kernel walks the set's automaton
// (sx_seltally_build.hpp) over the strings of 64 consecutive records per wavefront, a record per lane, every string to its end, and
// counts every keyword that ends at a step (sx_seltally_core.hpp).  As in selset_match_kernel the class map and the rows of the first
// lds_states states are copied into LDS once per workgroup, so a workgroup takes many wavefronts' worth of records: the grid is as
// large as the device holds at once and strides over the segment.  Next to the rows lie the workgroup's counters of the unique ids
// below lds_ids, flushed into hits[] when its wavefronts are done.  LDS per workgroup: 256 + 32 KiB + 16 KiB = 49 408 bytes.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_seltally_build.hpp"
#include "sx_seltally_core.hpp"

namespace sx {

// wavefronts [0, waves): waves = ceil(n / 64)
template <class E>
__global__ __launch_bounds__(64 * kRowsWaves) void seltally_kernel(SeltallyParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Rows16 rows16[kSeltallyLdsBytes / 16];
    __shared__ uint32_t counts[kSeltallyLdsIds];
    for (uint32_t c = threadIdx.x; c < P.set.lds_ids; c += 64 * kRowsWaves) counts[c] = 0;
    rows_load(P.set.map, P.set.next, P.set.lds_states, P.set.classes, (uint32_t)sizeof(E), map, rows16);
    const E* rows = (const E*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        SeltallyLane L = seltally_begin_lane(P, w, lane);
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) seltally_step_lane<E>(P, map, rows, counts, L);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < P.set.lds_ids; c += 64 * kRowsWaves) seltally_flush_lane(P, counts, c);
}

// The tally of one segment: P = the segment, its first record's ordinal and the set.
hipError_t seltally_launch(const SeltallyParams& P, hipStream_t stream) {
    const SeltallyDevice& set = P.set;
    hipError_t e = rows_check(set.classes, set.states, set.lds_states, set.entry_bytes, kSeltallyLdsBytes);
    if (e != hipSuccess) return e;
    if (set.lds_ids > kSeltallyLdsIds || set.lds_ids > set.unique) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    e = rows_grid(waves, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    const dim3 block(64 * kRowsWaves);
    if (set.entry_bytes == 2) hipLaunchKernelGGL(seltally_kernel<uint16_t>, grid, block, 0, stream, P, waves);
    else hipLaunchKernelGGL(seltally_kernel<uint32_t>, grid, block, 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
