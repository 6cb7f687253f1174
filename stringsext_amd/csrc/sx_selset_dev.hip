// sx_selset_dev.hip — pass 1 of the selection by a compiled keyword list (sx_result_select_set_device): selset_match_kernel walks the
// set's automaton (sx_selset_build.hpp) over the strings of 64 consecutive records per wavefront, a record per lane
// (sx_selset_core.hpp), and leaves what select_match_kernel leaves.  The class map and the rows of the first lds_states states are
// copied into LDS once per workgroup, so a workgroup takes many wavefronts' worth of records: the grid is as large as the device
// holds at once and strides over the segment.  select_measure (sx_select_dev.hip) launches it in select_match_kernel's place.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_selset_build.hpp"
#include "sx_selset_core.hpp"

namespace sx {

// wavefronts [0, waves]: the last one (behind the last record) selects nothing, as in select_match_kernel
template <class E>
__global__ __launch_bounds__(64 * kRowsWaves) void selset_match_kernel(SelsetParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Rows16 rows16[kSelsetLdsBytes / 16];
    rows_load(P.set.map, P.set.next, P.set.lds_states, P.set.classes, (uint32_t)sizeof(E), map, rows16);
    const E* rows = (const E*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w <= waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        SelsetLane L = selset_begin_lane(P, w, lane);
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) selset_step_lane<E>(P, map, rows, L);
        const bool sel = selset_lane_selected(P, w, lane, L);
        wave_store_selected(P.wmask, P.wcount, P.wbytes, w, sel, L.len);
    }
}

// Pass 1 of a segment with a set: S = the segment and the per-wavefront tables of a SelectParams that select_measure has laid out.
hipError_t selset_launch_match(const SelectParams& S, const SelsetDevice& set, uint64_t waves, hipStream_t stream) {
    hipError_t e = rows_check(set.classes, set.states, set.lds_states, set.entry_bytes, kSelsetLdsBytes);
    if (e != hipSuccess) return e;
    dim3 grid;
    e = rows_grid(waves + 1, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    SelsetParams P{};
    P.recs = S.recs; P.arena = S.arena; P.n = S.n; P.packed = S.packed; P.invert = S.pat.invert;
    P.wmask = S.wmask; P.wcount = S.wcount; P.wbytes = S.wbytes;
    P.set = set;
    const dim3 block(64 * kRowsWaves);
    if (set.entry_bytes == 2) hipLaunchKernelGGL(selset_match_kernel<uint16_t>, grid, block, 0, stream, P, waves);
    else hipLaunchKernelGGL(selset_match_kernel<uint32_t>, grid, block, 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
