// sx_selre_dev.hip — pass 1 of the selection by compiled regular expressions (sx_result_select_regex_device): selre_match_kernel
// walks the set's DFA (sx_selre_build.hpp) over the strings of 64 consecutive records per wavefront, a record per lane
// (sx_selre_core.hpp), and leaves what select_match_kernel leaves.  As in selset_match_kernel the class map and the rows of the first
// lds_states states are copied into LDS once per workgroup, and the grid is as large as the device holds at once and strides over
// the segment.  What the keyword automaton never had to do is in the lane functions: a lane stops at `dead` as well as at
// `matched`, the end of the string asks whether the state accepts there, and an empty string is decided by the root.
// select_measure (sx_select_dev.hip) launches it in select_match_kernel's place.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_selre_build.hpp"
#include "sx_selre_core.hpp"

namespace sx {

// wavefronts [0, waves]: the last one (behind the last record) selects nothing, as in select_match_kernel
__global__ __launch_bounds__(64 * kRowsWaves) void selre_match_kernel(SelreParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Rows16 rows16[kSelsetLdsBytes / 16];
    rows_load(P.re.map, P.re.next, P.re.lds_states, P.re.classes, 2u, map, rows16);
    const uint16_t* rows = (const uint16_t*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w <= waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        SelreLane L = selre_begin_lane(P, w, lane);
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) selre_step_lane(P, map, rows, L);
        const bool sel = selre_lane_selected(P, w, lane, L);
        wave_store_selected(P.wmask, P.wcount, P.wbytes, w, sel, L.len);
    }
}

// Pass 1 of a segment with a regex set: S = the segment and the per-wavefront tables of a SelectParams that select_measure has laid out.
hipError_t selre_launch_match(const SelectParams& S, const SelreDevice& re, uint64_t waves, hipStream_t stream) {
    hipError_t e = rows_check(re.classes, re.states, re.lds_states, 2u, kSelsetLdsBytes);
    if (e != hipSuccess) return e;
    if (re.states < 1 || re.states > SX_SELECT_REGEX_MAX_STATES) return hipErrorInvalidValue;
    if (re.end_first > re.stop_first || re.stop_first > re.states) return hipErrorInvalidValue;
    dim3 grid;
    e = rows_grid(waves + 1, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    SelreParams P{};
    P.recs = S.recs; P.arena = S.arena; P.n = S.n; P.packed = S.packed; P.invert = S.pat.invert;
    P.wmask = S.wmask; P.wcount = S.wcount; P.wbytes = S.wbytes;
    P.re = re;
    const dim3 block(64 * kRowsWaves);
    hipLaunchKernelGGL(selre_match_kernel, grid, block, 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
