// sx_selre_dev.hip — pass 1 of the selection by compiled regular expressions (sx_result_select_regex_device): selre_match_kernel
// walks the set's DFA (sx_selre_build.hpp) over the strings of 64 consecutive records per wavefront, a record per lane
// (sx_selre_core.hpp), and leaves what select_match_kernel leaves.  As in selset_match_kernel the class map and the rows of the first
// lds_states states are copied into LDS once per workgroup, and the grid is as large as the device holds at once and strides over
// the segment.  What the keyword automaton never had to do is in the lane functions: a lane stops at `dead` as well as at
// `matched`, the end of the string asks whether the state accepts there, and an empty string is decided by the root.
// select_measure (sx_select_dev.hip) launches it in select_match_kernel's place.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"

#define SXD __device__ __forceinline__
#include "sx_selre_build.hpp"
#include "sx_selre_core.hpp"

namespace sx {

constexpr uint32_t kSelreWaves = 8;          // wavefronts per workgroup, which share the rows in LDS
constexpr uint32_t kSelreGroupsPerCu = 3;    // 3 x (48 KiB of rows + the map) <= 160 KiB; 24 wavefronts per CU

struct alignas(16) Selre16 { uint32_t w[4]; };

// wavefronts [0, waves]: the last one (behind the last record) selects nothing, as in select_match_kernel
__global__ __launch_bounds__(64 * kSelreWaves) void selre_match_kernel(SelreParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Selre16 rows16[kSelsetLdsBytes / 16];
    if (threadIdx.x < 256 / 4) ((uint32_t*)map)[threadIdx.x] = ((const uint32_t*)P.re.map)[threadIdx.x];
    // (the table's allocation is a multiple of 16 bytes)
    const uint32_t chunks = (P.re.lds_states * P.re.classes * 2u + 15u) / 16u;
    for (uint32_t c = threadIdx.x; c < chunks; c += 64 * kSelreWaves) rows16[c] = ((const Selre16*)P.re.next)[c];
    __syncthreads();
    const uint16_t* rows = (const uint16_t*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kSelreWaves + wv; w <= waves; w += (uint64_t)gridDim.x * kSelreWaves) {
        SelreLane L = selre_begin_lane(P, w, lane);
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) selre_step_lane(P, map, rows, L);
        const bool sel = selre_lane_selected(P, w, lane, L);
        const uint64_t mask = __ballot(sel ? 1 : 0);
        uint64_t bytes = sel ? L.len : 0u;
#pragma unroll
        for (int d = 32; d; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
        if (lane == 0) { P.wmask[w] = mask; P.wcount[w] = (uint32_t)__popcll(mask); P.wbytes[w] = bytes; }
    }
}

// Pass 1 of a segment with a regex set: S = the segment and the per-wavefront tables of a SelectParams that select_measure has laid out.
hipError_t selre_launch_match(const SelectParams& S, const SelreDevice& re, uint64_t waves, hipStream_t stream) {
    if (re.classes < 1 || re.classes > 256 || re.states < 1 || re.states > SX_SELECT_REGEX_MAX_STATES) return hipErrorInvalidValue;
    if ((uint64_t)re.lds_states * re.classes * 2u > kSelsetLdsBytes || re.lds_states > re.states) return hipErrorInvalidValue;
    if (re.end_first > re.stop_first || re.stop_first > re.states) return hipErrorInvalidValue;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    SelreParams P{};
    P.recs = S.recs; P.arena = S.arena; P.n = S.n; P.packed = S.packed; P.invert = S.pat.invert;
    P.wmask = S.wmask; P.wcount = S.wcount; P.wbytes = S.wbytes;
    P.re = re;
    const uint64_t groups = (waves + 1 + kSelreWaves - 1) / kSelreWaves, most = (uint64_t)(cus > 0 ? cus : 1) * kSelreGroupsPerCu;
    const dim3 grid((unsigned)(groups < most ? groups : most)), block(64 * kSelreWaves);
    hipLaunchKernelGGL(selre_match_kernel, grid, block, 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
