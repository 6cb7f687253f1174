// sx_label_dev.hip — the labels of a segment in HBM (sx_result_label_device) and pass 1 of the selection by label
// (sx_result_select_labels_device).  label_match_kernel has selre_match_kernel's shape: it walks the set's DFA (sx_label_build.hpp)
// over the strings of 64 consecutive records per wavefront, a record per lane (sx_label_core.hpp); the class map and the rows of the
// first lds_states states are copied into LDS once per workgroup, and the grid is as large as the device holds at once and strides
// over the segment.  It writes a 64-bit label per record and counts, per pattern, the records that have its bit and the first of
// them: the lanes' labels are ORed across the wavefront, and for every bit of that lane p takes the ballot of bit p into the
// workgroup's counters in LDS, which are flushed when the workgroup ends.  LDS per workgroup: 256 + 48 KiB + 768 = 50 176 bytes.
// label_pick_kernel reads the labels and the records' lengths, no string byte, and leaves what select_match_kernel leaves;
// select_measure (sx_select_dev.hip) launches it in select_match_kernel's place.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_label_build.hpp"
#include "sx_label_core.hpp"

namespace sx {

constexpr uint32_t kLabelPickWaves = 4;      // wavefronts per workgroup of the pick: they share nothing

// wavefronts [0, waves): waves = ceil(n / 64)
__global__ __launch_bounds__(64 * kRowsWaves) void label_match_kernel(LabelParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Rows16 rows16[kSelsetLdsBytes / 16];
    __shared__ uint32_t counts[kLabelBits];
    __shared__ uint64_t mins[kLabelBits];
    if (threadIdx.x < kLabelBits) { counts[threadIdx.x] = 0; mins[threadIdx.x] = ~(uint64_t)0; }
    rows_load(P.set.map, P.set.next, P.set.lds_states, P.set.classes, 2u, map, rows16);
    const uint16_t* rows = (const uint16_t*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        LabelLane L = label_begin_lane(P, w, lane);
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) label_step_lane(P, map, rows, L);
        const uint64_t i = w * kSelectRecs + lane;
        if (i < P.n) P.labels[i] = L.acc;
        uint64_t any = L.acc;
#pragma unroll
        for (int d = 32; d; d >>= 1) any |= __shfl_xor(any, d, 64);
        // (the same in every lane: as scalars, so that the loop is the wavefront's)
        any = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)any) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(any >> 32)) << 32;
        for (uint64_t m = any; m; m &= m - 1u) {
            const uint32_t p = (uint32_t)__builtin_ctzll(m);
            const uint64_t b = __ballot((L.acc >> p) & 1u ? 1 : 0);
            if (lane == p) label_count_bit(counts, mins, p, b, P.ordinal + w * kSelectRecs);
        }
    }
    __syncthreads();
    if (threadIdx.x < kLabelBits) label_flush_lane(P, counts, mins, threadIdx.x);
}

// wavefronts [0, waves]: the last one (behind the last record) selects nothing, as in select_match_kernel
__global__ __launch_bounds__(64 * kLabelPickWaves) void label_pick_kernel(SelectParams S, LabelPick K, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * kLabelPickWaves + wv;
    if (w > waves) return;      // (a whole wavefront)
    uint32_t len;
    const bool sel = label_pick_lane(S, K, w, lane, &len);
    wave_store_selected(S.wmask, S.wcount, S.wbytes, w, sel, len);
}

// The labels of one segment: P = the segment, its first record's ordinal, the place of its labels and the set.
hipError_t label_launch(const LabelParams& P, hipStream_t stream) {
    const LabelDevice& set = P.set;
    hipError_t e = rows_check(set.classes, set.states, set.lds_states, 2u, kSelsetLdsBytes);
    if (e != hipSuccess) return e;
    if (set.states < 1 || set.states > SX_SELECT_REGEX_MAX_STATES) return hipErrorInvalidValue;
    if (set.here_first < 1 || set.here_first > set.states || set.n_patterns < 1 || set.n_patterns > kLabelBits) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    if (!P.labels) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    e = rows_grid(waves, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(label_match_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves);
    return hipGetLastError();
}

// Pass 1 of a segment by its labels: S = the segment and the per-wavefront tables of a SelectParams that select_measure has laid out.
hipError_t label_launch_pick(const SelectParams& S, const LabelPick& pick, uint64_t waves, hipStream_t stream) {
    if (!pick.labels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(label_pick_kernel, dim3((unsigned)((waves + 1 + kLabelPickWaves - 1) / kLabelPickWaves)), dim3(64 * kLabelPickWaves), 0, stream, S, pick, waves);
    return hipGetLastError();
}

}  // namespace sx
