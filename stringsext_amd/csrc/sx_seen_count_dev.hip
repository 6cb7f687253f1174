// sx_seen_count_dev.hip — a seen set that counts (SX_SEEN_COUNTED), its counts where the findings lie (sx_result_seen_counts_device)
// and the selection by a field of a label word (sx_result_select_labels_range_device): the four kernels that sx_seen_count_core.hpp
// describes.  seen_count_kernel and seen_counts_lookup_kernel walk a segment, seen_merge_count_kernel a source of entries: 64
// consecutive records or words per wavefront, one per lane, the grid as large as the device holds at once and striding.  The two
// count kernels run BEHIND the add pass of their call: a lane looks its string up, gets its slot and adds to the slot's count word
// with a plain load and store — no two lanes of a call have the same string —; per wavefront one add to the counted total and, where
// a lane did not find its string, to the error total.  label_range_pick_kernel is pass 1 of a selection in the shape of
// label_pick_kernel (sx_label_dev.hip).  No LDS, no barrier, and no lane waits for another.  The set and its walks are
// sx_seen_core.hpp's and sx_seen_merge_core.hpp's, the lane functions sx_seen_count_core.hpp's; this file owns the four kernels and
// their launchers.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_seen_count_core.hpp"

namespace sx {

constexpr uint32_t kSeenCountGroupsPerCu = 4;      // 4 x kRowsWaves = 32 wavefronts per CU: the kernels hold nothing in LDS
constexpr uint32_t kLabelRangeWaves = 4;           // wavefronts per workgroup of the pick: they share nothing

// wavefronts [0, waves): waves = ceil(n / 64)
__global__ __launch_bounds__(64 * kRowsWaves) void seen_count_kernel(SeenParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t counted = 0, lost = 0;                                        // (counted: the same in every lane; lost: this lane's)
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        bool did, gone;
        seen_count_lane(P, w, lane, &did, &gone);
        counted += (uint64_t)__popcll(__ballot(did ? 1 : 0));
        if (gone) lost++;
    }
    lost = wave_sum(lost);
    if (lane == 0 && counted) seltally_add64(P.totals + kSeenCounted, counted);
    if (lane == 0 && lost) seltally_add64(P.totals + kSeenError, lost);
}

__global__ __launch_bounds__(64 * kRowsWaves) void seen_merge_count_kernel(SeenMergeCountParams C, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t counted = 0, lost = 0;                                        // (counted: the same in every lane; lost: this lane's)
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        bool did, gone;
        seen_merge_count_lane(C, w, lane, &did, &gone);
        counted += (uint64_t)__popcll(__ballot(did ? 1 : 0));
        if (gone) lost++;
    }
    lost = wave_sum(lost);
    if (lane == 0 && counted) seltally_add64(C.m.totals + kSeenCounted, counted);
    if (lane == 0 && lost) seltally_add64(C.m.totals + kSeenMergeError, lost);
}

__global__ __launch_bounds__(64 * kRowsWaves) void seen_counts_lookup_kernel(SeenParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t lost = 0;                                                     // (the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves)
        lost += (uint64_t)__popcll(__ballot(seen_counts_lookup_lane(P, w, lane) ? 1 : 0));
    if (lane == 0 && lost) seltally_add64(P.totals + kSeenError, lost);
}

// wavefronts [0, waves]: the last one (behind the last record) selects nothing, as in select_match_kernel
__global__ __launch_bounds__(64 * kLabelRangeWaves) void label_range_pick_kernel(SelectParams S, LabelRange K, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * kLabelRangeWaves + wv;
    if (w > waves) return;      // (a whole wavefront)
    uint32_t len;
    const bool sel = label_range_pick_lane(S, K, w, lane, &len);
    wave_store_selected(S.wmask, S.wcount, S.wbytes, w, sel, len);
}

// One pass of one segment behind seen_launch's: kSeenCount = the count pass (the set counts), kSeenCountsLookup = the lookup (P.labels:
// the words it writes)
hipError_t seen_count_launch(const SeenParams& P, int phase, hipStream_t stream) {
    if (!seen_set_ok(P.set) || !P.set.counts || !P.totals) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    if (!P.recs || !P.arena || !P.labels) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    const hipError_t e = rows_grid(waves, kRowsWaves, kSeenCountGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    switch (phase) {
    case kSeenCount: hipLaunchKernelGGL(seen_count_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves); break;
    case kSeenCountsLookup: hipLaunchKernelGGL(seen_counts_lookup_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The count pass over one source, behind seen_merge_launch's add pass
hipError_t seen_merge_count_launch(const SeenMergeCountParams& C, hipStream_t stream) {
    const SeenMergeParams& P = C.m;
    if (!seen_set_ok(P.set) || !P.set.counts || !P.totals) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    if (!P.words || !P.src_arena || ((uintptr_t)P.src_arena & 7u)) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    const hipError_t e = rows_grid(waves, kRowsWaves, kSeenCountGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(seen_merge_count_kernel, grid, dim3(64 * kRowsWaves), 0, stream, C, waves);
    return hipGetLastError();
}

// Pass 1 of a segment by a field of its labels: S = the segment and the per-wavefront tables of a SelectParams that select_measure has laid out
hipError_t label_range_launch_pick(const SelectParams& S, const LabelRange& range, uint64_t waves, hipStream_t stream) {
    if (!range.labels || range.bits < 1 || range.bits > 64 || range.shift > 64 - range.bits) return hipErrorInvalidValue;
    hipLaunchKernelGGL(label_range_pick_kernel, dim3((unsigned)((waves + 1 + kLabelRangeWaves - 1) / kLabelRangeWaves)), dim3(64 * kLabelRangeWaves), 0, stream, S, range, waves);
    return hipGetLastError();
}

}  // namespace sx
