// sx_seen_dev.hip — the seen set of device-resident results (sx_result_seen_device): the two kernels that sx_seen_core.hpp describes,
// behind distinct's finalize, a segment per launch, 64 consecutive records per wavefront, a record per lane, the grid as large as the
// device holds at once and striding over the segment.  seen_mark_kernel looks every record's string up in the set, ORs
// SX_DISTINCT_SEEN into its word and sums the ballots, one add per wavefront and total; seen_add_kernel — behind every segment's mark
// and the host's look at the totals — puts the first record of every class the set does not hold into it: one add per wavefront to
// each cursor (wave_reserve, sx_rows_dev.hpp), the entry written by its lane, and a compare-and-swap into the first empty slot; an
// adder that found none is added to the error total.  No LDS, no barrier, and no lane waits for another.  The set, its walks and the
// lane functions are sx_seen_core.hpp's; this file owns the two kernels and their launcher.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_seen_core.hpp"

namespace sx {

constexpr uint32_t kSeenGroupsPerCu = 4;      // 4 x kRowsWaves = 32 wavefronts per CU: the kernels hold nothing in LDS

// wavefronts [0, waves): waves = ceil(n / 64)
__global__ __launch_bounds__(64 * kRowsWaves) void seen_mark_kernel(SeenParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t findings = 0, classes = 0, fresh = 0, fresh_bytes = 0;      // (the first three: the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        bool seen, first;
        uint64_t bytes;
        seen_mark_lane(P, w, lane, &seen, &first, &bytes);
        findings += (uint64_t)__popcll(__ballot(seen ? 1 : 0));
        classes += (uint64_t)__popcll(__ballot(seen && first ? 1 : 0));
        fresh += (uint64_t)__popcll(__ballot(first && !seen ? 1 : 0));
        fresh_bytes += bytes;
    }
    fresh_bytes = wave_sum(fresh_bytes);
    if (lane == 0 && findings) seltally_add64(P.totals + kSeenFindings, findings);
    if (lane == 0 && classes) seltally_add64(P.totals + kSeenClasses, classes);
    if (lane == 0 && fresh) seltally_add64(P.totals + kSeenNewClasses, fresh);
    if (lane == 0 && fresh_bytes) seltally_add64(P.totals + kSeenNewBytes, fresh_bytes);
}

__global__ __launch_bounds__(64 * kRowsWaves) void seen_add_kernel(SeenParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t lost = 0;                                                    // (this lane's)
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        const uint64_t bytes = seen_add_size_lane(P, w, lane);
        const uint64_t adders = __ballot(bytes ? 1 : 0);
        if (!adders) continue;                                            // (the same in every lane)
        const uint64_t at = wave_reserve(P.set.cursors + 1, bytes, lane);
        if (lane == 0) seltally_add64(P.set.cursors, (uint64_t)__popcll(adders));
        if (bytes && !seen_add_lane(P, w, lane, at)) lost++;
    }
    lost = wave_sum(lost);
    if (lane == 0 && lost) seltally_add64(P.totals + kSeenError, lost);
}

// One pass of one segment: P = the segment, its words, the call's totals and the set (phase: SeenPhase)
hipError_t seen_launch(const SeenParams& P, int phase, hipStream_t stream) {
    if (!seen_set_ok(P.set) || !P.totals) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    if (!P.recs || !P.arena || !P.labels) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    const hipError_t e = rows_grid(waves, kRowsWaves, kSeenGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    switch (phase) {
    case kSeenMark: hipLaunchKernelGGL(seen_mark_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves); break;
    case kSeenAdd: hipLaunchKernelGGL(seen_add_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sx
