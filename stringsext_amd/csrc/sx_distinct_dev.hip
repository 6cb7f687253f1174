// sx_distinct_dev.hip — the duplicate strings of a result in HBM (sx_result_distinct_device): the three kernels of the tournament by
// hash that sx_distinct_core.hpp describes, a segment per launch, 64 consecutive records per wavefront, a record per lane, the grid as
// large as the device holds at once and striding over the segment.  distinct_claim_kernel lowers the slots of the round's table to the
// smallest key that hashes there; distinct_resolve_kernel — behind every segment's claim — gives the records that equal their slot's
// winner their class, with one add to the winner's count per run of neighbouring lanes that found it, and counts the others, one add
// per wavefront; distinct_finalize_kernel — behind the last round — writes the words and sums the classes, one add per wavefront and
// total.  No LDS, no barrier, and no wavefront waits for another.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_distinct_core.hpp"

namespace sx {

constexpr uint32_t kDistinctGroupsPerCu = 4;      // 4 x kRowsWaves = 32 wavefronts per CU: the kernels hold nothing in LDS

// wavefronts [0, waves): waves = ceil(n / 64)
__global__ __launch_bounds__(64 * kRowsWaves) void distinct_claim_kernel(DistinctParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) distinct_claim_lane(P, w, lane);
}

__global__ __launch_bounds__(64 * kRowsWaves) void distinct_resolve_kernel(DistinctParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t left = 0;      // (the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        uint64_t widx;
        const uint32_t made = distinct_resolve_lane(P, w, lane, &widx);
        left += (uint64_t)__popcll(__ballot(made == kDistinctStays ? 1 : 0));
        // one add per run of neighbouring lanes that found the same winner
        const uint64_t left_widx = __shfl_up(widx, 1, 64);
        const uint32_t left_made = __shfl_up(made, 1, 64);
        const bool found = made == kDistinctFound, head = found && (lane == 0 || left_made != kDistinctFound || left_widx != widx);
        distinct_count_run(P, lane, __ballot(found ? 1 : 0), __ballot(head ? 1 : 0), widx);
    }
    if (lane == 0 && left) seltally_add64(P.unresolved, left);
}

__global__ __launch_bounds__(64 * kRowsWaves) void distinct_finalize_kernel(DistinctParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t distinct = 0, repeated = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        bool first, again;
        distinct_finalize_lane(P, w, lane, &first, &again);
        distinct += (uint64_t)__popcll(__ballot(first ? 1 : 0));
        repeated += (uint64_t)__popcll(__ballot(again ? 1 : 0));
    }
    if (lane == 0 && distinct) seltally_add64(P.totals, distinct);
    if (lane == 0 && repeated) seltally_add64(P.totals + 1, repeated);
}

// One phase of one segment: P = the segment, the result's segments and the call's tables (phase: DistinctPhase)
hipError_t distinct_launch(const DistinctParams& P, int phase, hipStream_t stream) {
    if (!P.segs || P.seg >= P.n_segs || P.table_log2 > 40 || !P.table || !P.rep || !P.count || !P.unresolved || !P.totals) return hipErrorInvalidValue;
    if (P.n >> 32) return hipErrorInvalidValue;      // (a key's low half is the record)
    if (P.n == 0) return hipSuccess;
    if (phase == kDistinctFinalize && !P.labels) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    const hipError_t e = rows_grid(waves, kRowsWaves, kDistinctGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    switch (phase) {
    case kDistinctClaim: hipLaunchKernelGGL(distinct_claim_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves); break;
    case kDistinctResolve: hipLaunchKernelGGL(distinct_resolve_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves); break;
    case kDistinctFinalize: hipLaunchKernelGGL(distinct_finalize_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sx
