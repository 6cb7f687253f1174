// sx_seen_merge_dev.hip — a set's entries into a seen set (sx_seen_set_merge, _grow, _import, _add_strings): the two kernels that
// sx_seen_merge_core.hpp describes, 64 consecutive source words per wavefront, a word per lane, the grid as large as the device holds
// at once and striding over the source.  seen_merge_mark_kernel looks every occupied word's entry up in the destination, writes the
// ballot "held" per wavefront and sums five totals, one add per wavefront and total; seen_merge_add_kernel — behind the host's look at
// the cursors and the totals — copies the entries the destination did not hold into it: one add to the byte cursor per wavefront and
// trip, a trip being kSeenMergeAddChunks chunks of 64 words, the entry copied by its lane eight bytes at a time, and a compare-and-swap
// into the first empty slot.  No LDS, no barrier, and no lane waits for another.  The set and its walks are sx_seen_core.hpp's, the
// lane functions sx_seen_merge_core.hpp's, the wavefront's sum and reserve sx_rows_dev.hpp's; this file owns the two kernels and
// their launcher.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_seen_merge_core.hpp"

namespace sx {

constexpr uint32_t kSeenMergeGroupsPerCu = 4;      // 4 x kRowsWaves = 32 wavefronts per CU: the kernels hold nothing in LDS

// wavefronts [0, waves): waves = ceil(n / 64)
__global__ __launch_bounds__(64 * kRowsWaves) void seen_merge_mark_kernel(SeenMergeParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t occupied = 0, held = 0, lost = 0, fresh_bytes = 0;          // (the first three: the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        bool occ, had, gone;
        uint64_t bytes;
        seen_merge_mark_lane(P, w, lane, &occ, &had, &bytes, &gone);
        const uint64_t had_mask = __ballot(had ? 1 : 0);
        if (lane == 0) P.held[w] = had_mask;
        occupied += (uint64_t)__popcll(__ballot(occ ? 1 : 0));
        held += (uint64_t)__popcll(had_mask);
        lost += (uint64_t)__popcll(__ballot(gone ? 1 : 0));
        fresh_bytes += bytes;
    }
    fresh_bytes = wave_sum(fresh_bytes);
    if (lane != 0) return;
    if (occupied) seltally_add64(P.totals + kSeenMergeOccupied, occupied);
    if (held) seltally_add64(P.totals + kSeenMergeHeld, held);
    if (occupied - held) seltally_add64(P.totals + kSeenMergeNew, occupied - held);
    if (fresh_bytes) seltally_add64(P.totals + kSeenMergeNewBytes, fresh_bytes);
    if (lost) seltally_add64(P.totals + kSeenMergeError, lost);
}

// batches [0, batches): batches = ceil(ceil(n / 64) / kSeenMergeAddChunks).  A wavefront's trip is a batch — kSeenMergeAddChunks
// chunks of 64 words, a word of every chunk per lane —, so that the byte cursor, ONE address for the whole grid, is added to once
// per 64 x kSeenMergeAddChunks words; the string cursor is added to once per wavefront, behind its last trip.
__global__ __launch_bounds__(64 * kRowsWaves) void seen_merge_add_kernel(SeenMergeParams P, uint64_t batches) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t lost = 0, added = 0;                                         // (this lane's)
    for (uint64_t b = (uint64_t)blockIdx.x * kRowsWaves + wv; b < batches; b += (uint64_t)gridDim.x * kRowsWaves) {
        uint64_t bytes = 0;
#pragma unroll
        for (uint32_t k = 0; k < kSeenMergeAddChunks; k++) bytes += seen_merge_add_size_lane(P, b * kSeenMergeAddChunks + k, lane);
        if (!__ballot(bytes ? 1 : 0)) continue;                           // (the same in every lane)
        uint64_t at = wave_reserve(P.set.cursors + 1, bytes, lane);       // this lane's entries lie one behind the other
        for (uint32_t k = 0; k < kSeenMergeAddChunks; k++) {
            const uint64_t w = b * kSeenMergeAddChunks + k, size = seen_merge_add_size_lane(P, w, lane);
            if (!size) continue;
            if (!seen_merge_add_lane(P, w, lane, at)) lost++;
            at += size; added++;
        }
    }
    added = wave_sum(added); lost = wave_sum(lost);
    if (lane == 0 && added) seltally_add64(P.set.cursors, added);
    if (lane == 0 && lost) seltally_add64(P.totals + kSeenMergeError, lost);
}

// One pass over one source: P = the source, held[], the call's totals and the destination (phase: SeenPhase)
hipError_t seen_merge_launch(const SeenMergeParams& P, int phase, hipStream_t stream) {
    if (!seen_set_ok(P.set) || !P.totals) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    if (!P.words || !P.src_arena || !P.held || ((uintptr_t)P.src_arena & 7u)) return hipErrorInvalidValue;
    if (phase != kSeenMark && phase != kSeenAdd) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs, batches = (waves + kSeenMergeAddChunks - 1) / kSeenMergeAddChunks;
    dim3 grid;
    const hipError_t e = rows_grid(phase == kSeenMark ? waves : batches, kRowsWaves, kSeenMergeGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    if (phase == kSeenMark) hipLaunchKernelGGL(seen_merge_mark_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves);
    else hipLaunchKernelGGL(seen_merge_add_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, batches);
    return hipGetLastError();
}

}  // namespace sx
