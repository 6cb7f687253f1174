// sx_fuzzy_dev.hip — the approximate matches of a segment in HBM (sx_result_fuzzy_device).  fuzzy_match_kernel has label_match_kernel's
// shape: 64 consecutive records per wavefront, a record per lane, which walks Myers' bit-vector recurrence over its string for the
// set's patterns, a group at a time (sx_fuzzy_core.hpp); the class map and the masks of the first lds_classes classes are copied into
// LDS once per workgroup, and the grid is as large as the device holds at once and strides over the segment.  It writes a 64-bit word
// per record and counts, per pattern, the records that have its bit and the first of them, as label_match_kernel does: the lanes'
// words are ORed across the wavefront, and for every bit of that lane p takes the ballot of bit p into the workgroup's counters in
// LDS, which are flushed when the workgroup ends.  LDS per workgroup: 512 + 48 KiB + 768 = 50 432 bytes, three workgroups to a CU.
// Two instances: 64-bit vectors, and 32-bit ones for sets whose longest pattern has at most 32 bytes.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_fuzzy_build.hpp"
#include "sx_fuzzy_core.hpp"

namespace sx {

// wavefronts [0, waves): waves = ceil(n / 64)
template <class W>
__global__ __launch_bounds__(64 * kRowsWaves) void fuzzy_match_kernel(FuzzyParams P, uint64_t waves) {
    __shared__ uint32_t map32[256 / 2];
    __shared__ Rows16 rows16[kSelsetLdsBytes / 16];
    __shared__ uint32_t counts[kLabelBits];
    __shared__ uint64_t mins[kLabelBits];
    if (threadIdx.x < kLabelBits) { counts[threadIdx.x] = 0; mins[threadIdx.x] = ~(uint64_t)0; }
    // (the table's allocation is a multiple of 16 bytes)
    if (threadIdx.x < 256 / 2) map32[threadIdx.x] = ((const uint32_t*)P.set.map)[threadIdx.x];
    const uint32_t chunks = (P.set.lds_classes * P.set.n_patterns * 8u + 15u) / 16u;
    for (uint32_t c = threadIdx.x; c < chunks; c += 64 * kRowsWaves) rows16[c] = ((const Rows16*)P.set.eq)[c];
    __syncthreads();
    const uint16_t* map = (const uint16_t*)map32;
    const uint64_t* rows = (const uint64_t*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        const uint64_t acc = fuzzy_lane<W>(P, map, rows, w, lane);
        uint64_t any = acc;
#pragma unroll
        for (int d = 32; d; d >>= 1) any |= __shfl_xor(any, d, 64);
        // (the same in every lane: as scalars, so that the loop is the wavefront's)
        any = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)any) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(any >> 32)) << 32;
        for (uint64_t m = any; m; m &= m - 1u) {
            const uint32_t p = (uint32_t)__builtin_ctzll(m);
            const uint64_t b = __ballot((acc >> p) & 1u ? 1 : 0);
            if (lane == p) label_count_bit(counts, mins, p, b, P.ordinal + w * kSelectRecs);
        }
    }
    __syncthreads();
    if (threadIdx.x < kLabelBits) label_flush_lane(P, counts, mins, threadIdx.x);
}

// The words of one segment: P = the segment, its first record's ordinal, the place of its words and the set.
hipError_t fuzzy_launch(const FuzzyParams& P, hipStream_t stream) {
    const FuzzyDevice& set = P.set;
    if (set.n_patterns < 1 || set.n_patterns > kLabelBits || set.classes < 1 || set.classes > 257 || set.lds_classes > set.classes) return hipErrorInvalidValue;
    if ((uint64_t)set.lds_classes * set.n_patterns * 8u > kSelsetLdsBytes || set.max_len < 1 || set.max_len > SX_FUZZY_MAX_PATTERN_BYTES) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    if (!P.labels) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    const hipError_t e = rows_grid(waves, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    if (set.max_len <= 32u) hipLaunchKernelGGL(fuzzy_match_kernel<uint32_t>, grid, dim3(64 * kRowsWaves), 0, stream, P, waves);
    else hipLaunchKernelGGL(fuzzy_match_kernel<uint64_t>, grid, dim3(64 * kRowsWaves), 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
