// sx_fold_dev.hip — a segment's strings folded by Unicode simple case folding where they lie (sx_result_fold_device): two kernels
// around one small scan (sx_fold_core.hpp).  fold_measure_kernel walks the strings of 64 consecutive records per wavefront, a record
// per lane, and leaves every record's folded length, per wavefront their sum, and adds per wavefront to the segment's totals: the
// records whose string changes, the longest folded string, the source's bytes; an exclusive scan over the wavefronts' sums says
// where every wavefront's bytes go and how many the segment has; fold_place_kernel repeats the walk and writes, per record, the
// source record with its new str_off and str_len and the folded bytes, back to back in record order.  Both kernels have
// extract_count_kernel's shape: 8 wavefronts share the table in LDS — kFoldLdsBytes and nothing else, so that kRowsGroupsPerCu
// workgroups fit a CU —, and the grid is as large as the device holds at once and strides over the segment.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#define SX_FOLD_TABLE_DEVICE __device__
#define SX_FOLD_TABLE_NO_PAIRS
#include "sx_fold_core.hpp"

namespace sx {

constexpr uint32_t kFoldLdsBytes = 9952;      // 35 pages of 128 halfwords and the index, 980 bytes: kFoldTableBytes, rounded up to 16
struct FoldLds {
    Rows16 pages16[(kFoldPageCount << kFoldPageShift) * 2 / 16];
    uint32_t index32[kFoldIndexCount / 4];
};
static_assert(sizeof(FoldLds) == kFoldLdsBytes && (kFoldTableBytes + 15) / 16 * 16 == kFoldLdsBytes && kFoldIndexCount % 4 == 0 && (kFoldPageCount << kFoldPageShift) * 2 % 16 == 0,
              "the table as fold_load copies it");
static_assert(kFoldLdsBytes <= 20 * 1024 && kRowsGroupsPerCu * kFoldLdsBytes <= 160 * 1024, "kRowsGroupsPerCu workgroups' tables fit a CU's LDS");

// The table into LDS by the workgroup's 64 * kRowsWaves threads; ends with the workgroup's barrier
__device__ __forceinline__ FoldTable fold_load(FoldLds& lds) {
    for (uint32_t c = threadIdx.x; c < sizeof lds.pages16 / 16; c += 64 * kRowsWaves) lds.pages16[c] = ((const Rows16*)kFoldPages)[c];
    for (uint32_t c = threadIdx.x; c < kFoldIndexCount / 4; c += 64 * kRowsWaves) lds.index32[c] = ((const uint32_t*)kFoldIndex)[c];
    __syncthreads();
    return FoldTable{ (const uint8_t*)lds.index32, (const uint16_t*)lds.pages16 };
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint64_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// wavefronts [0, waves]: the last one (behind the last record) has no byte, so that the scan's last word is the segment's total
__global__ __launch_bounds__(64 * kRowsWaves) void fold_measure_kernel(FoldParams P, uint64_t waves) {
    __shared__ FoldLds lds;
    const FoldTable T = fold_load(lds);
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t n_changed = 0, longest = 0, bytes_in = 0;      // of the wavefront's trips
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w <= waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        uint32_t len;
        bool changed;
        const uint64_t folded = fold_measure_lane(P, T, w, lane, &len, &changed);
        const uint64_t sum = wave_sum(folded);
        n_changed += (uint64_t)__popcll(__ballot(changed ? 1 : 0));
        longest = folded > longest ? folded : longest;
        bytes_in += len;
        if (lane == 0) P.wbytes[w] = sum;
    }
    longest = wave_max(longest);
    bytes_in = wave_sum(bytes_in);
    if (lane == 0) {
        if (n_changed) atomicAdd((unsigned long long*)&P.totals[kFoldChanged], (unsigned long long)n_changed);
        if (longest) atomicMax((unsigned long long*)&P.totals[kFoldLongest], (unsigned long long)longest);
        if (bytes_in) atomicAdd((unsigned long long*)&P.totals[kFoldBytesIn], (unsigned long long)bytes_in);
        if (blockIdx.x == 0 && wv == 0) P.totals[kFoldRecords] = P.n;
    }
}

__global__ __launch_bounds__(64 * kRowsWaves) void fold_place_kernel(FoldParams P, uint64_t waves) {
    __shared__ FoldLds lds;
    const FoldTable T = fold_load(lds);
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        const uint64_t i = w * kSelectRecs + lane;
        // the lane's base: the wavefront's, plus the folded bytes of the wavefront's earlier records
        const uint32_t own = i < P.n ? P.rlen[i] : 0u;
        const uint64_t upto = wave_prefix(own, lane);
        fold_place_lane(P, T, w, lane, P.wbase[w] + upto - own, own);
    }
}

static size_t fold_scan_bytes(uint64_t items) {
    size_t a = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)items, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return a;
}
// a segment of n records: rlen (4 bytes per record), wbytes and its scan (8 bytes per wavefront each), the totals, then the scan's own scratch
size_t fold_scratch_bytes(uint64_t n) {
    const uint64_t waves = (n + kSelectRecs - 1) / kSelectRecs;
    return up256((size_t)n * 4) + 2 * up256((size_t)(waves + 1) * 8) + 256 + up256(fold_scan_bytes(waves + 1)) + 256;
}

// Pass 1 of a segment (P.wbase, P.out_recs, P.out_arena are not read): fills P.rlen / wbytes / totals / wbase with places inside
// `scratch`; *count, *bytes, *totals: the device words that will hold the number of records, the folded bytes and the kFoldTotals
// totals, valid when `stream` has run this far.
hipError_t fold_measure(FoldParams* P, void* scratch, size_t scratch_bytes, hipStream_t stream, const uint64_t** count, const uint64_t** bytes, const uint64_t** totals) {
    if (P->n == 0 || P->n >= 0xFFFFFFFFull || scratch_bytes < fold_scratch_bytes(P->n) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    const uint64_t waves = (P->n + kSelectRecs - 1) / kSelectRecs;
    const size_t w8 = up256((size_t)(waves + 1) * 8);
    uint8_t* at = (uint8_t*)scratch;
    P->rlen = (uint32_t*)at; at += up256((size_t)P->n * 4);
    P->wbytes = (uint64_t*)at; at += w8;
    uint64_t* wbase = (uint64_t*)at; at += w8;
    P->totals = (uint64_t*)at; at += 256;
    size_t tmp_bytes = scratch_bytes - (size_t)(at - (uint8_t*)scratch);
    hipError_t e = hipMemsetAsync(P->totals, 0, kFoldTotals * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    dim3 grid;
    e = rows_grid(waves + 1, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fold_measure_kernel, grid, dim3(64 * kRowsWaves), 0, stream, *P, waves);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(at, tmp_bytes, (const uint64_t*)P->wbytes, wbase, (uint64_t)0, (size_t)(waves + 1), rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    P->wbase = wbase;
    *count = P->totals + kFoldRecords;
    *bytes = wbase + waves;
    *totals = P->totals;
    return hipSuccess;
}

// Pass 2: the segment's records to out_recs and their folded strings, back to back, to out_arena (P from fold_measure; the driver has
// seen that the folded bytes fit str_off and, in a packed segment, the longest folded string str_len).
hipError_t fold_place(const FoldParams& P0, void* out_recs, uint8_t* out_arena, hipStream_t stream) {
    FoldParams P = P0;
    P.out_recs = out_recs;
    P.out_arena = out_arena;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    hipError_t e = rows_grid(waves, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fold_place_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
