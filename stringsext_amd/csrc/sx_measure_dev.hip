// sx_measure_dev.hip — what a segment's strings look like, where they lie (sx_result_measure_device): the two kernels that
// sx_measure_core.hpp describes.  measure_narrow_kernel walks a segment in the family's shape — 64 consecutive records per wavefront,
// one per lane, the grid as large as the device holds at once and striding —; a lane measures its string if it has at most 255 bytes,
// and the wavefront lists the records of the longer ones behind one cursor (wave_reserve).  measure_wide_kernel takes the list, one
// WAVEFRONT per string.  Both add per wavefront, once, behind its trips, to the call's totals.
//
// The narrow kernel's LDS: per wavefront 64 lanes x 256 one-byte counters = 16 KiB, laid out DWORD-INTERLEAVED — the counter of lane l
// for byte b at block[(b >> 2) * 256 + 4 * l + (b & 3)].  Its dword is (b >> 2) * 64 + l, so its bank is l mod 32 for the byte reads
// and the byte writes alike, whatever b is: the 32 lanes of each half of the wavefront, which is the group an LDS instruction serves
// in one cycle, sit on 32 different banks, and lanes l and l + 32 are never in one group.  No string can make two lanes collide.
// (Lane-major, block[256 * l + b], puts every lane on bank (b >> 2) mod 32: text, whose letters fill seven of those, would serialize
// four- to fivefold; byte-interleaved, block[64 * b + l], leaves a half 16 banks and four lanes to a dword.)  Beside the counters the
// workgroup holds the 1 KiB table of c x LG(c), read with the lane's count: most counts are 1, 2 or 3, one address, a broadcast.
// kMeasureWaves wavefronts share nothing but that table, so there is one barrier, behind its load.
#include <hip/hip_runtime.h>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_measure_core.hpp"

namespace sx {

constexpr uint32_t kMeasureWaves = 3;            // wavefronts per workgroup of the narrow kernel: 3 x 16 KiB of counters + the table = 49 KiB
constexpr uint32_t kMeasureGroupsPerCu = 3;      // 3 x 49 KiB = 147 KiB <= 160 KiB: 9 wavefronts per CU
constexpr uint32_t kMeasureRow = 64 * 4;         // bytes between a lane's counters of b and of b + 4
constexpr uint32_t kMeasureWideGroupsPerCu = 4;  // the wide kernel: kRowsWaves wavefronts with 1 KiB of counters each, and the table

struct MeasureNarrowLds {
    uint32_t clg[256];
    uint32_t block[kMeasureWaves][64 * 256 / 4];
};
struct MeasureWideLds {
    uint32_t clg[256];
    uint32_t cnt[kRowsWaves][256];
};
static_assert(sizeof(MeasureNarrowLds) <= 64 * 1024 && kMeasureGroupsPerCu * sizeof(MeasureNarrowLds) <= 160 * 1024, "kMeasureGroupsPerCu workgroups' counters fit a CU's LDS");
static_assert(kMeasureWideGroupsPerCu * sizeof(MeasureWideLds) <= 160 * 1024, "and the wide kernel's");

__device__ const MeasureClg kMeasureClgDevice = measure_clg_table();

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v |= __shfl_xor(v, d, 64);
    return v;
}

// wavefronts [0, waves): waves = ceil(n / 64)
__global__ __launch_bounds__(64 * kMeasureWaves) void measure_narrow_kernel(MeasureParams P, uint64_t waves) {
    __shared__ MeasureNarrowLds lds;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t c = threadIdx.x; c < 256u; c += 64 * kMeasureWaves) lds.clg[c] = kMeasureClgDevice.v[c];
    for (uint32_t c = lane; c < 64u * 256u / 4u; c += 64u) lds.block[wv][c] = 0;      // (the wavefront's own block: every lane's counters)
    __syncthreads();
    uint8_t* const cnt = (uint8_t*)lds.block[wv] + 4u * lane;
    uint64_t findings = 0, bytes = 0, chars = 0, wide_n = 0, ascii_n = 0;             // (findings, wide_n, ascii_n: the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * kMeasureWaves + wv; w < waves; w += (uint64_t)gridDim.x * kMeasureWaves) {
        uint32_t len, ch;
        bool ascii;
        const bool wide = measure_narrow_lane(P, w, lane, cnt, kMeasureRow, lds.clg, &len, &ch, &ascii);
        const uint64_t listed = __ballot(wide ? 1 : 0);
        if (listed) {      // (the whole wavefront)
            const uint64_t at = wave_reserve(P.cursor, wide ? 1u : 0u, lane);
            if (wide) P.list[at] = (uint32_t)(w * kSelectRecs + lane);
        }
        const uint64_t left = P.n - w * kSelectRecs;
        findings += left < kSelectRecs ? left : kSelectRecs;
        bytes += len; chars += ch;
        wide_n += (uint64_t)__popcll(listed);
        ascii_n += (uint64_t)__popcll(__ballot(ascii ? 1 : 0));
    }
    bytes = wave_sum(bytes);
    chars = wave_sum(chars);
    if (lane == 0) {
        if (findings) atomicAdd((unsigned long long*)&P.totals[kMeasureFindings], (unsigned long long)findings);
        if (bytes) atomicAdd((unsigned long long*)&P.totals[kMeasureBytes], (unsigned long long)bytes);
        if (chars) atomicAdd((unsigned long long*)&P.totals[kMeasureChars], (unsigned long long)chars);
        if (wide_n) atomicAdd((unsigned long long*)&P.totals[kMeasureWide], (unsigned long long)wide_n);
        if (ascii_n) atomicAdd((unsigned long long*)&P.totals[kMeasureAscii], (unsigned long long)ascii_n);
    }
}

// the list's strings, a wavefront each: *P.cursor of them, which the narrow kernel in front has counted
__global__ __launch_bounds__(64 * kRowsWaves) void measure_wide_kernel(MeasureParams P) {
    __shared__ MeasureWideLds lds;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t c = threadIdx.x; c < 256u; c += 64 * kRowsWaves) lds.clg[c] = kMeasureClgDevice.v[c];
    uint32_t* const cnt32 = lds.cnt[wv];
    for (uint32_t k = 0; k < 4u; k++) cnt32[4u * lane + k] = 0;
    __syncthreads();
    const uint64_t listed = *P.cursor < P.n ? *P.cursor : P.n;
    uint64_t chars = 0, ascii_n = 0;                                                  // (the same in every lane)
    for (uint64_t j = (uint64_t)blockIdx.x * kRowsWaves + wv; j < listed; j += (uint64_t)gridDim.x * kRowsWaves) {
        const uint64_t i = P.list[j];
        if (i >= P.n) continue;      // (the whole wavefront)
        uint64_t off;
        uint32_t len;
        select_string(P, i, &off, &len);
        MeasureAcc a{ 0, 0 };
        measure_wide_count_lane(P.arena + off, len, lane, cnt32, &a);
        // every lane's adds, then every lane's reads: one wavefront, which runs in step — what is left is the order of its LDS traffic
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint64_t sum = 0;
        uint32_t distinct = 0;
        measure_wide_finish_lane(cnt32, lane, lds.clg, &sum, &distinct);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        sum = wave_sum(sum);
        a.classes = wave_or(a.classes);
        a.chars = (uint32_t)wave_sum(a.chars);
        distinct = (uint32_t)wave_sum(distinct);
        const uint64_t word = measure_finish(lds.clg, len, sum, distinct, a);
        if (lane == 0) P.labels[i] = word;
        chars += a.chars;
        if (!(word & SX_MEASURE_HIGH)) ascii_n++;
    }
    if (lane == 0) {
        if (chars) atomicAdd((unsigned long long*)&P.totals[kMeasureChars], (unsigned long long)chars);
        if (ascii_n) atomicAdd((unsigned long long*)&P.totals[kMeasureAscii], (unsigned long long)ascii_n);
    }
}

// One segment: the narrow kernel, then the wide kernel over what it listed (P.cursor is zeroed here, in the stream's order).  Only
// P.labels, P.list, P.cursor and P.totals are written, and they are valid once `stream` has got there.
hipError_t measure_launch(const MeasureParams& P, hipStream_t stream) {
    if (!P.totals || !P.cursor) return hipErrorInvalidValue;
    if (P.n == 0) return hipSuccess;
    if (!P.recs || !P.arena || !P.labels || !P.list || P.n >> 32) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(P.cursor, 0, sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    e = rows_grid(waves, kMeasureWaves, kMeasureGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(measure_narrow_kernel, grid, dim3(64 * kMeasureWaves), 0, stream, P, waves);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (how many strings are wide, only the device knows: a grid for all of them, whose wavefronts find the list shorter)
    e = rows_grid(P.n, kRowsWaves, kMeasureWideGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(measure_wide_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P);
    return hipGetLastError();
}

}  // namespace sx
