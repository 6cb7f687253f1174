// sx_extract_dev.hip — the regex matches of a segment's findings, cut out where they lie (sx_result_extract_regex_device): two kernels
// around the small scans (sx_extract_core.hpp).  extract_count_kernel walks the set's anchored DFA (sx_extract_build.hpp) over the
// strings of 64 consecutive records per wavefront, a record per lane, and leaves every record's number of matches and per wavefront
// their sum and the matches' bytes; exclusive scans over the wavefronts' words say where every wavefront's matches go and how large
// the output is; extract_place_kernel repeats the walk and writes one output record per match — one source record yields any
// number of them — with the address of its bytes, and order_part_strings (sx_result_dev.hip) lays the strings back to back in
// record order.  Both kernels have selre_match_kernel's shape: 8 wavefronts share the class map and the rows of the first
// lds_states states in LDS, and the grid is as large as the device holds at once and strides over the segment.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_extract_build.hpp"
#include "sx_extract_core.hpp"

namespace sx {

// wavefronts [0, waves]: the last one (behind the last record) has no match, so that the scans' last words are the segment's totals
__global__ __launch_bounds__(64 * kRowsWaves) void extract_count_kernel(ExtractParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Rows16 rows16[kSelsetLdsBytes / 16];
    rows_load(P.ex.map, P.ex.next, P.ex.lds_states, P.ex.classes, 2u, map, rows16);
    const uint16_t* rows = (const uint16_t*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w <= waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        ExtractLane L = extract_begin_lane(P, w, lane);
        uint32_t count = 0;
        uint64_t bytes = 0;
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) {
                uint32_t from;
                const uint32_t end = extract_step_lane(P, map, rows, L, &from);
                if (end) { count++; bytes += end - from; }
            }
        const uint64_t i = w * kSelectRecs + lane;
        if (i < P.n) P.rcount[i] = count;
        const uint64_t sum = wave_sum(count);
        bytes = wave_sum(bytes);
        if (lane == 0) { P.wcount[w] = sum; P.wbytes[w] = bytes; }
    }
}

__global__ __launch_bounds__(64 * kRowsWaves) void extract_place_kernel(ExtractParams P, uint64_t waves) {
    __shared__ uint8_t map[256];
    __shared__ Rows16 rows16[kSelsetLdsBytes / 16];
    rows_load(P.ex.map, P.ex.next, P.ex.lds_states, P.ex.classes, 2u, map, rows16);
    const uint16_t* rows = (const uint16_t*)rows16;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        const uint64_t i = w * kSelectRecs + lane;
        // the lane's base: the wavefront's, plus the matches of the wavefront's earlier records
        const uint32_t own = i < P.n ? P.rcount[i] : 0u;
        const uint64_t before = wave_prefix(own, lane);
        uint64_t rank = P.wbase[w] + before - own;
        const uint64_t rank_end = rank + own;
        ExtractLane L = extract_begin_lane(P, w, lane);
        if (!own) L.active = 0;
        while (__ballot(L.active ? 1 : 0) != 0)
            if (L.active) {
                uint32_t from;
                const uint32_t end = extract_step_lane(P, map, rows, L, &from);
                if (end) {
                    extract_place_match(P, i, rank, from, end);
                    if (++rank == rank_end) L.active = 0;      // (the record's last match: nothing behind it counts)
                }
            }
    }
}

static size_t extract_scan_bytes(uint64_t items) {
    size_t a = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)items, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return a;
}
// a segment of n records: rcount (4 bytes per record), wcount, wbytes and their scans (8 bytes per wavefront each), then the scans' own scratch
size_t extract_scratch_bytes(uint64_t n) {
    const uint64_t waves = (n + kSelectRecs - 1) / kSelectRecs;
    return up256((size_t)n * 4) + 4 * up256((size_t)(waves + 1) * 8) + up256(extract_scan_bytes(waves + 1)) + 256;
}

static hipError_t extract_check(const ExtractDevice& ex) {
    const hipError_t e = rows_check(ex.classes, ex.states, ex.lds_states, 2u, kSelsetLdsBytes);
    if (e != hipSuccess) return e;
    if (ex.states < 1 || ex.states > SX_SELECT_REGEX_MAX_STATES) return hipErrorInvalidValue;
    if (ex.end_first > ex.here_first || ex.here_first > ex.dead_first || ex.dead_first > ex.states) return hipErrorInvalidValue;
    if (ex.start0 >= ex.states || ex.start1 >= ex.states) return hipErrorInvalidValue;
    return hipSuccess;
}

// Pass 1 of a segment (P.wbase, P.out_recs, P.out_src are not read): fills P.rcount / wcount / wbytes / wbase with places inside
// `scratch`; *count and *bytes: the device words that will hold the number of matches and their bytes, valid when `stream` has run
// this far.
hipError_t extract_measure(ExtractParams* P, void* scratch, size_t scratch_bytes, hipStream_t stream, const uint64_t** count, const uint64_t** bytes) {
    if (P->n == 0 || P->n >= 0xFFFFFFFFull || scratch_bytes < extract_scratch_bytes(P->n) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    hipError_t e = extract_check(P->ex);
    if (e != hipSuccess) return e;
    const uint64_t waves = (P->n + kSelectRecs - 1) / kSelectRecs;
    const size_t w8 = up256((size_t)(waves + 1) * 8);
    uint8_t* at = (uint8_t*)scratch;
    P->rcount = (uint32_t*)at; at += up256((size_t)P->n * 4);
    P->wcount = (uint64_t*)at; at += w8;
    P->wbytes = (uint64_t*)at; at += w8;
    uint64_t* wbase = (uint64_t*)at; at += w8;
    uint64_t* bsum = (uint64_t*)at; at += w8;
    size_t tmp_bytes = scratch_bytes - (size_t)(at - (uint8_t*)scratch);
    dim3 grid;
    e = rows_grid(waves + 1, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(extract_count_kernel, grid, dim3(64 * kRowsWaves), 0, stream, *P, waves);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(at, tmp_bytes, (const uint64_t*)P->wcount, wbase, (uint64_t)0, (size_t)(waves + 1), rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(at, tmp_bytes, (const uint64_t*)P->wbytes, bsum, (uint64_t)0, (size_t)(waves + 1), rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    P->wbase = wbase;
    *count = wbase + waves;
    *bytes = bsum + waves;
    return hipSuccess;
}

// the sources of n_out output records, then what order_part_strings needs for them
size_t extract_place_scratch_bytes(uint64_t n_out) { return up256((size_t)n_out * 8) + order_strings_scratch_bytes(n_out); }

// Pass 2: the segment's n_out matches as records to out_recs and their bytes, back to back, to out_arena (P from extract_measure).
hipError_t extract_place(const ExtractParams& P0, void* out_recs, uint64_t n_out, uint8_t* out_arena, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (n_out == 0) return hipSuccess;
    if (n_out >= 0xFFFFFFFFull || scratch_bytes < extract_place_scratch_bytes(n_out) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    ExtractParams P = P0;
    P.out_recs = out_recs;
    P.out_src = (uint64_t*)scratch;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    hipError_t e = rows_grid(waves, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(extract_place_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t src_bytes = up256((size_t)n_out * 8);
    return order_part_strings(out_recs, n_out, (int)P.packed, P.out_src, out_arena, (uint8_t*)scratch + src_bytes, scratch_bytes - src_bytes, stream);
}

}  // namespace sx
