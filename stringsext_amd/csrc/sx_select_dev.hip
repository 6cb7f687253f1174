// sx_select_dev.hip — the findings of a segment that lies in HBM (SX_OPT_RESULT_ON_DEVICE), selected by substring without leaving
// it (sx_result_select_device).  Two kernels per segment around one small scan (sx_select_core.hpp): select_match_kernel looks for
// the patterns in the strings of 64 consecutive records per wavefront and leaves the mask of the selected ones, their number and
// their string bytes; exclusive scans over those (20 bytes per 64 records) say where every wavefront's selected records go and how
// large the output is; select_place_kernel copies the selected records there and notes where their strings lie, and
// order_part_strings (sx_result_dev.hip) lays the strings back to back in record order — the gather of the merged parts, not a
// second one.  Every record is read twice, every string byte once; of the selected ones every byte is read and written once more.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_select_core.hpp"

namespace sx {

constexpr uint32_t kSelectWaves = 4;   // wavefronts per workgroup, each with its own tables

// wavefronts [0, waves]: the last one (behind the last record) selects nothing, so that the scans' last words are the segment's totals
__global__ __launch_bounds__(64 * kSelectWaves) void select_match_kernel(SelectParams P, uint64_t waves) {
    __shared__ uint64_t offs[kSelectWaves][kSelectRecs + 1];
    __shared__ uint32_t lens[kSelectWaves][kSelectRecs];
    __shared__ uint32_t hit[kSelectWaves][2];
    __shared__ uint16_t first[kSelectFirst];
    static_assert(64 * kSelectWaves == kSelectFirst, "a thread per entry of the first-byte table");
    first[threadIdx.x] = select_first_entry(P, threadIdx.x);
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * kSelectWaves + wv;
    const bool one_range = __all(select_load_lane(P, w, lane, offs[wv], lens[wv], hit[wv]) ? 1 : 0) != 0;
    __syncthreads();
    if (one_range) select_scan_lane(P, first, lane, offs[wv], hit[wv]);
    else select_walk_lane(P, first, lane, offs[wv], lens[wv], hit[wv]);
    __syncthreads();
    const bool sel = select_lane_selected(P, w, lane, hit[wv]);
    if (w <= waves) wave_store_selected(P.wmask, P.wcount, P.wbytes, w, sel, lens[wv][lane]);      // (a whole wavefront)
}

__global__ __launch_bounds__(64 * kSelectWaves) void select_place_kernel(SelectParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * (64 * kSelectWaves) + threadIdx.x;
    select_place_lane(P, i / kSelectRecs, (uint32_t)(i % kSelectRecs));
}

static size_t select_scan_bytes(uint64_t items) {
    size_t a = 0, b = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)items, rocprim::plus<uint32_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)items, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return a > b ? a : b;
}
// a segment of n records: wmask, wbytes and their scan (8 bytes per wavefront each), wcount and wbase (4 bytes), then the scans' own scratch
size_t select_scratch_bytes(uint64_t n) {
    const uint64_t waves = (n + kSelectRecs - 1) / kSelectRecs;
    return 3 * up256((size_t)(waves + 1) * 8) + 2 * up256((size_t)(waves + 1) * 4) + up256(select_scan_bytes(waves + 1)) + 256;
}

// Pass 1 of a segment (P.wbase, P.out_recs, P.out_src are not read): fills P.wmask / wcount / wbytes / wbase with places inside
// `scratch`; *count and *bytes: the device words that will hold the number of selected records and their string bytes, valid when
// `stream` has run this far.  by: what the pass looks for (sx_device.hpp); the other kinds' kernels fill the same per-wavefront words.
hipError_t select_measure(SelectParams* P, const SelectBy& by, void* scratch, size_t scratch_bytes, hipStream_t stream, const uint32_t** count, const uint64_t** bytes) {
    if (P->n == 0 || P->n >= 0xFFFFFFFFull || scratch_bytes < select_scratch_bytes(P->n) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    const uint64_t waves = (P->n + kSelectRecs - 1) / kSelectRecs;
    const size_t w8 = up256((size_t)(waves + 1) * 8), w4 = up256((size_t)(waves + 1) * 4);
    uint8_t* at = (uint8_t*)scratch;
    P->wmask = (uint64_t*)at; at += w8;
    P->wbytes = (uint64_t*)at; at += w8;
    uint64_t* bsum = (uint64_t*)at; at += w8;
    P->wcount = (uint32_t*)at; at += w4;
    uint32_t* wbase = (uint32_t*)at; at += w4;
    size_t tmp_bytes = scratch_bytes - (size_t)(at - (uint8_t*)scratch);
    hipError_t e;
    switch (by.kind) {
    case SelectBy::kLabels: e = by.pick ? label_launch_pick(*P, *by.pick, waves, stream) : hipErrorInvalidValue; break;
    case SelectBy::kLabelRange: e = by.range ? label_range_launch_pick(*P, *by.range, waves, stream) : hipErrorInvalidValue; break;
    case SelectBy::kSet: e = by.set ? selset_launch_match(*P, *by.set, waves, stream) : hipErrorInvalidValue; break;
    case SelectBy::kRegex: e = by.re ? selre_launch_match(*P, *by.re, waves, stream) : hipErrorInvalidValue; break;
    default:
        hipLaunchKernelGGL(select_match_kernel, dim3((unsigned)((waves + 1 + kSelectWaves - 1) / kSelectWaves)), dim3(64 * kSelectWaves), 0, stream, *P, waves);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(at, tmp_bytes, (const uint32_t*)P->wcount, wbase, 0u, (size_t)(waves + 1), rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(at, tmp_bytes, (const uint64_t*)P->wbytes, bsum, (uint64_t)0, (size_t)(waves + 1), rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    P->wbase = wbase;
    *count = wbase + waves;
    *bytes = bsum + waves;
    return hipSuccess;
}

// the sources of n_sel selected records, then what order_part_strings needs for them
size_t select_place_scratch_bytes(uint64_t n_sel) { return up256((size_t)n_sel * 8) + order_strings_scratch_bytes(n_sel); }

// Pass 2: the segment's n_sel selected records to out_recs and their strings, back to back, to out_arena (P from select_measure).
hipError_t select_place(const SelectParams& P0, void* out_recs, uint64_t n_sel, uint8_t* out_arena, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (n_sel == 0) return hipSuccess;
    if (scratch_bytes < select_place_scratch_bytes(n_sel) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    SelectParams P = P0;
    P.out_recs = out_recs;
    P.out_src = (uint64_t*)scratch;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    hipLaunchKernelGGL(select_place_kernel, dim3((unsigned)((waves + kSelectWaves - 1) / kSelectWaves)), dim3(64 * kSelectWaves), 0, stream, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t src_bytes = up256((size_t)n_sel * 8);
    return order_part_strings(out_recs, n_sel, (int)P.packed, P.out_src, out_arena, (uint8_t*)scratch + src_bytes, scratch_bytes - src_bytes, stream);
}

}  // namespace sx
