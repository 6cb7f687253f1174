// sx_decode_dev.hip — a segment's strings read as base64, hex or percent escapes and replaced by what they stand for, where they lie
// (sx_result_decode_device): two kernels around one small scan (sx_decode_core.hpp), in the shape of sx_fold_dev.hip.
// decode_measure_kernel walks the strings of 64 consecutive records per wavefront, a record per lane, and leaves every record's word
// — whether it decodes, what the output looks like, its length —, per wavefront the sum of the output strings' bytes, and adds per
// wavefront to the segment's totals; an exclusive scan over the wavefronts' sums says where every wavefront's bytes go and how many
// the segment has; decode_place_kernel repeats the walk of the strings that decode, copies the others, and writes, per record, the
// source record with its new str_off and str_len and the bytes, back to back in record order.  The decoder has no table: the kernels
// use no LDS, and the grid is as large as the device holds at once and strides over the segment.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_decode_core.hpp"

namespace sx {

static_assert(SX_DECODE_OK == 1u && SX_DECODE_TEXT == 2u && SX_DECODE_WIDE == 4u, "decode_measure_kernel counts the words' low bits");

__device__ __forceinline__ uint64_t decode_wave_max(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint64_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// wavefronts [0, waves]: the last one (behind the last record) has no byte, so that the scan's last word is the segment's total
__global__ __launch_bounds__(64 * kRowsWaves) void decode_measure_kernel(DecodeParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t n_decoded = 0, n_text = 0, n_wide = 0;      // of the lane's trips: fewer than 2^32
    uint64_t longest = 0, bytes_in = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w <= waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        uint32_t len;
        uint64_t word;
        const uint64_t bytes = decode_measure_lane(P, w, lane, &len, &word);
        const uint64_t sum = wave_sum(bytes);
        n_decoded += (uint32_t)word & 1u; n_text += (uint32_t)word >> 1 & 1u; n_wide += (uint32_t)word >> 2 & 1u;
        longest = bytes > longest ? bytes : longest;
        bytes_in += len;
        if (lane == 0) P.wbytes[w] = sum;
    }
    const uint64_t decoded = wave_sum(n_decoded), text = wave_sum(n_text), wide = wave_sum(n_wide);
    longest = decode_wave_max(longest);
    bytes_in = wave_sum(bytes_in);
    if (lane == 0) {
        if (decoded) atomicAdd((unsigned long long*)&P.totals[kDecodeDecoded], (unsigned long long)decoded);
        if (text) atomicAdd((unsigned long long*)&P.totals[kDecodeText], (unsigned long long)text);
        if (wide) atomicAdd((unsigned long long*)&P.totals[kDecodeWide], (unsigned long long)wide);
        if (longest) atomicMax((unsigned long long*)&P.totals[kDecodeLongest], (unsigned long long)longest);
        if (bytes_in) atomicAdd((unsigned long long*)&P.totals[kDecodeBytesIn], (unsigned long long)bytes_in);
        if (blockIdx.x == 0 && wv == 0) P.totals[kDecodeRecords] = P.n;
    }
}

__global__ __launch_bounds__(64 * kRowsWaves) void decode_place_kernel(DecodeParams P, uint64_t waves) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + wv; w < waves; w += (uint64_t)gridDim.x * kRowsWaves) {
        const uint64_t i = w * kSelectRecs + lane;
        // the lane's base: the wavefront's, plus the output bytes of the wavefront's earlier records
        uint32_t own = 0;
        if (i < P.n) {
            uint64_t off;
            uint32_t len;
            select_string(P, i, &off, &len);
            own = decode_out_len(P.words[i], len);
        }
        const uint64_t upto = wave_prefix(own, lane);
        decode_place_lane(P, w, lane, P.wbase[w] + upto - own);
    }
}

static size_t decode_scan_bytes(uint64_t items) {
    size_t a = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)items, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return a;
}
// a segment of n records: wbytes and its scan (8 bytes per wavefront each), the totals, then the scan's own scratch
size_t decode_scratch_bytes(uint64_t n) {
    const uint64_t waves = (n + kSelectRecs - 1) / kSelectRecs;
    return 2 * up256((size_t)(waves + 1) * 8) + 256 + up256(decode_scan_bytes(waves + 1)) + 256;
}

// Pass 1 of a segment (P.words is the caller's; P.wbase, P.out_recs, P.out_arena are not read): fills P.words and P.wbytes / totals /
// wbase with places inside `scratch`; *count, *bytes, *totals: the device words that will hold the number of records, the output
// strings' bytes and the kDecodeTotals totals, valid when `stream` has run this far.
hipError_t decode_measure(DecodeParams* P, void* scratch, size_t scratch_bytes, hipStream_t stream, const uint64_t** count, const uint64_t** bytes, const uint64_t** totals) {
    if (P->n == 0 || P->n >= 0xFFFFFFFFull || !P->words || scratch_bytes < decode_scratch_bytes(P->n) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    if (P->kind < SX_DECODE_BASE64 || P->kind > SX_DECODE_PERCENT || (P->flags & ~(uint32_t)SX_DECODE_UTF16LE)) return hipErrorInvalidValue;
    const uint64_t waves = (P->n + kSelectRecs - 1) / kSelectRecs;
    const size_t w8 = up256((size_t)(waves + 1) * 8);
    uint8_t* at = (uint8_t*)scratch;
    P->wbytes = (uint64_t*)at; at += w8;
    uint64_t* wbase = (uint64_t*)at; at += w8;
    P->totals = (uint64_t*)at; at += 256;
    size_t tmp_bytes = scratch_bytes - (size_t)(at - (uint8_t*)scratch);
    hipError_t e = hipMemsetAsync(P->totals, 0, kDecodeTotals * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    dim3 grid;
    e = rows_grid(waves + 1, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(decode_measure_kernel, grid, dim3(64 * kRowsWaves), 0, stream, *P, waves);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(at, tmp_bytes, (const uint64_t*)P->wbytes, wbase, (uint64_t)0, (size_t)(waves + 1), rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    P->wbase = wbase;
    *count = P->totals + kDecodeRecords;
    *bytes = wbase + waves;
    *totals = P->totals;
    return hipSuccess;
}

// Pass 2: the segment's records to out_recs and their output strings, back to back, to out_arena (P from decode_measure; the driver
// has seen that the bytes fit str_off and, in a packed segment, the longest output string str_len).
hipError_t decode_place(const DecodeParams& P0, void* out_recs, uint8_t* out_arena, hipStream_t stream) {
    DecodeParams P = P0;
    P.out_recs = out_recs;
    P.out_arena = out_arena;
    const uint64_t waves = (P.n + kSelectRecs - 1) / kSelectRecs;
    dim3 grid;
    hipError_t e = rows_grid(waves, kRowsWaves, kRowsGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(decode_place_kernel, grid, dim3(64 * kRowsWaves), 0, stream, P, waves);
    return hipGetLastError();
}

}  // namespace sx
