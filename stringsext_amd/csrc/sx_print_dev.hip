// sx_print_dev.hip — Finding::print on the device (sx_print_findings_device): the findings of a segment that lies in HBM
// (SX_OPT_RESULT_ON_DEVICE) become the reference's text without leaving it.  Two kernels per segment around one small scan
// (sx_print_core.hpp): print_len_kernel sums, per wavefront of 64 consecutive records, the bytes of their lines; an exclusive
// scan over those sums (8 bytes per 64 records) says where every wavefront's range of the text begins; print_write_kernel
// formats the 64 prefixes into LDS and writes the range in 16-byte chunks.  Every record is read twice (16 bytes each time),
// every string byte once, every text byte written once.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_print_core.hpp"

namespace sx {

constexpr uint32_t kPrintWaves = 4;   // wavefronts per workgroup, each with its own tables

// wsum[w] for w in [0, waves]: the last one (behind the last record) is 0, so that the scan's last word is the segment's text bytes
__global__ __launch_bounds__(64 * kPrintWaves) void print_len_kernel(PrintParams P, uint64_t* wsum, uint64_t waves) {
    const uint64_t i = (uint64_t)blockIdx.x * (64 * kPrintWaves) + threadIdx.x;
    const uint64_t len = wave_sum(print_line_len(P, i));
    if ((threadIdx.x & 63u) == 0 && i / kPrintRecs <= waves) wsum[i / kPrintRecs] = len;
}

__global__ __launch_bounds__(64 * kPrintWaves) void print_write_kernel(PrintParams P) {
    __shared__ uint64_t lens[kPrintWaves][kPrintRecs];
    __shared__ uint64_t offs[kPrintWaves][kPrintRecs + 2];
    __shared__ uint64_t srcs[kPrintWaves][kPrintRecs];
    __shared__ uint8_t plens[kPrintWaves][kPrintRecs];
    __shared__ __attribute__((aligned(16))) uint8_t pre[kPrintWaves][kPrintRecs * kPrintPrefix];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * kPrintWaves + wv;   // (a wavefront behind the last record: empty lines only)
    print_load_lane(P, w, lane, lens[wv], srcs[wv], plens[wv], pre[wv]);
    __syncthreads();
    print_scan_lane(lane, lens[wv], offs[wv]);
    __syncthreads();
    if (w * kPrintRecs < P.n) print_copy_lane(P, w, lane, offs[wv], srcs[wv], plens[wv], pre[wv]);
}

static size_t print_scan_bytes(uint64_t items) {
    size_t t = 0;
    (void)rocprim::exclusive_scan(nullptr, t, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)items, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return t;
}
// a segment of n records: wsum and wbase (waves + 1 words each), then the scan's own scratch
size_t print_scratch_bytes(uint64_t n) {
    const uint64_t waves = (n + kPrintRecs - 1) / kPrintRecs;
    return 2 * up256((size_t)(waves + 1) * 8) + up256(print_scan_bytes(waves + 1)) + 256;
}

// Pass 1 of a segment (P.wbase, P.text, P.base are not read).  *wbase: where the wavefronts' offsets will be, *total: the
// device word that will hold the segment's text bytes — both inside `scratch`, valid when `stream` has run this far.
hipError_t print_measure(const PrintParams& P, void* scratch, size_t scratch_bytes, hipStream_t stream, const uint64_t** wbase, const uint64_t** total) {
    if (P.n == 0 || scratch_bytes < print_scratch_bytes(P.n) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    const uint64_t waves = (P.n + kPrintRecs - 1) / kPrintRecs;
    const size_t words = up256((size_t)(waves + 1) * 8);
    uint64_t* wsum = (uint64_t*)scratch;
    uint64_t* wb = (uint64_t*)((uint8_t*)scratch + words);
    void* tmp = (uint8_t*)scratch + 2 * words;
    size_t tmp_bytes = scratch_bytes - 2 * words;
    hipLaunchKernelGGL(print_len_kernel, dim3((unsigned)((waves + 1 + kPrintWaves - 1) / kPrintWaves)), dim3(64 * kPrintWaves), 0, stream, P, wsum, waves);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(tmp, tmp_bytes, (const uint64_t*)wsum, wb, (uint64_t)0, (size_t)(waves + 1), rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    *wbase = wb;
    *total = wb + waves;
    return hipSuccess;
}

// Pass 2: the segment's lines to P.text + P.base (P.wbase from print_measure).
hipError_t print_write(const PrintParams& P, hipStream_t stream) {
    if (P.n == 0) return hipSuccess;
    const uint64_t waves = (P.n + kPrintRecs - 1) / kPrintRecs;
    hipLaunchKernelGGL(print_write_kernel, dim3((unsigned)((waves + kPrintWaves - 1) / kPrintWaves)), dim3(64 * kPrintWaves), 0, stream, P);
    return hipGetLastError();
}

}  // namespace sx
