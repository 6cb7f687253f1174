// sx_result_dev.hip — a merged part that stays in HBM (SX_OPT_RESULT_ON_DEVICE with several Missions): its strings are laid
// back to back in record order, so that a device consumer that walks the records reads neighbouring bytes with neighbouring
// lanes.  The merger's placement (sx_sort.hip) notes where every placed record's string lies; here an exclusive scan over
// str_len in output order gives the new offsets and one kernel moves the strings (sx_result_core.hpp: a wavefront per 64
// consecutive records, its output range written in 16-byte chunks).  The string bytes are read once and written once, as by
// the per-Mission block copies this replaces.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "sx_device.hpp"

#define SXD __device__ __forceinline__
#include "sx_result_core.hpp"

namespace sx {

constexpr uint32_t kGatherWaves = 4;   // wavefronts per workgroup, each with its own tables

__global__ __launch_bounds__(64 * kGatherWaves) void result_gather_kernel(GatherParams P) {
    __shared__ uint32_t offs[kGatherWaves][kGatherRecs + 4];
    __shared__ uint64_t srcs[kGatherWaves][kGatherRecs];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * kGatherWaves + wv;   // (a wavefront behind the last record: empty strings only)
    gather_load_lane(P, w, lane, offs[wv], srcs[wv]);
    __syncthreads();
    gather_copy_lane(P, lane, offs[wv], srcs[wv]);
}

// str_len of placed record i; the scan runs over n + 1 items, the last one empty: noff[n] = the bytes of all strings
struct PlacedLen {
    const void* recs; uint32_t n; int packed;
    __device__ uint32_t operator()(uint32_t i) const {
        if (i >= n) return 0u;
        return packed ? (uint32_t)((const sx_finding16*)recs)[i].str_len : ((const sx_finding*)recs)[i].str_len;
    }
};
static size_t order_scan_bytes(uint64_t n) {
    size_t t = 0;
    auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), PlacedLen{ nullptr, 0, 0 });
    (void)rocprim::exclusive_scan(nullptr, t, lens, (uint32_t*)nullptr, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return t;
}
size_t order_strings_scratch_bytes(uint64_t n) {
    return (((size_t)n + 1) * 4 + 255) / 256 * 256 + order_scan_bytes(n) + 256;
}

hipError_t order_part_strings(void* recs, uint64_t n, int packed, const uint64_t* src, uint8_t* arena, void* scratch, size_t scratch_bytes,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n >= 0xFFFFFFFFull || scratch_bytes < order_strings_scratch_bytes(n) || ((uintptr_t)scratch & 255)) return hipErrorInvalidValue;
    uint32_t* noff = (uint32_t*)scratch;
    const size_t noff_bytes = (((size_t)n + 1) * 4 + 255) / 256 * 256;
    void* tmp = (uint8_t*)scratch + noff_bytes;
    size_t tmp_bytes = scratch_bytes - noff_bytes;
    auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), PlacedLen{ recs, (uint32_t)n, packed });
    hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, lens, noff, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    GatherParams P{ recs, src, noff, arena, n, packed ? 1u : 0u };
    const uint64_t waves = (n + kGatherRecs - 1) / kGatherRecs;
    hipLaunchKernelGGL(result_gather_kernel, dim3((unsigned)((waves + kGatherWaves - 1) / kGatherWaves)), dim3(64 * kGatherWaves), 0, stream, P);
    return hipGetLastError();
}

}  // namespace sx
