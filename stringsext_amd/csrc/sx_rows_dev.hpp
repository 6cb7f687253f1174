// sx_rows_dev.hpp — what the kernels that walk a table over a segment's records share (sx_selset_dev.hip, sx_selre_dev.hip,
// sx_extract_dev.hip, sx_seltally_dev.hip, sx_label_dev.hip, sx_fuzzy_dev.hip; sx_select_dev.hip for the epilogue; sx_seen_dev.hip, sx_seen_merge_dev.hip
// and sx_print_dev.hip for the wavefront's sum, prefix and reserve): the workgroup's shape, the class map and the first rows into
// LDS, the grid that strides over the segment, the words a pass 1 of the selection leaves per wavefront, and the table checks.  Device-only: included behind <hip/hip_runtime.h> and sx_device.hpp.  The walks themselves are the kernels'.
#pragma once

namespace sx {

constexpr uint32_t kRowsWaves = 8;          // wavefronts per workgroup, which share the rows (and a kernel's counters) in LDS
constexpr uint32_t kRowsGroupsPerCu = 3;    // 3 x (at most 48 KiB of rows + the map + 768 bytes of counters) <= 160 KiB; 24 wavefronts per CU

struct alignas(16) Rows16 { uint32_t w[4]; };

// The class map and the rows of the first lds_states states into LDS, by the workgroup's 64 * kRowsWaves threads, 16 bytes at a time
// (the table's allocation is a multiple of 16 bytes).  Ends with the workgroup's barrier: what a kernel zeroes in LDS, it zeroes before.
__device__ __forceinline__ void rows_load(const uint8_t* map_src, const void* next_src, uint32_t lds_states, uint32_t classes, uint32_t entry_bytes,
                                          uint8_t* map, Rows16* rows16) {
    if (threadIdx.x < 256 / 4) ((uint32_t*)map)[threadIdx.x] = ((const uint32_t*)map_src)[threadIdx.x];
    const uint32_t chunks = (lds_states * classes * entry_bytes + 15u) / 16u;
    for (uint32_t c = threadIdx.x; c < chunks; c += 64 * kRowsWaves) rows16[c] = ((const Rows16*)next_src)[c];
    __syncthreads();
}

// The wavefront's helpers; every lane of the wavefront calls them.  wave_sum: every lane gets the sum over the 64 lanes
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// the sum over the lanes up to and including this one; lane 63 holds the wavefront's
__device__ __forceinline__ uint64_t wave_prefix(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t left = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += left;
    }
    return v;
}
// Room for every lane's `bytes` behind *cursor, one address for the whole grid, with ONE add by lane 0: where this lane's bytes
// begin, the lanes' rooms one behind the other in lane order
__device__ __forceinline__ uint64_t wave_reserve(uint64_t* cursor, uint64_t bytes, uint32_t lane) {
    const uint64_t upto = wave_prefix(bytes, lane), all = __shfl(upto, 63, 64);
    uint64_t base = 0;
    if (lane == 0) base = atomicAdd((unsigned long long*)cursor, (unsigned long long)all);
    return __shfl(base, 0, 64) + upto - bytes;
}

// What pass 1 of a selection leaves of wavefront w: the mask of its selected records, their number, their strings' bytes
// (sel, len: the lane's record; every lane of the wavefront calls)
__device__ __forceinline__ void wave_store_selected(uint64_t* wmask, uint32_t* wcount, uint64_t* wbytes, uint64_t w, bool sel, uint32_t len) {
    const uint64_t mask = __ballot(sel ? 1 : 0);
    const uint64_t bytes = wave_sum(sel ? len : 0u);
    if (threadIdx.x % 64u == 0) { wmask[w] = mask; wcount[w] = (uint32_t)__popcll(mask); wbytes[w] = bytes; }
}

// The grid over `wavefronts` wavefronts' worth of records: as many workgroups as the device holds at once, which stride
inline hipError_t rows_grid(uint64_t wavefronts, uint32_t waves_per_group, uint32_t groups_per_cu, dim3* grid) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const uint64_t groups = (wavefronts + waves_per_group - 1) / waves_per_group, most = (uint64_t)(cus > 0 ? cus : 1) * groups_per_cu;
    *grid = dim3((unsigned)(groups < most ? groups : most));
    return hipSuccess;
}

// A table the kernels can walk: its classes, and the rows that go into LDS fit `lds_bytes` and are rows of the table
inline hipError_t rows_check(uint32_t classes, uint32_t states, uint32_t lds_states, uint32_t entry_bytes, uint32_t lds_bytes) {
    if (classes < 1 || classes > 256 || (entry_bytes != 2 && entry_bytes != 4)) return hipErrorInvalidValue;
    if ((uint64_t)lds_states * classes * entry_bytes > lds_bytes || lds_states > states) return hipErrorInvalidValue;
    return hipSuccess;
}

}  // namespace sx
