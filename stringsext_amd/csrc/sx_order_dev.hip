// sx_order_dev.hip — the findings of a result in HBM in sorted order (sx_result_order_device): the kernels around the lane functions
// of sx_order_core.hpp and the steps the driver in sx_result_api.cpp chains.  Every kernel works a lane per record, item, slot or
// position, 64 of them per wavefront, on a grid as large as the device holds at once that strides over the rest; none holds anything
// in LDS, none has a barrier, and no wavefront waits for another.  The sorts of the 64-bit and 32-bit keys and the scans are
// rocprim's, as in sx_sort.hip and sx_select_dev.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "sx_device.hpp"
#include "sx_rows_dev.hpp"

#define SXD __device__ __forceinline__
#include "sx_order_core.hpp"

namespace sx {

constexpr uint32_t kOrderGroupsPerCu = 4;      // 4 x kRowsWaves = 32 wavefronts per CU, 8 per SIMD: the kernels hold nothing in LDS and few registers

#define ORDER_TRIPS(w, waves) for (uint64_t w = (uint64_t)blockIdx.x * kRowsWaves + (threadIdx.x >> 6); w < (waves); w += (uint64_t)gridDim.x * kRowsWaves)

__global__ __launch_bounds__(64 * kRowsWaves) void order_pick_kernel(OrderPick P, uint64_t waves) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t count = 0, bytes = 0, longest = 0;      // (the same in every lane)
    ORDER_TRIPS(w, waves) {
        uint32_t len;
        const bool picked = order_pick_lane(P, w, lane, &len);
        const uint64_t mask = __ballot(picked ? 1 : 0);
        uint32_t most = len;
#pragma unroll
        for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(most, d, 64); most = o > most ? o : most; }
        if (lane == 0) { P.wmask[P.seg.wave0 + w] = mask; P.wcount[P.seg.wave0 + w] = (uint32_t)__popcll(mask); }
        count += (uint64_t)__popcll(mask); bytes += wave_sum(len); longest = most > longest ? most : longest;
    }
    if (lane == 0 && count) {
        seltally_add64(P.totals + kOrderCount, count);
        seltally_add64(P.totals + kOrderBytes, bytes);
        atomicMax((unsigned long long*)(P.totals + kOrderLongest), (unsigned long long)longest);
    }
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_number_kernel(OrderPick P, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_number_lane(P, w, threadIdx.x & 63u);
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_word_kernel(OrderRound P, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_word_lane(P, w * 64u + (threadIdx.x & 63u));
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_wkey_kernel(const uint64_t* wkey, const uint32_t* perm, uint64_t* out, uint64_t n, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_wkey_lane(wkey, perm, out, n, w * 64u + (threadIdx.x & 63u));
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_gkey_kernel(const uint32_t* slotgrp, const uint32_t* perm, uint32_t* out, uint64_t n, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_gkey_lane(slotgrp, perm, out, n, w * 64u + (threadIdx.x & 63u));
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_split_kernel(OrderRound P, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_split_lane(P, w * 64u + (threadIdx.x & 63u));
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_compact_kernel(OrderRound P, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_compact_lane(P, w * 64u + (threadIdx.x & 63u));
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_field_kernel(OrderField P, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_field_lane(P, w * 64u + (threadIdx.x & 63u));
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_measure_kernel(OrderOut P, uint64_t waves) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t bytes = 0, ties = 0;
    ORDER_TRIPS(w, waves) {
        uint32_t len; bool tied;
        order_measure_lane(P, w * 64u + lane, &len, &tied);
        bytes += wave_sum(len);
        ties += (uint64_t)__popcll(__ballot(tied ? 1 : 0));
    }
    if (lane == 0 && bytes) seltally_add64(P.totals + kOrderKeptBytes, bytes);
    if (lane == 0 && ties) seltally_add64(P.totals + kOrderTied, ties);
}

__global__ __launch_bounds__(64 * kRowsWaves) void order_gather_kernel(OrderOut P, uint64_t waves) {
    ORDER_TRIPS(w, waves) order_gather_lane(P, w * 64u + (threadIdx.x & 63u));
}

#undef ORDER_TRIPS

namespace {

// one kernel over n lanes' worth of wavefronts
template <class K, class... A>
hipError_t order_over(K kernel, uint64_t n, hipStream_t stream, A... args) {
    if (n == 0) return hipSuccess;
    const uint64_t waves = (n + 63) / 64;
    dim3 grid;
    const hipError_t e = rows_grid(waves, kRowsWaves, kOrderGroupsPerCu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(64 * kRowsWaves), 0, stream, args..., waves);
    return hipGetLastError();
}

size_t order_tmp_bytes(uint64_t n) {
    size_t a = 0, b = 0, c = 0, d = 0;
    uint64_t* k64 = nullptr; uint32_t* k32 = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, k64, k64, k32, k32, (size_t)n, 0, 64, (hipStream_t)0);
    (void)rocprim::radix_sort_pairs(nullptr, b, k32, k32, k32, k32, (size_t)n, 0, 32, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, c, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, d, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return std::max(std::max(a, b), std::max(c, d));
}

// One call of rocprim with the tables' own storage: call(storage, bytes) asked first what it needs — the storage is sized for the
// call's largest input, and a smaller one that asked for more would be an error here, never a write behind the storage
template <class F>
hipError_t order_prim(void* tmp, size_t have, F call) {
    size_t need = 0;
    hipError_t e = call(nullptr, need);
    if (e != hipSuccess) return e;
    if (need > have) return hipErrorInvalidValue;
    return call(tmp, have);
}

// `bytes` of the block behind *at, 256-byte aligned
template <class T>
T* order_take(uint8_t* base, size_t* at, size_t bytes) {
    T* p = base ? (T*)(base + *at) : nullptr;
    *at += up256(bytes);
    return p;
}

}  // namespace

// The pick's tables in `base` (NULL: only their size is wanted) for n_segs segments, n_packed of them packed, and `waves` wavefronts
size_t order_pick_tables(uint8_t* base, uint64_t n_segs, uint64_t n_packed, uint64_t waves, OrderPickTables* T) {
    size_t at = 0;
    OrderPickTables t;
    t.segs = order_take<OrderSeg>(base, &at, (size_t)n_segs * sizeof(OrderSeg));
    t.pos0 = order_take<uint64_t>(base, &at, (size_t)n_packed * 256 * sizeof(uint64_t));
    t.totals = order_take<uint64_t>(base, &at, kOrderTotals * sizeof(uint64_t));
    t.wmask = order_take<uint64_t>(base, &at, (size_t)(waves + 1) * 8);
    t.wcount = order_take<uint32_t>(base, &at, (size_t)(waves + 1) * 4);
    t.wbase = order_take<uint32_t>(base, &at, (size_t)(waves + 1) * 4);
    t.tmp_bytes = up256(order_tmp_bytes(waves + 1));
    t.tmp = order_take<uint8_t>(base, &at, t.tmp_bytes);
    if (T) *T = t;
    return at;
}

// The tables of the sort for m items
size_t order_sort_tables(uint8_t* base, uint64_t m, OrderSortTables* T) {
    size_t at = 0;
    OrderSortTables t;
    const size_t n = (size_t)m + 1;
    for (int k = 0; k < 2; k++) {
        t.ikey[k] = order_take<uint64_t>(base, &at, n * 8);
        t.slotpos[k] = order_take<uint32_t>(base, &at, n * 4);
        t.slotgrp[k] = order_take<uint32_t>(base, &at, n * 4);
        t.k64[k] = order_take<uint64_t>(base, &at, n * 8);
        t.k32[k] = order_take<uint32_t>(base, &at, n * 4);
        t.perm[k] = order_take<uint32_t>(base, &at, n * 4);
    }
    t.wkey = order_take<uint64_t>(base, &at, n * 8);
    t.rkey = order_take<uint32_t>(base, &at, n * 4);
    t.iota = order_take<uint32_t>(base, &at, n * 4);
    t.flags = order_take<uint64_t>(base, &at, n * 8);
    t.scan = order_take<uint64_t>(base, &at, n * 8);
    t.order = order_take<uint64_t>(base, &at, n * 8);
    t.classhead = order_take<uint32_t>(base, &at, n * 4);
    t.tmp_bytes = up256(order_tmp_bytes(m));
    t.tmp = order_take<uint8_t>(base, &at, t.tmp_bytes);
    if (T) *T = t;
    return at;
}

// pick of one segment: its wavefronts' masks and counts, and the call's totals
hipError_t order_launch_pick(const OrderPick& P, hipStream_t stream) {
    if (P.seg.n >> 32 || (P.filter && !P.seg.labels) || !P.wmask || !P.wcount || !P.totals) return hipErrorInvalidValue;
    return order_over(order_pick_kernel, P.seg.n, stream, P);
}

// behind every segment's pick: where every wavefront's picked records go (`waves`: the call's)
hipError_t order_scan_picks(const OrderPickTables& T, uint64_t waves, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(T.wcount + waves, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    return order_prim(T.tmp, T.tmp_bytes, [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, (const uint32_t*)T.wcount, T.wbase, 0u, (size_t)waves + 1, rocprim::plus<uint32_t>(), stream);
    });
}

hipError_t order_launch_number(const OrderPick& P, hipStream_t stream) {
    if (P.seg.n >> 32 || !P.wbase || !P.ikey || !P.slotpos || !P.slotgrp || (P.field && !P.seg.labels)) return hipErrorInvalidValue;
    return order_over(order_number_kernel, P.seg.n, stream, P);
}

// One round of the string key over the list `cur` (0 / 1) of n slots, with `groups` groups in it: word, the sorts, split, the scan,
// compact into the other list.  T.scan[n] then holds the next list's slots (low half) and groups (high half).
hipError_t order_round(const OrderSortTables& T, const OrderSeg* segs, int cur, uint64_t n, uint64_t groups, uint32_t depth, uint32_t nocase, uint32_t descending,
                       hipStream_t stream) {
    if (n == 0 || n >= 0xFFFFFFFFull || (cur != 0 && cur != 1)) return hipErrorInvalidValue;
    OrderRound P;
    memset(&P, 0, sizeof P);
    P.segs = segs; P.n = n; P.nocase = nocase; P.descending = descending; P.depth = depth;
    P.ikey = T.ikey[cur]; P.slotpos = T.slotpos[cur]; P.slotgrp = T.slotgrp[cur];
    P.wkey = T.wkey; P.rkey = T.rkey; P.iota = T.iota;
    P.order = T.order; P.classhead = T.classhead; P.flags = T.flags; P.scan = T.scan;
    P.ikey_next = T.ikey[cur ^ 1]; P.slotpos_next = T.slotpos[cur ^ 1]; P.slotgrp_next = T.slotgrp[cur ^ 1];
    hipError_t e = order_over(order_word_kernel, n, stream, P);
    if (e != hipSuccess) return e;
    // least significant key first: rem (0..8), the word, the group
    e = order_prim(T.tmp, T.tmp_bytes, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, T.rkey, T.k32[0], T.iota, T.perm[0], (size_t)n, 0, 4, stream); });
    if (e != hipSuccess) return e;
    e = order_over(order_wkey_kernel, n, stream, (const uint64_t*)T.wkey, (const uint32_t*)T.perm[0], T.k64[0], n);
    if (e != hipSuccess) return e;
    e = order_prim(T.tmp, T.tmp_bytes, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, T.k64[0], T.k64[1], T.perm[0], T.perm[1], (size_t)n, 0, 64, stream); });
    if (e != hipSuccess) return e;
    P.perm = T.perm[1];
    if (groups > 1) {
        unsigned bits = 1;
        while (bits < 32 && ((groups - 1) >> bits)) bits++;
        e = order_over(order_gkey_kernel, n, stream, (const uint32_t*)P.slotgrp, (const uint32_t*)T.perm[1], T.k32[0], n);
        if (e != hipSuccess) return e;
        e = order_prim(T.tmp, T.tmp_bytes, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, T.k32[0], T.k32[1], T.perm[1], T.perm[0], (size_t)n, 0, bits, stream); });
        if (e != hipSuccess) return e;
        P.perm = T.perm[0];
    }
    e = order_over(order_split_kernel, n, stream, P);
    if (e != hipSuccess) return e;
    e = order_prim(T.tmp, T.tmp_bytes, [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, (const uint64_t*)T.flags, T.scan, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), stream);
    });
    if (e != hipSuccess) return e;
    return order_over(order_compact_kernel, n, stream, P);
}

// The label key: the m items' fields lie in T.wkey (complemented if descending): one sort over `bits` bits, then the order
hipError_t order_by_field(const OrderSortTables& T, uint64_t m, uint32_t bits, hipStream_t stream) {
    if (m == 0 || m >= 0xFFFFFFFFull || bits < 1 || bits > 64) return hipErrorInvalidValue;
    const hipError_t e = order_prim(T.tmp, T.tmp_bytes, [&](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, T.wkey, T.k64[0], T.slotpos[0], T.perm[0], (size_t)m, 0, bits, stream); });
    if (e != hipSuccess) return e;
    const OrderField F{ m, T.k64[0], T.perm[0], T.ikey[0], T.order, T.classhead };
    return order_over(order_field_kernel, m, stream, F);
}

hipError_t order_launch_measure(const OrderOut& P, hipStream_t stream) {
    if (!P.segs || !P.order || !P.classhead || !P.totals) return hipErrorInvalidValue;
    return order_over(order_measure_kernel, P.kept, stream, P);
}

hipError_t order_launch_gather(const OrderOut& P, hipStream_t stream) {
    if (!P.segs || !P.order || !P.out || !P.out_src) return hipErrorInvalidValue;
    return order_over(order_gather_kernel, P.kept, stream, P);
}

}  // namespace sx
