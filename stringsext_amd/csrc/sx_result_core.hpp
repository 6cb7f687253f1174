// sx_result_core.hpp — the ordered string gather of a merged part that stays in HBM (SX_OPT_RESULT_ON_DEVICE with several
// Missions): what ONE wavefront does for its kGatherRecs consecutive output records, written as lane loops.  Included by
// sx_result_dev.hip with SXD = `__device__ __forceinline__`; the test-only harness tests/native/result_core_host.cpp
// includes it with SXD = `inline`, so the very same code is checked against a plain merge on a machine without GPU
// (tests/test_result_core.py).
//
// The merger's placement (sx_sort.hip merge_place_kernel) has put every record where it will be printed and noted, per placed
// record, the address of its string in its Mission's arena.  An exclusive scan over str_len in output order gives the strings'
// new places: back to back, in record order.  A wavefront owns the records [w * 64, w * 64 + 64); their strings are one
// contiguous range of the new arena, which the wavefront writes in 16-byte chunks, a chunk per lane and round: every output
// byte finds its record by a search over the wavefront's 65 offsets (LDS), then follows the records forward.  The sources are
// short gathers (a string is some 15 bytes on BASELINE config 5) out of lists that are themselves ordered by position: L2.
#pragma once
#include <stdint.h>

#include "../../include/stringsext_amd.h"

namespace sx {

constexpr uint32_t kGatherRecs = 64;   // records per wavefront: one per lane

struct GatherParams {
    void* recs;             // the placed records, sx_finding16 if `packed` else sx_finding: str_off is rewritten
    const uint64_t* src;    // per placed record: where its string lies (an address in its Mission's arena)
    const uint32_t* noff;   // n + 1 words: the exclusive scan of str_len in output order, noff[n] = all strings
    uint8_t* arena;         // the part's strings, noff[n] bytes
    uint64_t n;
    uint32_t packed;
};

struct alignas(16) Gather16 { uint32_t w[4]; };

// Step 1, lane `lane` of wavefront `w`: its record's new offset and source into the wavefront's tables (offs: kGatherRecs + 1
// words, srcs: kGatherRecs addresses) and into the record.  Lanes behind the last record hold empty strings at the end.
SXD void gather_load_lane(const GatherParams& P, uint64_t w, uint32_t lane, uint32_t* offs, uint64_t* srcs) {
    const uint64_t i = w * kGatherRecs + lane;
    const uint32_t off = P.noff[i < P.n ? i : P.n];
    offs[lane] = off;
    srcs[lane] = i < P.n ? P.src[i] : 0;
    if (i < P.n) {
        if (P.packed) ((sx_finding16*)P.recs)[i].str_off = off;
        else ((sx_finding*)P.recs)[i].str_off = off;
    }
    if (lane == kGatherRecs - 1) offs[kGatherRecs] = P.noff[i + 1 < P.n ? i + 1 : P.n];
}

// Step 2 (after every lane's step 1), lane `lane`: the 16-byte chunks lane, lane + 64, ... of the wavefront's output range.
// Chunks are aligned in memory; the first and the last may be shared with the neighbouring wavefronts and are written byte
// by byte, everything between them with one 16-byte store per lane.
SXD void gather_copy_lane(const GatherParams& P, uint32_t lane, const uint32_t* offs, const uint64_t* srcs) {
    const uint64_t start = offs[0], end = offs[kGatherRecs];
    if (start >= end) return;
    const uint64_t mis = ((uint64_t)(uintptr_t)P.arena + start) & 15u;   // the range's first chunk begins `mis` bytes in front of it
    for (uint64_t c = lane;; c += kGatherRecs) {
        // chunk c = the arena bytes [c0, c0 + 16), of which [lo, hi) are this wavefront's
        if (c * 16 >= end - start + mis) break;
        const uint64_t c0s = start + c * 16;          // (c0 + mis: no negative numbers)
        const uint64_t lo = c == 0 ? start : c0s - mis;
        const uint64_t hi = c0s - mis + 16 < end ? c0s - mis + 16 : end;
        // the record that holds byte lo: the last one that begins at or in front of it (empty strings share their successor's offset)
        uint32_t r = 0;
        for (uint32_t step = kGatherRecs / 2; step; step >>= 1)
            if (offs[r + step] <= lo) r += step;
        uint32_t r_off = offs[r], r_end = offs[r + 1];
        const uint8_t* s = (const uint8_t*)(uintptr_t)srcs[r];
        const bool whole = hi - lo == 16;
        Gather16 v{ { 0, 0, 0, 0 } };
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint64_t b = lo + k;
            if (b < hi) {
                while (b >= r_end) { r++; r_off = r_end; r_end = offs[r + 1]; s = (const uint8_t*)(uintptr_t)srcs[r]; }
                const uint32_t x = s[b - r_off];
                if (whole) v.w[k >> 2] |= x << ((k & 3u) * 8u);
                else P.arena[b] = (uint8_t)x;
            }
        }
        if (whole) *(Gather16*)(P.arena + lo) = v;
    }
}

}  // namespace sx
