// sx_seltally_core.hpp — the keyword tally over the findings of a segment that lies in HBM (sx_result_tally_device): what ONE lane
// does for its record, written as lane functions.  Included by sx_seltally_dev.hip with SXD = `__device__ __forceinline__`; the
// test-only harness tests/native/seltally_core_host.cpp includes it with SXD = `inline`, so the very same code is checked against
// Python's count by the rule on a machine without GPU (tests/test_seltally_core.py).
//
// The rule: a HIT of keyword k is a pair (finding i, offset o) with s_i[o, o + len_k) == p_k — bytes as they are, or after the ASCII
// fold of both sides, which is compiled into the set's classes —; occurrences that overlap, of one keyword or of several, all count;
// a hit never spans two findings.  hits[k] += the hits, first[k] = min(first[k], ordinal_base + i) over them.
//
// One lane, one record, as in sx_selset_core.hpp: the lane's state is the root in front of its record's first byte and takes one step
// per byte — next[state * classes + map[byte]], from LDS for the first lds_states states, from the table in HBM (through L2) for the
// others —, to the END of its string: there is no early exit.  An entry's top bit says that the target state or its dictionary chain
// ends a keyword; only then the lane walks own / dict (sx_seltally_build.hpp) and counts every keyword on the chain.  A record's state
// never sees another record's bytes: that is the whole no-spanning rule.  A lane reads the bytes [str_off, str_off + str_len) of its
// own record and no other byte of the arena.
//
// Counting: the unique ids below lds_ids have a 32-bit counter per workgroup in LDS (a keyword that occurs in most strings would
// otherwise send every lane to one address in L2; a segment holds less than 2 GiB of strings, so no keyword has 2^31 hits in one
// launch), flushed with one global add per non-zero counter when the workgroup ends (seltally_flush_lane); the other ids add to
// hits[] in HBM at once.  first[] is a 64-bit minimum in HBM behind a plain load: a lane issues the atomic only where its ordinal
// is smaller than what it reads, and what it reads is never smaller than the truth.  Sums and minima do not depend on the order:
// the counters are deterministic.
#pragma once
#include <stdint.h>

#include "sx_select_core.hpp"

namespace sx {

// a compiled set where the kernel reads it (device pointers; in the harness: the builder's)
struct SeltallyDevice {
    const uint8_t* map;      // 256 bytes: byte -> class
    const void* next;        // states * classes entries of entry_bytes
    const uint32_t* own;     // per state: the unique id that ends there, or 0xFFFFFFFF
    const uint32_t* dict;    // per state: the next state on the chain that has an own, or 0
    uint64_t* hits;          // per unique id
    uint64_t* first;
    uint32_t states, classes, lds_states, entry_bytes, unique, lds_ids;   // lds_ids = min(unique, the kernel's LDS counters)
};

struct SeltallyParams {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed, reserved;
    uint64_t ordinal;        // of the segment's record 0: ordinal_base + the findings of the segments in front of it
    SeltallyDevice set;
};

// a lane's walk
struct SeltallyLane {
    uint64_t at, end;        // the next byte, the end of the string
    uint64_t ordinal;        // of the lane's record
    uint32_t state, active;
};

// (the harness runs the lanes one after the other)
SXD void seltally_add32(uint32_t* word, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(word, v);
#else
    *word += v;
#endif
}
SXD void seltally_add64(uint64_t* word, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long*)word, (unsigned long long)v);
#else
    *word += v;
#endif
}
SXD void seltally_min64(uint64_t* word, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin((unsigned long long*)word, (unsigned long long)v);
#else
    if (*word > v) *word = v;
#endif
}

// Lane `lane` of wavefront `w` in front of its record's string (lanes behind the last record have none).
SXD SeltallyLane seltally_begin_lane(const SeltallyParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    SeltallyLane L{ 0, 0, 0, 0, 0 };
    if (i >= P.n) return L;
    uint64_t off; uint32_t len;
    select_string(P, i, &off, &len);
    L.at = off; L.end = off + len; L.ordinal = P.ordinal + i; L.active = len != 0;
    return L;
}

// One hit of unique id `id` in the lane's record.  counts: the workgroup's lds_ids counters (LDS).
SXD void seltally_count(const SeltallyParams& P, uint32_t* counts, uint32_t id, uint64_t ordinal) {
    if (id < P.set.lds_ids) seltally_add32(counts + id, 1u);
    else seltally_add64(P.set.hits + id, 1u);
    seltally_min64(P.set.first + id, ordinal);
}

// One byte of the lane's string (L.active holds).  map: the 256 classes, rows: the first lds_states rows (LDS), E: an entry.
template <class E>
SXD void seltally_step_lane(const SeltallyParams& P, const uint8_t* map, const E* rows, uint32_t* counts, SeltallyLane& L) {
    constexpr E kEnds = (E)((E)1 << (sizeof(E) * 8 - 1));
    const uint32_t at = L.state * P.set.classes + map[P.arena[L.at]];
    const E e = L.state < P.set.lds_states ? rows[at] : ((const E*)P.set.next)[at];
    L.state = (uint32_t)(e & (E)~kEnds);
    L.at++;
    if (e & kEnds)
        for (uint32_t u = L.state; u; u = P.set.dict[u]) {   // (the state itself may end nothing: then its chain does)
            const uint32_t id = P.set.own[u];
            if (id != 0xFFFFFFFFu) seltally_count(P, counts, id, L.ordinal);
        }
    if (L.at == L.end) L.active = 0;
}

// When the workgroup's wavefronts are done: counter c of the workgroup's LDS counters into hits[] (c < lds_ids).
SXD void seltally_flush_lane(const SeltallyParams& P, const uint32_t* counts, uint32_t c) {
    const uint32_t v = counts[c];
    if (v) seltally_add64(P.set.hits + c, v);
}

}  // namespace sx
