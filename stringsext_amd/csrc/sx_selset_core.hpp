// sx_selset_core.hpp — the selection by a compiled keyword list over the findings of a segment that lies in HBM
// (sx_result_select_set_device): what ONE lane does for its record, written as lane functions.  Included by sx_selset_dev.hip with
// SXD = `__device__ __forceinline__`; the test-only harness tests/native/selset_core_host.cpp includes it with SXD = `inline`, so
// the very same code is checked against Python's `p in s` on a machine without GPU (tests/test_selset_core.py).
//
// The rule is sx_select_core.hpp's: finding i matches if some keyword equals s[o, o + len) for some o; it is selected iff
// (matches) xor (invert); a match never spans two findings.  The keywords arrive as the automaton sx_selset_build.hpp describes,
// and this is pass 1 only: it leaves what select_match_kernel leaves — per wavefront of 64 consecutive records the mask of the
// selected ones, their number, their string bytes —, and the scans, select_place_kernel and order_part_strings go on from there.
//
// One lane, one record: the lane's state is the root in front of its record's first byte and takes one step per byte —
// next[state * classes + map[byte]], from LDS for the first lds_states states, from the table in HBM (through L2) for the others
// —; a lane that reaches `matched` or the end of its string is done, and the wavefront goes round until no lane is left.  A
// record's state never sees another record's bytes: that is the whole no-spanning rule.  A lane reads the bytes
// [str_off, str_off + str_len) of its own record and no other byte of the arena.
#pragma once
#include <stdint.h>

#include "sx_select_core.hpp"

namespace sx {

// a compiled set where the kernel reads it (device pointers; in the harness: the builder's)
struct SelsetDevice {
    const uint8_t* map;     // 256 bytes: byte -> class
    const void* next;       // states * classes entries of entry_bytes
    uint32_t states, classes, lds_states, matched, entry_bytes, reserved;
};

struct SelsetParams {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed, invert;
    uint64_t* wmask;         // per wavefront, as SelectParams (waves + 1 entries)
    uint32_t* wcount;
    uint64_t* wbytes;
    SelsetDevice set;
};

// a lane's walk
struct SelsetLane {
    uint64_t at, end;        // the next byte, the end of the string
    uint32_t state, len, hit, active;
};

// Lane `lane` of wavefront `w` in front of its record's string (lanes behind the last record have none).
SXD SelsetLane selset_begin_lane(const SelsetParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    SelsetLane L{ 0, 0, 0, 0, 0, 0 };
    if (i >= P.n) return L;
    uint64_t off;
    select_string(P, i, &off, &L.len);
    L.at = off; L.end = off + L.len; L.active = L.len != 0;
    return L;
}

// One byte of the lane's string (L.active holds).  map: the 256 classes, rows: the first lds_states rows (LDS), E: an entry.
template <class E>
SXD void selset_step_lane(const SelsetParams& P, const uint8_t* map, const E* rows, SelsetLane& L) {
    const uint32_t at = L.state * P.set.classes + map[P.arena[L.at]];
    L.state = L.state < P.set.lds_states ? rows[at] : ((const E*)P.set.next)[at];
    L.at++;
    if (L.state == P.set.matched) { L.hit = 1; L.active = 0; }
    else if (L.at == L.end) L.active = 0;
}

// Is the lane's record selected?  The wavefront's mask is the ballot over this.
SXD bool selset_lane_selected(const SelsetParams& P, uint64_t w, uint32_t lane, const SelsetLane& L) {
    if (w * kSelectRecs + lane >= P.n) return false;
    return (L.hit ^ P.invert) != 0;
}

}  // namespace sx
