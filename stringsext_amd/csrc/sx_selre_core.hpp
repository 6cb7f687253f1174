// sx_selre_core.hpp — the selection by compiled regular expressions over the findings of a segment that lies in HBM
// (sx_result_select_regex_device): what ONE lane does for its record, written as lane functions.  Included by sx_selre_dev.hip with
// SXD = `__device__ __forceinline__`; the test-only harness tests/native/selre_core_host.cpp includes it with SXD = `inline`, so
// the very same code is checked against Python's re.search on a machine without GPU (tests/test_selre_core.py).
//
// The rule: finding i matches if some pattern of the set is found somewhere in its string; it is selected iff (matches) xor
// (invert); a match never spans two findings.  The patterns arrive as the DFA sx_selre_build.hpp describes, and this is pass 1
// only: it leaves what select_match_kernel leaves — per wavefront of 64 consecutive records the mask of the selected ones, their
// number, their string bytes —, and the scans, select_place_kernel and order_part_strings go on from there.
//
// One lane, one record: the lane's state is the root in front of its record's first byte and takes one step per byte —
// next[state * classes + map[byte]], from LDS for the first lds_states states, from the table in HBM (through L2) for the others.
// A lane is done in a state >= stop_first — `matched`: a hit whatever follows; `dead`: nothing that follows can match — or behind
// its last byte, where it hits iff its state accepts at the end: `matched`, one of [end_first, stop_first), or the root if
// root_end says so.  An empty string is decided by the root alone (`a*`, `^$`, `^` select it).  A record's state never sees another
// record's bytes: a lane reads the bytes [str_off, str_off + str_len) of its own record and no other byte of the arena — `$` is
// decided by the length, never by a look at what follows.
#pragma once
#include <stdint.h>

#include "sx_select_core.hpp"

namespace sx {

// a compiled regex set where the kernel reads it (device pointers; in the harness: the builder's)
struct SelreDevice {
    const uint8_t* map;       // 256 bytes: byte -> class
    const uint16_t* next;     // states * classes entries
    uint32_t states, classes, lds_states, end_first, stop_first, matched, root_end, reserved;
};

struct SelreParams {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed, invert;
    uint64_t* wmask;         // per wavefront, as SelectParams (waves + 1 entries)
    uint32_t* wcount;
    uint64_t* wbytes;
    SelreDevice re;
};

// a lane's walk
struct SelreLane {
    uint64_t at, end;        // the next byte, the end of the string
    uint32_t state, len, active, reserved;
};

// Lane `lane` of wavefront `w` in front of its record's string (lanes behind the last record have none).
SXD SelreLane selre_begin_lane(const SelreParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    SelreLane L{ 0, 0, 0, 0, 0, 0 };
    if (i >= P.n) return L;
    uint64_t off;
    select_string(P, i, &off, &L.len);
    L.at = off; L.end = off + L.len; L.active = L.len != 0 && P.re.stop_first != 0;   // (stop_first == 0: the root is the only state)
    return L;
}

// One byte of the lane's string (L.active holds).  map: the 256 classes, rows: the first lds_states rows (LDS).
SXD void selre_step_lane(const SelreParams& P, const uint8_t* map, const uint16_t* rows, SelreLane& L) {
    const uint32_t at = L.state * P.re.classes + map[P.arena[L.at]];
    L.state = L.state < P.re.lds_states ? rows[at] : P.re.next[at];
    L.at++;
    if (L.state >= P.re.stop_first || L.at == L.end) L.active = 0;
}

// Is the lane's record selected (L.active no longer holds)?  The wavefront's mask is the ballot over this.
SXD bool selre_lane_selected(const SelreParams& P, uint64_t w, uint32_t lane, const SelreLane& L) {
    if (w * kSelectRecs + lane >= P.n) return false;
    const bool hit = L.state == P.re.matched || L.state - P.re.end_first < P.re.stop_first - P.re.end_first || (L.state == 0 && P.re.root_end);
    return hit != (P.invert != 0);
}

}  // namespace sx
