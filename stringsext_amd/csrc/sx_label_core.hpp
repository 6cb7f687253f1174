// sx_label_core.hpp — the labels of the findings of a segment that lies in HBM (sx_result_label_device) and the selection by label
// (sx_result_select_labels_device): what ONE lane does for its record, written as lane functions.  Included by sx_label_dev.hip with
// SXD = `__device__ __forceinline__`; the test-only harness tests/native/label_core_host.cpp includes it with SXD = `inline`, so the
// very same code is checked against Python's re.search per pattern on a machine without GPU (tests/test_label_core.py).
//
// The rule: bit p of finding i's label is set iff pattern p of the set is found somewhere in its string; a match never spans two
// findings; the bits of patterns the set does not have are 0.  The patterns arrive as the DFA sx_label_build.hpp describes.
//
// One lane, one record: the lane's label starts as the root's `here` (`a*`, `^`), its state is the root in front of its record's
// first byte and takes one step per byte — next[state * classes + map[byte]], from LDS for the first lds_states states, from the
// table in HBM (through L2) for the others —; a step into a state >= here_first ORs that state's `here` into the label.  A lane is
// done behind its last byte, where its state's `end` is ORed in (`$`), in `dead` — nothing that follows can match —, or when its label
// holds every pattern's bit: a one-pattern set then costs what the regex selection costs.  An empty string is decided by the root:
// its `here` and its `end`.  A record's state never sees another record's bytes: a lane reads the bytes [str_off, str_off + str_len)
// of its own record and no other byte of the arena — `$` is decided by the length, never by a look at what follows.
//
// Counting: findings[p] += the records with bit p, first[p] = min(first[p], ordinal of such a record).  Per wavefront the lanes' labels
// are ORed; for every bit of that the ballot over "my label has it" gives the count (its popcount) and the first record (its lowest
// lane).  A workgroup keeps 64 32-bit counters and 64 64-bit minima in LDS (a wavefront adds at most 64 to a counter, a segment has
// less than 2^32 records) and flushes them when it ends as seltally_kernel does: one 64-bit global add per non-zero counter, the
// minimum behind a plain load.  Sums and minima do not depend on the order: the counters are deterministic.
//
// The selection by label (label_pick_lane) is pass 1 of a selection: it reads a record's label and its str_len, no string byte,
// and leaves what select_match_kernel leaves.
#pragma once
#include <stdint.h>

#include "sx_select_core.hpp"
#include "sx_seltally_core.hpp"

namespace sx {

constexpr uint32_t kLabelBits = 64;      // patterns a set may hold: a label is one 64-bit word

// a compiled label set where the kernel reads it (device pointers; in the harness: the builder's)
struct LabelDevice {
    const uint8_t* map;       // 256 bytes: byte -> class
    const uint16_t* next;     // states * classes entries
    const uint64_t* here;     // states - here_first entries
    const uint64_t* end;      // states entries
    uint64_t* findings;       // kLabelBits counters
    uint64_t* first;          // kLabelBits minima
    uint64_t root_here, all;
    uint32_t states, classes, lds_states, here_first, dead, n_patterns;
};

struct LabelParams {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed, reserved;
    uint64_t ordinal;        // of the segment's record 0: ordinal_base + the findings of the segments in front of it
    uint64_t* labels;        // n words, in record order
    LabelDevice set;
};

// a lane's walk
struct LabelLane {
    uint64_t at, end;        // the next byte, the end of the string
    uint64_t acc;            // the label so far
    uint32_t state, active;
};

// Lane `lane` of wavefront `w` in front of its record's string (lanes behind the last record have none, and the label 0).
SXD LabelLane label_begin_lane(const LabelParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    LabelLane L{ 0, 0, 0, 0, 0 };
    if (i >= P.n) return L;
    uint64_t off; uint32_t len;
    select_string(P, i, &off, &len);
    L.at = off; L.end = off + len; L.acc = P.set.root_here;
    if (len == 0) L.acc |= P.set.end[0];
    else L.active = L.acc != P.set.all && P.set.dead != 0;      // (dead == 0: the root is the only state)
    return L;
}

// One byte of the lane's string (L.active holds).  map: the 256 classes, rows: the first lds_states rows (LDS).
SXD void label_step_lane(const LabelParams& P, const uint8_t* map, const uint16_t* rows, LabelLane& L) {
    const uint32_t at = L.state * P.set.classes + map[P.arena[L.at]];
    L.state = L.state < P.set.lds_states ? rows[at] : P.set.next[at];
    L.at++;
    if (L.state >= P.set.here_first) L.acc |= P.set.here[L.state - P.set.here_first];
    if (L.at == L.end) { L.acc |= P.set.end[L.state]; L.active = 0; }
    else if (L.state == P.set.dead || L.acc == P.set.all) L.active = 0;
}

// Bit p of the wavefront's ORed labels: `ballot` = the lanes whose label has it (not 0), ordinal0 = the ordinal of the wavefront's
// lane 0.  counts, mins: the workgroup's kLabelBits counters and minima (LDS).  On the device lane p calls this for bit p.
SXD void label_count_bit(uint32_t* counts, uint64_t* mins, uint32_t p, uint64_t ballot, uint64_t ordinal0) {
    seltally_add32(counts + p, (uint32_t)__builtin_popcountll(ballot));
    const uint64_t ordinal = ordinal0 + (uint32_t)__builtin_ctzll(ballot);
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin((unsigned long long*)(mins + p), (unsigned long long)ordinal);
#else
    if (mins[p] > ordinal) mins[p] = ordinal;
#endif
}

// When the workgroup's wavefronts are done: counter c of the workgroup's counters and minima into the set's (c < kLabelBits).
// (PP: LabelParams, or the FuzzyParams of sx_fuzzy_core.hpp)
template <class PP>
SXD void label_flush_lane(const PP& P, const uint32_t* counts, const uint64_t* mins, uint32_t c) {
    const uint32_t v = counts[c];
    if (!v) return;
    seltally_add64(P.set.findings + c, v);
    seltally_min64(P.set.first + c, mins[c]);
}

// The selection by label: one segment's labels and the call's three masks
struct LabelPick {
    const uint64_t* labels;      // n words, in record order
    uint64_t any, all, none;
};

SXD bool label_picked(uint64_t label, uint64_t any, uint64_t all, uint64_t none) {
    return (any == 0 || (label & any) != 0) && (label & all) == all && (label & none) == 0;
}

// Pass 1 of the selection by label, lane `lane` of wavefront `w`: is its record selected, and its string's length (S: the segment
// as SelectParams names it; nothing of the arena is read)
SXD bool label_pick_lane(const SelectParams& S, const LabelPick& K, uint64_t w, uint32_t lane, uint32_t* len) {
    const uint64_t i = w * kSelectRecs + lane;
    *len = 0;
    if (i >= S.n || !label_picked(K.labels[i], K.any, K.all, K.none)) return false;
    *len = S.packed ? ((const sx_finding16*)S.recs)[i].str_len : ((const sx_finding*)S.recs)[i].str_len;
    return true;
}

}  // namespace sx
