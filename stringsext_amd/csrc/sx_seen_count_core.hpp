// sx_seen_count_core.hpp — a seen set that COUNTS (SX_SEEN_COUNTED): per stored string how many results held it and how many findings
// they held of it; the counts read back where the findings lie (sx_result_seen_counts_device); and the selection by a bit field of a
// label word (sx_result_select_labels_range_device), which is how one selects by those counts.  What ONE lane does, written as lane
// functions.  Included by sx_seen_count_dev.hip with SXD = `__device__ __forceinline__`; the test-only harness
// tests/native/seen_count_host.cpp includes it with SXD = `inline`, so the very same code is checked against a Python Counter carried
// across calls on a machine without GPU (tests/test_seen_count_core.py).
//
// The counts: SeenSet::counts, one 64-bit word per SLOT, parallel to the slot table: results in the low half (SX_SEEN_RESULTS_SHIFT),
// findings in the high half (SX_SEEN_FINDINGS_SHIFT), each saturating at 2^32 - 1 on its own; the word of an empty slot is 0.  NULL:
// the set does not count, and nothing of this file runs for it.
// Counting is ONE rule, run BEHIND the add pass (sx_seen_core.hpp, sx_seen_merge_core.hpp) — every string of the call is held by
// then, so the lookup must succeed —, so that every dependency stays a kernel boundary:
//   count        a lane per record of a result; only SX_DISTINCT_FIRST records act.  The record looks its string up, gets the slot, and
//                adds (1, the class size in its word's high half) to counts[slot].
//   merge count  a lane per source word; every occupied lane looks its entry up in the destination, eight bytes at a time, and adds
//                the source's count: src_counts[i] if the source has counts, else (1, 1).
// The add is a plain load, add, store: FIRST records are pairwise different across the whole result, and so are a source's entries, so
// no two lanes of a call touch the same slot and no atomic is needed.  A lane that does not find its string, or exhausts the walk,
// raises the error total; the wavefront adds its number of counted classes to word kSeenCounted, behind the call's totals, which the
// host checks against what the mark pass counted.
//   lookup       a lane per record, no distinct pass in front: the record's word becomes counts[slot] of its string, or 0 if the set
//                does not hold it.  The set is read; only the words and the error total are written.
//   range pick   pass 1 of a selection: a record is selected iff lo <= ((label >> shift) & mask(bits)) <= hi.  It reads the label
//                and the record's str_len, no string byte, and leaves what label_pick_lane leaves.
#pragma once
#include <stdint.h>

#include "sx_seen_merge_core.hpp"

namespace sx {

constexpr uint32_t kSeenCounted = kSeenTotals;                 // the word behind a call's totals: the classes / entries the count pass counted
constexpr uint64_t kSeenCountOnce = (uint64_t)1 << SX_SEEN_FINDINGS_SHIFT | (uint64_t)1 << SX_SEEN_RESULTS_SHIFT;      // (1, 1): what a plain source's entry adds

// (results, findings) of a and of b added, each half saturating at 2^32 - 1 on its own
SXD uint64_t seen_count_sum(uint64_t a, uint64_t b) {
    uint64_t lo = (a & 0xFFFFFFFFu) + (b & 0xFFFFFFFFu), hi = (a >> 32) + (b >> 32);
    if (lo > 0xFFFFFFFFu) lo = 0xFFFFFFFFu;
    if (hi > 0xFFFFFFFFu) hi = 0xFFFFFFFFu;
    return hi << 32 | lo;
}

// count, lane `lane` of wavefront `w` of a segment (P as the add pass had it; P.set.counts is not NULL).  *counted = the record was
// the first of its class and its slot's word got (1, class size); *lost = it was, and the set did not hold its string or the walk
// tried every slot.  The wavefront adds the ballots' popcounts to P.totals[kSeenCounted] and P.totals[kSeenError].
SXD void seen_count_lane(const SeenParams& P, uint64_t w, uint32_t lane, bool* counted, bool* lost) {
    const uint64_t i = w * kSelectRecs + lane;
    *counted = *lost = false;
    if (i >= P.n) return;
    const uint64_t word = P.labels[i];
    if (!(word & SX_DISTINCT_FIRST)) return;
    uint64_t off, slot = 0; uint32_t len;
    select_string(P, i, &off, &len);
    bool exhausted = false;
    const bool held = seen_find_at(P.set, P.arena + off, len, &exhausted, &slot);
    if (held) P.set.counts[slot] = seen_count_sum(P.set.counts[slot], (word >> SX_DISTINCT_COUNT_SHIFT) << SX_SEEN_FINDINGS_SHIFT | (uint64_t)1 << SX_SEEN_RESULTS_SHIFT);
    *counted = held; *lost = !held;
}

// A source of entries and what its entries count: src_counts[i] belongs to source word i (a set's count table beside its slot table,
// or the array the host uploaded beside a list); NULL: every entry counts (1, 1)
struct SeenMergeCountParams {
    SeenMergeParams m;           // the source and the destination as the add pass had them (held is not read)
    const uint64_t* src_counts;
};

// merge count, lane `lane` of wavefront `w`: as seen_count_lane, for source word w * 64 + lane
SXD void seen_merge_count_lane(const SeenMergeCountParams& C, uint64_t w, uint32_t lane, bool* counted, bool* lost) {
    const SeenMergeParams& P = C.m;
    const uint64_t i = w * kSelectRecs + lane;
    *counted = *lost = false;
    const uint64_t* entry = seen_merge_entry(P, i);
    if (!entry) return;
    uint64_t slot = 0;
    bool exhausted = false;
    const bool held = seen_merge_find_at(P.set, entry, seen_merge_hash(entry, P.set.nocase), &exhausted, &slot);
    if (held) P.set.counts[slot] = seen_count_sum(P.set.counts[slot], C.src_counts ? C.src_counts[i] : kSeenCountOnce);
    *counted = held; *lost = !held;
}

// lookup, lane `lane` of wavefront `w` of a segment: P.labels[i] = the count word of record i's string, 0 if the set does not hold
// it.  true: the walk tried every slot (the wavefront adds that to P.totals[kSeenError])
SXD bool seen_counts_lookup_lane(const SeenParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    if (i >= P.n) return false;
    uint64_t off, slot = 0; uint32_t len;
    select_string(P, i, &off, &len);
    bool exhausted = false;
    const bool held = seen_find_at(P.set, P.arena + off, len, &exhausted, &slot);
    P.labels[i] = held ? P.set.counts[slot] : 0u;
    return exhausted;
}

// The selection by a field of a label word: one segment's labels and the call's field and bounds (1 <= bits, shift + bits <= 64)
struct LabelRange {
    const uint64_t* labels;      // n words, in record order
    uint64_t lo, hi;
    uint32_t shift, bits;
};

SXD bool label_in_range(uint64_t label, uint32_t shift, uint32_t bits, uint64_t lo, uint64_t hi) {
    const uint64_t v = (label >> shift) & (bits >= 64u ? ~(uint64_t)0 : ((uint64_t)1 << bits) - 1u);
    return lo <= v && v <= hi;
}

// Pass 1 of the selection by range, lane `lane` of wavefront `w`: as label_pick_lane
SXD bool label_range_pick_lane(const SelectParams& S, const LabelRange& K, uint64_t w, uint32_t lane, uint32_t* len) {
    const uint64_t i = w * kSelectRecs + lane;
    *len = 0;
    if (i >= S.n || !label_in_range(K.labels[i], K.shift, K.bits, K.lo, K.hi)) return false;
    *len = S.packed ? ((const sx_finding16*)S.recs)[i].str_len : ((const sx_finding*)S.recs)[i].str_len;
    return true;
}

}  // namespace sx
