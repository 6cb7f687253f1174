// sx_distinct_core.hpp — the duplicate strings of a result that lies in HBM (sx_result_distinct_device): what ONE lane does for its
// record, written as lane functions.  Included by sx_distinct_dev.hip with SXD = `__device__ __forceinline__`; the test-only harness
// tests/native/distinct_core_host.cpp includes it with SXD = `inline`, so the very same code is checked against a Python dict over the
// strings on a machine without GPU (tests/test_distinct_core.py).
//
// The rule: two findings are equal iff their strings are byte for byte equal — with `nocase` after 'A'..'Z' became 'a'..'z', no other
// byte —, across segments and Missions; empty strings are equal.  A finding's KEY is segment << 32 | record: the u64 order of keys is
// the print order.  Per finding one word: bit 0 (SX_DISTINCT_FIRST) no finding with a smaller key is equal to it, bit 1
// (SX_DISTINCT_REPEATED) some other finding is, bits 32..63 the size of its class, saturated.
//
// A tournament by hash, exact whatever the hash does.  The call holds a table of 2^table_log2 slots, per finding `rep` (unresolved at
// first) and `count`, and one counter.  Round r = two launches per segment, lane per record:
//   claim    an unresolved record hashes its (folded) string with a hash seeded by r, takes its slot from the hash's high bits, notes
//            the slot in its `rep` (top bit set: still unresolved) and lowers the slot to its key — a 64-bit minimum behind a plain
//            load, as seltally's first[]: a string that occurs a million times issues a handful of atomics, not a million.
//   resolve  (behind every segment's claim: a kernel boundary) an unresolved record reads its slot's winner and compares its own
//            string with the winner's, length first.  Equal: rep = the winner's key, count[winner] += 1 (the winner meets itself).
//            Not equal: it stays unresolved; the wavefront adds the popcount of the ballot over that to the counter.
//            The adds to `count` are one per RUN of neighbouring lanes that found the same winner (distinct_count_run): a merged
//            result holds the Missions' findings of one place side by side, and a line that fills a region holds it a million times
//            in a row — a lane per add put them all on one address (54 ms where the part without that line takes 5, r18a).
// Equal strings hash alike under every seed: they share slot and winner in every round and resolve in the same one, to the smallest
// key among them.  A slot that anyone claimed resolves at least its winner's class: every round lowers the counter, and the host stops
// at 0 (a round that does not lower it is an error there, never a reason to go on).
//   finalize (behind the last round) word = (rep == own key) | (count[rep] > 1) << 1 | min(count[rep], 2^32 - 1) << 32, and per
//            wavefront one add each of the ballots' popcounts to `distinct` and `repeated`.
// No lane waits for another; sums and minima do not depend on the order: words and counters are deterministic.  A lane reads the bytes
// [str_off, str_off + str_len) of its own record and of its slot's winner, and no other byte of any arena.
// `count` is 64 bits wide: a class larger than 2^32 - 1 saturates in finalize instead of wrapping in the add.
#pragma once
#include <stdint.h>

#include "sx_select_core.hpp"
#include "sx_seltally_core.hpp"

namespace sx {

constexpr uint64_t kDistinctUnresolved = (uint64_t)1 << 63;    // rep's top bit: no class yet; the other bits = the slot claimed this round
constexpr uint64_t kDistinctEmptySlot = ~(uint64_t)0;          // a slot nobody has claimed: larger than every key

// a segment of the source where it lies (device pointers; in the harness: the test's), and where its findings' rep and count begin
struct DistinctSeg {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed, reserved;
    uint64_t base;           // the findings of the segments in front of it
};

struct DistinctParams {
    const void* recs;        // the segment this launch walks, as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed;
    uint32_t seg;            // its index: the high half of its records' keys
    uint64_t base;           // as DistinctSeg
    const DistinctSeg* segs; // every segment of the result: a key leads to its string
    uint32_t n_segs, nocase, round, table_log2;
    uint64_t* table;         // 2^table_log2 slots, kDistinctEmptySlot in front of every claim
    uint64_t* rep;           // per finding of the result
    uint64_t* count;         // per finding of the result: the members of the class it is the first of
    uint64_t* unresolved;    // resolve adds the records it leaves
    uint64_t* labels;        // finalize: the segment's n words
    uint64_t* totals;        // finalize adds: [0] distinct, [1] repeated
};

SXD uint64_t distinct_mix(uint64_t h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ h >> 33;
}

// The 64-bit hash of a (folded) string and its length under round `round`'s seed
SXD uint64_t distinct_hash(const uint8_t* s, uint32_t len, uint32_t nocase, uint32_t round) {
    uint64_t h = distinct_mix(0xcbf29ce484222325ull + (uint64_t)(round + 1u) * 0x9e3779b97f4a7c15ull);
    for (uint32_t j = 0; j < len; j++) h = (h ^ select_fold(nocase, s[j])) * 0x100000001b3ull;
    return distinct_mix(h ^ (uint64_t)len << 32);
}

SXD uint64_t distinct_slot(uint64_t hash, uint32_t table_log2) { return table_log2 ? hash >> (64u - table_log2) : 0u; }

// claim, lane `lane` of wavefront `w`
SXD void distinct_claim_lane(const DistinctParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    if (i >= P.n || !(P.rep[P.base + i] & kDistinctUnresolved)) return;
    uint64_t off; uint32_t len;
    select_string(P, i, &off, &len);
    const uint64_t slot = distinct_slot(distinct_hash(P.arena + off, len, P.nocase, P.round), P.table_log2);
    P.rep[P.base + i] = kDistinctUnresolved | slot;
    seltally_min64(P.table + slot, (uint64_t)P.seg << 32 | i);
}

// what resolve made of a lane's record
enum DistinctResolved : uint32_t {
    kDistinctNothing = 0,    // no record, or one that has its class from an earlier round
    kDistinctStays = 1,      // still unresolved (the wavefront adds the ballot's popcount to P.unresolved)
    kDistinctFound = 2       // it equals its slot's winner: rep is written, *widx = where the winner's count lies (distinct_count_run adds)
};

// resolve, lane `lane` of wavefront `w`
SXD uint32_t distinct_resolve_lane(const DistinctParams& P, uint64_t w, uint32_t lane, uint64_t* widx) {
    const uint64_t i = w * kSelectRecs + lane;
    *widx = 0;
    if (i >= P.n) return kDistinctNothing;
    const uint64_t mine = P.rep[P.base + i];
    if (!(mine & kDistinctUnresolved)) return kDistinctNothing;
    const uint64_t key = (uint64_t)P.seg << 32 | i, winner = P.table[mine & ~kDistinctUnresolved];
    if (winner >> 32 >= P.n_segs) return kDistinctStays;      // (an empty slot, which no record's own slot is: it stays unresolved, and the host sees a round without progress)
    const DistinctSeg& W = P.segs[winner >> 32];
    const uint64_t wi = winner & 0xFFFFFFFFu;
    if (winner != key) {
        uint64_t off, woff; uint32_t len, wlen;
        select_string(P, i, &off, &len);
        select_string(W, wi, &woff, &wlen);
        if (len != wlen) return kDistinctStays;
        const uint8_t* a = P.arena + off;
        const uint8_t* b = W.arena + woff;
        for (uint32_t j = 0; j < len; j++)
            if (select_fold(P.nocase, a[j]) != select_fold(P.nocase, b[j])) return kDistinctStays;
    }
    P.rep[P.base + i] = winner;
    *widx = W.base + wi;
    return kDistinctFound;
}

// The adds of one wavefront's resolve, lane `lane`: `found` = the ballot over kDistinctFound, `heads` = the ballot over "found, and
// the lane to the left did not find the same winner" (lane 0 is a head if it found).  A head adds the length of its run: the lanes
// from it to the next head or the next lane that found nothing.
SXD void distinct_count_run(const DistinctParams& P, uint32_t lane, uint64_t found, uint64_t heads, uint64_t widx) {
    if (!((heads >> lane) & 1u)) return;
    const uint64_t behind = lane == kSelectRecs - 1 ? 0u : ~(uint64_t)0 << (lane + 1u);
    const uint64_t stop = (heads | ~found) & behind;
    const uint32_t end = stop ? (uint32_t)__builtin_ctzll(stop) : kSelectRecs;
    seltally_add64(P.count + widx, end - lane);
}

// finalize, lane `lane` of wavefront `w`: its record's word is written; *first = it is the first of its class, *repeated = and the
// class has other members (the wavefront adds the two ballots' popcounts to P.totals)
SXD void distinct_finalize_lane(const DistinctParams& P, uint64_t w, uint32_t lane, bool* first, bool* repeated) {
    const uint64_t i = w * kSelectRecs + lane;
    *first = *repeated = false;
    if (i >= P.n) return;
    const uint64_t rep = P.rep[P.base + i];
    if (rep >> 32 >= P.n_segs) { P.labels[i] = 0; return; }      // (unresolved: the host launches this behind a counter of 0 only)
    const uint64_t c = P.count[P.segs[rep >> 32].base + (rep & 0xFFFFFFFFu)];
    *first = rep == ((uint64_t)P.seg << 32 | i);
    *repeated = *first && c > 1;
    P.labels[i] = (*first ? (uint64_t)SX_DISTINCT_FIRST : 0u) | (c > 1 ? (uint64_t)SX_DISTINCT_REPEATED : 0u)
                  | (c < 0xFFFFFFFFu ? c : 0xFFFFFFFFu) << SX_DISTINCT_COUNT_SHIFT;
}

}  // namespace sx
