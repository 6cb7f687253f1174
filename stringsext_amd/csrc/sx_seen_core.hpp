// sx_seen_core.hpp — the seen set (sx_seen_set, sx_result_seen_device): strings remembered in HBM from one result to the next.  This
// file owns THE SET — its slot words (seen_entry_at), its bounded walk for lookups (seen_lookup) and for inserts (seen_claim), its
// call totals (SeenTotal) and its validity (seen_set_ok) — and what ONE lane does for a RECORD of a result, written as lane functions;
// sx_seen_merge_core.hpp puts entries that are already a set's through the same two walks, and sx_seen_count_core.hpp, for a set that
// counts (SeenSet::counts), through the lookup's walk once more, which says on which slot it ended.  Included by sx_seen_dev.hip with SXD =
// `__device__ __forceinline__`; the test-only harness tests/native/seen_core_host.cpp includes it with SXD = `inline`, so the very same
// code is checked against a Python set carried across calls on a machine without GPU (tests/test_seen_core.py).
//
// The set: 2^table_log2 slots — the power of two >= 2 x capacity_strings, so a probe always meets an empty slot — and one arena of
// capacity_bytes.  A slot is kSeenEmpty or tag << 40 | entry_offset / 8; an entry is [u32 len][u32 0][the (folded) bytes, zero-padded
// to 8], 8-byte aligned: SX_SEEN_ENTRY_BYTES(len).  Two cursors count what the arena holds: strings and bytes.  A string's hash is
// distinct_hash under the set's own seed; its home slot is the hash's high bits, its tag the hash's low tag_bits (0: every occupied
// slot on the way is compared byte for byte).  Equality is the distinct pass's, under the SET's fold: the set stores folded bytes.
//
// Behind distinct's finalize, which has written every record's word, two passes, lane per record:
//   mark  walks from the home slot: empty = not seen; another tag = next slot; the same tag = the entry's length, then its bytes,
//         against the record's (folded) string: equal = seen, else next slot.  The walk is bounded by the number of slots; a lane that
//         exhausts it raises the error word (the host gives up, as for a distinct round without progress).  SX_DISTINCT_SEEN is ORed
//         into the record's word, and per wavefront the ballots' popcounts are added: seen findings, seen classes (FIRST && SEEN),
//         new classes (FIRST && !SEEN) and the new classes' entry bytes.  The table is read; only words and counters are written.
//   add   (behind every segment's mark, and behind the host's look at the totals: what is new fits) only FIRST && !SEEN records act.
//         They are pairwise different and different from everything the set holds, so no inserter reads another's entry.  A
//         wavefront takes its entries' room with ONE add to the byte cursor — the lanes share it by an exclusive prefix of their
//         entry sizes (wave_reserve, sx_rows_dev.hpp) — and counts them with one add to the string cursor; a lane writes its entry
//         and then walks from its home slot with a 64-bit compare-and-swap kSeenEmpty -> its word until one succeeds.  It compares no
//         string.  A lane whose walk tried every slot says so, and the wavefront adds that to the error word.
// No lane waits for another: every dependency is a kernel boundary.  Words, totals and cursors are sums: deterministic.  WHERE an
// entry lies depends on the order of the adds, and is no part of the contract.  A lane reads the bytes [str_off, str_off + str_len)
// of its own record and the bytes of entries of the set, and no other byte of any arena.
#pragma once
#include <stdint.h>

#include "sx_distinct_core.hpp"

namespace sx {

constexpr uint64_t kSeenEmpty = ~(uint64_t)0;                  // a slot without an entry (no word of an entry is all ones: offsets end below 2^40)
constexpr uint32_t kSeenOffsetBits = 40;                       // a slot's low bits: entry_offset / 8
constexpr uint32_t kSeenMaxTagBits = 24;
constexpr uint32_t kSeenSeed = 0x5EE25E70u;                    // the set's own seed: distinct_hash's `round`, unlike any round of a tournament
// A call's totals.  Words 0 and 1 are, for a result, the seen findings and the seen classes; for a source of entries (sx_seen_merge_core.hpp),
// the occupied words and those the destination held.  What is new, its entry bytes and the error — a lookup that walked every slot, an
// adder that found none — are the same words for both.
enum SeenTotal : uint32_t { kSeenFindings = 0, kSeenClasses = 1, kSeenNewClasses = 2, kSeenNewBytes = 3, kSeenError = 4, kSeenTotals = 5,
                            // (the same words, as a source of entries names them)
                            kSeenMergeOccupied = 0, kSeenMergeHeld = 1, kSeenMergeNew = 2, kSeenMergeNewBytes = 3, kSeenMergeError = 4, kSeenMergeTotals = 5 };

// the set where it lies (device pointers; in the harness: the test's)
struct SeenSet {
    uint64_t* slots;         // 2^table_log2
    uint8_t* arena;          // capacity_bytes, 8-byte aligned
    uint64_t* cursors;       // [0] the strings the set holds, [1] their entries' bytes: where the next entry begins
    uint32_t table_log2, tag_bits, nocase, reserved;
    uint64_t* counts;        // NULL: the set does not count; else 2^table_log2 words, one per slot (sx_seen_count_core.hpp), 0 where the slot is empty
};
// (a set the kernels can walk: what both launchers ask)
inline bool seen_set_ok(const SeenSet& S) {
    return S.slots && S.arena && S.cursors && S.table_log2 >= 1 && S.table_log2 <= 41 && S.tag_bits <= kSeenMaxTagBits;
}

struct SeenParams {
    const void* recs;        // the segment this launch walks, as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed, reserved;
    uint64_t* labels;        // the segment's n words, as distinct's finalize wrote them; mark ORs SX_DISTINCT_SEEN
    uint64_t* totals;        // kSeenTotals words: mark adds; add adds to the error alone
    SeenSet set;
};

// (the harness runs the lanes one after the other; on the device the add to the byte cursor is wave_reserve's)
SXD uint64_t seen_fetch_add64(uint64_t* word, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd((unsigned long long*)word, (unsigned long long)v);
#else
    const uint64_t old = *word;
    *word += v;
    return old;
#endif
}
SXD bool seen_claim_slot(uint64_t* slot, uint64_t word) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS((unsigned long long*)slot, (unsigned long long)kSeenEmpty, (unsigned long long)word) == (unsigned long long)kSeenEmpty;
#else
    if (*slot != kSeenEmpty) return false;
    *slot = word;
    return true;
#endif
}

SXD uint64_t seen_entry_bytes(uint32_t len) { return SX_SEEN_ENTRY_BYTES(len); }
SXD uint64_t seen_tag(const SeenSet& S, uint64_t hash) { return hash & (((uint64_t)1 << S.tag_bits) - 1u); }
// The entry an occupied slot's (or source's) word points to; the bits above the offset are not read
SXD const uint8_t* seen_entry_at(const uint8_t* arena, uint64_t word) { return arena + (word & (((uint64_t)1 << kSeenOffsetBits) - 1u)) * 8u; }

// THE walk of a lookup.  Does the set hold the string whose hash is `hash`?  From the home slot on: empty = no; another tag = next
// slot; the same tag = same(entry) decides, the caller's comparison, inlined.  *exhausted: every slot was looked at and none was empty.
// *slot_out: the slot the string's entry has, written only where the answer is yes
template <class Same>
SXD bool seen_lookup_at(const SeenSet& S, uint64_t hash, Same same, bool* exhausted, uint64_t* slot_out) {
    const uint64_t mask = ((uint64_t)1 << S.table_log2) - 1u, tag = seen_tag(S, hash);
    uint64_t slot = distinct_slot(hash, S.table_log2);
    for (uint64_t walked = 0; walked <= mask; walked++, slot = (slot + 1u) & mask) {
        const uint64_t word = S.slots[slot];
        if (word == kSeenEmpty) return false;
        if (word >> kSeenOffsetBits == tag && same(seen_entry_at(S.arena, word))) { *slot_out = slot; return true; }
    }
    *exhausted = true;
    return false;
}
template <class Same>
SXD bool seen_lookup(const SeenSet& S, uint64_t hash, Same same, bool* exhausted) {
    uint64_t slot;
    return seen_lookup_at(S, hash, same, exhausted, &slot);
}

// THE walk of an insert: the entry at arena offset `at`, whose hash is `hash`, takes the first empty slot from its home slot on.
// false: every slot was tried (the host has checked strings <= slots / 2, so it is an error of the table's, not a full set)
SXD bool seen_claim(const SeenSet& S, uint64_t hash, uint64_t at) {
    const uint64_t mask = ((uint64_t)1 << S.table_log2) - 1u, word = seen_tag(S, hash) << kSeenOffsetBits | at / 8u;
    uint64_t slot = distinct_slot(hash, S.table_log2);
    for (uint64_t walked = 0; walked <= mask; walked++, slot = (slot + 1u) & mask)
        if (seen_claim_slot(S.slots + slot, word)) return true;
    return false;
}

// Does the set hold the (folded) string s[0, len)?  Byte for byte: a record's string is neither aligned nor padded.  *slot_out: as
// seen_lookup_at's
SXD bool seen_find_at(const SeenSet& S, const uint8_t* s, uint32_t len, bool* exhausted, uint64_t* slot_out) {
    return seen_lookup_at(S, distinct_hash(s, len, S.nocase, kSeenSeed), [&](const uint8_t* entry) {
        if (*(const uint32_t*)entry != len) return false;
        uint32_t j = 0;
        while (j < len && entry[8u + j] == select_fold(S.nocase, s[j])) j++;
        return j == len;
    }, exhausted, slot_out);
}
SXD bool seen_find(const SeenSet& S, const uint8_t* s, uint32_t len, bool* exhausted) {
    uint64_t slot;
    return seen_find_at(S, s, len, exhausted, &slot);
}

// mark, lane `lane` of wavefront `w`: its record's word gets SX_DISTINCT_SEEN if the set holds its string.  *seen = it does; *first =
// the record is the first of its class; *bytes = the entry a new class will take (0 unless first and not seen).  The wavefront adds
// the ballots' popcounts and the sum of *bytes to P.totals.
SXD void seen_mark_lane(const SeenParams& P, uint64_t w, uint32_t lane, bool* seen, bool* first, uint64_t* bytes) {
    const uint64_t i = w * kSelectRecs + lane;
    *seen = *first = false; *bytes = 0;
    if (i >= P.n) return;
    uint64_t off; uint32_t len;
    select_string(P, i, &off, &len);
    bool exhausted = false;
    *seen = seen_find(P.set, P.arena + off, len, &exhausted);
    if (exhausted) seltally_add64(P.totals + kSeenError, 1u);
    const uint64_t word = P.labels[i];
    *first = (word & SX_DISTINCT_FIRST) != 0;
    if (*seen) P.labels[i] = word | SX_DISTINCT_SEEN;
    else if (*first) *bytes = seen_entry_bytes(len);
}

// add, step 1, lane `lane` of wavefront `w`: the bytes of the entry its record adds, 0 = it adds none (an entry has 8 bytes at least)
SXD uint64_t seen_add_size_lane(const SeenParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    if (i >= P.n || (P.labels[i] & (SX_DISTINCT_FIRST | SX_DISTINCT_SEEN)) != SX_DISTINCT_FIRST) return 0;
    uint64_t off; uint32_t len;
    select_string(P, i, &off, &len);
    return seen_entry_bytes(len);
}

// add, step 2, a lane whose step 1 gave bytes: `at` = where its entry begins — what the wavefront's one add to the byte cursor gave
// back, plus the entry bytes of the lanes in front of it.  The entry is written, folded, 8 bytes at a time; then seen_claim.  false:
// it found no slot (the wavefront adds that to the error total)
SXD bool seen_add_lane(const SeenParams& P, uint64_t w, uint32_t lane, uint64_t at) {
    const SeenSet& S = P.set;
    uint64_t off; uint32_t len;
    select_string(P, w * kSelectRecs + lane, &off, &len);
    const uint8_t* s = P.arena + off;
    uint64_t* entry = (uint64_t*)(S.arena + at);
    entry[0] = len;                                              // [u32 len][u32 0]
    for (uint32_t j = 0; j < len; j += 8) {
        uint64_t v = 0;
        for (uint32_t k = 0; k < 8 && j + k < len; k++) v |= (uint64_t)select_fold(S.nocase, s[j + k]) << (8u * k);
        entry[1u + j / 8u] = v;
    }
    return seen_claim(S, distinct_hash(s, len, S.nocase, kSeenSeed), at);
}

}  // namespace sx
