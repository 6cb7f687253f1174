// sx_seen_merge_core.hpp — entries that are ALREADY a set, put into a seen set (sx_seen_set_merge, _grow, _import, _add_strings): what
// ONE lane does for its source word, written as lane functions.  The set itself — its slot words, the walk of a lookup, the walk of an
// insert, the totals — is sx_seen_core.hpp's; this file owns the source, the hash of an entry and the word-wise comparison.  Included by sx_seen_merge_dev.hip with SXD = `__device__
// __forceinline__`; the test-only harness tests/native/seen_merge_host.cpp includes it with SXD = `inline`, so the very same code is
// checked against Python sets on a machine without GPU (tests/test_seen_merge_core.py).
//
// The source: n words and the arena their entries lie in.  A word is kSeenEmpty — skipped — or a word whose low kSeenOffsetBits bits
// are entry_offset / 8 into that arena; the high bits are not read.  So a live set's slot table is a source as it lies, and so is a
// dense list the host built from a blob or from strings.  An entry is a seen set's: [u32 len][u32 0][the bytes, zero-padded to 8],
// 8-byte aligned.  What the source promises — a set's invariant, which the host establishes for what it builds —: its entries are
// pairwise different and folded under the DESTINATION's fold.  That splits the work as seen_mark and seen_add split it:
//   mark  a lane per source word.  An occupied lane hashes its entry and looks it up in the destination; lane 0 of the wavefront
//         writes the ballot "the destination held it" to held[w], and the wavefront adds five totals: occupied, held, new, the new
//         entries' bytes, error (a probe that walked every slot).  The destination is read; only held[] and the totals are written.
//   add   (behind mark, and behind the host's look at the cursors and the totals: what is new fits) only occupied lanes whose bit of
//         held[w] is clear act.  They are pairwise different and different from everything the destination holds, so no inserter
//         reads another's entry.  Room is taken as seen_add takes it — wave_reserve: an exclusive prefix of the lanes' entry sizes,
//         then one add to the byte cursor — but for kSeenMergeAddChunks chunks of 64 words at once, a word of every chunk per lane, whose entries
//         then lie one behind the other; the string cursor gets one add per wavefront, behind its last trip.  A lane copies an
//         entry, then walks from the home slot with a compare-and-swap.
// ENTRIES ARE MOVED AND COMPARED EIGHT BYTES AT A TIME.  Both sides are 8-byte aligned and zero-padded and their second u32 is 0, so
// two entries are equal iff their 1 + ceil(len / 8) words are, the first of which carries the length; a copy is those words.  The hash
// is distinct_hash(bytes, len, nocase, kSeenSeed) bit for bit, its bytes taken out of the words (seen_merge_hash); folding folded bytes
// changes nothing, so the destination's nocase is passed as it is.
// No lane waits for another: every dependency is a kernel boundary.  held[], the totals and the cursors are ballots and sums:
// deterministic.  A lane reads its own source word, its own entry and entries of the destination, and no other byte of any arena.
#pragma once
#include <stdint.h>

#include "sx_seen_core.hpp"

namespace sx {

// The chunks of 64 source words a wavefront of the add pass takes per trip, a word of every chunk per lane, with ONE add to the byte
// cursor: every wavefront of the grid adds to that one address, and at a chunk per add the adds alone took 24 ns per chunk — 25 ms for a
// table of 2^26 slots, whatever it held.
constexpr uint32_t kSeenMergeAddChunks = 8;

struct SeenMergeParams {
    const uint64_t* words;       // the source's n words
    const uint8_t* src_arena;    // where their entries lie, 8-byte aligned
    uint64_t n;
    uint64_t* held;              // ceil(n / 64) words: mark writes, add reads
    uint64_t* totals;            // kSeenMergeTotals words (occupied, held, new, new bytes, error): mark adds; add adds to the error alone
    SeenSet set;                 // the destination
};

// The entry of source word i; NULL: there is no such word, or it is empty
SXD const uint64_t* seen_merge_entry(const SeenMergeParams& P, uint64_t i) {
    if (i >= P.n) return nullptr;
    const uint64_t word = P.words[i];
    if (word == kSeenEmpty) return nullptr;
    return (const uint64_t*)seen_entry_at(P.src_arena, word);
}

// distinct_hash(the entry's bytes, len, nocase, kSeenSeed), a word of the entry at a time: begin, every word with the bytes it holds
// (8, the last one len % 8 if that is not 0), end
SXD uint64_t seen_merge_hash_begin() { return distinct_mix(0xcbf29ce484222325ull + (uint64_t)(kSeenSeed + 1u) * 0x9e3779b97f4a7c15ull); }
SXD uint64_t seen_merge_hash_word(uint64_t h, uint64_t v, uint32_t bytes, uint32_t nocase) {
    for (uint32_t k = 0; k < bytes; k++, v >>= 8) h = (h ^ select_fold(nocase, (uint32_t)(v & 255u))) * 0x100000001b3ull;
    return h;
}
SXD uint64_t seen_merge_hash_end(uint64_t h, uint32_t len) { return distinct_mix(h ^ (uint64_t)len << 32); }
SXD uint64_t seen_merge_hash(const uint64_t* entry, uint32_t nocase) {
    const uint32_t len = (uint32_t)entry[0];
    uint64_t h = seen_merge_hash_begin();
    for (uint64_t j = 0, k = 1; j < len; j += 8, k++) h = seen_merge_hash_word(h, entry[k], len - j < 8u ? (uint32_t)(len - j) : 8u, nocase);
    return seen_merge_hash_end(h, len);
}

// Does the set hold `entry` (whose hash is `hash`)?  Word for word, the length first: a comparison ends at the first word that
// differs, so it never leaves the shorter entry.  *exhausted: every slot was looked at and none was empty; *slot_out: as seen_lookup_at's
SXD bool seen_merge_find_at(const SeenSet& S, const uint64_t* entry, uint64_t hash, bool* exhausted, uint64_t* slot_out) {
    const uint64_t words = 1u + ((entry[0] & 0xFFFFFFFFu) + 7u) / 8u;
    return seen_lookup_at(S, hash, [&](const uint8_t* at) {
        const uint64_t* have = (const uint64_t*)at;
        uint64_t j = 0;
        while (j < words && have[j] == entry[j]) j++;
        return j == words;
    }, exhausted, slot_out);
}
SXD bool seen_merge_find(const SeenSet& S, const uint64_t* entry, uint64_t hash, bool* exhausted) {
    uint64_t slot;
    return seen_merge_find_at(S, entry, hash, exhausted, &slot);
}

// mark, lane `lane` of wavefront `w`.  *occupied = its source word has an entry; *held = the destination holds it; *bytes = the entry
// a new one will take (0 unless occupied and not held); *lost = its probe walked every slot.  The wavefront writes the ballot over
// *held to P.held[w] and adds the ballots' popcounts and the sum of *bytes to P.totals.
SXD void seen_merge_mark_lane(const SeenMergeParams& P, uint64_t w, uint32_t lane, bool* occupied, bool* held, uint64_t* bytes, bool* lost) {
    *occupied = *held = *lost = false; *bytes = 0;
    const uint64_t* entry = seen_merge_entry(P, w * kSelectRecs + lane);
    if (!entry) return;
    *occupied = true;
    *held = seen_merge_find(P.set, entry, seen_merge_hash(entry, P.set.nocase), lost);
    if (!*held) *bytes = seen_entry_bytes((uint32_t)entry[0]);
}

// add, step 1, lane `lane` of wavefront `w`: the bytes of the entry it adds, 0 = it adds none (an entry has 8 bytes at least)
SXD uint64_t seen_merge_add_size_lane(const SeenMergeParams& P, uint64_t w, uint32_t lane) {
    const uint64_t* entry = seen_merge_entry(P, w * kSelectRecs + lane);
    if (!entry || ((P.held[w] >> lane) & 1u)) return 0;
    return seen_entry_bytes((uint32_t)entry[0]);
}

// add, step 2, a lane whose step 1 gave bytes: `at` = where its entry begins, as seen_add_lane's.  The entry is copied word for word
// and hashed on the way; then seen_claim.  false: it found no slot (the wavefront adds that to the error total)
SXD bool seen_merge_add_lane(const SeenMergeParams& P, uint64_t w, uint32_t lane, uint64_t at) {
    const SeenSet& S = P.set;
    const uint64_t* entry = seen_merge_entry(P, w * kSelectRecs + lane);
    const uint32_t len = (uint32_t)entry[0];
    uint64_t* to = (uint64_t*)(S.arena + at);
    to[0] = len;                                                 // [u32 len][u32 0]
    uint64_t h = seen_merge_hash_begin();
    for (uint64_t j = 0, k = 1; j < len; j += 8, k++) {
        const uint64_t v = entry[k];
        to[k] = v;
        h = seen_merge_hash_word(h, v, len - j < 8u ? (uint32_t)(len - j) : 8u, S.nocase);
    }
    return seen_claim(S, seen_merge_hash_end(h, len), at);
}

}  // namespace sx
