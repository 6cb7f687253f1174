// Test-only: what the harnesses of the seen set share (distinct_core_host.cpp for the memory, seen_core_host.cpp, seen_merge_host.cpp):
// memory that ends where a page without access begins (guarded_host.hpp), and ONE set in such memory, which both the result path's
// and the merge path's lane functions work on.  The exported names are what tests/test_seen_core.py and tests/test_seen_merge_core.py bind.
#pragma once
#include <stdint.h>
#include <string.h>
#ifndef SXD
#define SXD inline
#endif
#include "../../stringsext_amd/csrc/sx_seen_core.hpp"
#include "guarded_host.hpp"

struct SxsGuarded {
    void* at = nullptr;
    void* region = nullptr;
    uint64_t region_bytes = 0;
    bool get(uint64_t bytes) { at = sxs_guarded(bytes, &region, &region_bytes); return at != nullptr; }
    void drop() { if (region) sxs_unmap(region, region_bytes); region = nullptr; }
};

// The set.  It takes table_log2 and tag_bits directly: tiny tables make long probe chains, few tag bits make the tags collide.  Its
// slot table and its arena each end where a page without access begins.
struct SxsSeen {
    sx::SeenSet dev;
    SxsGuarded slots, arena;
    uint64_t cursors[2];
    uint64_t capacity_strings, capacity_bytes;
};

extern "C" void sxs_seen_reset(SxsSeen* S) {
    for (uint64_t s = 0; s < (uint64_t)1 << S->dev.table_log2; s++) S->dev.slots[s] = sx::kSeenEmpty;
    memset(S->dev.arena, 0xA5, S->capacity_bytes);
    S->cursors[0] = S->cursors[1] = 0;
}

// table_log2 < 0: the power of two >= 2 x capacity_strings, at least 2 slots
extern "C" SxsSeen* sxs_seen_new(int32_t table_log2, uint32_t tag_bits, uint32_t nocase, uint64_t capacity_strings, uint64_t capacity_bytes) {
    SxsSeen* S = new SxsSeen;
    uint32_t log2 = 1;
    if (table_log2 >= 0) log2 = (uint32_t)table_log2;
    else while (((uint64_t)1 << log2) < 2 * capacity_strings) log2++;
    S->capacity_strings = capacity_strings; S->capacity_bytes = capacity_bytes;
    // (the arena's room rounded up to 8: entries are 8-byte aligned, and so is the page it ends at)
    if (!S->slots.get(sizeof(uint64_t) << log2) || !S->arena.get(capacity_bytes ? (capacity_bytes + 7u) & ~(uint64_t)7u : 8)) { S->slots.drop(); delete S; return nullptr; }
    S->dev = sx::SeenSet{ (uint64_t*)S->slots.at, (uint8_t*)S->arena.at, S->cursors, log2, tag_bits, nocase, 0u };
    sxs_seen_reset(S);
    return S;
}
extern "C" void sxs_seen_free(SxsSeen* S) { S->slots.drop(); S->arena.drop(); delete S; }

// out: strings, bytes, capacity_strings, capacity_bytes, table_log2, tag_bits
extern "C" void sxs_seen_state(const SxsSeen* S, uint64_t* out) {
    out[0] = S->cursors[0]; out[1] = S->cursors[1]; out[2] = S->capacity_strings; out[3] = S->capacity_bytes; out[4] = S->dev.table_log2; out[5] = S->dev.tag_bits;
}

// The set's memory as it lies: the 2^table_log2 slots and the capacity_bytes of the arena
extern "C" void sxs_seen_raw(const SxsSeen* S, uint64_t* slots, uint8_t* arena) {
    memcpy(slots, S->dev.slots, sizeof(uint64_t) << S->dev.table_log2);
    memcpy(arena, S->dev.arena, S->capacity_bytes);
}

// The stored strings, by a walk over the table: per occupied slot its index, its word, its entry's length, and the entry's bytes (all
// of them, the padding too) appended to `bytes`.  Returns the number of occupied slots, or ~0 if something does not fit — the room
// given, or an entry the byte cursor.
extern "C" uint64_t sxs_seen_dump(const SxsSeen* S, uint64_t* slot_of, uint64_t* word_of, uint64_t* len_of, uint64_t cap, uint8_t* bytes, uint64_t bytes_cap) {
    uint64_t k = 0, at = 0;
    for (uint64_t s = 0; s < (uint64_t)1 << S->dev.table_log2; s++) {
        const uint64_t word = S->dev.slots[s];
        if (word == sx::kSeenEmpty) continue;
        const uint8_t* entry = sx::seen_entry_at(S->dev.arena, word);
        const uint64_t off = (uint64_t)(entry - S->dev.arena);
        if (off + 8 > S->cursors[1]) return ~(uint64_t)0;
        const uint64_t len = *(const uint32_t*)entry, padded = (len + 7u) & ~(uint64_t)7u;
        if (k >= cap || at + padded > bytes_cap || off + 8 + padded > S->cursors[1] || ((const uint32_t*)entry)[1] != 0) return ~(uint64_t)0;
        slot_of[k] = s; word_of[k] = word; len_of[k] = len;
        memcpy(bytes + at, entry + 8, padded);
        at += padded; k++;
    }
    return k;
}
