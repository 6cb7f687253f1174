// Test-only harness: compiles the lane functions of a seen set's merge (sx_seen_merge_core.hpp) as host code and drives them the way
// the entry points and sx_seen_merge_dev.hip do: mark over the source — a grid of workgroups of 8 wavefronts that strides over the
// source's words, every lane of a wavefront, the ballot "held" written per wavefront and the five totals added per wavefront —, then
// the host's look at the cursors and the totals — what is new has to fit, else the call ends with 1 and the destination is as it was
// —, then add: per wavefront and batch of kSeenMergeAddChunks chunks the exclusive prefix of the lanes' entry sizes, one add to the
// byte cursor, and the lanes that add; per wavefront one add to the string cursor.
// A set takes table_log2 and tag_bits directly: tiny tables make long probe chains, few tag bits make the tags collide.  Every slot
// table, every word list and every arena ends where a page without access begins: a word or a byte read behind one is a fault.
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_seen_merge_core.hpp"

constexpr uint32_t kWaves = 8;      // wavefronts per workgroup, as kRowsWaves

// `bytes` of memory that end at a page without access; *region, *region_bytes: what sxm_unmap takes
extern "C" void* sxm_guarded(uint64_t bytes, void** region, uint64_t* region_bytes) {
    const uint64_t page = (uint64_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
    uint8_t* p = (uint8_t*)mmap(nullptr, body + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) return nullptr;
    if (mprotect(p + body, page, PROT_NONE) != 0) { munmap(p, body + page); return nullptr; }
    *region = p; *region_bytes = body + page;
    return p + body - bytes;
}
extern "C" void sxm_unmap(void* region, uint64_t region_bytes) { munmap(region, region_bytes); }

struct SxmGuarded {
    void* at = nullptr;
    void* region = nullptr;
    uint64_t region_bytes = 0;
    bool get(uint64_t bytes) { at = sxm_guarded(bytes, &region, &region_bytes); return at != nullptr; }
    void drop() { if (region) sxm_unmap(region, region_bytes); region = nullptr; }
};

struct SxmSet {
    sx::SeenSet dev;
    SxmGuarded slots, arena;
    uint64_t cursors[2];
    uint64_t capacity_strings, capacity_bytes;
};

// table_log2 < 0: the power of two >= 2 x capacity_strings, at least 2 slots
extern "C" SxmSet* sxm_set_new(int32_t table_log2, uint32_t tag_bits, uint32_t nocase, uint64_t capacity_strings, uint64_t capacity_bytes) {
    SxmSet* S = new SxmSet;
    uint32_t log2 = 1;
    if (table_log2 >= 0) log2 = (uint32_t)table_log2;
    else while (((uint64_t)1 << log2) < 2 * capacity_strings) log2++;
    S->capacity_strings = capacity_strings; S->capacity_bytes = capacity_bytes;
    // (the arena's room rounded up to 8: entries are 8-byte aligned, and so is the page it ends at)
    if (!S->slots.get(sizeof(uint64_t) << log2) || !S->arena.get(capacity_bytes ? (capacity_bytes + 7u) & ~(uint64_t)7u : 8)) { S->slots.drop(); delete S; return nullptr; }
    S->dev = sx::SeenSet{ (uint64_t*)S->slots.at, (uint8_t*)S->arena.at, S->cursors, log2, tag_bits, nocase, 0u };
    for (uint64_t s = 0; s < (uint64_t)1 << log2; s++) S->dev.slots[s] = sx::kSeenEmpty;
    memset(S->dev.arena, 0xA5, capacity_bytes);
    S->cursors[0] = S->cursors[1] = 0;
    return S;
}
extern "C" void sxm_set_free(SxmSet* S) { S->slots.drop(); S->arena.drop(); delete S; }

// out: strings, bytes, capacity_strings, capacity_bytes, table_log2, tag_bits
extern "C" void sxm_set_state(const SxmSet* S, uint64_t* out) {
    out[0] = S->cursors[0]; out[1] = S->cursors[1]; out[2] = S->capacity_strings; out[3] = S->capacity_bytes; out[4] = S->dev.table_log2; out[5] = S->dev.tag_bits;
}

// The set's memory as it lies: the 2^table_log2 slots and the capacity_bytes of the arena
extern "C" void sxm_set_raw(const SxmSet* S, uint64_t* slots, uint8_t* arena) {
    memcpy(slots, S->dev.slots, sizeof(uint64_t) << S->dev.table_log2);
    memcpy(arena, S->dev.arena, S->capacity_bytes);
}

// The stored strings, by a walk over the table: per occupied slot its index, its word, its entry's length, and the entry's bytes (all
// of them, the padding too) appended to `bytes`.  Returns the number of occupied slots, or ~0 if something does not fit.
extern "C" uint64_t sxm_set_dump(const SxmSet* S, uint64_t* slot_of, uint64_t* word_of, uint64_t* len_of, uint64_t cap, uint8_t* bytes, uint64_t bytes_cap) {
    uint64_t k = 0, at = 0;
    for (uint64_t s = 0; s < (uint64_t)1 << S->dev.table_log2; s++) {
        const uint64_t word = S->dev.slots[s];
        if (word == sx::kSeenEmpty) continue;
        const uint64_t off = (word & (((uint64_t)1 << sx::kSeenOffsetBits) - 1u)) * 8u;
        if (off + 8 > S->cursors[1]) return ~(uint64_t)0;
        const uint8_t* entry = S->dev.arena + off;
        const uint64_t len = *(const uint32_t*)entry, padded = (len + 7u) & ~(uint64_t)7u;
        if (k >= cap || at + padded > bytes_cap || off + 8 + padded > S->cursors[1] || ((const uint32_t*)entry)[1] != 0) return ~(uint64_t)0;
        slot_of[k] = s; word_of[k] = word; len_of[k] = len;
        memcpy(bytes + at, entry + 8, padded);
        at += padded; k++;
    }
    return k;
}

// A source the test built: n words and arena_bytes of entries, each copied to where a page without access begins behind it
struct SxmList {
    SxmGuarded words, arena;
    uint64_t n;
};
extern "C" SxmList* sxm_list_new(const uint64_t* words, uint64_t n, const uint8_t* arena, uint64_t arena_bytes) {
    SxmList* L = new SxmList;
    L->n = n;
    if (!L->words.get(n ? n * sizeof(uint64_t) : 8) || !L->arena.get(arena_bytes ? arena_bytes : 8)) { L->words.drop(); delete L; return nullptr; }
    if (((uintptr_t)L->arena.at & 7u) != 0) { L->words.drop(); L->arena.drop(); delete L; return nullptr; }      // (arena_bytes is a multiple of 8)
    memcpy(L->words.at, words, n * sizeof(uint64_t));
    memcpy(L->arena.at, arena, arena_bytes);
    return L;
}
extern "C" void sxm_list_free(SxmList* L) { L->words.drop(); L->arena.drop(); delete L; }

// the two hashes of one string: distinct_hash over its bytes, and seen_merge_hash over its entry (built here, at the end of a guarded region)
extern "C" uint64_t sxm_hash_bytes(const uint8_t* s, uint32_t len, uint32_t nocase) { return sx::distinct_hash(s, len, nocase, sx::kSeenSeed); }
extern "C" uint64_t sxm_hash_entry(const uint8_t* s, uint32_t len, uint32_t nocase) {
    SxmGuarded g;
    const uint64_t size = sx::seen_entry_bytes(len);
    if (!g.get(size)) return 0;
    memset(g.at, 0, size);
    *(uint32_t*)g.at = len;
    memcpy((uint8_t*)g.at + 8, s, len);
    const uint64_t h = sx::seen_merge_hash((const uint64_t*)g.at, nocase);
    g.drop();
    return h;
}

// One call: the source (words, src_arena, n) into dst.  groups: the grid of either pass.  held: ceil(n / 64) words, as mark leaves
// them.  info: source_strings, already_held, added_strings, added_bytes (for a refused call: what would have been added).  Returns 0;
// 1 what is new does not fit (nothing was added); -3 a probe walked every slot, or an adder found no slot; -4 a lane without an entry
// was occupied, held or adding; -5 the cursors after the add are not the sums.
static int sxm_merge(SxmSet* D, const uint64_t* words, const uint8_t* src_arena, uint64_t n, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
    uint64_t totals[sx::kSeenMergeTotals] = { 0, 0, 0, 0, 0 };
    sx::SeenMergeParams P;
    memset(&P, 0, sizeof P);
    P.words = words; P.src_arena = src_arena; P.n = n; P.held = held; P.totals = totals; P.set = D->dev;
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    int bad = 0;
    auto no_entry = [&](uint64_t i) { return i >= n || words[i] == sx::kSeenEmpty; };
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t wv = 0; wv < kWaves; wv++) {
            uint64_t occupied = 0, had = 0, lost = 0, fresh_bytes = 0;
            for (uint64_t w = (uint64_t)g * kWaves + wv; w < waves; w += (uint64_t)groups * kWaves) {
                uint64_t mask = 0;
                for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                    bool occ, was, gone;
                    uint64_t bytes;
                    sx::seen_merge_mark_lane(P, w, lane, &occ, &was, &bytes, &gone);
                    if ((occ || was || bytes || gone) && no_entry(w * sx::kSelectRecs + lane)) bad = 1;
                    occupied += occ; had += was; lost += gone; fresh_bytes += bytes;
                    mask |= (uint64_t)was << lane;
                }
                P.held[w] = mask;                                                    // (lane 0's store)
            }
            if (occupied) sx::seltally_add64(P.totals + sx::kSeenMergeOccupied, occupied);
            if (had) sx::seltally_add64(P.totals + sx::kSeenMergeHeld, had);
            if (occupied - had) sx::seltally_add64(P.totals + sx::kSeenMergeNew, occupied - had);
            if (fresh_bytes) sx::seltally_add64(P.totals + sx::kSeenMergeNewBytes, fresh_bytes);
            if (lost) sx::seltally_add64(P.totals + sx::kSeenMergeError, lost);
        }
    const uint64_t had[2] = { D->cursors[0], D->cursors[1] }, fresh = totals[sx::kSeenMergeNew], fresh_bytes = totals[sx::kSeenMergeNewBytes];
    info[0] = totals[sx::kSeenMergeOccupied]; info[1] = totals[sx::kSeenMergeHeld]; info[2] = lookup_only ? 0 : fresh; info[3] = lookup_only ? 0 : fresh_bytes;
    if (totals[sx::kSeenMergeError]) return -3;
    if (bad) return -4;
    if (lookup_only) return 0;
    if (had[0] + fresh > D->capacity_strings || had[1] + fresh_bytes > D->capacity_bytes) return 1;
    if (!fresh) return 0;
    const uint64_t batches = (waves + sx::kSeenMergeAddChunks - 1) / sx::kSeenMergeAddChunks;
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t wv = 0; wv < kWaves; wv++) {
            uint64_t lost = 0, added = 0;
            for (uint64_t b = (uint64_t)g * kWaves + wv; b < batches; b += (uint64_t)groups * kWaves) {
                uint64_t bytes[sx::kSelectRecs], all = 0;      // per lane: its entries of the batch's chunks
                for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                    bytes[lane] = 0;
                    for (uint32_t k = 0; k < sx::kSeenMergeAddChunks; k++) {
                        const uint64_t w = b * sx::kSeenMergeAddChunks + k, size = sx::seen_merge_add_size_lane(P, w, lane);
                        if (size && no_entry(w * sx::kSelectRecs + lane)) bad = 1;
                        bytes[lane] += size;
                    }
                    all += bytes[lane];
                }
                if (!all) continue;
                uint64_t at = sx::seen_fetch_add64(P.set.cursors + 1, all);      // (lane 0's add)
                for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++)
                    for (uint32_t k = 0; k < sx::kSeenMergeAddChunks; k++) {
                        const uint64_t w = b * sx::kSeenMergeAddChunks + k, size = sx::seen_merge_add_size_lane(P, w, lane);
                        if (!size) continue;
                        if (!sx::seen_merge_add_lane(P, w, lane, at)) lost++;
                        at += size; added++;
                    }
            }
            if (added) sx::seltally_add64(P.set.cursors, added);
            if (lost) sx::seltally_add64(P.totals + sx::kSeenMergeError, lost);
        }
    if (totals[sx::kSeenMergeError]) return -3;
    if (bad) return -4;
    return D->cursors[0] == had[0] + fresh && D->cursors[1] == had[1] + fresh_bytes ? 0 : -5;
}

extern "C" int sxm_merge_list(SxmSet* D, const SxmList* L, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
    return sxm_merge(D, (const uint64_t*)L->words.at, (const uint8_t*)L->arena.at, L->n, groups, lookup_only, held, info);
}
// (the source set's slot table as it lies)
extern "C" int sxm_merge_set(SxmSet* D, const SxmSet* S, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
    return sxm_merge(D, S->dev.slots, S->dev.arena, (uint64_t)1 << S->dev.table_log2, groups, lookup_only, held, info);
}
