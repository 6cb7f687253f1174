// Test-only harness: compiles the lane functions of a seen set's merge (sx_seen_merge_core.hpp) as host code and drives them the way
// the entry points and sx_seen_merge_dev.hip do: mark over the source — a grid of workgroups of 8 wavefronts that strides over the
// source's words, every lane of a wavefront, the ballot "held" written per wavefront and the five totals added per wavefront —, then
// the host's look at the cursors and the totals — what is new has to fit, else the call ends with 1 and the destination is as it was
// —, then add: per wavefront and batch of kSeenMergeAddChunks chunks the exclusive prefix of the lanes' entry sizes, one add to the
// byte cursor, and the lanes that add; per wavefront one add to the string cursor.
// The set is seen_set_host.hpp's, and the result path's calls (seen_core_host.cpp, included as it is) are in this library too: the two
// paths work on ONE set.  Every slot table, every word list and every arena ends where a page without access begins: a word or a
// byte read behind one is a fault.
#include "seen_core_host.cpp"

#include "../../stringsext_amd/csrc/sx_seen_merge_core.hpp"

// A source the test built: n words and arena_bytes of entries, each copied to where a page without access begins behind it
struct SxmList {
    SxsGuarded words, arena;
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
    SxsGuarded g;
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
static int sxm_merge(SxsSeen* D, const uint64_t* words, const uint8_t* src_arena, uint64_t n, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
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
                uint64_t at = sx::seen_fetch_add64(P.set.cursors + 1, all);      // (wave_reserve: lane 0's add)
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

extern "C" int sxm_merge_list(SxsSeen* D, const SxmList* L, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
    return sxm_merge(D, (const uint64_t*)L->words.at, (const uint8_t*)L->arena.at, L->n, groups, lookup_only, held, info);
}
// (the source set's slot table as it lies)
extern "C" int sxm_merge_set(SxsSeen* D, const SxsSeen* S, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
    return sxm_merge(D, S->dev.slots, S->dev.arena, (uint64_t)1 << S->dev.table_log2, groups, lookup_only, held, info);
}
