// Test-only harness: compiles the lane functions of a seen set that counts (sx_seen_count_core.hpp) as host code and drives them the
// way the entry points and sx_seen_count_dev.hip do: BEHIND a call that added — the result path's (sxs_seen_call of
// seen_core_host.cpp) or the merge path's (sxm_merge of seen_merge_host.cpp), both included as they are — one more pass, a grid of
// workgroups of 8 wavefronts that strides, every lane of a wavefront, the counted total and the error total added per wavefront; then
// the host's check of the counted total.  A refused call (1), a failed one and a lookup-only one run no count pass.  Also the lookup
// of the counts where the findings lie, and pass 1 of the selection by a field of a label word.
// The set is seen_set_host.hpp's, built with seven initialisers: its `counts` is NULL until sxc_counts_new gives it count words, which
// end where a page without access begins, as a list's count array does.
#include "seen_merge_host.cpp"

#include "../../stringsext_amd/csrc/sx_seen_count_core.hpp"

// The count words of a set: 2^table_log2 of them, zeroed; the set counts from here on
struct SxcCounts {
    SxsGuarded words;
    uint64_t n;
};
extern "C" SxcCounts* sxc_counts_new(SxsSeen* S) {
    if (S->dev.counts) return nullptr;      // (built without: seen_set_host.hpp's initialisers leave the last member 0)
    SxcCounts* K = new SxcCounts;
    K->n = (uint64_t)1 << S->dev.table_log2;
    if (!K->words.get(K->n * sizeof(uint64_t))) { delete K; return nullptr; }
    memset(K->words.at, 0, K->n * sizeof(uint64_t));
    S->dev.counts = (uint64_t*)K->words.at;
    return K;
}
extern "C" void sxc_counts_free(SxsSeen* S, SxcCounts* K) { S->dev.counts = nullptr; K->words.drop(); delete K; }
// (sx_seen_set_reset: the set's own reset, and the counts zeroed)
extern "C" void sxc_reset(SxsSeen* S, SxcCounts* K) { sxs_seen_reset(S); memset(K->words.at, 0, K->n * sizeof(uint64_t)); }
// the count words as they lie, a word per slot
extern "C" void sxc_counts_raw(const SxcCounts* K, uint64_t* out) { memcpy(out, K->words.at, K->n * sizeof(uint64_t)); }

extern "C" uint64_t sxc_sum(uint64_t a, uint64_t b) { return sx::seen_count_sum(a, b); }

// One pass of `lanes(w, lane, &counted, &lost)` over `waves` wavefronts as a grid of `groups` workgroups walks them; returns the
// error total, *counted_total = the counted total
template <class Lane>
static uint64_t sxc_pass(uint64_t waves, uint32_t groups, Lane lanes, uint64_t* totals) {
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t wv = 0; wv < kWaves; wv++) {
            uint64_t counted = 0, lost = 0;
            for (uint64_t w = (uint64_t)g * kWaves + wv; w < waves; w += (uint64_t)groups * kWaves)
                for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                    bool did = false, gone = false;
                    lanes(w, lane, &did, &gone);
                    counted += did; lost += gone;
                }
            if (counted) sx::seltally_add64(totals + sx::kSeenCounted, counted);
            if (lost) sx::seltally_add64(totals + sx::kSeenError, lost);
        }
    return totals[sx::kSeenError];
}

// sxs_seen_call, and behind it — if it added (0, not lookup-only) and the set counts — the count pass over every segment.  Returns what
// sxs_seen_call returns; -3 also: a first record whose string the set did not hold; -6 the counted total is not `distinct`; -4 also: a
// lane behind the last record counted
extern "C" int sxc_seen_call(SxsSeen* S, uint32_t n_segs, const void* const* recs, const uint8_t* const* arenas, const uint64_t* ns, const int32_t* packed,
                             int32_t distinct_log2, uint32_t groups, uint32_t lookup_only, uint64_t* const* labels, uint64_t* info) {
    const int rc = sxs_seen_call(S, n_segs, recs, arenas, ns, packed, distinct_log2, groups, lookup_only, labels, info);
    if (rc != 0 || lookup_only || !S->dev.counts) return rc;
    uint64_t totals[sx::kSeenTotals + 1] = { 0, 0, 0, 0, 0, 0 };
    int bad = 0;
    for (uint32_t s = 0; s < n_segs; s++) {
        sx::SeenParams P;
        memset(&P, 0, sizeof P);
        P.recs = recs[s]; P.arena = arenas[s]; P.n = ns[s]; P.packed = packed[s] ? 1u : 0u; P.labels = labels[s]; P.totals = totals; P.set = S->dev;
        sxc_pass((P.n + sx::kSelectRecs - 1) / sx::kSelectRecs, groups, [&](uint64_t w, uint32_t lane, bool* did, bool* gone) {
            sx::seen_count_lane(P, w, lane, did, gone);
            if ((*did || *gone) && w * sx::kSelectRecs + lane >= P.n) bad = 1;
        }, totals);
    }
    if (totals[sx::kSeenError]) return -3;
    if (bad) return -4;
    return totals[sx::kSeenCounted] == info[1] ? 0 : -6;
}

// sxm_merge, and behind it — if it added and the destination counts — the count pass over the source.  src_counts: a count word per
// source word, or NULL: (1, 1) each.  Returns what sxm_merge returns; -3, -4 as above; -6 the counted total is not the occupied words
static int sxc_merge(SxsSeen* D, const uint64_t* words, const uint8_t* src_arena, uint64_t n, const uint64_t* src_counts, uint32_t groups, uint32_t lookup_only,
                     uint64_t* held, uint64_t* info) {
    const int rc = sxm_merge(D, words, src_arena, n, groups, lookup_only, held, info);
    if (rc != 0 || lookup_only || !D->dev.counts) return rc;
    uint64_t totals[sx::kSeenTotals + 1] = { 0, 0, 0, 0, 0, 0 };
    sx::SeenMergeCountParams C;
    memset(&C, 0, sizeof C);
    C.m.words = words; C.m.src_arena = src_arena; C.m.n = n; C.m.held = held; C.m.totals = totals; C.m.set = D->dev;
    C.src_counts = src_counts;
    int bad = 0;
    sxc_pass((n + sx::kSelectRecs - 1) / sx::kSelectRecs, groups, [&](uint64_t w, uint32_t lane, bool* did, bool* gone) {
        sx::seen_merge_count_lane(C, w, lane, did, gone);
        const uint64_t i = w * sx::kSelectRecs + lane;
        if ((*did || *gone) && (i >= n || words[i] == sx::kSeenEmpty)) bad = 1;
    }, totals);
    if (totals[sx::kSeenError]) return -3;
    if (bad) return -4;
    return totals[sx::kSeenCounted] == info[0] ? 0 : -6;
}

// (counts: NULL, or L->n words, copied to where a page without access begins)
extern "C" int sxc_merge_list(SxsSeen* D, const SxmList* L, const uint64_t* counts, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
    SxsGuarded g;
    if (counts) {
        if (!g.get(L->n ? L->n * sizeof(uint64_t) : 8)) return -7;
        memcpy(g.at, counts, L->n * sizeof(uint64_t));
    }
    const int rc = sxc_merge(D, (const uint64_t*)L->words.at, (const uint8_t*)L->arena.at, L->n, counts ? (const uint64_t*)g.at : nullptr, groups, lookup_only, held, info);
    g.drop();
    return rc;
}
// (the source set's slot table, and its count table if it has one, as they lie)
extern "C" int sxc_merge_set(SxsSeen* D, const SxsSeen* S, uint32_t groups, uint32_t lookup_only, uint64_t* held, uint64_t* info) {
    return sxc_merge(D, S->dev.slots, S->dev.arena, (uint64_t)1 << S->dev.table_log2, S->dev.counts, groups, lookup_only, held, info);
}

// sx_result_seen_counts_device: every record's word = the count word of its string, 0 if the set does not hold it.  Returns 0; -3 a
// probe walked every slot
extern "C" int sxc_lookup(const SxsSeen* S, uint32_t n_segs, const void* const* recs, const uint8_t* const* arenas, const uint64_t* ns, const int32_t* packed,
                          uint32_t groups, uint64_t* const* labels) {
    uint64_t totals[sx::kSeenTotals + 1] = { 0, 0, 0, 0, 0, 0 };
    for (uint32_t s = 0; s < n_segs; s++) {
        sx::SeenParams P;
        memset(&P, 0, sizeof P);
        P.recs = recs[s]; P.arena = arenas[s]; P.n = ns[s]; P.packed = packed[s] ? 1u : 0u; P.labels = labels[s]; P.totals = totals; P.set = S->dev;
        sxc_pass((P.n + sx::kSelectRecs - 1) / sx::kSelectRecs, groups, [&](uint64_t w, uint32_t lane, bool* did, bool* gone) {
            *gone = sx::seen_counts_lookup_lane(P, w, lane);
        }, totals);
    }
    return totals[sx::kSeenError] ? -3 : 0;
}

// Pass 1 of the selection by range over n records, wavefronts [0, ceil(n / 64)] as the kernel walks them: sel[i] and len[i] per
// record.  The labels end where a page without access begins.  Returns 0; -4 a lane behind the last record was selected or had a length
extern "C" int sxc_range_pick(const void* recs, uint64_t n, int32_t packed, const uint64_t* labels, uint32_t shift, uint32_t bits, uint64_t lo, uint64_t hi,
                              uint8_t* sel, uint32_t* len) {
    SxsGuarded g;
    if (!g.get(n ? n * sizeof(uint64_t) : 8)) return -7;
    memcpy(g.at, labels, n * sizeof(uint64_t));
    sx::SelectParams S;
    memset(&S, 0, sizeof S);
    S.recs = recs; S.n = n; S.packed = packed ? 1u : 0u;
    const sx::LabelRange K{ (const uint64_t*)g.at, lo, hi, shift, bits };
    int bad = 0;
    for (uint64_t w = 0; w <= (n + sx::kSelectRecs - 1) / sx::kSelectRecs; w++)
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            uint32_t l = 0;
            const bool picked = sx::label_range_pick_lane(S, K, w, lane, &l);
            const uint64_t i = w * sx::kSelectRecs + lane;
            if (i >= n) { if (picked || l) bad = 1; continue; }
            sel[i] = picked ? 1 : 0; len[i] = l;
        }
    g.drop();
    return bad ? -4 : 0;
}
