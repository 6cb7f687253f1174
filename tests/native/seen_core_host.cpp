// Test-only harness: compiles the lane functions of the seen set (sx_seen_core.hpp) as host code and drives them the way
// sx_result_seen_device and sx_seen_dev.hip do, over a SEQUENCE of results against one set that lives between the calls: the distinct
// pass under the set's fold (the driver of distinct_core_host.cpp, included as it is), then mark over every segment — a grid of
// workgroups of 8 wavefronts that strides over the segment, every lane of a wavefront, the totals added per wavefront —, then the
// host's look at the totals — what is new has to fit, else the call ends with 1 and the set is as it was —, then add over every
// segment: per wavefront the exclusive prefix of the lanes' entry sizes, one add to each cursor, and the lanes that add.
// The set is seen_set_host.hpp's, which distinct_core_host.cpp includes.
#include "distinct_core_host.cpp"

// the home slot and the tag of one string, for the tests that plant strings at the end of the table
extern "C" uint64_t sxs_seen_home(const uint8_t* s, uint32_t len, uint32_t nocase, uint32_t table_log2) {
    return sx::distinct_slot(sx::distinct_hash(s, len, nocase, sx::kSeenSeed), table_log2);
}
extern "C" uint64_t sxs_seen_tag(const uint8_t* s, uint32_t len, uint32_t nocase, uint32_t tag_bits) {
    sx::SeenSet T{};
    T.tag_bits = tag_bits;
    return sx::seen_tag(T, sx::distinct_hash(s, len, nocase, sx::kSeenSeed));
}

// One call.  The segments as sxs_distinct_host takes them; distinct_log2: its table; groups: the grid of every pass.  labels[s]: ns[s]
// words.  info: findings, distinct, repeated, seen_findings, seen_distinct, added_strings, added_bytes, rounds, table_log2 (the distinct
// pass's).  Returns 0; 1 what is new does not fit (nothing was added; info holds what the mark pass counted, added_* = what would have
// been); -1, -2 as sxs_distinct_host; -3 a probe walked every slot, or an adder found no slot; -4 a lane behind the last record was seen, first or adding.
extern "C" int sxs_seen_call(SxsSeen* S, uint32_t n_segs, const void* const* recs, const uint8_t* const* arenas, const uint64_t* ns, const int32_t* packed,
                             int32_t distinct_log2, uint32_t groups, uint32_t lookup_only, uint64_t* const* labels, uint64_t* info) {
    uint64_t dinfo[5], left[1];
    const int rc = sxs_distinct_host(n_segs, recs, arenas, ns, packed, S->dev.nocase, distinct_log2, groups, labels, dinfo, left, 0);
    if (rc != 0) return rc;
    uint64_t totals[sx::kSeenTotals] = { 0, 0, 0, 0, 0 };
    auto of = [&](uint32_t s) {
        sx::SeenParams p;
        memset(&p, 0, sizeof p);
        p.recs = recs[s]; p.arena = arenas[s]; p.n = ns[s]; p.packed = packed[s] ? 1u : 0u; p.labels = labels[s]; p.totals = totals; p.set = S->dev;
        return p;
    };
    int bad = 0;
    // (kernel: 0 mark, 1 add) over segment s as the grid walks it
    auto launch = [&](int kernel, const sx::SeenParams& P) {
        const uint64_t waves = (P.n + sx::kSelectRecs - 1) / sx::kSelectRecs;
        for (uint32_t g = 0; g < groups; g++)
            for (uint32_t wv = 0; wv < kWaves; wv++) {
                uint64_t findings = 0, classes = 0, fresh = 0, fresh_bytes = 0, lost = 0;
                for (uint64_t w = (uint64_t)g * kWaves + wv; w < waves; w += (uint64_t)groups * kWaves) {
                    if (kernel == 0) {
                        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                            bool seen, first;
                            uint64_t bytes;
                            sx::seen_mark_lane(P, w, lane, &seen, &first, &bytes);
                            if ((seen || first || bytes) && w * sx::kSelectRecs + lane >= P.n) bad = 1;
                            findings += seen; classes += seen && first; fresh += first && !seen; fresh_bytes += bytes;
                        }
                        continue;
                    }
                    uint64_t bytes[sx::kSelectRecs], all = 0, adders = 0;
                    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                        bytes[lane] = sx::seen_add_size_lane(P, w, lane);
                        if (bytes[lane] && w * sx::kSelectRecs + lane >= P.n) bad = 1;
                        all += bytes[lane]; adders += bytes[lane] != 0;
                    }
                    if (!adders) continue;
                    uint64_t at = sx::seen_fetch_add64(P.set.cursors + 1, all);      // (wave_reserve: lane 0's add; and its add to the string cursor)
                    sx::seltally_add64(P.set.cursors, adders);
                    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                        if (bytes[lane] && !sx::seen_add_lane(P, w, lane, at)) lost++;
                        at += bytes[lane];
                    }
                }
                if (findings) sx::seltally_add64(P.totals + sx::kSeenFindings, findings);
                if (classes) sx::seltally_add64(P.totals + sx::kSeenClasses, classes);
                if (fresh) sx::seltally_add64(P.totals + sx::kSeenNewClasses, fresh);
                if (fresh_bytes) sx::seltally_add64(P.totals + sx::kSeenNewBytes, fresh_bytes);
                if (lost) sx::seltally_add64(P.totals + sx::kSeenError, lost);
            }
    };
    for (uint32_t s = 0; s < n_segs; s++) launch(0, of(s));
    info[0] = dinfo[0]; info[1] = dinfo[1]; info[2] = dinfo[2];
    info[3] = totals[sx::kSeenFindings]; info[4] = totals[sx::kSeenClasses];
    info[5] = lookup_only ? 0 : totals[sx::kSeenNewClasses]; info[6] = lookup_only ? 0 : totals[sx::kSeenNewBytes];
    info[7] = dinfo[3]; info[8] = dinfo[4];
    if (totals[sx::kSeenError]) return -3;
    if (bad) return -4;
    if (lookup_only) return 0;
    if (S->cursors[0] + totals[sx::kSeenNewClasses] > S->capacity_strings || S->cursors[1] + totals[sx::kSeenNewBytes] > S->capacity_bytes) return 1;
    if (totals[sx::kSeenNewClasses])
        for (uint32_t s = 0; s < n_segs; s++) launch(1, of(s));
    if (totals[sx::kSeenError]) return -3;
    return bad ? -4 : 0;
}
