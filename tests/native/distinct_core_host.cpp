// Test-only harness: compiles the lane functions of the duplicate strings (sx_distinct_core.hpp) as host code and drives them the way
// sx_result_distinct_device and sx_distinct_dev.hip do: per round the table emptied and the counter zeroed, claim over every segment —
// a grid of workgroups of 8 wavefronts that strides over the segment, every lane of a wavefront —, then resolve over every segment with
// the ballot's popcount added per wavefront and one add to a winner's count per run of neighbouring lanes that found it, until the
// counter is 0 (a round that does not lower it ends the call with -1), then finalize over every segment with the two totals summed per
// wavefront.
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_distinct_core.hpp"
#include "seen_set_host.hpp"      // (sxs_guarded, sxs_unmap: the arenas end where a page without access begins)

constexpr uint32_t kWaves = 8;      // wavefronts per workgroup, as kRowsWaves

// n_segs segments: recs[s] = ns[s] records (sx_finding16 if packed[s]), arenas[s] = their strings.  table_log2 < 0: the power of two
// >= 2 x findings.  groups: the grid.  labels[s]: ns[s] words.  info: findings, distinct, repeated, rounds, table_log2.
// left: the counter after each round (left_cap entries at most are written).  Returns 0; -1 a round without progress; -2 a lane
// behind the last record claimed to be first or unresolved.
extern "C" int sxs_distinct_host(uint32_t n_segs, const void* const* recs, const uint8_t* const* arenas, const uint64_t* ns, const int32_t* packed,
                                 uint32_t nocase, int32_t table_log2, uint32_t groups, uint64_t* const* labels, uint64_t* info, uint64_t* left,
                                 uint32_t left_cap) {
    std::vector<sx::DistinctSeg> segs;
    uint64_t findings = 0;
    for (uint32_t s = 0; s < n_segs; s++) {
        segs.push_back(sx::DistinctSeg{ recs[s], arenas[s], ns[s], packed[s] ? 1u : 0u, 0u, findings });
        findings += ns[s];
    }
    uint32_t log2 = 1;
    if (table_log2 >= 0) log2 = (uint32_t)table_log2;
    else while (((uint64_t)1 << log2) < 2 * findings) log2++;
    std::vector<uint64_t> table((size_t)1 << log2), rep(findings ? findings : 1, ~(uint64_t)0), count(findings ? findings : 1, 0);
    uint64_t words[3] = { 0, 0, 0 };      // the counter, distinct, repeated
    sx::DistinctParams base;
    memset(&base, 0, sizeof base);
    base.segs = segs.data(); base.n_segs = n_segs; base.nocase = nocase; base.table_log2 = log2;
    base.table = table.data(); base.rep = rep.data(); base.count = count.data(); base.unresolved = words; base.totals = words + 1;
    auto of = [&](uint32_t s, uint32_t round) {
        sx::DistinctParams p = base;
        p.recs = segs[s].recs; p.arena = segs[s].arena; p.n = segs[s].n; p.packed = segs[s].packed; p.seg = s; p.base = segs[s].base;
        p.round = round; p.labels = labels[s];
        return p;
    };
    // (kernel: 0 claim, 1 resolve, 2 finalize) over segment s as the grid walks it
    auto launch = [&](int kernel, const sx::DistinctParams& P) {
        const uint64_t waves = (P.n + sx::kSelectRecs - 1) / sx::kSelectRecs;
        int bad = 0;
        for (uint32_t g = 0; g < groups; g++)
            for (uint32_t wv = 0; wv < kWaves; wv++) {
                uint64_t left_here = 0, distinct = 0, repeated = 0;
                for (uint64_t w = (uint64_t)g * kWaves + wv; w < waves; w += (uint64_t)groups * kWaves) {
                    uint64_t widx[sx::kSelectRecs], found = 0, heads = 0;
                    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                        const bool behind = w * sx::kSelectRecs + lane >= P.n;
                        if (kernel == 0) sx::distinct_claim_lane(P, w, lane);
                        else if (kernel == 1) {
                            const uint32_t made = sx::distinct_resolve_lane(P, w, lane, &widx[lane]);
                            if (made != sx::kDistinctNothing && behind) bad = 1;
                            left_here += made == sx::kDistinctStays;
                            if (made != sx::kDistinctFound) continue;
                            // (the kernel: the ballots over "found" and over "found, and the lane to the left did not find the same winner")
                            if (lane == 0 || !((found >> (lane - 1)) & 1u) || widx[lane - 1] != widx[lane]) heads |= (uint64_t)1 << lane;
                            found |= (uint64_t)1 << lane;
                        } else {
                            bool first, again;
                            sx::distinct_finalize_lane(P, w, lane, &first, &again);
                            if ((first || again) && behind) bad = 1;
                            distinct += first; repeated += again;
                        }
                    }
                    if (kernel == 1)
                        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) sx::distinct_count_run(P, lane, found, heads, widx[lane]);
                }
                if (left_here) sx::seltally_add64(P.unresolved, left_here);
                if (distinct) sx::seltally_add64(P.totals, distinct);
                if (repeated) sx::seltally_add64(P.totals + 1, repeated);
            }
        return bad;
    };
    uint64_t before = findings;
    uint32_t rounds = 0;
    int bad = 0;
    while (before != 0) {
        for (uint64_t& slot : table) slot = sx::kDistinctEmptySlot;
        words[0] = 0;
        for (uint32_t s = 0; s < n_segs; s++) bad |= launch(0, of(s, rounds));
        for (uint32_t s = 0; s < n_segs; s++) bad |= launch(1, of(s, rounds));
        if (rounds < left_cap) left[rounds] = words[0];
        rounds++;
        if (words[0] >= before) return -1;
        before = words[0];
    }
    for (uint32_t s = 0; s < n_segs; s++) bad |= launch(2, of(s, rounds));
    info[0] = findings; info[1] = words[1]; info[2] = words[2]; info[3] = rounds; info[4] = log2;
    return bad ? -2 : 0;
}

// the hash and the slot of one string, for the test that every seed spreads the strings anew
extern "C" uint64_t sxs_distinct_slot(const uint8_t* s, uint32_t len, uint32_t nocase, uint32_t round, uint32_t table_log2) {
    return sx::distinct_slot(sx::distinct_hash(s, len, nocase, round), table_log2);
}
