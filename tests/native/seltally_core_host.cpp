// Test-only harness: compiles the tally set's builder (sx_seltally_build.cpp) and the tally core (sx_seltally_core.hpp) as host code
// and drives them the way sx_seltally_dev.hip does: the class map and the rows of the first lds_states states copied to a place of
// their own ("LDS" — the table the core takes for the other states has those rows overwritten, so a look-up on the wrong side
// shows), `groups` workgroups of 8 wavefronts that stride over the segment, each with counters of its own for the unique ids below
// lds_ids, wavefront after wavefront every lane in front of its string, rounds of one step per active lane until no lane is
// active, and the flush of the workgroup's counters at its end.
#include <stdint.h>
#include <string.h>
#include <vector>
#define SXD inline
#include "guarded_host.hpp"
#include "../../stringsext_amd/csrc/sx_seltally_build.cpp"
#include "../../stringsext_amd/csrc/sx_seltally_core.hpp"

struct HostTally {
    sx::SeltallyTable T;
    std::vector<uint8_t> lds, far;   // the first lds_states rows; the whole table with those rows spoilt
    std::vector<uint64_t> hits, first;
};

static void reset(HostTally* S) {
    S->hits.assign(S->T.unique, 0);
    S->first.assign(S->T.unique, UINT64_MAX);
}

// *rc: seltally_build's code; NULL unless SX_OK
extern "C" void* sxs_seltally_create(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, int* rc) {
    HostTally* S = new HostTally;
    std::string err;
    *rc = sx::seltally_build(patterns, n_patterns, flags, &S->T, &err);
    if (*rc != SX_OK) { delete S; return nullptr; }
    const size_t lds_bytes = (size_t)S->T.lds_states * S->T.classes * S->T.entry_bytes;
    S->lds.assign(S->T.next.begin(), S->T.next.begin() + (ptrdiff_t)lds_bytes);
    S->far = S->T.next;
    memset(S->far.data(), 0xEE, lds_bytes);
    reset(S);
    return S;
}
extern "C" void sxs_seltally_free(void* set) { delete (HostTally*)set; }
extern "C" void sxs_seltally_reset(void* set) { reset((HostTally*)set); }
// (table_bytes: what sx_tally_set_create puts into HBM apart from the counters)
extern "C" void sxs_seltally_info(const void* set, sx_tally_set_info* out) {
    const sx::SeltallyTable& T = ((const HostTally*)set)->T;
    *out = sx_tally_set_info{ T.n_patterns, T.unique, T.states, T.classes, T.nocase, T.entry_bytes,
                              (uint64_t)(sizeof T.map + T.next.size() + 2 * (size_t)T.states * 4 + (size_t)T.n_patterns * 4), T.lds_states, 0 };
}
// the builder's per-state and per-pattern tables, and the entries as the kernel reads them (widened to 32 bits: `wide` has states * classes words)
extern "C" void sxs_seltally_tables(const void* set, const uint32_t** own, const uint32_t** dict, const uint32_t** unique_of_pattern, uint32_t* wide) {
    const sx::SeltallyTable& T = ((const HostTally*)set)->T;
    *own = T.own.data(); *dict = T.dict.data(); *unique_of_pattern = T.unique_of_pattern.data();
    if (!wide) return;
    for (size_t i = 0; i < (size_t)T.states * T.classes; i++)
        wide[i] = T.entry_bytes == 2 ? ((const uint16_t*)T.next.data())[i] : ((const uint32_t*)T.next.data())[i];
}

template <class E>
static void tally_wave(const sx::SeltallyParams& P, const HostTally& S, uint64_t w, uint32_t* counts, uint64_t* far_steps) {
    sx::SeltallyLane L[sx::kSelectRecs];
    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) L[lane] = sx::seltally_begin_lane(P, w, lane);
    for (;;) {
        bool any = false;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            if (!L[lane].active) continue;
            any = true;
            if (L[lane].state >= P.set.lds_states) (*far_steps)++;
            sx::seltally_step_lane<E>(P, S.T.map, (const E*)S.lds.data(), counts, L[lane]);
        }
        if (!any) break;
    }
}

// recs: n records (sx_finding16 if packed), arena: their strings; ordinal: of record 0.  lds_ids: the kernel's number of LDS counters
// (the set's lds_ids is min(unique, that)); groups: workgroups.  *far_steps: the steps that read a row outside "LDS"; *lds_adds: the
// hits counted in a workgroup's counters.  Adds to the set's counters.
extern "C" int sxs_seltally_tally(void* set, const void* recs, uint64_t n, int packed, const uint8_t* arena, uint64_t ordinal,
                                  uint32_t lds_ids, uint32_t groups, uint64_t* far_steps, uint64_t* lds_adds) {
    HostTally& S = *(HostTally*)set;
    *far_steps = 0; *lds_adds = 0;
    if (n == 0 || groups == 0) return 0;   // (sx_result_tally_device refuses a segment without findings)
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    sx::SeltallyParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs; P.arena = arena; P.n = n; P.packed = packed ? 1u : 0u; P.ordinal = ordinal;
    P.set = sx::SeltallyDevice{ S.T.map, S.far.data(), S.T.own.data(), S.T.dict.data(), S.hits.data(), S.first.data(),
                                S.T.states, S.T.classes, S.T.lds_states, S.T.entry_bytes, S.T.unique, S.T.unique < lds_ids ? S.T.unique : lds_ids };
    for (uint32_t g = 0; g < groups; g++) {
        std::vector<uint32_t> counts(P.set.lds_ids ? P.set.lds_ids : 1, 0);
        for (uint32_t wv = 0; wv < 8; wv++)
            for (uint64_t w = (uint64_t)g * 8 + wv; w < waves; w += (uint64_t)groups * 8) {
                if (S.T.entry_bytes == 2) tally_wave<uint16_t>(P, S, w, counts.data(), far_steps);
                else tally_wave<uint32_t>(P, S, w, counts.data(), far_steps);
            }
        for (uint32_t c = 0; c < P.set.lds_ids; c++) { *lds_adds += counts[c]; sx::seltally_flush_lane(P, counts.data(), c); }
    }
    return 0;
}

// per input pattern, as sx_tally_set_read
extern "C" int sxs_seltally_read(const void* set, uint64_t* hits, uint64_t* first, uint32_t n_patterns) {
    const HostTally& S = *(const HostTally*)set;
    if (n_patterns != S.T.n_patterns) return SX_E_INVALID;
    for (uint32_t p = 0; p < n_patterns; p++) {
        if (hits) hits[p] = S.hits[S.T.unique_of_pattern[p]];
        if (first) first[p] = S.first[S.T.unique_of_pattern[p]];
    }
    return SX_OK;
}
