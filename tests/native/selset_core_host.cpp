// Test-only harness: compiles the keyword-set builder (sx_selset_build.cpp) and the set's match core (sx_selset_core.hpp) as host
// code and drives them the way sx_selset_dev.hip does: the class map and the rows of the first lds_states states copied to a
// place of their own ("LDS" — the table the core takes for the other states has those rows overwritten, so a look-up on the
// wrong side shows), wavefront after wavefront every lane in front of its string, rounds of one step per active lane until no
// lane is active, the ballot, the count and the string bytes; then, as select_core_host.cpp, the exclusive scan over the
// wavefronts' counts, select_place_lane and the ordered string gather of sx_result_core.hpp (select_pass2_host.hpp).
#include <stdint.h>
#include <string.h>
#include <vector>
#define SXD inline
#include "guarded_host.hpp"
#include "select_pass2_host.hpp"
#include "../../stringsext_amd/csrc/sx_selset_build.cpp"
#include "../../stringsext_amd/csrc/sx_selset_core.hpp"

struct HostSet {
    sx::SelsetTable T;
    std::vector<uint8_t> lds, far;   // the first lds_states rows; the whole table with those rows spoilt
};

// *rc: selset_build's code; NULL unless SX_OK
extern "C" void* sxs_selset_create(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, int* rc) {
    HostSet* S = new HostSet;
    std::string err;
    *rc = sx::selset_build(patterns, n_patterns, flags, &S->T, &err);
    if (*rc != SX_OK) { delete S; return nullptr; }
    const size_t lds_bytes = (size_t)S->T.lds_states * S->T.classes * S->T.entry_bytes;
    S->lds.assign(S->T.next.begin(), S->T.next.begin() + (ptrdiff_t)lds_bytes);
    S->far = S->T.next;
    memset(S->far.data(), 0xEE, lds_bytes);
    return S;
}
extern "C" void sxs_selset_free(void* set) { delete (HostSet*)set; }
extern "C" void sxs_selset_info(const void* set, sx_select_set_info* out, uint32_t* entry_bytes, uint32_t* matched) {
    const sx::SelsetTable& T = ((const HostSet*)set)->T;
    *out = sx_select_set_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)T.next.size(), T.lds_states, 0 };
    *entry_bytes = T.entry_bytes; *matched = T.matched;
}

template <class E>
static void match_wave(const sx::SelsetParams& P, const HostSet& S, uint64_t w, uint64_t* mask, uint64_t* bytes, uint64_t* far_steps) {
    sx::SelsetLane L[sx::kSelectRecs];
    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) L[lane] = sx::selset_begin_lane(P, w, lane);
    for (;;) {
        bool any = false;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            if (!L[lane].active) continue;
            any = true;
            if (L[lane].state >= P.set.lds_states) (*far_steps)++;
            sx::selset_step_lane<E>(P, S.T.map, (const E*)S.lds.data(), L[lane]);
        }
        if (!any) break;
    }
    *mask = 0; *bytes = 0;
    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++)
        if (sx::selset_lane_selected(P, w, lane, L[lane])) { *mask |= (uint64_t)1 << lane; *bytes += L[lane].len; }
}

// recs: n records (sx_finding16 if packed), arena: their strings.  out_recs: room for n records, out_arena: arena_cap bytes.
// masks (may be NULL): waves + 1 words.  *n_sel, *sel_bytes: the totals as the scans give them; *far_steps: the steps that
// read a row outside "LDS".
extern "C" int sxs_selset_select_host(const void* set, const void* recs, uint64_t n, int packed, const uint8_t* arena, uint32_t invert,
                                      void* out_recs, uint8_t* out_arena, uint64_t arena_cap, uint64_t* masks, uint64_t* n_sel,
                                      uint64_t* sel_bytes, uint64_t* far_steps) {
    const HostSet& S = *(const HostSet*)set;
    *n_sel = 0; *sel_bytes = 0; *far_steps = 0;
    if (n == 0) return 0;   // (sx_result_select_set_device refuses a segment without findings)
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    std::vector<uint64_t> wmask(waves + 1), wbytes(waves + 1);
    std::vector<uint32_t> wcount(waves + 1);
    sx::SelsetParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs; P.arena = arena; P.n = n; P.packed = packed ? 1u : 0u; P.invert = invert ? 1u : 0u;
    P.wmask = wmask.data(); P.wcount = wcount.data(); P.wbytes = wbytes.data();
    P.set = sx::SelsetDevice{ S.T.map, S.far.data(), S.T.states, S.T.classes, S.T.lds_states, S.T.matched, S.T.entry_bytes, 0 };
    for (uint64_t w = 0; w <= waves; w++) {
        if (S.T.entry_bytes == 2) match_wave<uint16_t>(P, S, w, &wmask[w], &wbytes[w], far_steps);
        else match_wave<uint32_t>(P, S, w, &wmask[w], &wbytes[w], far_steps);
        wcount[w] = (uint32_t)__builtin_popcountll(wmask[w]);
    }
    // pass 2 is the list selection's (the set's kernel has filled the same per-wavefront words)
    return sxs_select_pass2(recs, n, packed, arena, wmask, wcount, wbytes, out_recs, out_arena, arena_cap, masks, n_sel, sel_bytes);
}
