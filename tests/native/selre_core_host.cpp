// Test-only harness: compiles the regex builder (sx_selre_build.cpp) and the regex match core (sx_selre_core.hpp) as host code and
// drives them the way sx_selre_dev.hip does: the class map and the rows of the first lds_states states copied to a place of their
// own ("LDS" — the table the core takes for the other states has those rows overwritten, so a look-up on the wrong side shows),
// wavefront after wavefront every lane in front of its string, rounds of one step per active lane until no lane is active, the
// ballot, the count and the string bytes; then, as selset_core_host.cpp, the exclusive scan over the wavefronts' counts,
// select_place_lane and the ordered string gather of sx_result_core.hpp (select_pass2_host.hpp).  It also hands out the table as bytes.
#include <stdint.h>
#include <string.h>
#include <vector>
#define SXD inline
#include "guarded_host.hpp"
#include "select_pass2_host.hpp"
#include "../../stringsext_amd/csrc/sx_selre_build.cpp"
#include "../../stringsext_amd/csrc/sx_selre_core.hpp"

struct HostRegex {
    sx::SelreTable T;
    std::vector<uint16_t> lds, far;   // the first lds_states rows; the whole table with those rows spoilt
};

// *rc: selre_build's code; NULL unless SX_OK.  err: room for err_cap bytes of selre_build's text.
extern "C" void* sxs_selre_create(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, int* rc, char* err, uint32_t err_cap) {
    HostRegex* S = new HostRegex;
    std::string text;
    *rc = sx::selre_build(patterns, n_patterns, flags, &S->T, &text);
    if (err && err_cap) { strncpy(err, text.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    if (*rc != SX_OK) { delete S; return nullptr; }
    const size_t lds_entries = (size_t)S->T.lds_states * S->T.classes;
    S->lds.assign(S->T.next.begin(), S->T.next.begin() + (ptrdiff_t)lds_entries);
    S->far = S->T.next;
    memset(S->far.data(), 0xEE, lds_entries * 2);
    return S;
}
extern "C" void sxs_selre_free(void* re) { delete (HostRegex*)re; }
// shape: end_first, stop_first, matched, root_end
extern "C" void sxs_selre_info(const void* re, sx_select_regex_info* out, uint32_t* shape) {
    const sx::SelreTable& T = ((const HostRegex*)re)->T;
    *out = sx_select_regex_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)T.next.size() * 2, T.lds_states, T.end_states };
    shape[0] = T.end_first; shape[1] = T.stop_first; shape[2] = T.matched; shape[3] = T.root_end;
}
// the table selre_build makes of the patterns as bytes: ten words, the class map, the entries; 0 if refused or if it does not fit
extern "C" uint64_t sxs_selre_table(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, uint8_t* out, uint64_t cap) {
    sx::SelreTable T;
    std::string err;
    if (sx::selre_build(patterns, n_patterns, flags, &T, &err) != SX_OK) return 0;
    const uint32_t words[10] = { T.n_patterns, T.states, T.classes, T.nocase, T.lds_states, T.end_first, T.stop_first, T.matched, T.root_end, T.end_states };
    const uint64_t bytes = sizeof words + 256 + T.next.size() * 2;
    if (bytes > cap) return 0;
    memcpy(out, words, sizeof words);
    memcpy(out + sizeof words, T.map, 256);
    memcpy(out + sizeof words + 256, T.next.data(), T.next.size() * 2);
    return bytes;
}

static void match_wave(const sx::SelreParams& P, const HostRegex& S, uint64_t w, uint64_t* mask, uint64_t* bytes, uint64_t* far_steps, uint64_t* steps) {
    sx::SelreLane L[sx::kSelectRecs];
    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) L[lane] = sx::selre_begin_lane(P, w, lane);
    for (;;) {
        bool any = false;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            if (!L[lane].active) continue;
            any = true;
            (*steps)++;
            if (L[lane].state >= P.re.lds_states) (*far_steps)++;
            sx::selre_step_lane(P, S.T.map, S.lds.data(), L[lane]);
        }
        if (!any) break;
    }
    *mask = 0; *bytes = 0;
    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++)
        if (sx::selre_lane_selected(P, w, lane, L[lane])) { *mask |= (uint64_t)1 << lane; *bytes += L[lane].len; }
}

// recs: n records (sx_finding16 if packed), arena: their strings.  out_recs: room for n records, out_arena: arena_cap bytes.
// masks (may be NULL): waves + 1 words.  *n_sel, *sel_bytes: the totals as the scans give them; *far_steps: the steps that
// read a row outside "LDS"; *steps: all steps (a lane that stops early takes fewer than its string has bytes).
extern "C" int sxs_selre_select_host(const void* re, const void* recs, uint64_t n, int packed, const uint8_t* arena, uint32_t invert,
                                     void* out_recs, uint8_t* out_arena, uint64_t arena_cap, uint64_t* masks, uint64_t* n_sel,
                                     uint64_t* sel_bytes, uint64_t* far_steps, uint64_t* steps) {
    const HostRegex& S = *(const HostRegex*)re;
    *n_sel = 0; *sel_bytes = 0; *far_steps = 0; *steps = 0;
    if (n == 0) return 0;   // (sx_result_select_regex_device refuses a segment without findings)
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    std::vector<uint64_t> wmask(waves + 1), wbytes(waves + 1);
    std::vector<uint32_t> wcount(waves + 1);
    sx::SelreParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs; P.arena = arena; P.n = n; P.packed = packed ? 1u : 0u; P.invert = invert ? 1u : 0u;
    P.wmask = wmask.data(); P.wcount = wcount.data(); P.wbytes = wbytes.data();
    P.re = sx::SelreDevice{ S.T.map, S.far.data(), S.T.states, S.T.classes, S.T.lds_states, S.T.end_first, S.T.stop_first, S.T.matched, S.T.root_end, 0 };
    for (uint64_t w = 0; w <= waves; w++) {
        match_wave(P, S, w, &wmask[w], &wbytes[w], far_steps, steps);
        wcount[w] = (uint32_t)__builtin_popcountll(wmask[w]);
    }
    // pass 2 is the list selection's (the regex kernel has filled the same per-wavefront words)
    return sxs_select_pass2(recs, n, packed, arena, wmask, wcount, wbytes, out_recs, out_arena, arena_cap, masks, n_sel, sel_bytes);
}
