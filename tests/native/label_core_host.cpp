// Test-only harness: compiles the label builder (sx_label_build.cpp) and the label core (sx_label_core.hpp) as host code and drives
// them the way sx_label_dev.hip does: the class map and the rows of the first lds_states states copied to a place of their own
// ("LDS" — the table the core takes for the other states has those rows overwritten, so a look-up on the wrong side shows), a grid
// of workgroups of 8 wavefronts that strides over the segment, per wavefront every lane in front of its string, rounds of one step
// per active lane until no lane is active, the labels, the OR over the lanes, per bit of it the ballot into the workgroup's
// counters, and the flush when the workgroup ends; then, for the selection by label, label_pick_lane per lane, and as
// selre_core_host.cpp the exclusive scan over the wavefronts' counts, select_place_lane and the ordered string gather of
// sx_result_core.hpp (select_pass2_host.hpp).  It also hands out the table as bytes.
#include <stdint.h>
#include <string.h>
#include <vector>
#define SXD inline
#include "guarded_host.hpp"
#include "select_pass2_host.hpp"
#include "../../stringsext_amd/csrc/sx_label_build.cpp"
#include "../../stringsext_amd/csrc/sx_label_core.hpp"

struct HostLabels {
    sx::LabelTable T;
    std::vector<uint16_t> lds, far;   // the first lds_states rows; the whole table with those rows spoilt
};

// *rc: label_build's code; NULL unless SX_OK.  err: room for err_cap bytes of label_build's text.
extern "C" void* sxs_label_create(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, int* rc, char* err, uint32_t err_cap) {
    HostLabels* S = new HostLabels;
    std::string text;
    *rc = sx::label_build(patterns, n_patterns, flags, &S->T, &text);
    if (err && err_cap) { strncpy(err, text.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    if (*rc != SX_OK) { delete S; return nullptr; }
    const size_t lds_entries = (size_t)S->T.lds_states * S->T.classes;
    S->lds.assign(S->T.next.begin(), S->T.next.begin() + (ptrdiff_t)lds_entries);
    S->far = S->T.next;
    memset(S->far.data(), 0xEE, lds_entries * 2);
    return S;
}
extern "C" void sxs_label_free(void* set) { delete (HostLabels*)set; }
// shape: here_first, dead, root_here, all, the entries of here[], the entries of end[]
extern "C" void sxs_label_info(const void* set, sx_label_set_info* out, uint64_t* shape) {
    const sx::LabelTable& T = ((const HostLabels*)set)->T;
    *out = sx_label_set_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)(256 + T.next.size() * 2 + T.here.size() * 8 + T.end.size() * 8), T.lds_states, (uint32_t)T.here.size() };
    shape[0] = T.here_first; shape[1] = T.dead; shape[2] = T.root_here; shape[3] = T.all; shape[4] = T.here.size(); shape[5] = T.end.size();
}
// the set's table as bytes: LabelTable's seven words, its two masks, the class map, then next, here, end; 0 if it does not fit
extern "C" uint64_t sxs_label_table(const void* set, uint8_t* out, uint64_t cap) {
    const sx::LabelTable& T = ((const HostLabels*)set)->T;
    const uint32_t words[7] = { T.n_patterns, T.states, T.classes, T.nocase, T.lds_states, T.here_first, T.dead };
    const uint64_t masks[2] = { T.root_here, T.all };
    const struct { const void* at; uint64_t bytes; } parts[6] = { { words, sizeof words }, { masks, sizeof masks }, { T.map, 256 }, { T.next.data(), T.next.size() * 2 },
                                                                  { T.here.data(), T.here.size() * 8 }, { T.end.data(), T.end.size() * 8 } };
    uint64_t bytes = 0;
    for (const auto& p : parts) bytes += p.bytes;
    if (bytes > cap) return 0;
    for (const auto& p : parts) if (p.bytes) { memcpy(out, p.at, p.bytes); out += p.bytes; }
    return bytes;
}

constexpr uint32_t kWaves = 8;      // wavefronts per workgroup, as kLabelWaves

// recs: n records (sx_finding16 if packed), arena: their strings; ordinal: of record 0; groups: the grid.  labels: n words.
// findings, first: 64 words each, added to (the caller resets them: 0 and all ones).  *far_steps: the steps that read a row outside
// "LDS"; *steps: all steps (a lane that stops early takes fewer than its string has bytes).
extern "C" int sxs_label_host(const void* set, const void* recs, uint64_t n, int packed, const uint8_t* arena, uint64_t ordinal, uint32_t groups,
                              uint64_t* labels, uint64_t* findings, uint64_t* first, uint64_t* far_steps, uint64_t* steps) {
    const HostLabels& S = *(const HostLabels*)set;
    *far_steps = 0; *steps = 0;
    if (n == 0) return 0;
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    sx::LabelParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs; P.arena = arena; P.n = n; P.packed = packed ? 1u : 0u; P.ordinal = ordinal; P.labels = labels;
    P.set = sx::LabelDevice{ S.T.map, S.far.data(), S.T.here.data(), S.T.end.data(), findings, first, S.T.root_here, S.T.all,
                             S.T.states, S.T.classes, S.T.lds_states, S.T.here_first, S.T.dead, S.T.n_patterns };
    for (uint32_t g = 0; g < groups; g++) {
        uint32_t counts[sx::kLabelBits];
        uint64_t mins[sx::kLabelBits];
        for (uint32_t c = 0; c < sx::kLabelBits; c++) { counts[c] = 0; mins[c] = ~(uint64_t)0; }
        for (uint32_t wv = 0; wv < kWaves; wv++)
            for (uint64_t w = (uint64_t)g * kWaves + wv; w < waves; w += (uint64_t)groups * kWaves) {
                sx::LabelLane L[sx::kSelectRecs];
                for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) L[lane] = sx::label_begin_lane(P, w, lane);
                for (;;) {
                    bool any = false;
                    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                        if (!L[lane].active) continue;
                        any = true;
                        (*steps)++;
                        if (L[lane].state >= P.set.lds_states) (*far_steps)++;
                        sx::label_step_lane(P, S.T.map, S.lds.data(), L[lane]);
                    }
                    if (!any) break;
                }
                uint64_t ored = 0;
                for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                    const uint64_t i = w * sx::kSelectRecs + lane;
                    if (i < n) labels[i] = L[lane].acc;
                    else if (L[lane].acc) return -1;
                    ored |= L[lane].acc;
                }
                for (uint64_t m = ored; m; m &= m - 1u) {
                    const uint32_t p = (uint32_t)__builtin_ctzll(m);
                    uint64_t ballot = 0;
                    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) ballot |= ((L[lane].acc >> p) & 1u) << lane;
                    sx::label_count_bit(counts, mins, p, ballot, P.ordinal + w * sx::kSelectRecs);
                }
            }
        for (uint32_t c = 0; c < sx::kLabelBits; c++) sx::label_flush_lane(P, counts, mins, c);
    }
    return 0;
}

// The selection by label.  recs: n records (sx_finding16 if packed), arena: their strings, labels: n words.  out_recs: room for n
// records, out_arena: arena_cap bytes.  masks (may be NULL): waves + 1 words.  *n_sel, *sel_bytes: the totals as the scans give them.
extern "C" int sxs_label_pick_host(const void* recs, uint64_t n, int packed, const uint8_t* arena, const uint64_t* labels, uint64_t any,
                                   uint64_t all, uint64_t none, void* out_recs, uint8_t* out_arena, uint64_t arena_cap, uint64_t* masks,
                                   uint64_t* n_sel, uint64_t* sel_bytes) {
    *n_sel = 0; *sel_bytes = 0;
    if (n == 0) return 0;
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    std::vector<uint64_t> wmask(waves + 1), wbytes(waves + 1);
    std::vector<uint32_t> wcount(waves + 1);
    sx::SelectParams Q;
    memset(&Q, 0, sizeof Q);
    Q.recs = recs; Q.arena = nullptr; Q.n = n; Q.packed = packed ? 1u : 0u;      // (pass 1 has no arena: it reads no string byte)
    const sx::LabelPick K{ labels, any, all, none };
    for (uint64_t w = 0; w <= waves; w++) {
        uint64_t mask = 0, bytes = 0;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            uint32_t len;
            if (sx::label_pick_lane(Q, K, w, lane, &len)) mask |= (uint64_t)1 << lane;
            bytes += len;
        }
        wmask[w] = mask; wcount[w] = (uint32_t)__builtin_popcountll(mask); wbytes[w] = bytes;
    }
    // pass 2 is the list selection's (the pick has filled the same per-wavefront words)
    return sxs_select_pass2(recs, n, packed, arena, wmask, wcount, wbytes, out_recs, out_arena, arena_cap, masks, n_sel, sel_bytes);
}
