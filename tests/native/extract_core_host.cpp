// Test-only harness: compiles the extract builder (sx_extract_build.cpp) and the extraction core (sx_extract_core.hpp) as host code and
// drives them the way sx_extract_dev.hip does: the class map and the rows of the first lds_states states copied to a place of their
// own ("LDS" — the table the core takes for the other states has those rows overwritten, so a look-up on the wrong side shows; the
// caller may force fewer rows into "LDS" than the builder allows), wavefront after wavefront every lane in front of its string,
// rounds of one step per active lane until no lane is active, the per-record counts and the wavefront's sums; then the exclusive
// scan over the wavefronts' counts, pass 2 with the lane's base from the stored per-record counts, and the ordered string gather
// of sx_result_core.hpp.  It also hands out the table as bytes.
#include <stdint.h>
#include <string.h>
#include <vector>
#define SXD inline
#include "guarded_host.hpp"
#include "../../stringsext_amd/csrc/sx_result_core.hpp"
#include "../../stringsext_amd/csrc/sx_extract_build.cpp"
#include "../../stringsext_amd/csrc/sx_extract_core.hpp"

struct HostExtract {
    sx::ExtractTable T;
    uint32_t lds_states;
    std::vector<uint16_t> lds, far;   // the first lds_states rows; the whole table with those rows spoilt
};

// *rc: extract_build's code; NULL unless SX_OK.  err: room for err_cap bytes of its text.  lds_cap: 0, or the most rows in "LDS".
extern "C" void* sxs_extract_create(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, uint32_t lds_cap, int* rc, char* err, uint32_t err_cap) {
    HostExtract* S = new HostExtract;
    std::string text;
    *rc = sx::extract_build(patterns, n_patterns, flags, &S->T, &text);
    if (err && err_cap) { strncpy(err, text.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    if (*rc != SX_OK) { delete S; return nullptr; }
    S->lds_states = lds_cap && lds_cap < S->T.lds_states ? lds_cap : S->T.lds_states;
    const size_t lds_entries = (size_t)S->lds_states * S->T.classes;
    S->lds.assign(S->T.next.begin(), S->T.next.begin() + (ptrdiff_t)lds_entries);
    S->far = S->T.next;
    memset(S->far.data(), 0xEE, lds_entries * 2);
    return S;
}
extern "C" void sxs_extract_free(void* ex) { delete (HostExtract*)ex; }
// shape: end_first, here_first, dead_first, start0, start1
extern "C" void sxs_extract_info(const void* ex, sx_extract_regex_info* out, uint32_t* shape) {
    const sx::ExtractTable& T = ((const HostExtract*)ex)->T;
    *out = sx_extract_regex_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)T.next.size() * 2, T.lds_states, 0 };
    shape[0] = T.end_first; shape[1] = T.here_first; shape[2] = T.dead_first; shape[3] = T.start0; shape[4] = T.start1;
}

// the set's table as bytes: ten words, the class map, the entries; 0 if it does not fit
extern "C" uint64_t sxs_extract_table(const void* ex, uint8_t* out, uint64_t cap) {
    const sx::ExtractTable& T = ((const HostExtract*)ex)->T;
    const uint32_t words[10] = { T.n_patterns, T.states, T.classes, T.nocase, T.lds_states, T.end_first, T.here_first, T.dead_first, T.start0, T.start1 };
    const uint64_t bytes = sizeof words + 256 + T.next.size() * 2;
    if (bytes > cap) return 0;
    memcpy(out, words, sizeof words);
    memcpy(out + sizeof words, T.map, 256);
    memcpy(out + sizeof words + 256, T.next.data(), T.next.size() * 2);
    return bytes;
}

// recs: n records (sx_finding16 if packed), arena: their strings.  counts: n words, the matches per record.  out_recs: room for
// out_cap records, out_arena: arena_cap bytes.  *n_out, *out_bytes: the totals as the scans give them; *far_steps: the steps that
// read a row outside "LDS"; *steps: all steps of pass 1.
extern "C" int sxs_extract_host(const void* ex, const void* recs, uint64_t n, int packed, const uint8_t* arena, uint32_t* counts,
                                void* out_recs, uint64_t out_cap, uint8_t* out_arena, uint64_t arena_cap, uint64_t* n_out,
                                uint64_t* out_bytes, uint64_t* far_steps, uint64_t* steps) {
    const HostExtract& S = *(const HostExtract*)ex;
    *n_out = 0; *out_bytes = 0; *far_steps = 0; *steps = 0;
    if (n == 0) return 0;   // (sx_result_extract_regex_device refuses a segment without findings)
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    std::vector<uint64_t> wcount(waves + 1), wbytes(waves + 1), wbase(waves + 1);
    std::vector<uint32_t> rcount(n);
    sx::ExtractParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs; P.arena = arena; P.n = n; P.packed = packed ? 1u : 0u;
    P.rcount = rcount.data(); P.wcount = wcount.data(); P.wbytes = wbytes.data();
    P.ex = sx::ExtractDevice{ S.T.map, S.far.data(), S.T.states, S.T.classes, S.lds_states, S.T.end_first, S.T.here_first, S.T.dead_first, S.T.start0, S.T.start1 };
    sx::ExtractLane L[sx::kSelectRecs];
    for (uint64_t w = 0; w <= waves; w++) {
        uint32_t count[sx::kSelectRecs] = {};
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) L[lane] = sx::extract_begin_lane(P, w, lane);
        for (bool any = true; any;) {
            any = false;
            for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                if (!L[lane].active) continue;
                any = true;
                (*steps)++;
                if (L[lane].state >= P.ex.lds_states) (*far_steps)++;
                uint32_t from = 0;
                const uint32_t end = sx::extract_step_lane(P, S.T.map, S.lds.data(), L[lane], &from);
                if (end) { count[lane]++; wbytes[w] += end - from; }
            }
        }
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            const uint64_t i = w * sx::kSelectRecs + lane;
            if (i < n) rcount[i] = count[lane];
            wcount[w] += count[lane];
        }
    }
    uint64_t total = 0, bytes = 0;
    for (uint64_t w = 0; w <= waves; w++) { wbase[w] = total; total += wcount[w]; bytes += wbytes[w]; }
    if (wcount[waves] || wbytes[waves]) return -1;
    memcpy(counts, rcount.data(), n * 4);
    *n_out = total; *out_bytes = bytes;
    if (bytes > arena_cap || total > out_cap) return -2;
    std::vector<uint64_t> src(total ? total : 1, 0);
    P.wbase = wbase.data(); P.out_recs = out_recs; P.out_src = src.data();
    for (uint64_t w = 0; w < waves; w++) {
        uint64_t rank[sx::kSelectRecs], rank_end[sx::kSelectRecs], before = 0;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            const uint64_t i = w * sx::kSelectRecs + lane;
            const uint32_t own = i < n ? rcount[i] : 0u;
            rank[lane] = wbase[w] + before; rank_end[lane] = rank[lane] + own;
            before += own;
            L[lane] = sx::extract_begin_lane(P, w, lane);
            if (!own) L[lane].active = 0;
        }
        for (bool any = true; any;) {
            any = false;
            for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
                if (!L[lane].active) continue;
                any = true;
                uint32_t from = 0;
                const uint32_t end = sx::extract_step_lane(P, S.T.map, S.lds.data(), L[lane], &from);
                if (end) {
                    sx::extract_place_match(P, w * sx::kSelectRecs + lane, rank[lane], from, end);
                    if (++rank[lane] == rank_end[lane]) L[lane].active = 0;
                }
            }
        }
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) if (rank[lane] != rank_end[lane]) return -4;
    }
    if (total == 0) return 0;
    std::vector<uint32_t> noff(total + 1);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < total; i++) {
        noff[i] = (uint32_t)sum;
        sum += packed ? ((const sx_finding16*)out_recs)[i].str_len : ((const sx_finding*)out_recs)[i].str_len;
    }
    noff[total] = (uint32_t)sum;
    if (sum != bytes) return -3;
    sx::GatherParams G{ out_recs, src.data(), noff.data(), out_arena, total, packed ? 1u : 0u };
    const uint64_t gwaves = (total + sx::kGatherRecs - 1) / sx::kGatherRecs + 1;
    for (uint64_t w = 0; w < gwaves; w++) {
        uint32_t offs[sx::kGatherRecs + 1];
        uint64_t srcs[sx::kGatherRecs];
        for (uint32_t lane = 0; lane < sx::kGatherRecs; lane++) sx::gather_load_lane(G, w, lane, offs, srcs);
        for (uint32_t lane = 0; lane < sx::kGatherRecs; lane++) sx::gather_copy_lane(G, lane, offs, srcs);
    }
    return 0;
}
