// Test-only harness: compiles the substring selection (sx_select_core.hpp) as host code and drives it the way sx_select_dev.hip
// does: wavefront after wavefront the load step, the vote of its 64 lanes on "one range", the scan or the walk, the ballot, the
// count and the string bytes; then select_pass2_host.hpp: an exclusive scan over the wavefronts' counts, the placement, and the
// ordered string gather of sx_result_core.hpp.
#include <stdint.h>
#include <string.h>
#include <vector>
#define SXD inline
#include "guarded_host.hpp"
#include "select_pass2_host.hpp"

// recs: n records (sx_finding16 if packed), arena: their strings; pat_bytes: n_pat rows of 64 bytes, pat_len: their lengths.
// out_recs: room for n records, out_arena: arena_cap bytes.  masks (may be NULL): waves + 1 words, the wavefronts' selected
// masks.  *n_sel, *sel_bytes: the totals as the scans give them; *range_waves: the wavefronts that took the one-range path.
extern "C" int sxs_select_host(const void* recs, uint64_t n, int packed, const uint8_t* arena, const uint8_t* pat_bytes,
                               const uint32_t* pat_len, int n_pat, uint32_t flags, void* out_recs, uint8_t* out_arena,
                               uint64_t arena_cap, uint64_t* masks, uint64_t* n_sel, uint64_t* sel_bytes, uint64_t* range_waves) {
    *n_sel = 0; *sel_bytes = 0; *range_waves = 0;
    if (n == 0) return 0;   // (sx_result_select_device refuses a segment without findings)
    std::vector<sx_pattern> pats((size_t)n_pat);
    for (int p = 0; p < n_pat; p++) pats[(size_t)p] = sx_pattern{ pat_bytes + 64 * p, pat_len[p] };
    const uint64_t waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    std::vector<uint64_t> wmask(waves + 1), wbytes(waves + 1);
    std::vector<uint32_t> wcount(waves + 1);
    sx::SelectParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs; P.arena = arena; P.n = n; P.packed = packed ? 1u : 0u;
    P.wmask = wmask.data(); P.wcount = wcount.data(); P.wbytes = wbytes.data();
    sx::select_fill_patterns(&P.pat, pats.data(), n_pat, flags);
    uint16_t first[sx::kSelectFirst];
    for (uint32_t x = 0; x < sx::kSelectFirst; x++) first[x] = sx::select_first_entry(P, x);
    for (uint64_t w = 0; w <= waves; w++) {
        uint64_t offs[sx::kSelectRecs + 1];
        uint32_t lens[sx::kSelectRecs], hit[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu };
        bool one_range = true;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) one_range &= sx::select_load_lane(P, w, lane, offs, lens, hit);
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            if (one_range) sx::select_scan_lane(P, first, lane, offs, hit);
            else sx::select_walk_lane(P, first, lane, offs, lens, hit);
        }
        uint64_t mask = 0, bytes = 0;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++)
            if (sx::select_lane_selected(P, w, lane, hit)) { mask |= (uint64_t)1 << lane; bytes += lens[lane]; }
        wmask[w] = mask; wcount[w] = (uint32_t)__builtin_popcountll(mask); wbytes[w] = bytes;
        if (one_range && w < waves) (*range_waves)++;
    }
    return sxs_select_pass2(recs, n, packed, arena, wmask, wcount, wbytes, out_recs, out_arena, arena_cap, masks, n_sel, sel_bytes);
}
