// Test-only harness: compiles the substring selection (sx_select_core.hpp) as host code and drives it the way sx_select_dev.hip
// does: wavefront after wavefront the load step, the vote of its 64 lanes on "one range", the scan or the walk, the ballot, the
// count and the string bytes; an exclusive scan over the wavefronts' counts; the placement; then the ordered string gather of
// sx_result_core.hpp as order_part_strings runs it (a scan over str_len in output order, its two lane loops).
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_result_core.hpp"
#include "../../stringsext_amd/csrc/sx_select_core.hpp"

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
    std::vector<uint32_t> wcount(waves + 1), wbase(waves + 1);
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
    uint64_t count = 0, bytes = 0;
    for (uint64_t w = 0; w <= waves; w++) { wbase[w] = (uint32_t)count; count += wcount[w]; bytes += wbytes[w]; }
    if (wcount[waves] || wbytes[waves]) return -1;
    if (masks) memcpy(masks, wmask.data(), (waves + 1) * 8);
    *n_sel = count; *sel_bytes = bytes;
    if (bytes > arena_cap) return -2;
    std::vector<uint64_t> src(count ? count : 1, 0);
    P.wbase = wbase.data(); P.out_recs = out_recs; P.out_src = src.data();
    for (uint64_t w = 0; w < waves; w++)
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) sx::select_place_lane(P, w, lane);
    if (count == 0) return 0;
    std::vector<uint32_t> noff(count + 1);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < count; i++) {
        noff[i] = (uint32_t)sum;
        sum += packed ? ((const sx_finding16*)out_recs)[i].str_len : ((const sx_finding*)out_recs)[i].str_len;
    }
    noff[count] = (uint32_t)sum;
    if (sum != bytes) return -3;
    sx::GatherParams G{ out_recs, src.data(), noff.data(), out_arena, count, packed ? 1u : 0u };
    const uint64_t gwaves = (count + sx::kGatherRecs - 1) / sx::kGatherRecs + 1;
    for (uint64_t w = 0; w < gwaves; w++) {
        uint32_t offs[sx::kGatherRecs + 1];
        uint64_t srcs[sx::kGatherRecs];
        for (uint32_t lane = 0; lane < sx::kGatherRecs; lane++) sx::gather_load_lane(G, w, lane, offs, srcs);
        for (uint32_t lane = 0; lane < sx::kGatherRecs; lane++) sx::gather_copy_lane(G, lane, offs, srcs);
    }
    return 0;
}

// `bytes` bytes that end where a page without access begins: a read behind the arena faults
extern "C" void* sxs_guarded(uint64_t bytes, void** region, uint64_t* region_bytes) {
    const uint64_t page = (uint64_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
    uint8_t* p = (uint8_t*)mmap(nullptr, body + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED || mprotect(p + body, page, PROT_NONE) != 0) return nullptr;
    *region = p; *region_bytes = body + page;
    return p + body - bytes;
}
extern "C" void sxs_unmap(void* region, uint64_t region_bytes) { munmap(region, region_bytes); }
