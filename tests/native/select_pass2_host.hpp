// Test-only: what follows pass 1 of every selection (select_core_host.cpp, selset_core_host.cpp, selre_core_host.cpp,
// label_core_host.cpp: their kernels fill the same per-wavefront words), driven the way the device drives it: the exclusive scan
// over the wavefronts' counts, select_place_lane, then the ordered string gather of sx_result_core.hpp as order_part_strings runs
// it (a scan over str_len in output order, its two lane loops).
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#ifndef SXD
#define SXD inline
#endif
#include "../../stringsext_amd/csrc/sx_result_core.hpp"
#include "../../stringsext_amd/csrc/sx_select_core.hpp"

// wmask, wcount, wbytes: waves + 1 words each, as pass 1 left them.  out_recs: room for n records, out_arena: arena_cap bytes.
// masks (may be NULL): waves + 1 words.  *n_sel, *sel_bytes: the totals as the scans give them.  0; -1: the wavefront behind the
// last record selected something; -2: the strings do not fit; -3: the placed records' lengths do not add up to the bytes counted.
inline int sxs_select_pass2(const void* recs, uint64_t n, int packed, const uint8_t* arena, std::vector<uint64_t>& wmask,
                            const std::vector<uint32_t>& wcount, const std::vector<uint64_t>& wbytes, void* out_recs, uint8_t* out_arena,
                            uint64_t arena_cap, uint64_t* masks, uint64_t* n_sel, uint64_t* sel_bytes) {
    const uint64_t waves = wmask.size() - 1;
    std::vector<uint32_t> wbase(waves + 1);
    uint64_t count = 0, bytes = 0;
    for (uint64_t w = 0; w <= waves; w++) { wbase[w] = (uint32_t)count; count += wcount[w]; bytes += wbytes[w]; }
    if (wcount[waves] || wbytes[waves]) return -1;
    if (masks) memcpy(masks, wmask.data(), (waves + 1) * 8);
    *n_sel = count; *sel_bytes = bytes;
    if (bytes > arena_cap) return -2;
    std::vector<uint64_t> src(count ? count : 1, 0);
    sx::SelectParams Q;
    memset(&Q, 0, sizeof Q);
    Q.recs = recs; Q.arena = arena; Q.n = n; Q.packed = packed ? 1u : 0u;
    Q.wmask = wmask.data(); Q.wbase = wbase.data(); Q.out_recs = out_recs; Q.out_src = src.data();
    for (uint64_t w = 0; w < waves; w++)
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) sx::select_place_lane(Q, w, lane);
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
