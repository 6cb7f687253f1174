// The pure decisions of stage B's host drivers (stringsext_amd/csrc/sx_stage_b_plan.hpp) behind one C entry point, for
// tests/test_stage_b_plan.py (through ctypes) and for the stand-alone sanitizer program (stage_b_plan_main.cpp, which includes
// this file).  A case is a function name and a list of u64 arguments; the answer is a list of u64.
#include <string.h>

#include "../../stringsext_amd/csrc/sx_stage_b_plan.hpp"

using namespace sx::plan;

// returns the number of words written to out (at most out_cap), or -1: unknown function / too few arguments / no room
extern "C" long sbp_eval(const char* fn, const uint64_t* a, size_t na, uint64_t* out, size_t out_cap) {
    auto is = [&](const char* name, size_t need) { return strcmp(fn, name) == 0 && na >= need; };
    size_t n = 0;
    auto put = [&](uint64_t v) { if (n < out_cap) out[n] = v; n++; };
    if (is("win_start", 2)) put(win_start_h(a[0], (size_t)a[1]));
    else if (is("exit_from", 6)) put(exit_replay_from(a[0], (size_t)a[1], a[2], a[3], a[4], a[5] != 0));
    else if (is("slab_cuts", 3)) {   // K, n, job_hi, then K - 1 cut indices, then K - 1 region starts -> idx..., his...
        const size_t K = (size_t)a[0];
        if (na < 3 + 2 * (K - 1)) return -1;
        std::vector<uint64_t> idx, his;
        accept_slab_cuts(a + 3, a + 3 + (K - 1), K, a[1], a[2], &idx, &his);
        put(idx.size());
        for (uint64_t v : idx) put(v);
        for (uint64_t v : his) put(v);
    } else if (is("merge_first_k", 4)) {   // bytes, total, the two switches -> part_bytes, part_findings, K
        const MergeLimits l = merge_limits(a[2], a[3]);
        put(l.part_bytes); put(l.part_findings); put(merge_first_k(a[0], a[1], l));
    } else if (is("merge_clamp_k", 2)) put(merge_clamp_k(a[0], a[1]));
    else if (is("merge_parts", 4)) {   // nm, K, part_findings, n_slices, then per Mission K + 1 indices and K + 1 offsets -> fits, (pf, pb) per part
        const size_t nm = (size_t)a[0];
        const uint64_t K = a[1];
        if (na < 4 + nm * 2 * (K + 1)) return -1;
        std::vector<std::vector<uint64_t>> idx(nm), off(nm);
        const uint64_t* p = a + 4;
        for (size_t k = 0; k < nm; k++) { idx[k].assign(p, p + K + 1); p += K + 1; off[k].assign(p, p + K + 1); p += K + 1; }
        std::vector<PartSize> parts;
        merge_part_sizes(idx, off, K, &parts);
        put(merge_parts_fit(parts, a[2], K, a[3]) ? 1 : 0);
        for (const PartSize& s : parts) { put(s.pf); put(s.pb); }
    } else if (is("part_room", 3)) put(merge_part_room(a[0], (size_t)a[1], a[2]));
    else if (is("slab_out", 5)) {
        const SlabOut o = slab_out_layout(a[0], a[1], a[2], a[3], (size_t)a[4]);
        put(o.dev_f); put(o.host_s); put(o.dev_s); put(o.bytes); put(o.findings()); put(o.strings()); put(o.strings_fit() ? 1 : 0);
    } else if (is("cache_arena", 3)) { put(cache_arena_asks_free(a[0]) ? 1 : 0); put(cache_arena_bytes(a[0], a[1], (int64_t)a[2])); }
    else return -1;
    return n <= out_cap ? (long)n : -1;
}
