// Test-only harness: compiles the ordered string gather (sx_result_core.hpp) as host code and drives it the way
// sx_sort.hip / sx_result_dev.hip do: every record is placed by its rank (its index in its own list plus, per other list, the
// records in front of it: upper bound for the lists before its own, lower bound for those behind), the placement notes where
// the record's string lies, an exclusive scan over str_len in output order gives the new offsets, then wavefront after
// wavefront runs the two lane loops of the core.
#include <stdint.h>
#include <string.h>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_result_core.hpp"

static uint64_t bound(const sx_finding* f, uint64_t n, uint64_t p, bool upper) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (upper ? f[mid].position <= p : f[mid].position < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// list m: nf[m] records f[m], whose str_off count from off0[m]; a[m] points at the string of offset off0[m].
// out_recs: room for all records (sx_finding16 if packed), out_arena: arena_cap bytes, filled with 0xEE beyond what is written.
extern "C" int sxr_merge_ordered_host(int nm, const sx_finding* const* f, const uint8_t* const* a, const uint64_t* nf,
                                      const uint32_t* off0, int packed, void* out_recs, uint8_t* out_arena, uint64_t arena_cap,
                                      uint64_t* arena_len) {
    uint64_t n = 0;
    for (int m = 0; m < nm; m++) n += nf[m];
    std::vector<uint64_t> src(n);
    for (int m = 0; m < nm; m++)
        for (uint64_t i = 0; i < nf[m]; i++) {
            const sx_finding r = f[m][i];
            uint64_t rank = i;
            for (int o = 0; o < nm; o++)
                if (o != m && nf[o]) rank += bound(f[o], nf[o], r.position, o < m);
            if (rank >= n) return -1;
            src[rank] = (uint64_t)(uintptr_t)(a[m] + (uint32_t)(r.str_off - off0[m]));
            if (packed) {
                sx_finding16 p;
                p.position = r.position; p.str_off = 0xDEADBEEFu; p.str_len = (uint16_t)r.str_len;
                p.flags = (uint8_t)((r.precision & 3u) | (r.completes_previous ? 4u : 0u)); p.mission_id = r.mission_id;
                ((sx_finding16*)out_recs)[rank] = p;
            } else { ((sx_finding*)out_recs)[rank] = r; ((sx_finding*)out_recs)[rank].str_off = 0xDEADBEEFu; }
        }
    std::vector<uint32_t> noff(n + 1);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) {
        noff[i] = (uint32_t)sum;
        sum += packed ? ((const sx_finding16*)out_recs)[i].str_len : ((const sx_finding*)out_recs)[i].str_len;
    }
    noff[n] = (uint32_t)sum;
    if (sum > arena_cap) return -2;
    *arena_len = sum;
    sx::GatherParams P{ out_recs, src.data(), noff.data(), out_arena, n, packed ? 1u : 0u };
    const uint64_t waves = (n + sx::kGatherRecs - 1) / sx::kGatherRecs + 1;   // (one more: a wavefront behind the last record writes nothing)
    for (uint64_t w = 0; w < waves; w++) {
        uint32_t offs[sx::kGatherRecs + 1];
        uint64_t srcs[sx::kGatherRecs];
        for (uint32_t lane = 0; lane < sx::kGatherRecs; lane++) sx::gather_load_lane(P, w, lane, offs, srcs);
        for (uint32_t lane = 0; lane < sx::kGatherRecs; lane++) sx::gather_copy_lane(P, lane, offs, srcs);
    }
    return 0;
}
