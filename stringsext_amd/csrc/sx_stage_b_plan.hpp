// sx_stage_b_plan.hpp — the decisions of stage B's host drivers (sx_stage_b.cpp, sx_merge.cpp, sx_wave.cpp) that are pure arithmetic:
// where the exit state is replayed from, which slab cuts stand, how device_merge sizes its parts, how a slab's output block is
// laid out, how large pass 1's cache arena is.  The drivers call these; nothing here touches the device.  No HIP header: the
// test-only harness compiles it with g++ (tests/test_stage_b_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sx {
namespace plan {

constexpr uint64_t kBufLen = 4096;   // kInputBufLen (sx_host.hpp; sx_stage_b.cpp asserts they agree)

inline uint64_t up256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

// the start of the window of size W that holds p (windows restart at every input buffer)
inline uint64_t win_start_h(uint64_t p, size_t W) {
    const uint64_t s0 = p / kBufLen * kBufLen;
    return s0 + (p - s0) / W * W;
}

// Where the host replays from for the state handed to the next chunk: the Mission's start if the entry region was the last one,
// the last region's start if the replay ran into the buffer's last four windows (ts: three windows back from the tail's), else ts.
inline uint64_t exit_replay_from(uint64_t len, size_t W, uint64_t lo0, uint64_t E, uint64_t last_start, bool last_is_entry) {
    const uint64_t tail = len ? len - 1 : 0;
    uint64_t ts = win_start_h(tail, W);
    for (int t = 0; t < 3 && ts > 0; t++) ts = win_start_h(ts - 1, W);
    uint64_t from = last_is_entry ? lo0 : (E > ts ? last_start : ts);
    if (from < lo0) from = lo0;
    return from;
}

// The K - 1 cuts slab_cuts_kernel proposed (run index h_idx[j], its region's start h_hi[j]): a cut stands if it lies behind the one
// before, inside the list of n runs and in front of the job's end.  idx / his begin with 0; the caller closes idx with n.
inline void accept_slab_cuts(const uint64_t* h_idx, const uint64_t* h_hi, size_t K, uint64_t n, uint64_t job_hi,
                             std::vector<uint64_t>* idx, std::vector<uint64_t>* his) {
    idx->assign(1, 0); his->assign(1, 0);
    for (size_t j = 1; j < K; j++)
        if (h_idx[j - 1] > idx->back() && h_idx[j - 1] < n && h_hi[j - 1] < job_hi) { idx->push_back(h_idx[j - 1]); his->push_back(h_hi[j - 1]); }
}

// ---- device_merge's parts
struct MergeLimits { uint64_t part_bytes, part_findings; };
// (the switches' values, 0 = unset: 2 GiB of strings — 3.5 GiB at most, str_off has 32 bits — and 96 Mi findings per part)
inline MergeLimits merge_limits(uint64_t part_mib, uint64_t part_findings) {
    MergeLimits l{ 2048ull << 20, 96ull << 20 };
    if (part_mib) l.part_bytes = part_mib << 20;
    if (part_findings) l.part_findings = part_findings;
    if (l.part_bytes > (3584ull << 20)) l.part_bytes = 3584ull << 20;
    return l;
}
inline uint64_t merge_first_k(uint64_t bytes, uint64_t total, const MergeLimits& l) {
    return std::max<uint64_t>(1, std::max((bytes + l.part_bytes - 1) / l.part_bytes, (total + l.part_findings - 1) / l.part_findings));
}
inline uint64_t merge_clamp_k(uint64_t K, uint64_t n_slices) { return K > n_slices ? std::max<uint64_t>(1, n_slices) : K; }   // no finer than a slice per part
struct PartSize { uint64_t pf = 0, pb = 0; };   // findings and string bytes of one part, all Missions
// idx[k] / off[k]: per Mission K + 1 finding indices and string offsets
inline void merge_part_sizes(const std::vector<std::vector<uint64_t>>& idx, const std::vector<std::vector<uint64_t>>& off, uint64_t K,
                             std::vector<PartSize>* parts) {
    parts->assign(K, PartSize{});
    for (uint64_t j = 0; j < K; j++)
        for (size_t k = 0; k < idx.size(); k++) { (*parts)[j].pb += off[k][j + 1] - off[k][j]; (*parts)[j].pf += idx[k][j + 1] - idx[k][j]; }
}
// every part's strings within str_off's reach, and no more than twice the findings asked for (unless the parts are single slices)
inline bool merge_parts_fit(const std::vector<PartSize>& parts, uint64_t part_findings, uint64_t K, uint64_t n_slices) {
    for (const PartSize& p : parts)
        if (!(p.pb <= 0xFFFFFFF0ull && (p.pf <= 2 * part_findings || K >= n_slices))) return false;
    return true;
}
inline uint64_t merge_part_room(uint64_t pf, size_t rec, uint64_t pb) { return up256(pf * rec + pb); }

// ---- a slab's output block: [host findings][device findings][host strings][device strings], records of `rec` bytes
struct SlabOut {
    uint64_t nfh = 0, nf = 0, nbh = 0, nb = 0;
    size_t rec = 0;
    uint64_t dev_f = 0, host_s = 0, dev_s = 0, bytes = 0;   // byte offsets of the parts behind the first, and the block's size
    uint64_t findings() const { return nfh + nf; }
    uint64_t strings() const { return nbh + nb; }
    bool strings_fit() const { return nbh + nb <= 0xFFFFFFFFull; }   // str_off has 32 bits
};
inline SlabOut slab_out_layout(uint64_t nfh, uint64_t nf, uint64_t nbh, uint64_t nb, size_t rec) {
    SlabOut o;
    o.nfh = nfh; o.nf = nf; o.nbh = nbh; o.nb = nb; o.rec = rec;
    o.dev_f = nfh * rec; o.host_s = (nfh + nf) * rec; o.dev_s = o.host_s + nbh; o.bytes = o.dev_s + nb;
    return o;
}

// ---- pass 1's output cache: the arena for n runs.  At most 1 KiB per run within a budget of 8 GiB; for a flood of runs (slots of the
// minimum size, 160 bytes, would not fit) up to a third of the device's free memory + what the cache holds already (free_plus_held;
// 0: not known), at most 40 GiB.  cache_mib >= 0: SX_REPLAY_CACHE_MIB is the budget.
inline bool cache_arena_asks_free(uint64_t n) { return n * 160 > (8192ull << 20); }
inline uint64_t cache_arena_bytes(uint64_t n, uint64_t free_plus_held, int64_t cache_mib) {
    uint64_t budget = 8192ull << 20;
    if (cache_arena_asks_free(n) && free_plus_held) budget = std::max(budget, std::min<uint64_t>(40960ull << 20, free_plus_held / 3));
    if (cache_mib >= 0) budget = (uint64_t)cache_mib << 20;
    return std::max<uint64_t>(4096, std::min<uint64_t>(budget, n * 1024));
}

}  // namespace plan
}  // namespace sx
