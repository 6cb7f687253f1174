// Test-only harness: compiles the lane functions of the sorted order (sx_order_core.hpp) as host code and drives them the way
// sx_order_dev.hip and the driver of sx_result_order_device do: pick over every segment — a grid of workgroups of 8 wavefronts that
// strides over the segment, every lane of a wavefront, the wavefront's ballot, count, bytes and longest string —, the exclusive scan
// over the wavefronts' counts, number over every segment; then the label key's one stable sort, or the rounds of the string key:
// word, three stable sorts with the least significant key first (std::stable_sort stands where rocprim's radix sort stands), split,
// the exclusive scan over the flag words, compact, and one look at the scan's total, until no slot is undecided — a round more than
// longest / 8 + 2 ends the call with -1 —; then measure, gather, and the strings laid back to back as order_part_strings lays them.
// With SXS_ORDER_MAIN the file is a program of its own that runs inputs of its own against std::stable_sort with memcmp: the
// sanitizer run of tests/test_order_core.py.
#include <algorithm>
#include <numeric>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_order_core.hpp"
#include "seen_set_host.hpp"      // (sxs_guarded, sxs_unmap: the arenas end where a page without access begins)

namespace {

constexpr uint32_t kWaves = 8;      // wavefronts per workgroup, as kRowsWaves

// the wavefronts of `n` lanes as a grid of `groups` workgroups walks them
template <class F>
void over_waves(uint64_t n, uint32_t groups, F f) {
    const uint64_t waves = (n + 63) / 64;
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t wv = 0; wv < kWaves; wv++)
            for (uint64_t w = (uint64_t)g * kWaves + wv; w < waves; w += (uint64_t)groups * kWaves) f(w);
}
template <class F>
void over_lanes(uint64_t n, uint32_t groups, F f) {
    over_waves(n, groups, [&](uint64_t w) { for (uint32_t lane = 0; lane < 64; lane++) f(w * 64 + lane); });
}

struct Spec {
    uint32_t by, flags, shift, bits;
    uint64_t any, all, none, limit;
};

// info: findings, kept, rounds, tied, max_depth.  left: the undecided slots after each round.  order: the keys of the whole order
// (findings of them).  out / out_arena: the kept records and their strings.  Returns 0; -1: a round too many; -2: a list grew.
int order_host(std::vector<sx::OrderSeg> segs, const Spec& spec, uint32_t groups, uint64_t* info, uint64_t* left, uint32_t left_cap, uint64_t* order_out,
               sx_finding* out, uint8_t* out_arena) {
    const uint32_t descending = spec.flags & SX_ORDER_DESCENDING ? 1u : 0u, nocase = spec.flags & SX_ORDER_NOCASE ? 1u : 0u;
    const bool by_field = spec.by == SX_ORDER_BY_LABEL_FIELD;
    uint64_t waves = 0, all = 0;
    for (sx::OrderSeg& s : segs) { s.wave0 = waves; waves += (s.n + 63) / 64; all += s.n; }
    std::vector<uint64_t> wmask(waves + 1, 0xEEEEEEEEEEEEEEEEull);
    std::vector<uint32_t> wcount(waves + 1, 0xEEEEEEEEu), wbase(waves + 1, 0);
    uint64_t totals[sx::kOrderTotals] = { 0 };
    sx::OrderPick pick;
    memset(&pick, 0, sizeof pick);
    pick.filter = (spec.any | spec.all | spec.none) != 0; pick.any = spec.any; pick.all = spec.all; pick.none = spec.none;
    pick.wmask = wmask.data(); pick.wcount = wcount.data(); pick.wbase = wbase.data(); pick.totals = totals;
    pick.shift = spec.shift; pick.descending = descending; pick.mask = spec.bits >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << spec.bits) - 1u;
    for (size_t s = 0; s < segs.size(); s++) {
        pick.seg = segs[s]; pick.seg_index = (uint32_t)s;
        for (uint32_t g = 0; g < groups; g++)
            for (uint32_t wv = 0; wv < kWaves; wv++) {      // (order_pick_kernel: a wavefront's trips, then its adds)
                uint64_t count = 0, bytes = 0, longest = 0;
                for (uint64_t w = (uint64_t)g * kWaves + wv; w < (segs[s].n + 63) / 64; w += (uint64_t)groups * kWaves) {
                    uint64_t mask = 0;
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        uint32_t len;
                        if (sx::order_pick_lane(pick, w, lane, &len)) mask |= (uint64_t)1 << lane;
                        bytes += len; longest = std::max<uint64_t>(longest, len);
                    }
                    wmask[segs[s].wave0 + w] = mask; wcount[segs[s].wave0 + w] = (uint32_t)__builtin_popcountll(mask);
                    count += (uint64_t)__builtin_popcountll(mask);
                }
                if (count) { totals[sx::kOrderCount] += count; totals[sx::kOrderBytes] += bytes; totals[sx::kOrderLongest] = std::max(totals[sx::kOrderLongest], longest); }
            }
    }
    wcount[waves] = 0;
    for (uint64_t w = 0, at = 0; w <= waves; w++) { wbase[w] = (uint32_t)at; at += wcount[w]; }
    const uint64_t m = totals[sx::kOrderCount];
    info[0] = m; info[1] = info[2] = info[3] = info[4] = 0;
    if (m == 0) return 0;
    // the sort's tables: m + 1 entries each, as order_sort_tables sizes them
    std::vector<uint64_t> ikey[2] = { std::vector<uint64_t>(m + 1), std::vector<uint64_t>(m + 1) }, wkey(m + 1), k64(m + 1), flags(m + 1), scan(m + 1), order(m + 1, ~(uint64_t)0);
    std::vector<uint32_t> slotpos[2] = { std::vector<uint32_t>(m + 1), std::vector<uint32_t>(m + 1) }, slotgrp[2] = { std::vector<uint32_t>(m + 1), std::vector<uint32_t>(m + 1) };
    std::vector<uint32_t> rkey(m + 1), iota(m + 1), k32(m + 1), perm(m + 1), classhead(m + 1, 0xEEEEEEEEu);
    pick.ikey = ikey[0].data(); pick.slotpos = slotpos[0].data(); pick.slotgrp = slotgrp[0].data(); pick.field = by_field ? wkey.data() : nullptr;
    for (size_t s = 0; s < segs.size(); s++) {
        pick.seg = segs[s]; pick.seg_index = (uint32_t)s;
        over_waves(segs[s].n, groups, [&](uint64_t w) { for (uint32_t lane = 0; lane < 64; lane++) sx::order_number_lane(pick, w, lane); });
    }
    uint64_t rounds = 0;
    if (by_field) {
        const uint64_t keep = spec.bits >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << spec.bits) - 1u;      // (the sort looks at `bits` bits)
        std::copy(slotpos[0].begin(), slotpos[0].begin() + m, perm.begin());
        std::stable_sort(perm.begin(), perm.begin() + m, [&](uint32_t a, uint32_t b) { return (wkey[a] & keep) < (wkey[b] & keep); });
        for (uint64_t p = 0; p < m; p++) k64[p] = wkey[perm[p]];
        const sx::OrderField F{ m, k64.data(), perm.data(), ikey[0].data(), order.data(), classhead.data() };
        over_lanes(m, groups, [&](uint64_t p) { sx::order_field_lane(F, p); });
    } else {
        const uint64_t most = totals[sx::kOrderLongest] / 8 + 2;
        uint64_t n = m, n_groups = 1;
        int cur = 0;
        while (n != 0) {
            if (rounds >= most) return -1;
            sx::OrderRound P;
            memset(&P, 0, sizeof P);
            P.segs = segs.data(); P.n = n; P.nocase = nocase; P.descending = descending; P.depth = (uint32_t)rounds;
            P.ikey = ikey[cur].data(); P.slotpos = slotpos[cur].data(); P.slotgrp = slotgrp[cur].data();
            P.wkey = wkey.data(); P.rkey = rkey.data(); P.iota = iota.data(); P.perm = perm.data();
            P.order = order.data(); P.classhead = classhead.data(); P.flags = flags.data(); P.scan = scan.data();
            P.ikey_next = ikey[cur ^ 1].data(); P.slotpos_next = slotpos[cur ^ 1].data(); P.slotgrp_next = slotgrp[cur ^ 1].data();
            over_lanes(n, groups, [&](uint64_t j) { sx::order_word_lane(P, j); });
            // least significant key first: rem in 4 bits, the word, the group in the bits its ids need
            std::copy(iota.begin(), iota.begin() + n, perm.begin());
            std::stable_sort(perm.begin(), perm.begin() + n, [&](uint32_t a, uint32_t b) { return (rkey[a] & 15u) < (rkey[b] & 15u); });
            over_lanes(n, groups, [&](uint64_t j) { sx::order_wkey_lane(wkey.data(), perm.data(), k64.data(), n, j); });
            {
                std::vector<uint32_t> at(n), next(n);
                std::iota(at.begin(), at.end(), 0u);
                std::stable_sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return k64[a] < k64[b]; });
                for (uint64_t j = 0; j < n; j++) next[j] = perm[at[j]];
                std::copy(next.begin(), next.end(), perm.begin());
            }
            if (n_groups > 1) {
                unsigned bits = 1;
                while (bits < 32 && ((n_groups - 1) >> bits)) bits++;
                const uint32_t keep = bits >= 32 ? ~0u : (1u << bits) - 1u;
                over_lanes(n, groups, [&](uint64_t j) { sx::order_gkey_lane(P.slotgrp, perm.data(), k32.data(), n, j); });
                std::vector<uint32_t> at(n), next(n);
                std::iota(at.begin(), at.end(), 0u);
                std::stable_sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return (k32[a] & keep) < (k32[b] & keep); });
                for (uint64_t j = 0; j < n; j++) next[j] = perm[at[j]];
                std::copy(next.begin(), next.end(), perm.begin());
            }
            over_lanes(n, groups, [&](uint64_t j) { sx::order_split_lane(P, j); });
            for (uint64_t j = 0, at = 0; j <= n; j++) { scan[j] = at; at += flags[j]; }
            over_lanes(n, groups, [&](uint64_t j) { sx::order_compact_lane(P, j); });
            const uint64_t word = scan[n];
            if (rounds < left_cap) left[rounds] = word & 0xFFFFFFFFu;
            rounds++;
            if ((word & 0xFFFFFFFFu) > n) return -2;
            n = word & 0xFFFFFFFFu; n_groups = word >> 32; cur ^= 1;
        }
    }
    const uint64_t kept = spec.limit && spec.limit < m ? spec.limit : m;
    std::vector<uint64_t> src(kept + 1);
    sx::OrderOut O;
    memset(&O, 0, sizeof O);
    O.segs = segs.data(); O.order = order.data(); O.classhead = classhead.data(); O.kept = kept; O.totals = totals; O.out = out; O.out_src = src.data();
    over_waves(kept, groups, [&](uint64_t w) {
        for (uint32_t lane = 0; lane < 64; lane++) {
            uint32_t len; bool tied;
            sx::order_measure_lane(O, w * 64 + lane, &len, &tied);
            totals[sx::kOrderKeptBytes] += len; totals[sx::kOrderTied] += tied;
        }
    });
    over_lanes(kept, groups, [&](uint64_t p) { sx::order_gather_lane(O, p); });
    uint64_t at = 0;      // (order_part_strings)
    for (uint64_t p = 0; p < kept; p++) {
        memcpy(out_arena + at, (const void*)(uintptr_t)src[p], out[p].str_len);
        out[p].str_off = (uint32_t)at; at += out[p].str_len;
    }
    if (at != totals[sx::kOrderKeptBytes]) return -3;
    for (uint64_t p = 0; p < m; p++) order_out[p] = order[p];
    info[1] = kept; info[2] = rounds; info[3] = totals[sx::kOrderTied]; info[4] = rounds ? rounds - 1 : 0;
    return 0;
}

}  // namespace

// n_segs segments: recs[s] = ns[s] records (sx_finding16 if packed[s]: then file_ids[s], slice_bases[s] and pos0[s] — 256 words — say
// what they share), arenas[s] = their strings, labels[s] = their label words (labels NULL: the call has none).  spec: by, flags,
// shift, bits; masks: any, all, none, limit.  groups: the grid.
extern "C" int sxs_order_host(uint32_t n_segs, const void* const* recs, const uint8_t* const* arenas, const uint64_t* ns, const int32_t* packed,
                              const int32_t* file_ids, const uint32_t* slice_bases, const uint64_t* const* pos0, const uint64_t* const* labels,
                              const uint32_t* spec, const uint64_t* masks, uint32_t groups, uint64_t* info, uint64_t* left, uint32_t left_cap,
                              uint64_t* order_out, sx_finding* out, uint8_t* out_arena) {
    std::vector<sx::OrderSeg> segs(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) {
        memset(&segs[s], 0, sizeof segs[s]);
        segs[s].recs = recs[s]; segs[s].arena = arenas[s]; segs[s].n = ns[s]; segs[s].packed = packed[s] ? 1u : 0u;
        segs[s].file_id = file_ids[s]; segs[s].slice_base = slice_bases[s]; segs[s].pos0 = pos0[s]; segs[s].labels = labels ? labels[s] : nullptr;
    }
    return order_host(segs, Spec{ spec[0], spec[1], spec[2], spec[3], masks[0], masks[1], masks[2], masks[3] }, groups, info, left, left_cap, order_out, out, out_arena);
}

// one word of the string key, for the tests of the loads and the fold: the (w, rem) of `s` at `depth` as word writes them
extern "C" void sxs_order_word(const uint8_t* s, uint32_t len, uint32_t depth, uint32_t nocase, uint32_t descending, uint64_t* w, uint32_t* rem) {
    sx_finding f;
    memset(&f, 0, sizeof f);
    f.str_len = len;
    sx::OrderSeg seg;
    memset(&seg, 0, sizeof seg);
    seg.recs = &f; seg.arena = s; seg.n = 1;
    uint64_t ikey = 0;
    uint32_t iota = 7;
    sx::OrderRound P;
    memset(&P, 0, sizeof P);
    P.segs = &seg; P.n = 1; P.nocase = nocase; P.descending = descending; P.depth = depth; P.ikey = &ikey; P.wkey = w; P.rkey = rem; P.iota = &iota;
    sx::order_word_lane(P, 0);
}

#ifdef SXS_ORDER_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string>

// The program of the sanitizer run: a few hundred strings — every length 0..40, long shared prefixes, letter case, bytes from 0x80 on,
// trailing NULs — in two segments, one packed and one not, each string in memory of exactly its segment's size, under every
// combination of key, direction, fold, filter and limit, against std::stable_sort over the strings.
int main() {
    std::vector<std::string> strings;
    uint64_t x = 88172645463325252ull;
    auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint32_t len = 0; len <= 40; len++)
        for (int k = 0; k < 3; k++) {
            std::string s(len, 'a');
            for (char& c : s) c = "abAB\x7f\x80\xff\0z"[rnd() % 9];
            strings.push_back(s);
        }
    const std::string stem(300, 'q');
    for (int k = 0; k < 40; k++) strings.push_back(stem.substr(0, 250 + rnd() % 50) + std::string(1, (char)('a' + k % 3)));
    for (int k = 0; k < 6; k++) strings.push_back(std::string("a") + std::string(k % 3, '\0'));
    for (int k = 0; k < 30; k++) strings.push_back(strings[rnd() % strings.size()]);
    const size_t n = strings.size(), cut = n / 3;
    int bad = 0;
    for (uint32_t variant = 0; variant < 32; variant++) {
        const uint32_t by = variant & 1u, flags = (variant >> 1) & (by ? 1u : 3u);
        const bool filter = (variant >> 3) & 1u;
        const uint64_t limit = (variant >> 4) & 1u ? 37 : 0;
        // two segments in memory of exactly their size
        sx_finding16* r0 = (sx_finding16*)malloc(cut * sizeof(sx_finding16));
        sx_finding* r1 = (sx_finding*)malloc((n - cut) * sizeof(sx_finding));
        size_t b0 = 0, b1 = 0;
        for (size_t i = 0; i < n; i++) (i < cut ? b0 : b1) += strings[i].size();
        uint8_t* a0 = (uint8_t*)malloc(b0 ? b0 : 1);
        uint8_t* a1 = (uint8_t*)malloc(b1 ? b1 : 1);
        std::vector<uint64_t> l0(cut), l1(n - cut), pos0(256, 0);
        pos0[3] = 4096;
        size_t at0 = 0, at1 = 0;
        for (size_t i = 0; i < n; i++) {
            const std::string& s = strings[i];
            const uint64_t label = (rnd() & 0xFFFFFFFF00000000ull) | (i % 5 ? 1u : 0u) | (uint64_t)(i % 7) << 8;
            if (i < cut) {
                memcpy(a0 + at0, s.data(), s.size());
                r0[i] = sx_finding16{ 8192 + 5 * i, (uint32_t)at0, (uint16_t)s.size(), (uint8_t)(i % 8), 3 };
                l0[i] = label; at0 += s.size();
            } else {
                memcpy(a1 + at1, s.data(), s.size());
                sx_finding f;
                memset(&f, 0, sizeof f);
                f.position = 100 + i; f.str_off = (uint32_t)at1; f.str_len = (uint32_t)s.size(); f.mission_id = 1; f.input_file_id = 2; f.slice_index = (uint32_t)i;
                r1[i - cut] = f; l1[i - cut] = label; at1 += s.size();
            }
        }
        const void* recs[2] = { r0, r1 };
        const uint8_t* arenas[2] = { a0, a1 };
        const uint64_t ns[2] = { cut, n - cut };
        const int32_t packed[2] = { 1, 0 }, file_ids[2] = { 5, -1 };
        const uint32_t slice_bases[2] = { 9, 0 };
        const uint64_t* p0[2] = { pos0.data(), nullptr };
        const uint64_t* labels[2] = { l0.data(), l1.data() };
        const uint32_t spec[4] = { by, flags, 8, 3 };
        const uint64_t masks[4] = { filter ? 1u : 0u, 0, 0, limit };
        std::vector<uint64_t> order(n + 1), left(4096);
        uint64_t info[5];
        sx_finding* out = (sx_finding*)malloc(n * sizeof(sx_finding));
        uint8_t* out_arena = (uint8_t*)malloc(b0 + b1 + 1);
        const int rc = sxs_order_host(2, recs, arenas, ns, packed, file_ids, slice_bases, p0, labels, spec, masks, 1 + variant % 3, info, left.data(), 4096, order.data(), out, out_arena);
        // the model
        std::vector<size_t> want;
        for (size_t i = 0; i < n; i++)
            if (!filter || ((i < cut ? l0[i] : l1[i - cut]) & 1u)) want.push_back(i);
        auto folded = [&](const std::string& s) { std::string t = s; if (flags & 2u) for (char& c : t) if (c >= 'A' && c <= 'Z') c = (char)(c | 0x20); return t; };
        auto field = [&](size_t i) { return ((i < cut ? l0[i] : l1[i - cut]) >> 8) & 7u; };
        auto less = [&](size_t a, size_t b) {
            if (by) return flags & 1u ? field(a) > field(b) : field(a) < field(b);
            const std::string s = folded(strings[a]), t = folded(strings[b]);
            const int c = memcmp(s.data(), t.data(), std::min(s.size(), t.size()));
            const bool lt = c < 0 || (c == 0 && s.size() < t.size()), gt = c > 0 || (c == 0 && s.size() > t.size());
            return flags & 1u ? gt : lt;
        };
        std::stable_sort(want.begin(), want.end(), less);
        const size_t kept = limit && limit < want.size() ? limit : want.size();
        int here = rc != 0 || info[0] != want.size() || info[1] != kept;
        for (size_t p = 0; !here && p < want.size(); p++) {
            const size_t i = want[p];
            here |= order[p] != (i < cut ? (uint64_t)i : (uint64_t)1 << 32 | (i - cut));
            if (p < kept) here |= out[p].str_len != strings[i].size() || memcmp(out_arena + out[p].str_off, strings[i].data(), strings[i].size()) != 0;
        }
        if (here) { fprintf(stderr, "variant %u: rc %d, %llu findings of %zu\n", variant, rc, (unsigned long long)info[0], want.size()); bad = 1; }
        free(r0); free(r1); free(a0); free(a1); free(out); free(out_arena);
    }
    puts(bad ? "order core: DIFFERENT" : "order core: ok");
    return bad;
}
#endif
