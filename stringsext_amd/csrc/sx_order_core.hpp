// sx_order_core.hpp — the findings of a result that lies in HBM, in sorted order (sx_result_order_device): what ONE lane does, written
// as lane functions.  Included by sx_order_dev.hip with SXD = `__device__ __forceinline__`; the test-only harness
// tests/native/order_core_host.cpp includes it with SXD = `inline`, so the very same code is checked against Python's sorted() on a
// machine without GPU (tests/test_order_core.py).
//
// The rule: the findings that the label pick lets through (all three masks 0: every finding) are ordered by their KEY — the string as
// unsigned bytes, memcmp and then the shorter one first, with `nocase` after 'A'..'Z' became 'a'..'z'; or a bit field of the label
// word as an unsigned number —; findings with equal keys keep print order, segment << 32 | record; `descending` reverses the order of
// the distinct keys and leaves the ties in print order.  It is sorted(range(n), key = ..., reverse = ...).
//
// The string key is an MSD refinement in words of eight bytes, exact whatever the data:
//   pick     a lane per record of a segment: the label pick or "all", the wavefront's ballot and count into the call's wavefront
//            tables, and three adds per wavefront and trip end: the count, the string bytes, the longest string.
//   number   (behind an exclusive scan over the wavefronts' counts) a picked record's rank in print order is its wavefront's base
//            plus the picked lanes below it: item `rank` gets its finding's key, slot `rank` the position `rank` and the group 0.
//   A ROUND d works on the list of u undecided items.  Slot j of the list stands for a fixed position of the final order (slotpos)
//   and belongs to a group (slotgrp: the slots of a group are neighbours, the ids ascend); which ITEM sits in a slot is what the
//   round decides, inside every group:
//   word     item j gets (w, rem): w = the bytes [8d, 8d + 8) of its (folded) string as one big-endian word, zero behind its end,
//            rem = min(len - 8d, 8), 0 behind the end.  A string that is a prefix of another or differs from it by trailing NUL
//            bytes only has the same w and a smaller rem.  descending: ~w and 8 - rem.  A lane reads [str_off + 8d, str_off + 8d +
//            rem) of its own string and no other byte: one 8-byte load where that address is 8-byte aligned and rem is 8, two 4-byte
//            loads where it is 4-byte aligned, bytes otherwise.
//   sort     stable, by (group, w, rem): three stable radix sorts, least significant key first (rem, w, group; round 0 has one group).
//   split    slot j looks at the item it got and at its neighbours': a run of equal (group, w, rem) is a new group.  A group of one
//            is decided; a group with rem < 8 is decided — its strings ended inside this word and are equal, and the stable sorts
//            left them in print order —; the others go on.  Every slot writes its item's key to its position — a later round
//            rewrites the positions of its groups and no others —, a decided one also whether a new key begins at its position
//            (classhead), and every slot a flag word: bit 0 undecided, bit 32 undecided and its group's first.
//   compact  (behind an exclusive 64-bit scan over the flag words, whose two halves count the undecided slots and their groups) an
//            undecided slot moves to the next round's list with its position, its item's key and its group's new id.
//   The host reads ONE word per round, the scan's total.  Rounds end when no slot is undecided: at most (longest string) / 8 + 1.
// The label key is one stable radix sort over `bits` bits of the field, complemented when descending; no rounds.
//   measure  a lane per position below `kept`: the string bytes and the ties — positions whose key equals a kept neighbour's.
//   gather   a lane per position below `kept`: the source record, expanded if it is packed, to its place, and where its string lies;
//            order_part_strings (sx_result_dev.hip) then lays the strings back to back.
// No lane waits for another: every dependency is a kernel boundary.  Nothing depends on the order of the adds.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sx_label_core.hpp"

namespace sx {

// a segment of the source where it lies (device pointers; in the harness: the test's)
struct OrderSeg {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed;
    int32_t file_id;         // packed: what sx_segment_info says of its records
    uint32_t slice_base, reserved;
    const uint64_t* pos0;    // packed: 256 words, by mission_id
    const uint64_t* labels;  // the segment's n label words (NULL: the call has none)
    uint64_t wave0;          // its first wavefront among the call's
};

enum OrderTotal : uint32_t { kOrderCount = 0, kOrderBytes = 1, kOrderLongest = 2, kOrderKeptBytes = 3, kOrderTied = 4, kOrderTotals = 8 };

// The call's tables where sx_order_dev.hip lays them out.  The pick's: per wavefront of the call, in segment order
struct OrderPickTables {
    OrderSeg* segs;
    uint64_t* pos0;          // 256 words per packed segment
    uint64_t* totals;        // kOrderTotals words
    uint64_t* wmask;
    uint32_t *wcount, *wbase;
    void* tmp;               // the scan's own
    size_t tmp_bytes;
};
// The sort's: two lists that take turns (item keys, slot positions, slot groups), a round's keys and values, the order
struct OrderSortTables {
    uint64_t* ikey[2];
    uint32_t *slotpos[2], *slotgrp[2];
    uint64_t* k64[2];
    uint32_t *k32[2], *perm[2];
    uint64_t* wkey;
    uint32_t *rkey, *iota;
    uint64_t *flags, *scan, *order;
    uint32_t* classhead;
    void* tmp;               // the sorts' and the scan's own
    size_t tmp_bytes;
};

// pick and number: one segment
struct OrderPick {
    OrderSeg seg;
    uint32_t seg_index;
    uint32_t filter;         // 0: every finding (seg.labels is not read)
    uint64_t any, all, none;
    uint64_t* wmask;         // per wavefront of the call: the picked lanes
    uint32_t* wcount;        // their number
    const uint32_t* wbase;   // number: the exclusive scan of wcount
    uint64_t* totals;        // kOrderCount, kOrderBytes, kOrderLongest
    uint64_t* ikey;          // number: per item its finding's key
    uint32_t* slotpos;       // per slot its position: the identity
    uint32_t* slotgrp;       // per slot its group: 0
    uint64_t* field;         // NULL, or per item its (complemented) field
    uint32_t shift, descending;
    uint64_t mask;           // of the field, at bit 0
};

SXD uint32_t order_len(const OrderSeg& S, uint64_t i) {
    return S.packed ? ((const sx_finding16*)S.recs)[i].str_len : ((const sx_finding*)S.recs)[i].str_len;
}

// pick, lane `lane` of the segment's wavefront `w`: is its record picked, and its string's length
SXD bool order_pick_lane(const OrderPick& P, uint64_t w, uint32_t lane, uint32_t* len) {
    const uint64_t i = w * kSelectRecs + lane;
    *len = 0;
    if (i >= P.seg.n) return false;
    if (P.filter && !label_picked(P.seg.labels[i], P.any, P.all, P.none)) return false;
    *len = order_len(P.seg, i);
    return true;
}

// number, lane `lane` of the segment's wavefront `w`
SXD void order_number_lane(const OrderPick& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane, mask = P.wmask[P.seg.wave0 + w];
    if (i >= P.seg.n || !((mask >> lane) & 1u)) return;
    const uint32_t rank = P.wbase[P.seg.wave0 + w] + (uint32_t)__builtin_popcountll(mask & (((uint64_t)1 << lane) - 1u));
    P.ikey[rank] = (uint64_t)P.seg_index << 32 | i;
    P.slotpos[rank] = rank;
    P.slotgrp[rank] = 0;
    if (P.field) {
        const uint64_t f = (P.seg.labels[i] >> P.shift) & P.mask;
        P.field[rank] = P.descending ? f ^ P.mask : f;
    }
}

// a round of the string key: the list of n undecided slots and their items
struct OrderRound {
    const OrderSeg* segs;
    uint64_t n;
    uint32_t nocase, descending, depth, reserved;
    const uint64_t* ikey;    // per item (an item's index is the slot it sat in when the round began)
    const uint32_t* slotpos; // per slot
    const uint32_t* slotgrp; // per slot
    uint64_t* wkey;          // word writes, per item
    uint32_t* rkey;
    uint32_t* iota;          // word writes j: the first sort's values
    const uint32_t* perm;    // split, compact: the item that the sorts put into slot j
    uint64_t* order;         // per position of the final order: a finding's key
    uint32_t* classhead;     // per position: a new key begins here
    uint64_t* flags;         // split writes n + 1 words
    const uint64_t* scan;    // compact: their exclusive scan
    uint64_t* ikey_next;     // compact writes the next round's list
    uint32_t* slotpos_next;
    uint32_t* slotgrp_next;
};

// 'A'..'Z' of the eight bytes of a word as 'a'..'z', no other byte
SXD uint64_t order_fold8(uint64_t w) {
    const uint64_t ones = 0x0101010101010101ull, low = w & (0x7F * ones);
    const uint64_t from_a = low + (0x80 - 'A') * ones, past_z = low + (0x80 - 'Z' - 1) * ones;      // bit 7: the low seven bits are >= 'A', > 'Z'
    return w | ((from_a & ~past_z & ~w & (0x80 * ones)) >> 2);
}

SXD uint64_t order_swap8(uint64_t v) { return __builtin_bswap64(v); }

// word, item j
SXD void order_word_lane(const OrderRound& P, uint64_t j) {
    if (j >= P.n) return;
    const uint64_t key = P.ikey[j];
    const OrderSeg& S = P.segs[key >> 32];
    uint64_t off; uint32_t len;
    select_string(S, key & 0xFFFFFFFFu, &off, &len);
    const uint64_t at = (uint64_t)P.depth * 8u;
    const uint32_t rem = len > at ? (len - at < 8u ? (uint32_t)(len - at) : 8u) : 0u;
    const uint8_t* p = S.arena + off + at;
    uint64_t w = 0;
    if (rem == 8u && !((uintptr_t)p & 7u)) w = order_swap8(*(const uint64_t*)p);
    else if (rem == 8u && !((uintptr_t)p & 3u)) w = order_swap8((uint64_t)((const uint32_t*)p)[0] | (uint64_t)((const uint32_t*)p)[1] << 32);
    else
        for (uint32_t k = 0; k < rem; k++) w |= (uint64_t)p[k] << (56u - 8u * k);
    if (P.nocase) w = order_fold8(w);
    P.wkey[j] = P.descending ? ~w : w;
    P.rkey[j] = P.descending ? 8u - rem : rem;
    P.iota[j] = (uint32_t)j;
}

// the keys of the second and third sort, slot j: the word and the group of the item that the sort before put there
SXD void order_wkey_lane(const uint64_t* wkey, const uint32_t* perm, uint64_t* out, uint64_t n, uint64_t j) { if (j < n) out[j] = wkey[perm[j]]; }
SXD void order_gkey_lane(const uint32_t* slotgrp, const uint32_t* perm, uint32_t* out, uint64_t n, uint64_t j) { if (j < n) out[j] = slotgrp[perm[j]]; }

SXD bool order_same(const OrderRound& P, uint64_t j, uint64_t k) {
    const uint32_t a = P.perm[j], b = P.perm[k];
    return P.slotgrp[j] == P.slotgrp[k] && P.wkey[a] == P.wkey[b] && P.rkey[a] == P.rkey[b];
}

// split, slot j
SXD void order_split_lane(const OrderRound& P, uint64_t j) {
    if (j >= P.n) return;
    if (j == 0) P.flags[P.n] = 0;      // (the scan's last word is the total)
    const uint32_t a = P.perm[j];
    const bool head = j == 0 || !order_same(P, j, j - 1), last = j + 1 == P.n || !order_same(P, j, j + 1);
    const bool more = P.rkey[a] == (P.descending ? 0u : 8u);      // the string goes on behind this word
    const bool undecided = more && !(head && last);
    const uint32_t pos = P.slotpos[j];
    P.order[pos] = P.ikey[a];
    if (!undecided) P.classhead[pos] = head ? 1u : 0u;
    P.flags[j] = undecided ? (uint64_t)1 | (head ? (uint64_t)1 << 32 : 0u) : 0u;
}

// compact, slot j
SXD void order_compact_lane(const OrderRound& P, uint64_t j) {
    if (j >= P.n) return;
    const uint64_t f = P.flags[j];
    if (!(f & 1u)) return;
    const uint64_t s = P.scan[j];
    const uint32_t to = (uint32_t)s;
    P.ikey_next[to] = P.ikey[P.perm[j]];
    P.slotpos_next[to] = P.slotpos[j];
    P.slotgrp_next[to] = (uint32_t)(s >> 32) + (uint32_t)(f >> 32) - 1u;      // the heads up to and including this slot, less one
}

// the label key behind its one sort: position p
struct OrderField {
    uint64_t n;
    const uint64_t* sorted;  // the fields in order
    const uint32_t* perm;    // the item at position p
    const uint64_t* ikey;
    uint64_t* order;
    uint32_t* classhead;
};
SXD void order_field_lane(const OrderField& P, uint64_t p) {
    if (p >= P.n) return;
    P.order[p] = P.ikey[P.perm[p]];
    P.classhead[p] = p == 0 || P.sorted[p] != P.sorted[p - 1] ? 1u : 0u;
}

// the output: the first `kept` positions of the order
struct OrderOut {
    const OrderSeg* segs;
    const uint64_t* order;
    const uint32_t* classhead;
    uint64_t kept;
    uint64_t* totals;        // measure adds kOrderKeptBytes and kOrderTied
    sx_finding* out;         // gather: kept records
    uint64_t* out_src;       // and the addresses of their strings
};

// measure, position p: its string's length, and whether a kept neighbour has its key
SXD void order_measure_lane(const OrderOut& P, uint64_t p, uint32_t* len, bool* tied) {
    *len = 0; *tied = false;
    if (p >= P.kept) return;
    const uint64_t key = P.order[p];
    *len = order_len(P.segs[key >> 32], key & 0xFFFFFFFFu);
    *tied = !(P.classhead[p] && (p + 1 >= P.kept || P.classhead[p + 1]));
}

// gather, position p
SXD void order_gather_lane(const OrderOut& P, uint64_t p) {
    if (p >= P.kept) return;
    const uint64_t key = P.order[p], i = key & 0xFFFFFFFFu;
    const OrderSeg& S = P.segs[key >> 32];
    sx_finding f;
    if (S.packed) {      // (expand_finding of sx_host.hpp)
        const sx_finding16 q = ((const sx_finding16*)S.recs)[i];
        f.position = q.position; f.str_off = q.str_off; f.str_len = q.str_len;
        f.precision = (uint8_t)(q.flags & 3u); f.completes_previous = (uint8_t)((q.flags >> 2) & 1u);
        f.mission_id = q.mission_id; f.reserved = 0; f.input_file_id = (int16_t)S.file_id; f.reserved2 = 0;
        f.slice_index = S.slice_base + (uint32_t)((q.position - S.pos0[q.mission_id]) / 4096u);
    } else
        f = ((const sx_finding*)S.recs)[i];
    P.out_src[p] = (uint64_t)(uintptr_t)(S.arena + f.str_off);
    f.str_off = 0;           // (order_part_strings writes it)
    P.out[p] = f;
}

}  // namespace sx
