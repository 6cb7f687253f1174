// sx_fuzzy_core.hpp — which keywords occur in a finding's string with at most k errors (sx_result_fuzzy_device, sx_fuzzy_bytes): what
// ONE lane does for its record, written as lane functions.  Included by sx_fuzzy_dev.hip with SXD = `__device__ __forceinline__`;
// sx_result_api.cpp (sx_fuzzy_bytes) and the test-only harness tests/native/fuzzy_core_host.cpp include it with SXD = `inline`, so the
// very same code is checked against Sellers' table restated in Python on a machine without GPU (tests/test_fuzzy_core.py).
//
// The rule (include/stringsext_amd.h): bit p of finding i's word is set iff some substring of its string has Levenshtein distance at
// most k_p from pattern p, in bytes; a match never spans two findings; the bits of patterns the set does not have are 0.
//
// One lane, one record.  Per pattern the lane carries a column of Sellers' table as Myers' two bit vectors — Pv: the column goes up
// by one at this row, Mv: it goes down — and the score of the column's last row, len in front of the first byte (the column 0, 1,
// ..., len: Pv all ones).  A byte of the string gives Eq, the pattern positions that hold it — eq[class][p] of sx_fuzzy_build.hpp; a
// byte of class 0 is held by none: Eq = 0 without a look —, and one step of the recurrence, which does not depend on k and has no
// branch, gives the next column.  It is the SEARCH form: nothing is ORed into Ph's bit 0, row 0 stays 0, a match may begin anywhere.
// The add wraps at bit 63 of a 64-byte pattern, by design: carries leave at the top.  Bit p is set as soon as the score is <= k_p.
// Sets whose longest pattern has at most 32 bytes take the recurrence in 32-bit words (W = uint32_t), half the vector work.
//
// Registers are the layout: a pattern costs two vectors and a score, so a lane takes the set's patterns in GROUPS (kFuzzyGroup32/64) and
// walks its string once per group; a group is left when all its bits are set or the string ends, and is not walked at all where
// str_len < len_p - k_p for every pattern of it (such a string cannot match: exact, no heuristic).  A set of at most a group's
// patterns walks once.  The last group's empty places repeat the set's last pattern and own no bit.  len_p, k_p and the bits are the
// same in every lane: the compiler keeps them in scalar registers.
//
// The string is read as sx_measure_core.hpp reads it — its 8-byte ALIGNED words, the two ends in the aligned pieces that lie inside the
// string, no byte that is not the string's —, not byte by byte: a one-pattern set is bound by the latency of the chain load -> class
// -> masks -> recurrence, and a load per eight bytes takes the longest link out of seven steps in eight.
//
// Counting is the label kernel's: label_count_bit and label_flush_lane of sx_label_core.hpp.
#pragma once
#include <stdint.h>

#include "sx_label_core.hpp"
#include "sx_measure_core.hpp"

namespace sx {

// patterns a lane carries at once, each two vectors and a score: 8 in 32-bit words (40 registers of state), 4 in 64-bit words (20) —
// 8 of those compile to 95 vector registers, which leaves a CU room for two workgroups where the grid counts on three
constexpr uint32_t kFuzzyGroup32 = 8;
constexpr uint32_t kFuzzyGroup64 = 4;
template <class W> constexpr uint32_t fuzzy_group() { return sizeof(W) == 4 ? kFuzzyGroup32 : kFuzzyGroup64; }

// a compiled fuzzy set where the kernel reads it (device pointers; on the host: the builder's)
struct FuzzyDevice {
    const uint16_t* map;      // 256 entries: byte -> class
    const uint64_t* eq;       // classes * n_patterns words
    const uint32_t* lenk;     // n_patterns words: len | k << 8
    uint64_t* findings;       // kLabelBits counters
    uint64_t* first;          // kLabelBits minima
    uint32_t n_patterns, classes, lds_classes, max_len;
};

struct FuzzyParams {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed, reserved;
    uint64_t ordinal;        // of the segment's record 0: ordinal_base + the findings of the segments in front of it
    uint64_t* labels;        // n words, in record order
    FuzzyDevice set;
};

// One pattern's next column: Eq = the pattern positions that hold the string's byte, top = len - 1
template <class W>
SXD void fuzzy_step(W Eq, uint32_t top, W& Pv, W& Mv, uint32_t& score) {
    const W Xv = Eq | Mv, Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    W Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
    score += (uint32_t)(Ph >> top) & 1u;
    score -= (uint32_t)(Mh >> top) & 1u;      // (never both)
    Ph <<= 1; Mh <<= 1;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}

// The bits of the patterns [p0, p0 + G) of the set in s[0, len).  map: the 256 classes, rows: the masks of the first lds_classes
// classes (LDS; on the host: the table)
template <class W, uint32_t G>
SXD uint64_t fuzzy_walk_group(const FuzzyDevice& S, const uint16_t* map, const uint64_t* rows, const uint8_t* s, uint32_t len, uint32_t p0) {
    const uint32_t np = S.n_patterns;
    uint32_t at[G], top[G], k[G], score[G], need = ~0u;
    uint64_t bit[G], want = 0;
    W Pv[G], Mv[G];
#pragma unroll
    for (uint32_t j = 0; j < G; j++) {
        at[j] = p0 + j < np ? p0 + j : np - 1u;
        const uint32_t lk = S.lenk[at[j]], plen = lk & 0xFFu;
        top[j] = plen - 1u; k[j] = lk >> 8; score[j] = plen;
        bit[j] = p0 + j < np ? (uint64_t)1 << (p0 + j) : 0u;
        want |= bit[j];
        if (plen - k[j] < need) need = plen - k[j];
        Pv[j] = ~(W)0; Mv[j] = 0;
    }
    if (len < need) return 0;
    uint64_t acc = 0;
    const uint32_t words = measure_words(s, len);
    for (uint32_t w = 0; w < words && acc != want; w++) {
        uint32_t nb;
        uint64_t v = measure_load(s, len, w, &nb);
        for (uint32_t b = 0; b < nb; b++, v >>= 8) {
            const uint32_t c = map[(uint32_t)v & 0xFFu];
            W Eq[G];
#pragma unroll
            for (uint32_t j = 0; j < G; j++) Eq[j] = 0;
            if (c != 0) {
                if (c < S.lds_classes) {
#pragma unroll
                    for (uint32_t j = 0; j < G; j++) Eq[j] = (W)rows[c * np + at[j]];
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < G; j++) Eq[j] = (W)S.eq[c * np + at[j]];
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < G; j++) {
                fuzzy_step<W>(Eq[j], top[j], Pv[j], Mv[j], score[j]);
                if (score[j] <= k[j]) acc |= bit[j];
            }
        }
    }
    return acc;
}

// The word of s[0, len): group by group
template <class W>
SXD uint64_t fuzzy_string(const FuzzyDevice& S, const uint16_t* map, const uint64_t* rows, const uint8_t* s, uint32_t len) {
    uint64_t acc = 0;
    for (uint32_t p0 = 0; p0 < S.n_patterns; p0 += fuzzy_group<W>()) acc |= fuzzy_walk_group<W, fuzzy_group<W>()>(S, map, rows, s, len, p0);
    return acc;
}

// Lane `lane` of wavefront `w`: its record's word (lanes behind the last record have none, and the word 0)
template <class W>
SXD uint64_t fuzzy_lane(const FuzzyParams& P, const uint16_t* map, const uint64_t* rows, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    if (i >= P.n) return 0;
    uint64_t off; uint32_t len;
    select_string(P, i, &off, &len);
    const uint64_t acc = fuzzy_string<W>(P.set, map, rows, P.arena + off, len);
    P.labels[i] = acc;
    return acc;
}

// On the host: the word of s[0, len) by a set's tables as the builder left them — the kernel's choice of W
SXD uint64_t fuzzy_string_host(const FuzzyDevice& S, const uint8_t* s, uint32_t len) {
    return S.max_len <= 32u ? fuzzy_string<uint32_t>(S, S.map, S.eq, s, len) : fuzzy_string<uint64_t>(S, S.map, S.eq, s, len);
}

}  // namespace sx
