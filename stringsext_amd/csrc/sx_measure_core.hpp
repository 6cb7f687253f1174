// sx_measure_core.hpp — what a string LOOKS like (sx_result_measure_device, sx_measure_bytes): per finding one 64-bit word with the
// entropy of its bytes, how many different bytes it has, which classes of bytes, and how many characters — the rule of
// include/stringsext_amd.h, in integers.  What ONE lane does, written as lane functions.  Included by sx_measure_dev.hip with SXD =
// `__device__ __forceinline__`; sx_result_api.cpp (sx_measure_bytes) and the test-only harness tests/native/measure_core_host.cpp
// include it with SXD = `inline`, so the very same code is checked against a Python restatement on a machine without GPU
// (tests/test_measure_core.py).
//
// The histogram is the work, and it has two shapes:
//   narrow  str_len <= kMeasureNarrowMax (255): a LANE has the string and 256 one-byte counters of its own — no count can overflow.
//           It walks the string once and increments; it walks it again and, for every byte whose counter is not zero, takes
//           c x LG(c) from the table, counts a distinct value and ZEROES the counter: clearing costs string bytes, not 256 bytes per
//           record, and the counters are all zero again behind every string.  The counter of byte b lies at
//           cnt[(b >> 2) * row + (b & 3)]: the harness gives every "lane" a block of 256 bytes (row = 4); the kernel interleaves the
//           64 lanes' counters dword by dword (row = 256, cnt = the wavefront's block + 4 x lane), see sx_measure_dev.hip.
//   wide    str_len > 255: a WAVEFRONT has the string and 256 32-bit counters.  Lane l takes the 8-byte words l, l + 64, ... of the
//           string and adds to the counters (LDS atomics; the harness runs the lanes one after the other); then lane l finishes the
//           counters 4l .. 4l + 3 — c x LG(c), distinct, zero — and the wavefront sums.
// Both walk the string as its 8-byte ALIGNED words: a whole word is one load, the words at the string's two ends are read in the
// aligned pieces that lie inside the string, so that no byte is read that is not the string's.  Chars and the class bits come from
// the words as they pass, by SWAR.
#pragma once
#include <stdint.h>

#include "sx_select_core.hpp"

namespace sx {

constexpr uint32_t kMeasureNarrowMax = 255;       // the longest string a lane measures: its counts fit a byte
constexpr uint32_t kMeasureClassShift = 25;       // SX_MEASURE_LOWER: class k of the SWAR walk is bit 25 + k of the word
enum MeasureTotal { kMeasureFindings = 0, kMeasureBytes = 1, kMeasureChars = 2, kMeasureWide = 3, kMeasureAscii = 4, kMeasureTotals = 5 };

// LG(x), 1 <= x < 2^32: log2(x) in units of 2^-16, by sixteen squarings of the mantissa (constexpr: the table below is made by it)
constexpr inline uint32_t measure_lg(uint32_t x) {
    const uint32_t e = 31u - (uint32_t)__builtin_clz(x);
    uint64_t m = (uint64_t)x << (31u - e);
    uint32_t f = 0;
    for (int k = 0; k < 16; k++) {
        m = (m * m) >> 31;
        f <<= 1;
        if (m >> 32) { f |= 1u; m >>= 1; }
    }
    return e << 16 | f;
}

// c x LG(c) for c < 256: every count of a narrow string, and most of a wide one (255 x LG(255) < 2^28)
struct MeasureClg { uint32_t v[256]; };
constexpr inline MeasureClg measure_clg_table() {
    MeasureClg t{};
    for (uint32_t c = 1; c < 256; c++) t.v[c] = c * measure_lg(c);
    return t;
}
SXD uint64_t measure_clg(const uint32_t* clg, uint32_t c) { return c < 256u ? clg[c] : (uint64_t)c * measure_lg(c); }

// What the words of a string leave as they pass: classes — bit k of ANY of its eight bytes: a byte of class k was there (k = 0 lower
// ... 6 high, the order of the word's class bits) —, and the bytes outside 0x80..0xBF
struct MeasureAcc {
    uint64_t classes;
    uint32_t chars;
};

// The word w, of which the low nb bytes (1..8) are the string's
SXD void measure_word(uint64_t w, uint32_t nb, MeasureAcc* a) {
    const uint64_t ones = 0x0101010101010101ull, H = 0x80 * ones, low = w & (0x7F * ones);
    const uint64_t V = nb >= 8u ? H : H & (((uint64_t)1 << (8u * nb)) - 1u);                    // bit 7 of the valid bytes
#define SX_MEASURE_GE(k) ((low + (uint64_t)(0x80 - (k)) * ones) & H)                              /* bit 7: the low seven bits are >= k */
    const uint64_t high = w & H, asc = ~w & V;
    const uint64_t lower = SX_MEASURE_GE('a') & ~SX_MEASURE_GE('z' + 1) & asc, upper = SX_MEASURE_GE('A') & ~SX_MEASURE_GE('Z' + 1) & asc,
                   digit = SX_MEASURE_GE('0') & ~SX_MEASURE_GE('9' + 1) & asc;
    const uint64_t ge20 = SX_MEASURE_GE(0x20), ge21 = SX_MEASURE_GE(0x21), del = SX_MEASURE_GE(0x7F), tab = SX_MEASURE_GE(0x09) & ~SX_MEASURE_GE(0x0A);
#undef SX_MEASURE_GE
    const uint64_t space = ((ge20 & ~ge21) | tab) & asc, control = ((~ge20 & ~tab) | del) & asc;
    const uint64_t punct = ge21 & ~del & asc & ~(lower | upper | digit);
    const uint64_t cont = high & (~w << 1);                                                        // 10xxxxxx
    a->classes |= lower >> 7 | upper >> 6 | digit >> 5 | space >> 4 | punct >> 3 | control >> 2 | (high & V) >> 1;
    a->chars += (uint32_t)__builtin_popcountll(V & ~cont);
}

// The string s[0, len) as 8-byte aligned words: how many, and word j — its bytes in the low *nb bytes, in memory order.  A word that
// lies in the string is ONE load; of the first and the last, where the string covers them in part, only its bytes are read.
SXD uint32_t measure_words(const uint8_t* s, uint32_t len) { return len ? (uint32_t)(((uint64_t)((uintptr_t)s & 7u) + len + 7u) >> 3) : 0u; }
SXD uint64_t measure_load(const uint8_t* s, uint32_t len, uint32_t j, uint32_t* nb) {
    const uint64_t head = (uintptr_t)s & 7u;
    const uint64_t b0 = j ? 8u * (uint64_t)j - head : 0u, b1 = 8u * (uint64_t)j + 8u - head < len ? 8u * (uint64_t)j + 8u - head : len;
    *nb = (uint32_t)(b1 - b0);
    if (b1 - b0 == 8u) return *(const uint64_t*)(s + b0);
    // n bytes from the place a of an aligned word, a + n <= 8, in ALIGNED pieces and no loop, so that the loads are in flight
    // together: a byte and a halfword going up to a multiple of 4, then a word, a halfword and a byte going down
    const uint8_t* p = s + b0;
    const uint32_t a = (uint32_t)((uintptr_t)p & 7u), n = (uint32_t)(b1 - b0);
    uint32_t at = 0, at1 = 0, at2 = 0, at3 = 0, at4 = 0;
    uint64_t v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0;
    if (a & 1u) { v0 = p[0]; at = 1; }                                                      // (n >= 1)
    if (((a + at) & 2u) && at + 2u <= n) { v1 = *(const uint16_t*)(p + at); at1 = at; at += 2; }
    if (at + 4u <= n) { v2 = *(const uint32_t*)(p + at); at2 = at; at += 4; }
    if (at + 2u <= n) { v3 = *(const uint16_t*)(p + at); at3 = at; at += 2; }
    if (at + 1u <= n) { v4 = p[at]; at4 = at; }
    return v0 | v1 << (8u * at1) | v2 << (8u * at2) | v3 << (8u * at3) | v4 << (8u * at4);
}

SXD uint32_t measure_slot(uint32_t b, uint32_t row) { return (b >> 2) * row + (b & 3u); }

// The word of a string of n bytes: sum = the c x LG(c) of its counts, distinct = how many counts are not zero
SXD uint64_t measure_finish(const uint32_t* clg, uint32_t n, uint64_t sum, uint32_t distinct, const MeasureAcc& a) {
    if (n == 0) return 0;
    const uint64_t T = measure_clg(clg, n) - sum, q = T / (16u * (uint64_t)n), ent = q < 65535u ? q : 65535u;
    uint64_t c = a.classes;
    c |= c >> 32; c |= c >> 16; c |= c >> 8;
    return ent << SX_MEASURE_ENTROPY_SHIFT | (uint64_t)distinct << SX_MEASURE_DISTINCT_SHIFT | (c & 0x7Fu) << kMeasureClassShift | (uint64_t)a.chars << SX_MEASURE_CHARS_SHIFT;
}

// narrow: the word of s[0, len), len <= kMeasureNarrowMax, with the lane's counters (all zero before, all zero behind)
SXD uint64_t measure_narrow_string(const uint8_t* s, uint32_t len, uint8_t* cnt, uint32_t row, const uint32_t* clg) {
    MeasureAcc a{ 0, 0 };
    const uint32_t words = measure_words(s, len);
    for (uint32_t j = 0; j < words; j++) {
        uint32_t nb;
        uint64_t w = measure_load(s, len, j, &nb);
        measure_word(w, nb, &a);
        for (uint32_t k = 0; k < nb; k++, w >>= 8) cnt[measure_slot((uint32_t)w & 0xFFu, row)]++;
    }
    uint64_t sum = 0;
    uint32_t distinct = 0;
    for (uint32_t j = 0; j < words; j++) {
        uint32_t nb;
        uint64_t w = measure_load(s, len, j, &nb);
        for (uint32_t k = 0; k < nb; k++, w >>= 8) {
            const uint32_t at = measure_slot((uint32_t)w & 0xFFu, row), c = cnt[at];
            if (!c) continue;
            sum += clg[c];
            distinct++;
            cnt[at] = 0;
        }
    }
    return measure_finish(clg, len, sum, distinct, a);
}

// (the harness runs the lanes one after the other)
SXD void measure_add32(uint32_t* word) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(word, 1u);
#else
    ++*word;
#endif
}

// wide, lane `lane` of the wavefront that has s[0, len): its words into the wavefront's 256 counters and into the lane's *a
SXD void measure_wide_count_lane(const uint8_t* s, uint32_t len, uint32_t lane, uint32_t* cnt32, MeasureAcc* a) {
    const uint32_t words = measure_words(s, len);
    for (uint32_t j = lane; j < words; j += kSelectRecs) {
        uint32_t nb;
        uint64_t w = measure_load(s, len, j, &nb);
        measure_word(w, nb, a);
        for (uint32_t k = 0; k < nb; k++, w >>= 8) measure_add32(&cnt32[(uint32_t)w & 0xFFu]);
    }
}
// wide, behind every lane's count: the counters 4 x lane .. 4 x lane + 3 into the lane's *sum and *distinct, and zeroed
SXD void measure_wide_finish_lane(uint32_t* cnt32, uint32_t lane, const uint32_t* clg, uint64_t* sum, uint32_t* distinct) {
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t c = cnt32[4u * lane + k];
        if (!c) continue;
        *sum += measure_clg(clg, c);
        ++*distinct;
        cnt32[4u * lane + k] = 0;
    }
}

// One segment as the kernels take it
struct MeasureParams {
    const void* recs;        // n records: sx_finding16 if `packed`, else sx_finding
    const uint8_t* arena;
    uint64_t n;              // < 2^32
    uint32_t packed;
    uint64_t* labels;        // n words, in record order
    uint32_t* list;          // the records of the wide strings, in any order: room for n
    uint64_t* cursor;        // how many the list holds
    uint64_t* totals;        // kMeasureTotals words of the call
};

// narrow, lane `lane` of wavefront `w`: the record's word, if its string is narrow.  true: it is wide, and the caller lists the
// record.  *len: the string's bytes (0 behind the last record); *chars, *ascii: of a narrow string
SXD bool measure_narrow_lane(const MeasureParams& P, uint64_t w, uint32_t lane, uint8_t* cnt, uint32_t row, const uint32_t* clg, uint32_t* len, uint32_t* chars, bool* ascii) {
    const uint64_t i = w * kSelectRecs + lane;
    *len = *chars = 0; *ascii = false;
    if (i >= P.n) return false;
    uint64_t off;
    select_string(P, i, &off, len);
    if (*len > kMeasureNarrowMax) return true;
    const uint64_t word = measure_narrow_string(P.arena + off, *len, cnt, row, clg);
    P.labels[i] = word;
    *chars = (uint32_t)(word >> SX_MEASURE_CHARS_SHIFT);
    *ascii = !(word & SX_MEASURE_HIGH);
    return false;
}

// One string of any length below 2^32 on the host, by the lane functions: a lane's 256 byte counters, or a wavefront's 256 words
// and its 64 lanes one after the other (no kernel calls it)
SXD uint64_t measure_string_host(const uint8_t* s, uint32_t len, const uint32_t* clg) {
    if (len <= kMeasureNarrowMax) {
        uint8_t cnt[256] = { 0 };
        return measure_narrow_string(s, len, cnt, 4, clg);
    }
    uint32_t cnt32[256] = { 0 }, distinct = 0;
    MeasureAcc a{ 0, 0 };
    uint64_t sum = 0;
    for (uint32_t lane = 0; lane < kSelectRecs; lane++) measure_wide_count_lane(s, len, lane, cnt32, &a);
    for (uint32_t lane = 0; lane < kSelectRecs; lane++) measure_wide_finish_lane(cnt32, lane, clg, &sum, &distinct);
    return measure_finish(clg, len, sum, distinct, a);
}

}  // namespace sx
