// sx_fold_core.hpp — the strings of a result that lies in HBM, folded by Unicode SIMPLE case folding (sx_result_fold_device), and the
// same fold of one byte string on the host (sx_fold_utf8): what ONE lane does for its own string, written as lane functions.
// Included by sx_fold_dev.hip with SXD = `__device__ __forceinline__`, by sx_result_api.cpp and by the test-only program
// tests/native/fold_core_host.cpp with SXD = `inline`, so the very same code is checked against Python's str.casefold() / str.lower()
// on a machine without GPU (tests/test_fold_core.py).
//
// The rule, SX_FOLD_SIMPLE: the string is walked from the left.  At a well-formed UTF-8 sequence (Unicode Table 3-7: no overlong form,
// no surrogate, nothing above U+10FFFF, the whole sequence inside the string) of the code point c, fold(c) is written as UTF-8; any
// other byte is copied as it is, and the walk goes on at the NEXT byte.  fold() is CaseFolding.txt's statuses C and S as
// gen_fold_table.py derives them; a code point that has only a full folding (ß, İ) stays.  It is
// b.decode('utf-8', 'surrogateescape'), fold per character, .encode('utf-8', 'surrogateescape').
// Most foldings keep their UTF-8 length; 32 get shorter (U+212A KELVIN SIGN: 3 bytes -> 'k') and 2 get LONGER (U+023A, U+023E: 2 -> 3
// bytes), so a folded string has between a third and one and a half times its source's bytes: the length has to be measured before
// anything can be placed.
//
// The table (sx_fold_table.inc) has two stages: kFoldIndex by c >> 7, a page number or kFoldNoPage, then a page of 128 entries, each
// the low 16 bits of fold(c) — no folding leaves its plane.  ASCII does not look into it.
//
// The walk's fast path is order_word_lane's loading rule (sx_order_core.hpp): where the next byte's address is 8-byte aligned and
// eight more bytes are the string's, one 8-byte load; a word without a byte >= 0x80 is folded by order_fold8 and keeps its length.
// Anything else goes byte by byte through the decoder, one character at a time.  A lane reads [s, s + len) and no other byte, and
// the placing walk writes [out, out + measured length) and no other byte: both walks take every decision from the same bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sx_order_core.hpp"

namespace sx {

static_assert(sizeof(sx_finding) == 32 && sizeof(sx_finding16) == 16, "fold_place_lane copies the records as 64-bit words");

#include "sx_fold_table.inc"

// the table where the lane reads it: the kernels' copy in LDS, the host's arrays
struct FoldTable {
    const uint8_t* index;    // kFoldIndexCount page numbers
    const uint16_t* pages;   // kFoldPageCount pages of 128 entries
};

SXD uint32_t fold_code_point(const FoldTable& T, uint32_t c) {
    if (c < 0x80u) return c - 'A' < 26u ? c | 0x20u : c;
    if (c >= kFoldLimit) return c;
    const uint32_t page = T.index[c >> kFoldPageShift];
    if (page == kFoldNoPage) return c;
    return (c & ~0xFFFFu) | T.pages[(page << kFoldPageShift) | (c & ((1u << kFoldPageShift) - 1u))];
}

// The well-formed sequence that begins at p[0], of which `left` >= 1 bytes are the string's: its length, 1..4, and its code point;
// 0: p[0] begins none
SXD uint32_t fold_decode(const uint8_t* p, uint64_t left, uint32_t* c) {
    const uint32_t b0 = p[0];
    if (b0 < 0x80u) { *c = b0; return 1u; }
    if (b0 < 0xC2u || b0 > 0xF4u) return 0u;      // a continuation byte, the overlong C0 and C1, F5..FF
    const uint32_t n = b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : 4u;
    if (left < n) return 0u;
    // the second byte's range: E0 no overlong form, ED no surrogate, F0 no overlong form, F4 nothing above U+10FFFF
    const uint32_t lo = b0 == 0xE0u ? 0xA0u : b0 == 0xF0u ? 0x90u : 0x80u, hi = b0 == 0xEDu ? 0x9Fu : b0 == 0xF4u ? 0x8Fu : 0xBFu;
    const uint32_t b1 = p[1];
    if (b1 < lo || b1 > hi) return 0u;
    if (n == 2u) { *c = (b0 & 0x1Fu) << 6 | (b1 & 0x3Fu); return 2u; }
    const uint32_t b2 = p[2];
    if ((b2 & 0xC0u) != 0x80u) return 0u;
    if (n == 3u) { *c = (b0 & 0x0Fu) << 12 | (b1 & 0x3Fu) << 6 | (b2 & 0x3Fu); return 3u; }
    const uint32_t b3 = p[3];
    if ((b3 & 0xC0u) != 0x80u) return 0u;
    *c = (b0 & 0x07u) << 18 | (b1 & 0x3Fu) << 12 | (b2 & 0x3Fu) << 6 | (b3 & 0x3Fu);
    return 4u;
}

// where a walk's bytes go: nowhere, counted ...
struct FoldCount {
    uint64_t n = 0;
    SXD void byte(uint32_t) { n++; }
    SXD void word(uint64_t) { n += 8u; }
};
// ... or to out[n].  A word (eight bytes, the first in the low byte) goes out as it came in: one 8-byte store where the place is
// 8-byte aligned, two 4-byte stores where it is 4-byte aligned, bytes otherwise
struct FoldWrite {
    uint8_t* out;
    uint64_t n = 0;
    SXD void byte(uint32_t b) { out[n++] = (uint8_t)b; }
    SXD void word(uint64_t w) {
        uint8_t* p = out + n;
        if (!((uintptr_t)p & 7u)) *(uint64_t*)p = w;
        else if (!((uintptr_t)p & 3u)) { ((uint32_t*)p)[0] = (uint32_t)w; ((uint32_t*)p)[1] = (uint32_t)(w >> 32); }
        else
            for (uint32_t k = 0; k < 8u; k++) p[k] = (uint8_t)(w >> (8u * k));
        n += 8u;
    }
};

// THE walk over s[0, len).  Returns whether any byte of the output differs from the input (a changed length is a changed byte)
template <class Sink>
SXD bool fold_walk(const FoldTable& T, const uint8_t* s, uint64_t len, Sink& out) {
    bool changed = false;
    uint64_t k = 0;
    while (k < len) {
        if (!((uintptr_t)(s + k) & 7u) && len - k >= 8u) {
            const uint64_t w = *(const uint64_t*)(s + k);
            if (!(w & 0x8080808080808080ull)) {
                const uint64_t f = order_fold8(w);
                changed |= f != w;
                out.word(f);
                k += 8u;
                continue;
            }
        }
        uint32_t c = 0;
        const uint32_t n = fold_decode(s + k, len - k, &c);
        if (!n) { out.byte(s[k]); k++; continue; }
        const uint32_t f = fold_code_point(T, c);
        changed |= f != c;
        // (the decoder takes the shortest form only: f == c writes the bytes that were read)
        if (f < 0x80u) out.byte(f);
        else if (f < 0x800u) { out.byte(0xC0u | f >> 6); out.byte(0x80u | (f & 0x3Fu)); }
        else if (f < 0x10000u) { out.byte(0xE0u | f >> 12); out.byte(0x80u | (f >> 6 & 0x3Fu)); out.byte(0x80u | (f & 0x3Fu)); }
        else { out.byte(0xF0u | f >> 18); out.byte(0x80u | (f >> 12 & 0x3Fu)); out.byte(0x80u | (f >> 6 & 0x3Fu)); out.byte(0x80u | (f & 0x3Fu)); }
        k += n;
    }
    return changed;
}

// The two walks of a string.  measure: the folded length, and whether the fold changes the string
SXD uint64_t fold_measure_string(const FoldTable& T, const uint8_t* s, uint64_t len, bool* changed) {
    FoldCount count;
    *changed = fold_walk(T, s, len, count);
    return count.n;
}
// place: the folded bytes to out[0, the measured length); returns that length
SXD uint64_t fold_place_string(const FoldTable& T, const uint8_t* s, uint64_t len, uint8_t* out) {
    FoldWrite write{ out };
    (void)fold_walk(T, s, len, write);
    return write.n;
}

// A segment's two passes (sx_fold_dev.hip).  The totals are per segment
enum FoldTotal : uint32_t { kFoldRecords = 0, kFoldChanged = 1, kFoldLongest = 2, kFoldBytesIn = 3, kFoldTotals = 4 };
struct FoldParams {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed;
    // measure writes
    uint32_t* rlen;          // per record: its folded length (0xFFFFFFFF: that or more — the driver refuses such a segment by its bytes)
    uint64_t* wbytes;        // per wavefront (waves + 1 entries: the one behind the last record has no byte): its records' folded bytes
    uint64_t* totals;        // kFoldTotals words: the records, those whose string changes, the longest folded string, the source's string bytes
    // place reads rlen and
    const uint64_t* wbase;   // the exclusive scan of wbytes
    void* out_recs;          // n records of the source's type
    uint8_t* out_arena;      // the folded strings, back to back in record order
};

// What the driver asks between the passes, of a segment's measured totals: do the folded strings fit the records that place writes —
// str_off has 32 bits, a packed record's str_len 16 (fold_place_lane masks to them: it runs only where this said yes).  The library
// itself packs only where every Mission's -q is at most 16 000 characters, and a folded character has at most four bytes, so the packed
// bound guards sources that the library does not make today.
enum FoldFit : uint32_t { kFoldFits = 0, kFoldTooManyBytes = 1, kFoldPackedTooLong = 2 };
SXD FoldFit fold_segment_fits(uint32_t packed, uint64_t folded_bytes, uint64_t longest) {
    if (folded_bytes >> 32) return kFoldTooManyBytes;
    if (packed && longest > 0xFFFFu) return kFoldPackedTooLong;
    return kFoldFits;
}

// measure, lane `lane` of wavefront `w`: its record's folded length (0 behind the last record), its source length, whether it changes
SXD uint64_t fold_measure_lane(const FoldParams& P, const FoldTable& T, uint64_t w, uint32_t lane, uint32_t* len, bool* changed) {
    const uint64_t i = w * kSelectRecs + lane;
    *len = 0; *changed = false;
    if (i >= P.n) return 0;
    uint64_t off;
    select_string(P, i, &off, len);
    const uint64_t folded = fold_measure_string(T, P.arena + off, *len, changed);
    P.rlen[i] = folded < 0xFFFFFFFFull ? (uint32_t)folded : 0xFFFFFFFFu;
    return folded;
}

// place, lane `lane` of wavefront `w`, whose record's string begins at out_arena[at] and has `folded` bytes: the source record with
// the new str_off and str_len and nothing else changed, and the folded bytes
SXD void fold_place_lane(const FoldParams& P, const FoldTable& T, uint64_t w, uint32_t lane, uint64_t at, uint32_t folded) {
    const uint64_t i = w * kSelectRecs + lane;
    if (i >= P.n) return;
    // (the record goes as the 64-bit words it is made of, its padding with it; little-endian: str_off is the low half of word 1,
    // str_len the 32 bits above it — in a packed record the 16 bits above it, under flags and mission_id)
    uint32_t off, len;
    if (P.packed) {
        uint64_t q[2];
        memcpy(q, (const sx_finding16*)P.recs + i, sizeof q);
        off = (uint32_t)q[1]; len = (uint32_t)(q[1] >> 32) & 0xFFFFu;
        q[1] = (q[1] & 0xFFFF000000000000ull) | (uint64_t)(folded & 0xFFFFu) << 32 | (uint32_t)at;
        memcpy((sx_finding16*)P.out_recs + i, q, sizeof q);
    } else {
        uint64_t q[4];
        memcpy(q, (const sx_finding*)P.recs + i, sizeof q);
        off = (uint32_t)q[1]; len = (uint32_t)(q[1] >> 32);
        q[1] = (uint64_t)folded << 32 | (uint32_t)at;
        memcpy((sx_finding*)P.out_recs + i, q, sizeof q);
    }
    (void)fold_place_string(T, P.arena + off, len, P.out_arena + at);
}

}  // namespace sx
