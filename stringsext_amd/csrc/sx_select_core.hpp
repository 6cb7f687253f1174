// sx_select_core.hpp — the substring selection over the findings of a segment that lies in HBM (sx_result_select_device): what
// ONE wavefront does for its kSelectRecs consecutive records, written as lane loops.  Included by sx_select_dev.hip with
// SXD = `__device__ __forceinline__`; the test-only harness tests/native/select_core_host.cpp includes it with SXD = `inline`,
// so the very same code is checked against Python's `p in s` on a machine without GPU (tests/test_select_core.py).
//
// The rule: finding i matches if some pattern p equals s[o, o + len_p) for some 0 <= o <= str_len - len_p — bytes as they are, or
// with 'A'..'Z' of string and pattern as 'a'..'z' (the patterns arrive folded) —; it is selected iff (matches) xor (invert).
// A match never spans two findings.
//
// Pass 1 (select_match_kernel): the wavefront's 64 offsets and lengths go into LDS.  Where its strings are ONE contiguous range
// of the arena — every merged segment, every earlier selection — the lanes read that range in aligned 16-byte chunks, a chunk per
// lane and round, and test every byte of the chunk as the place where a pattern begins — a table in LDS says which patterns begin
// with that byte, mostly none —: the place finds its record by the search over the offsets that gather_copy_lane
// (sx_result_core.hpp) uses, a hit counts only if it ends inside that record, and the record's bit is ORed into the wavefront's
// mask in LDS.  The bytes behind a first byte that fits are read from the arena again (at most 63 of them: the neighbouring
// lanes' chunks, L1).  Where the strings are not one range (a single Mission's
// segment: strings where the writer put them) a lane walks its own record's string.  Per wavefront: the mask of selected records,
// their number, their string bytes.
// Pass 2 (select_place_kernel), behind an exclusive scan over the wavefronts' numbers: a selected record goes to base + rank and
// notes where its string lies; order_part_strings (sx_result_dev.hip) then lays the strings back to back.
#pragma once
#include <stdint.h>

#include "../../include/stringsext_amd.h"

namespace sx {

constexpr uint32_t kSelectRecs = 64;     // records per wavefront: one per lane
constexpr uint32_t kSelectFirst = 256;   // entries of the first-byte table

struct SelectPatterns {
    uint32_t n, nocase, invert, reserved;
    uint8_t len[SX_SELECT_MAX_PATTERNS];
    uint8_t bytes[SX_SELECT_MAX_PATTERNS][SX_SELECT_MAX_PATTERN_BYTES];   // folded if nocase
};

struct SelectParams {
    const void* recs;        // n records: sx_finding16 if `packed`, else sx_finding
    const uint8_t* arena;    // the segment's strings: a record's string is arena[str_off, str_off + str_len)
    uint64_t n;
    uint32_t packed;
    // pass 1 writes, per wavefront (waves + 1 entries: the one behind the last record selects nothing)
    uint64_t* wmask;         // bit l: record w * 64 + l is selected
    uint32_t* wcount;        // popcount(wmask)
    uint64_t* wbytes;        // the selected records' string bytes
    // pass 2 reads wmask and
    const uint32_t* wbase;   // the exclusive scan of wcount
    void* out_recs;          // the selected records, in order (str_off still the source's)
    uint64_t* out_src;       // per selected record: the address of its string
    SelectPatterns pat;
};

struct alignas(16) Select16 { uint32_t w[4]; };

// (the harness runs the lanes one after the other)
SXD void select_or(uint32_t* word, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(word, bits);
#else
    *word |= bits;
#endif
}

// SX_SELECT_ASCII_NOCASE: 'A'..'Z' as 'a'..'z', no other byte
SXD uint32_t select_fold(uint32_t nocase, uint32_t x) { return nocase && x - 'A' < 26u ? x | 0x20u : x; }

// The call's patterns as the kernels take them (host only; sx_result_select_device has checked n and every len).
static inline void select_fill_patterns(SelectPatterns* out, const sx_pattern* patterns, int n, uint32_t flags) {
    *out = SelectPatterns{};
    out->n = (uint32_t)n; out->nocase = (flags & SX_SELECT_ASCII_NOCASE) ? 1u : 0u; out->invert = (flags & SX_SELECT_INVERT) ? 1u : 0u;
    for (int p = 0; p < n; p++) {
        out->len[p] = (uint8_t)patterns[p].len;
        for (uint32_t j = 0; j < patterns[p].len; j++) {
            const uint32_t x = patterns[p].bytes[j];
            out->bytes[p][j] = (uint8_t)(out->nocase && x - 'A' < 26u ? x | 0x20u : x);
        }
    }
}

// (PP: SelectParams, or the SelsetParams of sx_selset_core.hpp)
template <class PP>
SXD void select_string(const PP& P, uint64_t i, uint64_t* off, uint32_t* len) {
    if (P.packed) { const sx_finding16 p = ((const sx_finding16*)P.recs)[i]; *off = p.str_off; *len = p.str_len; }
    else { const sx_finding f = ((const sx_finding*)P.recs)[i]; *off = f.str_off; *len = f.str_len; }
}

// Entry x of the first-byte table (kSelectFirst halfwords, LDS): bit p says that pattern p begins with byte x.  A place in a
// string then costs one look into the table, whatever the number of patterns, and only the patterns that can begin there are compared.
SXD uint16_t select_first_entry(const SelectParams& P, uint32_t x) {
    uint32_t m = 0;
    for (uint32_t p = 0; p < P.pat.n; p++)
        if (P.pat.bytes[p][0] == x) m |= 1u << p;
    return (uint16_t)m;
}

// Does a pattern begin at arena[b] (x: that byte, folded) and end at or in front of `lim`, the end of b's record?
SXD bool select_match_at(const SelectParams& P, const uint16_t* first, uint64_t b, uint32_t x, uint64_t lim) {
    for (uint32_t m = first[x]; m; m &= m - 1u) {
        const uint32_t p = (uint32_t)__builtin_ctz(m), len = P.pat.len[p];
        if (b + len > lim) continue;
        uint32_t j = 1;
        while (j < len && select_fold(P.pat.nocase, P.arena[b + j]) == P.pat.bytes[p][j]) j++;
        if (j == len) return true;
    }
    return false;
}

// Step 1, lane `lane` of wavefront `w`: its record's offset and length into the wavefront's tables (offs: kSelectRecs + 1 words,
// lens: kSelectRecs), the mask cleared (hit: 2 words).  Lanes behind the last record hold empty strings at the end of the last
// record's.  Returns whether the record's string ends where the next lane's begins: if that holds for all lanes, offs is what
// gather_load_lane makes of a part — the strings are one range, offs[0] to offs[kSelectRecs].
SXD bool select_load_lane(const SelectParams& P, uint64_t w, uint32_t lane, uint64_t* offs, uint32_t* lens, uint32_t* hit) {
    const uint64_t i = w * kSelectRecs + lane;
    uint64_t off; uint32_t len;
    select_string(P, i < P.n ? i : P.n - 1, &off, &len);
    if (i >= P.n) { off += len; len = 0; }
    offs[lane] = off;
    lens[lane] = len;
    if (lane < 2) hit[lane] = 0;
    if (lane == kSelectRecs - 1) offs[kSelectRecs] = off + len;
    if (lane == kSelectRecs - 1 || i + 1 >= P.n) return true;
    uint64_t noff; uint32_t nlen;
    select_string(P, i + 1, &noff, &nlen);
    return noff == off + len;
}

// Step 2 where all lanes' step 1 said yes, lane `lane`: the 16-byte chunks lane, lane + 64, ... of the wavefront's range.  Chunks
// are aligned in memory; the first and the last may be shared with the neighbouring wavefronts and are read byte by byte,
// everything between them with one 16-byte load per lane.  Nothing outside [offs[0], offs[kSelectRecs]) is read.
SXD void select_scan_lane(const SelectParams& P, const uint16_t* first, uint32_t lane, const uint64_t* offs, uint32_t* hit) {
    const uint64_t start = offs[0], end = offs[kSelectRecs];
    if (start >= end) return;
    const uint64_t mis = ((uint64_t)(uintptr_t)P.arena + start) & 15u;   // the range's first chunk begins `mis` bytes in front of it
    for (uint64_t c = lane;; c += kSelectRecs) {
        // chunk c = the arena bytes [c0, c0 + 16), of which [lo, hi) are this wavefront's
        if (c * 16 >= end - start + mis) break;
        const uint64_t c0s = start + c * 16;          // (c0 + mis: no negative numbers)
        const uint64_t lo = c == 0 ? start : c0s - mis;
        const uint64_t hi = c0s - mis + 16 < end ? c0s - mis + 16 : end;
        // the record that holds byte lo: the last one that begins at or in front of it (empty strings share their successor's offset)
        uint32_t r = 0;
        for (uint32_t step = kSelectRecs / 2; step; step >>= 1)
            if (offs[r + step] <= lo) r += step;
        uint64_t r_end = offs[r + 1];
        const bool whole = hi - lo == 16;
        Select16 v{ { 0, 0, 0, 0 } };
        if (whole) v = *(const Select16*)(P.arena + lo);
        uint32_t found = ~0u;   // the record this lane has just found a pattern in: its other bytes need no look
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint64_t b = lo + k;
            if (b < hi) {
                while (b >= r_end) { r++; r_end = offs[r + 1]; }
                if (r != found) {
                    const uint32_t x = select_fold(P.pat.nocase, whole ? (v.w[k >> 2] >> ((k & 3u) * 8u)) & 255u : P.arena[b]);
                    if (select_match_at(P, first, b, x, r_end)) { select_or(hit + (r >> 5), 1u << (r & 31u)); found = r; }
                }
            }
        }
    }
}

// Step 2 otherwise, lane `lane`: its own record's string, addressed by str_off (no layout of the arena is assumed).
SXD void select_walk_lane(const SelectParams& P, const uint16_t* first, uint32_t lane, const uint64_t* offs, const uint32_t* lens, uint32_t* hit) {
    const uint64_t off = offs[lane], end = off + lens[lane];
    for (uint64_t b = off; b < end; b++)
        if (select_match_at(P, first, b, select_fold(P.pat.nocase, P.arena[b]), end)) { select_or(hit + (lane >> 5), 1u << (lane & 31u)); return; }
}

// Step 3 (after every lane's step 2): is the lane's record selected?  The wavefront's mask is the ballot over this.
SXD bool select_lane_selected(const SelectParams& P, uint64_t w, uint32_t lane, const uint32_t* hit) {
    if (w * kSelectRecs + lane >= P.n) return false;
    return (((hit[lane >> 5] >> (lane & 31u)) & 1u) ^ P.pat.invert) != 0;
}

// Pass 2, lane `lane` of wavefront `w`: a selected record to its place, and where its string lies.
SXD void select_place_lane(const SelectParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    if (i >= P.n) return;
    const uint64_t mask = P.wmask[w];
    if (!((mask >> lane) & 1u)) return;
    const uint64_t rank = (uint64_t)P.wbase[w] + (uint32_t)__builtin_popcountll(mask & (((uint64_t)1 << lane) - 1u));
    uint32_t off;
    if (P.packed) { const sx_finding16 p = ((const sx_finding16*)P.recs)[i]; off = p.str_off; ((sx_finding16*)P.out_recs)[rank] = p; }
    else { const sx_finding f = ((const sx_finding*)P.recs)[i]; off = f.str_off; ((sx_finding*)P.out_recs)[rank] = f; }
    P.out_src[rank] = (uint64_t)(uintptr_t)(P.arena + off);
}

}  // namespace sx
