// sx_extract_core.hpp — the regex matches of the findings of a segment that lies in HBM, cut out where they lie
// (sx_result_extract_regex_device): what ONE lane does for its record, written as lane functions.  Included by sx_extract_dev.hip
// with SXD = `__device__ __forceinline__`; the test-only harness tests/native/extract_core_host.cpp includes it with SXD = `inline`,
// so the very same code is checked against a brute force over Python's `re` on a machine without GPU (tests/test_extract_core.py).
//
// The rule (`grep -oE`): for a finding with the string s of n bytes, o = 0; while o < n: let e be the largest end in (o, n] such
// that some pattern matches exactly s[o, e) — `^` holds only at offset 0, `$` only at offset n, for every match of the string —;
// if there is one, (o, e) is a match and o = e, else o = o + 1.  Leftmost start, longest end over all patterns, no overlap, no empty
// match; a match never spans two findings.  Every match gives one output record: the finding's record with another str_off and
// str_len.
//
// The patterns arrive as the anchored DFA sx_extract_build.hpp describes.  One lane, one record, one byte per step: a walk begins
// at o in start0 (o == 0) or start1 and takes next[state * classes + map[byte]] — from LDS for the first lds_states states, from
// the table in HBM (through L2) for the others —, remembering the last position behind which a match may end (a `here` state, or an
// `end` state behind the last byte).  The walk is over in `dead` or behind the last byte; then the remembered end is a match and
// the next walk begins there, or there is none and the next walk begins at o + 1.  A byte that can begin no match costs one step:
// the start row leads to `dead`.  A walk that runs far and fails is repeated from the next offset: the worst case is quadratic in
// the string's length (`a*b` over a run of a).  A lane reads the bytes [str_off, str_off + str_len) of its own record and no other
// byte of the arena: `$` is decided by the length, never by a look at what follows.
//
// Pass 1 (extract_count_kernel) keeps each record's number of matches and per wavefront their sum and the matches' bytes; behind the
// exclusive scans over those, pass 2 (extract_place_kernel) repeats the walk and writes match k of record i to
// wbase[w] + (the matches of the wavefront's earlier records) + k, noting where its bytes lie; order_part_strings
// (sx_result_dev.hip) then lays the strings back to back.
#pragma once
#include <stdint.h>

#include "sx_select_core.hpp"

namespace sx {

// a compiled extract set where the kernels read it (device pointers; in the harness: the builder's)
struct ExtractDevice {
    const uint8_t* map;       // 256 bytes: byte -> class
    const uint16_t* next;     // states * classes entries
    uint32_t states, classes, lds_states, end_first, here_first, dead_first, start0, start1;
};

struct ExtractParams {
    const void* recs;        // n records: sx_finding16 if `packed`, else sx_finding
    const uint8_t* arena;    // the segment's strings: a record's string is arena[str_off, str_off + str_len)
    uint64_t n;
    uint32_t packed, reserved;
    uint32_t* rcount;        // pass 1 writes, pass 2 reads: per record, its matches
    uint64_t* wcount;        // pass 1 writes, per wavefront (waves + 1 entries: the one behind the last record has none): its records' matches
    uint64_t* wbytes;        // and their bytes
    const uint64_t* wbase;   // pass 2 reads: the exclusive scan of wcount
    void* out_recs;          // the output records, in order (str_off: an offset into the SOURCE arena until the strings are ordered)
    uint64_t* out_src;       // per output record: the address of its bytes
    ExtractDevice ex;
};

// a lane's walks over its record's string
struct ExtractLane {
    uint64_t off;            // the string in the arena
    uint32_t len, o, at;     // its length; where the current walk began; the next byte
    uint32_t last;           // the end of the longest match of the current walk so far (0: none — a match is not empty)
    uint32_t state, active;
};

// Lane `lane` of wavefront `w` in front of its record's string (lanes behind the last record have none).
SXD ExtractLane extract_begin_lane(const ExtractParams& P, uint64_t w, uint32_t lane) {
    const uint64_t i = w * kSelectRecs + lane;
    ExtractLane L{ 0, 0, 0, 0, 0, 0, 0 };
    if (i >= P.n) return L;
    select_string(P, i, &L.off, &L.len);
    L.state = P.ex.start0;
    L.active = L.len != 0;
    return L;
}

// One byte of the lane's string (L.active holds).  map: the 256 classes, rows: the first lds_states rows (LDS).  Returns the end of
// a match [*from, end) that this step has completed, or 0.
SXD uint32_t extract_step_lane(const ExtractParams& P, const uint8_t* map, const uint16_t* rows, ExtractLane& L, uint32_t* from) {
    const uint32_t at = L.state * P.ex.classes + map[P.arena[L.off + L.at]];
    L.state = L.state < P.ex.lds_states ? rows[at] : P.ex.next[at];
    L.at++;
    bool over = L.state >= P.ex.dead_first;
    if (!over) {
        over = L.at == L.len;
        if (L.state >= P.ex.here_first || (over && L.state >= P.ex.end_first)) L.last = L.at;
    }
    if (!over) return 0;
    const uint32_t end = L.last;
    *from = L.o;
    L.o = end ? end : L.o + 1;
    L.at = L.o; L.last = 0; L.state = P.ex.start1;      // (o > 0 from here on)
    L.active = L.o < L.len;
    return end;
}

// Pass 2: match [from, end) of record i, the `rank`-th of the segment, to its place, and where its bytes lie.
SXD void extract_place_match(const ExtractParams& P, uint64_t i, uint64_t rank, uint32_t from, uint32_t end) {
    uint32_t off;      // (the record is copied and two of its words written again: a changed copy of its own would live in scratch memory)
    if (P.packed) {
        const sx_finding16* src = (const sx_finding16*)P.recs + i;
        sx_finding16* dst = (sx_finding16*)P.out_recs + rank;
        off = src->str_off + from;
        *dst = *src;
        dst->str_off = off; dst->str_len = (uint16_t)(end - from);
    } else {
        const sx_finding* src = (const sx_finding*)P.recs + i;
        sx_finding* dst = (sx_finding*)P.out_recs + rank;
        off = src->str_off + from;
        *dst = *src;
        dst->str_off = off; dst->str_len = end - from;
    }
    P.out_src[rank] = (uint64_t)(uintptr_t)(P.arena + off);
}

}  // namespace sx
