// sx_print_core.hpp — Finding::print (src/finding.rs:112-155) for the findings of a segment that lies in HBM
// (sx_print_findings_device): what ONE wavefront does for its kPrintRecs consecutive records, written as lane loops.  Included by
// sx_print_dev.hip with SXD = `__device__ __forceinline__`; the test-only harness tests/native/print_core_host.cpp includes it
// with SXD = `inline`, so the very same code is checked against a plain formatter on a machine without GPU
// (tests/test_print_core.py).  print_findings (sx_replay.cpp) is the host's statement of the same rule.
//
// A line is '\n', then unless no_metadata: [file letter ' '] if there are several inputs and the file id is >= 0; if a radix is
// given: the precision mark, the position in that radix without padding, "+\t" or " \t"; "(" Mission letter ' ' label ")\t" if the
// context has several Missions; then the string.  Everything in front of the string is the line's PREFIX, at most
// 1 + 2 + 1 + 22 + 2 + 3 + 14 + 2 = 47 bytes (22 octal digits, the longest label has 14 bytes).
//
// Offsets have 64 bits throughout: a wavefront's records give one contiguous range of the text, which begins at
// base (the segment's first byte in the text block) + wbase[w] (an exclusive scan over the wavefronts' line bytes, pass 1);
// inside the range the 65 line offsets are a scan over the 64 line lengths (LDS).  The range is written in aligned 16-byte chunks,
// a chunk per lane and round: every output byte finds its record by a search over the offsets and is either a prefix byte (LDS)
// or a string byte (global, addressed by str_off: no layout of the arena is assumed); the first and the last chunk, which may be
// shared with the neighbouring wavefronts, byte by byte.
#pragma once
#include <stdint.h>

#include "../../include/stringsext_amd.h"

namespace sx {

constexpr uint32_t kPrintRecs = 64;     // records per wavefront: one per lane
constexpr uint32_t kPrintPrefix = 48;   // bytes of LDS per record's prefix (47 used at most)

struct PrintMission {        // by mission_id: what the "(a utf-8)\t" part needs
    uint8_t present;         // the context has a Mission of this id
    uint8_t len;             // bytes of label, <= 14
    uint8_t label[14];       // "ascii" if print_encoding_as_ascii, else Encoding::name()
};

struct PrintParams {
    const void* recs;              // n records: sx_finding16 if `packed`, else sx_finding
    const uint8_t* arena;          // the segment's strings: a record's string is arena[str_off, str_off + str_len)
    uint64_t n;
    uint32_t packed;
    int32_t file_id;               // packed records: the segment's input_file_id (sx_segment_info)
    uint32_t several_inputs;       // n_inputs > 1
    uint32_t radix;                // 0 | 'x' | 'd' | 'o'
    uint32_t no_metadata;
    uint32_t several_missions;     // the context has more than one Mission
    const PrintMission* missions;  // 256 entries
    const uint64_t* wbase;         // per wavefront: the text bytes of the segment's wavefronts in front of it
    uint8_t* text;                 // the text block
    uint64_t base;                 // where the segment's text begins in it
};

struct PrintRec { uint64_t position; uint32_t str_off, str_len; uint32_t precision, completes, mission_id; int32_t file_id; };
struct alignas(16) Print16 { uint32_t w[4]; };

SXD PrintRec print_record(const PrintParams& P, uint64_t i) {
    PrintRec r;
    if (P.packed) {
        const sx_finding16 p = ((const sx_finding16*)P.recs)[i];
        r.position = p.position; r.str_off = p.str_off; r.str_len = p.str_len;
        r.precision = p.flags & 3u; r.completes = (p.flags >> 2) & 1u; r.mission_id = p.mission_id; r.file_id = P.file_id;
    } else {
        const sx_finding f = ((const sx_finding*)P.recs)[i];
        r.position = f.position; r.str_off = f.str_off; r.str_len = f.str_len;
        r.precision = f.precision; r.completes = f.completes_previous; r.mission_id = f.mission_id; r.file_id = f.input_file_id;
    }
    return r;
}

// The position's digits, most significant first, to dst (dst == nullptr: count only).  Hex and octal are shifts, decimal divides
// by the constant 10; the digits go straight to their places, last one first: no array of digits per lane.
SXD uint32_t print_digits(uint64_t v, uint32_t radix, uint8_t* dst) {
    const uint32_t bits = 64u - (uint32_t)__builtin_clzll(v | 1u);
    uint32_t nd;
    if (radix == 'x') nd = (bits + 3u) / 4u;
    else if (radix == 'o') nd = (bits + 2u) / 3u;
    else {
        nd = 1;
        for (uint64_t p = 10; nd < 20u && v >= p; p *= 10u) nd++;   // (10^19 < 2^64 <= 10^20: the product is not used after it wraps)
    }
    if (dst) {
        for (uint32_t k = nd; k-- > 0;) {
            uint32_t d;
            if (radix == 'x') { d = (uint32_t)v & 15u; v >>= 4; }
            else if (radix == 'o') { d = (uint32_t)v & 7u; v >>= 3; }
            else { const uint64_t q = v / 10u; d = (uint32_t)(v - q * 10u); v = q; }
            dst[k] = (uint8_t)(d < 10u ? '0' + d : 'a' + (d - 10u));
        }
    }
    return nd;
}

// A record's prefix to `pre` (kPrintPrefix bytes; nullptr: count only); returns its length.
SXD uint32_t print_prefix(const PrintParams& P, const PrintRec& r, uint8_t* pre) {
    uint32_t k = 0;
    if (pre) pre[k] = '\n';
    k++;
    if (P.no_metadata) return k;
    if (P.several_inputs && r.file_id >= 0) {
        if (pre) { pre[k] = (uint8_t)(r.file_id + 64); pre[k + 1] = ' '; }
        k += 2;
    }
    if (P.radix) {
        if (pre) pre[k] = r.precision == SX_PRECISION_AFTER ? '>' : r.precision == SX_PRECISION_EXACT ? ' ' : '<';
        k++;
        k += print_digits(r.position, P.radix, pre ? pre + k : nullptr);
        if (pre) { pre[k] = r.completes ? '+' : ' '; pre[k + 1] = '\t'; }
        k += 2;
    }
    if (P.several_missions) {
        const PrintMission* m = P.missions + r.mission_id;
        if (m->present) {
            const uint32_t len = m->len;
            if (pre) {
                pre[k] = '('; pre[k + 1] = (uint8_t)(r.mission_id + 97u); pre[k + 2] = ' ';
                for (uint32_t j = 0; j < len; j++) pre[k + 3 + j] = m->label[j];
                pre[k + 3 + len] = ')'; pre[k + 4 + len] = '\t';
            }
            k += 5 + len;
        }
    }
    return k;
}

// Pass 1: the bytes of record i's line (0 behind the last record).  A wavefront's sum is wsum[w]; wbase = its exclusive scan.
SXD uint64_t print_line_len(const PrintParams& P, uint64_t i) {
    if (i >= P.n) return 0;
    const PrintRec r = print_record(P, i);
    return (uint64_t)print_prefix(P, r, nullptr) + r.str_len;
}

// Pass 2, step 1, lane `lane` of wavefront `w`: its record's prefix (pre: kPrintRecs * kPrintPrefix bytes), prefix length, string
// address and line length into the wavefront's tables.  Lanes behind the last record hold empty lines at the end.
SXD void print_load_lane(const PrintParams& P, uint64_t w, uint32_t lane, uint64_t* lens, uint64_t* srcs, uint8_t* plens, uint8_t* pre) {
    const uint64_t i = w * kPrintRecs + lane;
    if (i < P.n) {
        const PrintRec r = print_record(P, i);
        const uint32_t pl = print_prefix(P, r, pre + lane * kPrintPrefix);
        plens[lane] = (uint8_t)pl;
        lens[lane] = (uint64_t)pl + r.str_len;
        srcs[lane] = (uint64_t)(uintptr_t)(P.arena + r.str_off);
    } else { plens[lane] = 0; lens[lane] = 0; srcs[lane] = 0; }
}

// Step 2 (after every lane's step 1): offs[lane] = the line bytes of the lanes in front; offs[kPrintRecs] = all of them.
SXD void print_scan_lane(uint32_t lane, const uint64_t* lens, uint64_t* offs) {
    uint64_t sum = 0;
    for (uint32_t j = 0; j < lane; j++) sum += lens[j];
    offs[lane] = sum;
    if (lane == kPrintRecs - 1) offs[kPrintRecs] = sum + lens[lane];
}

// Step 3 (after every lane's step 2), lane `lane`: the 16-byte chunks lane, lane + 64, ... of the wavefront's range.  Chunks are
// aligned in memory; bytes are counted from the range's start.
SXD void print_copy_lane(const PrintParams& P, uint64_t w, uint32_t lane, const uint64_t* offs, const uint64_t* srcs, const uint8_t* plens,
                         const uint8_t* pre) {
    const uint64_t total = offs[kPrintRecs];
    if (total == 0) return;
    uint8_t* const out = P.text + (P.base + P.wbase[w]);
    const uint64_t mis = (uint64_t)(uintptr_t)out & 15u;   // the range's first chunk begins `mis` bytes in front of it
    for (uint64_t c = lane;; c += kPrintRecs) {
        // chunk c = the bytes [c * 16 - mis, c * 16 - mis + 16), of which [lo, hi) are this wavefront's
        if (c * 16 >= total + mis) break;
        const uint64_t lo = c == 0 ? 0 : c * 16 - mis;
        const uint64_t hi = c * 16 + 16 - mis < total ? c * 16 + 16 - mis : total;
        // the record that holds byte lo: the last one that begins at or in front of it (every line has a byte; the empty
        // lines behind the last record begin at `total`)
        uint32_t r = 0;
        for (uint32_t step = kPrintRecs / 2; step; step >>= 1)
            if (offs[r + step] <= lo) r += step;
        uint64_t r_off = offs[r], r_end = offs[r + 1];
        uint32_t pl = plens[r];
        const uint8_t* s = (const uint8_t*)(uintptr_t)srcs[r];
        const uint8_t* p = pre + r * kPrintPrefix;
        const bool whole = hi - lo == 16;
        Print16 v{ { 0, 0, 0, 0 } };
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint64_t b = lo + k;
            if (b < hi) {
                while (b >= r_end) {
                    r++; r_off = r_end; r_end = offs[r + 1]; pl = plens[r];
                    s = (const uint8_t*)(uintptr_t)srcs[r]; p = pre + r * kPrintPrefix;
                }
                const uint64_t j = b - r_off;
                const uint32_t x = j < pl ? p[j] : s[j - pl];
                if (whole) v.w[k >> 2] |= x << ((k & 3u) * 8u);
                else out[b] = (uint8_t)x;
            }
        }
        if (whole) *(Print16*)(out + lo) = v;
    }
}

}  // namespace sx
