// sx_decode_core.hpp — the strings of a result that lies in HBM read as base64, hex or percent escapes and replaced by the bytes they
// stand for (sx_result_decode_device), and the same decoding of one byte string on the host (sx_decode_bytes): what ONE lane does for
// its own string, written as lane functions.  Included by sx_decode_dev.hip with SXD = `__device__ __forceinline__`, by
// sx_result_api.cpp and by the test-only program tests/native/decode_core_host.cpp with SXD = `inline`, so the very same code is
// checked against Python's base64, binascii, urllib.parse and codecs on a machine without GPU (tests/test_decode_core.py).
//
// The rule.  A string s of n bytes, a kind and flags give raw bytes D, or "does not decode":
//  SX_DECODE_BASE64   pad = the trailing '=', two at most; body = the rest, of m bytes.  Decodes iff m >= 2, m % 4 != 1, pad == 0 or
//                     (m + pad) % 4 == 0, every body byte is of A-Za-z0-9 or one of + / - _, and the body does not hold both a byte of
//                     "+/" and one of "-_".  Six bits a byte, the first the highest; what is left of the last byte is dropped.
//  SX_DECODE_HEX      n even, n >= 2, every byte a hex digit of either case: a byte per pair.
//  SX_DECODE_PERCENT  from the left: '%' with two hex digits behind it inside the string is that byte, and the walk goes on three bytes
//                     further; any other byte is copied.  Decodes iff there was an escape.
// With SX_DECODE_UTF16LE, D is read as UTF-16LE and written as UTF-8; an odd length or a lone surrogate: does not decode.  A BOM is an
// ordinary U+FEFF.
//
// The decoder streams: the walk of a kind hands raw bytes to DecodeRaw, which keeps the WIDE bit's state and, under SX_DECODE_UTF16LE,
// puts two bytes together to a unit and a surrogate pair to a code point; what it writes goes to a sink that counts (and keeps the TEXT
// bit's state) or stores.  There is no table and no array: the sextet and the nibble come out of range compares.  A lane reads
// [s, s + n) and no other byte, and the placing walk writes [out, out + measured length) and no other byte.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sx_select_core.hpp"

namespace sx {

static_assert(sizeof(sx_finding) == 32 && sizeof(sx_finding16) == 16, "decode_place_lane copies the records as 64-bit words");

// 0x20..0x7E, tab, line feed, carriage return: the bytes of SX_DECODE_TEXT and SX_DECODE_WIDE
SXD bool decode_is_text(uint32_t b) { return b - 0x20u < 0x5Fu || b == 0x09u || b == 0x0Au || b == 0x0Du; }
// the value of a hex digit, or 16
SXD uint32_t decode_nibble(uint32_t b) {
    if (b - '0' < 10u) return b - '0';
    const uint32_t l = b | 0x20u;
    return l - 'a' < 6u ? l - 'a' + 10u : 16u;
}
// the six bits of a base64 byte of either alphabet, or 64; *special: |= 1 for "+/", 2 for "-_"
SXD uint32_t decode_sextet(uint32_t b, uint32_t* special) {
    if (b - 'A' < 26u) return b - 'A';
    if (b - 'a' < 26u) return b - 'a' + 26u;
    if (b - '0' < 10u) return b - '0' + 52u;
    if (b == '+' || b == '/') { *special |= 1u; return b == '+' ? 62u : 63u; }
    if (b == '-' || b == '_') { *special |= 2u; return b == '-' ? 62u : 63u; }
    return 64u;
}

// where the output's bytes go: nowhere, counted, with the TEXT bit's state ...
struct DecodeCount {
    uint64_t n = 0;
    bool text = true;
    SXD void byte(uint32_t b) { n++; text = text && decode_is_text(b); }
};
// ... or to out[n]
struct DecodeWrite {
    uint8_t* out;
    uint64_t n = 0;
    SXD void byte(uint32_t b) { out[n++] = (uint8_t)b; }
};

// The raw bytes D on their way to the sink: as they are, or (U16) as UTF-16LE written as UTF-8
template <bool U16, class Sink>
struct DecodeRaw {
    Sink& out;
    uint32_t raw_n = 0;          // bytes of D so far: no more than the string has, and that is below 2^32
    bool wide = true;            // so far every odd-index byte 0 and every even-index byte of the TEXT class
    bool bad = false;            // U16: a lone surrogate was met
    uint32_t low = 0, high = 0;  // U16: a unit's first byte; a high surrogate that waits for its low one (0: none)
    SXD explicit DecodeRaw(Sink& s) : out(s) {}
    SXD void unit(uint32_t u) {
        uint32_t c = u;
        if (high) {
            if (u - 0xDC00u >= 0x400u) { bad = true; high = 0; return; }
            c = 0x10000u + ((high - 0xD800u) << 10) + (u - 0xDC00u);
            high = 0;
        } else if (u - 0xD800u < 0x400u) { high = u; return; }
        else if (u - 0xDC00u < 0x400u) { bad = true; return; }
        if (c < 0x80u) out.byte(c);
        else if (c < 0x800u) { out.byte(0xC0u | c >> 6); out.byte(0x80u | (c & 0x3Fu)); }
        else if (c < 0x10000u) { out.byte(0xE0u | c >> 12); out.byte(0x80u | (c >> 6 & 0x3Fu)); out.byte(0x80u | (c & 0x3Fu)); }
        else { out.byte(0xF0u | c >> 18); out.byte(0x80u | (c >> 12 & 0x3Fu)); out.byte(0x80u | (c >> 6 & 0x3Fu)); out.byte(0x80u | (c & 0x3Fu)); }
    }
    SXD void raw(uint32_t b) {
        const bool odd = raw_n & 1u;
        wide = wide && (odd ? b == 0u : decode_is_text(b));
        raw_n++;
        if (!U16) out.byte(b);
        else if (odd) unit(low | b << 8);
        else low = b;
    }
    // D is whole: does it stand as it is read?
    SXD bool whole() const { return !U16 || (!(raw_n & 1u) && !bad && !high); }
    SXD bool is_wide() const { return wide && raw_n >= 2u && !(raw_n & 1u); }
};

// The walks: s[0, n) to D, byte by byte (a string of a result has fewer than 2^32 bytes, and sx_decode_bytes takes no more).  Each
// returns the word's bits that only it knows (SX_DECODE_OK among them), or 0 where the string does not decode — then what it has
// handed on counts for nothing
template <class Raw>
SXD uint64_t decode_walk_base64(const uint8_t* s, uint32_t n, Raw& D) {
    uint32_t pad = 0;
    if (n >= 1u && s[n - 1] == '=') pad = n >= 2u && s[n - 2] == '=' ? 2u : 1u;
    const uint32_t m = n - pad;
    if (m < 2u || m % 4u == 1u || (pad && (m + pad) % 4u)) return 0;
    uint32_t acc = 0, bits = 0, special = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t v = decode_sextet(s[k], &special);
        if (v > 63u) return 0;
        acc = (acc << 6 | v) & 0xFFFFu;
        bits += 6u;
        if (bits >= 8u) { bits -= 8u; D.raw(acc >> bits & 0xFFu); }
    }
    if (special == 3u) return 0;
    return SX_DECODE_OK | (pad ? SX_DECODE_PADDED : 0u) | (special == 2u ? SX_DECODE_URLSAFE : 0u);
}
template <class Raw>
SXD uint64_t decode_walk_hex(const uint8_t* s, uint32_t n, Raw& D) {
    if (n < 2u || (n & 1u)) return 0;
    for (uint32_t k = 0; k < n; k += 2u) {
        const uint32_t hi = decode_nibble(s[k]), lo = decode_nibble(s[k + 1]);
        if ((hi | lo) > 15u) return 0;
        D.raw(hi << 4 | lo);
    }
    return SX_DECODE_OK;
}
template <class Raw>
SXD uint64_t decode_walk_percent(const uint8_t* s, uint32_t n, Raw& D) {
    bool escaped = false;
    for (uint32_t k = 0; k < n;) {
        const uint32_t b = s[k];
        if (b == '%' && n - k >= 3u) {
            const uint32_t hi = decode_nibble(s[k + 1]), lo = decode_nibble(s[k + 2]);
            if ((hi | lo) <= 15u) { D.raw(hi << 4 | lo); escaped = true; k += 3u; continue; }
        }
        D.raw(b);
        k++;
    }
    return escaped ? SX_DECODE_OK : 0u;
}

// s[0, n) under `kind` (checked: one of the three) to `out`: the word's bits but SX_DECODE_TEXT and the length, or 0
template <bool U16, class Sink>
SXD uint64_t decode_to(uint32_t kind, const uint8_t* s, uint32_t n, Sink& out) {
    DecodeRaw<U16, Sink> D(out);
    const uint64_t bits = kind == SX_DECODE_BASE64 ? decode_walk_base64(s, n, D) : kind == SX_DECODE_HEX ? decode_walk_hex(s, n, D) : decode_walk_percent(s, n, D);
    if (!bits || !D.whole()) return 0;
    return bits | (D.is_wide() ? SX_DECODE_WIDE : 0u);
}

// The two walks of a string.  measure: its word — the length field holds at most 2^32 - 1 —, and in *out_len the bytes that the
// output record's string will have: the decoded length, or n where the string does not decode and is copied
SXD uint64_t decode_measure_string(uint32_t kind, uint32_t flags, const uint8_t* s, uint32_t n, uint64_t* out_len) {
    DecodeCount count;
    const uint64_t bits = (flags & SX_DECODE_UTF16LE) ? decode_to<true>(kind, s, n, count) : decode_to<false>(kind, s, n, count);
    *out_len = bits ? count.n : n;
    if (!bits) return 0;
    return bits | (count.text ? SX_DECODE_TEXT : 0u) | (count.n < 0xFFFFFFFFull ? count.n : 0xFFFFFFFFull) << SX_DECODE_LEN_SHIFT;
}
// place: what measure said of the string (`word`) decides — the decoded bytes, or the source's, to out[0, *out_len of measure)
SXD void decode_place_string(uint32_t kind, uint32_t flags, uint64_t word, const uint8_t* s, uint32_t n, uint8_t* out) {
    DecodeWrite write{ out };
    if (!(word & SX_DECODE_OK))
        for (uint32_t k = 0; k < n; k++) write.byte(s[k]);
    else if (flags & SX_DECODE_UTF16LE) (void)decode_to<true>(kind, s, n, write);
    else (void)decode_to<false>(kind, s, n, write);
}

// A segment's two passes (sx_decode_dev.hip).  The totals are per segment
enum DecodeTotal : uint32_t { kDecodeRecords = 0, kDecodeDecoded = 1, kDecodeText = 2, kDecodeWide = 3, kDecodeBytesIn = 4, kDecodeLongest = 5, kDecodeTotals = 6 };
struct DecodeParams {
    const void* recs;        // as SelectParams
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed;
    uint32_t kind, flags;    // checked by the driver
    // measure writes
    uint64_t* words;         // per record: its word (the labels of the call)
    uint64_t* wbytes;        // per wavefront (waves + 1 entries: the one behind the last record has no byte): its records' output bytes
    uint64_t* totals;        // kDecodeTotals words
    // place reads words and
    const uint64_t* wbase;   // the exclusive scan of wbytes
    void* out_recs;          // n records of the source's type
    uint8_t* out_arena;      // the output strings, back to back in record order
};

// What the driver asks between the passes, as fold_segment_fits asks it: do the output strings fit the records that place writes
enum DecodeFit : uint32_t { kDecodeFits = 0, kDecodeTooManyBytes = 1, kDecodePackedTooLong = 2 };
SXD DecodeFit decode_segment_fits(uint32_t packed, uint64_t out_bytes, uint64_t longest) {
    if (out_bytes >> 32) return kDecodeTooManyBytes;
    if (packed && longest > 0xFFFFu) return kDecodePackedTooLong;
    return kDecodeFits;
}

// The output string's bytes of a record whose source has `len` and whose word is `word` (a segment that place sees fits 32 bits)
SXD uint32_t decode_out_len(uint64_t word, uint32_t len) { return (word & SX_DECODE_OK) ? (uint32_t)(word >> SX_DECODE_LEN_SHIFT) : len; }

// measure, lane `lane` of wavefront `w`: its record's output bytes (0 behind the last record), its source length, its word
SXD uint64_t decode_measure_lane(const DecodeParams& P, uint64_t w, uint32_t lane, uint32_t* len, uint64_t* word) {
    const uint64_t i = w * kSelectRecs + lane;
    *len = 0; *word = 0;
    if (i >= P.n) return 0;
    uint64_t off, out_len;
    select_string(P, i, &off, len);
    *word = decode_measure_string(P.kind, P.flags, P.arena + off, *len, &out_len);
    P.words[i] = *word;
    return out_len;
}

// place, lane `lane` of wavefront `w`, whose record's string begins at out_arena[at]: the source record with the new str_off and
// str_len and nothing else changed (as fold_place_lane writes it), and the string's bytes
SXD void decode_place_lane(const DecodeParams& P, uint64_t w, uint32_t lane, uint64_t at) {
    const uint64_t i = w * kSelectRecs + lane;
    if (i >= P.n) return;
    const uint64_t word = P.words[i];
    uint32_t off, len;
    if (P.packed) {
        uint64_t q[2];
        memcpy(q, (const sx_finding16*)P.recs + i, sizeof q);
        off = (uint32_t)q[1]; len = (uint32_t)(q[1] >> 32) & 0xFFFFu;
        q[1] = (q[1] & 0xFFFF000000000000ull) | (uint64_t)(decode_out_len(word, len) & 0xFFFFu) << 32 | (uint32_t)at;
        memcpy((sx_finding16*)P.out_recs + i, q, sizeof q);
    } else {
        uint64_t q[4];
        memcpy(q, (const sx_finding*)P.recs + i, sizeof q);
        off = (uint32_t)q[1]; len = (uint32_t)(q[1] >> 32);
        q[1] = (uint64_t)decode_out_len(word, len) << 32 | (uint32_t)at;
        memcpy((sx_finding*)P.out_recs + i, q, sizeof q);
    }
    decode_place_string(P.kind, P.flags, word, P.arena + off, len, P.out_arena + at);
}

}  // namespace sx
