// Test-only program: compiles the lane functions of the Unicode case fold (sx_fold_core.hpp) as host code and runs them, under the
// address and undefined-behaviour sanitizers (tests/test_fold_core.py builds it so), over the vectors of that test's ill-formed and
// word-path cases: every two-byte string; every lead byte in front of 0 to 3 continuation bytes at the edges of Unicode's Table 3-7,
// whole and cut short by the end of the string; strings of 0 to 25 bytes at each of the 8 alignments with one non-ASCII character at
// every offset.  Every input lies in an allocation of its own that ENDS where the string ends and begins `alignment` bytes in front
// of it, and every output in one of exactly the measured length: a byte read or written outside is the sanitizer's finding.  The
// folded bytes are compared with a plain reference of the rule: a decoder written after Table 3-7 line by line and a binary search
// in the table's pair list.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_fold_core.hpp"

namespace {

const sx::FoldTable kTable{ sx::kFoldIndex, sx::kFoldPages };

uint32_t ref_fold(uint32_t c) {
    uint32_t lo = 0, hi = sx::kFoldPairCount;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (sx::kFoldPairs[mid][0] < c) lo = mid + 1; else hi = mid;
    }
    return lo < sx::kFoldPairCount && sx::kFoldPairs[lo][0] == c ? sx::kFoldPairs[lo][1] : c;
}

void ref_encode(uint32_t c, std::string* out) {
    if (c < 0x80) *out += (char)c;
    else if (c < 0x800) { *out += (char)(0xC0 | c >> 6); *out += (char)(0x80 | (c & 63)); }
    else if (c < 0x10000) { *out += (char)(0xE0 | c >> 12); *out += (char)(0x80 | (c >> 6 & 63)); *out += (char)(0x80 | (c & 63)); }
    else { *out += (char)(0xF0 | c >> 18); *out += (char)(0x80 | (c >> 12 & 63)); *out += (char)(0x80 | (c >> 6 & 63)); *out += (char)(0x80 | (c & 63)); }
}

bool cont(uint8_t b, uint8_t lo = 0x80, uint8_t hi = 0xBF) { return b >= lo && b <= hi; }

// Table 3-7, a row per `if`
std::string ref(const std::string& in) {
    std::string out;
    const size_t n = in.size();
    const uint8_t* s = (const uint8_t*)in.data();
    size_t k = 0;
    while (k < n) {
        const uint8_t b = s[k];
        size_t len = 0;
        if (b <= 0x7F) len = 1;
        else if (b >= 0xC2 && b <= 0xDF) { if (k + 1 < n && cont(s[k + 1])) len = 2; }
        else if (b == 0xE0) { if (k + 2 < n && cont(s[k + 1], 0xA0) && cont(s[k + 2])) len = 3; }
        else if ((b >= 0xE1 && b <= 0xEC) || b == 0xEE || b == 0xEF) { if (k + 2 < n && cont(s[k + 1]) && cont(s[k + 2])) len = 3; }
        else if (b == 0xED) { if (k + 2 < n && cont(s[k + 1], 0x80, 0x9F) && cont(s[k + 2])) len = 3; }
        else if (b == 0xF0) { if (k + 3 < n && cont(s[k + 1], 0x90) && cont(s[k + 2]) && cont(s[k + 3])) len = 4; }
        else if (b >= 0xF1 && b <= 0xF3) { if (k + 3 < n && cont(s[k + 1]) && cont(s[k + 2]) && cont(s[k + 3])) len = 4; }
        else if (b == 0xF4) { if (k + 3 < n && cont(s[k + 1], 0x80, 0x8F) && cont(s[k + 2]) && cont(s[k + 3])) len = 4; }
        if (!len) { out += (char)b; k++; continue; }
        uint32_t c = b;
        if (len == 2) c = (b & 0x1F) << 6 | (s[k + 1] & 63);
        if (len == 3) c = (b & 0x0F) << 12 | (s[k + 1] & 63) << 6 | (s[k + 2] & 63);
        if (len == 4) c = (b & 0x07) << 18 | (s[k + 1] & 63) << 12 | (s[k + 2] & 63) << 6 | (s[k + 3] & 63);
        ref_encode(ref_fold(c), &out);
        k += len;
    }
    return out;
}

uint64_t cases = 0;

// the two walks over `in` at `alignment` (0 .. 7) of an 8-byte word; false: they differ from the reference
bool check(const std::string& in, uint32_t alignment) {
    cases++;
    const std::string want = ref(in);
    // (malloc aligns to 16: the string begins `alignment` bytes behind that and ends where the allocation ends)
    uint8_t* src = (uint8_t*)malloc(alignment + in.size() ? alignment + in.size() : 1);
    if (!src) return false;
    uint8_t* s = src + alignment;
    memcpy(s, in.data(), in.size());
    bool changed = false;
    const uint64_t need = sx::fold_measure_string(kTable, s, in.size(), &changed);
    bool ok = need == want.size() && changed == (want != in);
    for (uint32_t out_alignment = 0; ok && out_alignment < 8; out_alignment += 2) {      // the output's stores: 8-byte words, bytes, 4-byte words, bytes
        uint8_t* dst = (uint8_t*)malloc(out_alignment + need ? out_alignment + need : 1);
        if (!dst) { ok = false; break; }
        const uint64_t wrote = sx::fold_place_string(kTable, s, in.size(), dst + out_alignment);
        ok = wrote == need && !memcmp(dst + out_alignment, want.data(), need);
        free(dst);
    }
    if (!ok) {
        fprintf(stderr, "fold core: alignment %u, input", alignment);
        for (unsigned char ch : in) fprintf(stderr, " %02x", ch);
        fprintf(stderr, ": measured %llu, the reference has %zu bytes\n", (unsigned long long)need, want.size());
    }
    free(src);
    return ok;
}

}  // namespace

int main() {
    bool ok = true;
    // every two-byte string
    for (uint32_t a = 0; ok && a < 256; a++)
        for (uint32_t b = 0; ok && b < 256; b++) ok = check(std::string{ (char)a, (char)b }, (a + b) & 7u);
    // every lead byte, 0 to 3 bytes behind it drawn from the edges of the second byte's ranges and the continuation range, then a letter or the end
    const uint8_t seconds[] = { 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0 }, thirds[] = { 0x7F, 0x80, 0xBF, 0xC0 };
    for (uint32_t lead = 0x80; ok && lead < 256; lead++)
        for (uint32_t tail = 0; ok && tail < 2; tail++) {
            const std::string end = tail ? "Z" : "";
            ok = check(std::string{ (char)lead } + end, lead & 7u);
            for (uint8_t b1 : seconds) {
                ok = ok && check(std::string{ (char)lead, (char)b1 } + end, b1 & 7u);
                for (uint8_t b2 : thirds) {
                    ok = ok && check(std::string{ (char)lead, (char)b1, (char)b2 } + end, (b1 + b2) & 7u);
                    for (uint8_t b3 : thirds) ok = ok && check(std::string{ (char)lead, (char)b1, (char)b2, (char)b3 } + end, (lead + b3) & 7u);
                }
            }
        }
    // the word path: 0 .. 25 bytes of upper-case ASCII at every alignment, one non-ASCII character at every offset: one that keeps its
    // length, one that grows, two that shrink, one of four bytes, and a byte that is no character
    const char* chars[] = { "\xD0\x9F", "\xC8\xBA", "\xE2\x84\xAA", "\xE1\xBA\x9E", "\xF0\x90\x90\x80", "\xFF" };
    for (uint32_t alignment = 0; ok && alignment < 8; alignment++)
        for (size_t len = 0; ok && len <= 25; len++) {
            std::string ascii;
            for (size_t i = 0; i < len; i++) ascii += (char)('A' + (i * 7 + len) % 26);
            ok = check(ascii, alignment);
            for (const char* ch : chars)
                for (size_t at = 0; ok && at + strlen(ch) <= len; at++) {
                    std::string s = ascii;
                    s.replace(at, strlen(ch), ch);
                    ok = check(s, alignment);
                }
        }
    // what the driver asks between the passes.  21 846 times U+023A, 43 692 bytes that a packed record's 16-bit str_len holds, are 65 538
    // bytes when they are folded: a packed segment with that string is refused, an unpacked one is not; one byte less passes either way
    {
        std::string grown, most;
        for (int i = 0; i < 21846; i++) grown += "\xC8\xBA";
        most = grown.substr(0, 2 * 21845);
        bool changed = false;
        const uint64_t longest = sx::fold_measure_string(kTable, (const uint8_t*)grown.data(), grown.size(), &changed);
        const uint64_t fits = sx::fold_measure_string(kTable, (const uint8_t*)most.data(), most.size(), &changed);
        ok = ok && grown.size() <= 0xFFFFu && longest == 65538 && fits == 65535;
        ok = ok && sx::fold_segment_fits(1u, longest, longest) == sx::kFoldPackedTooLong && sx::fold_segment_fits(0u, longest, longest) == sx::kFoldFits;
        ok = ok && sx::fold_segment_fits(1u, fits, fits) == sx::kFoldFits;
        ok = ok && sx::fold_segment_fits(0u, 0xFFFFFFFFull, 100) == sx::kFoldFits && sx::fold_segment_fits(0u, 0x100000000ull, 100) == sx::kFoldTooManyBytes;
        ok = ok && sx::fold_segment_fits(1u, 0x100000000ull, 0x10000) == sx::kFoldTooManyBytes;
        // and the records that place writes where it fits: a packed and an unpacked one, every byte but str_off and str_len kept
        sx_finding16 p16 = { 0x1122334455667788ull, 7u, (uint16_t)most.size(), 0x05, 0xA7 }, o16;
        sx_finding p32, o32;
        memset(&p32, 0x5A, sizeof p32);       // (its padding too)
        p32.str_off = 7; p32.str_len = (uint32_t)grown.size();
        memset(&o16, 0, sizeof o16); memset(&o32, 0, sizeof o32);
        std::vector<uint8_t> arena(7 + grown.size()), out(3 + 65538);
        memcpy(arena.data() + 7, grown.data(), grown.size());
        sx::FoldParams P;
        memset(&P, 0, sizeof P);
        P.arena = arena.data(); P.n = 1; P.out_arena = out.data();
        P.recs = &p16; P.packed = 1; P.out_recs = &o16;
        sx::fold_place_lane(P, kTable, 0, 0, 3, 65535);
        ok = ok && o16.position == p16.position && o16.str_off == 3 && o16.str_len == 65535 && o16.flags == 0x05 && o16.mission_id == 0xA7;
        P.recs = &p32; P.packed = 0; P.out_recs = &o32;
        sx::fold_place_lane(P, kTable, 0, 0, 3, 65538);
        sx_finding want32 = p32;
        want32.str_off = 3; want32.str_len = 65538;
        ok = ok && !memcmp(&o32, &want32, sizeof o32) && !memcmp(out.data() + 3, ref(grown).data(), 65538);
        cases += 8;
    }
    if (!ok) return 1;
    printf("fold core: ok, %llu cases\n", (unsigned long long)cases);
    return 0;
}
