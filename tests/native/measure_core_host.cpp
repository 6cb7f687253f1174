// Test-only program: compiles the lane functions of sx_result_measure_device (sx_measure_core.hpp) as host code and runs them, under
// the address and undefined-behaviour sanitizers (tests/test_measure_core.py builds it so): the narrow walk with a block of 256
// one-byte counters per "lane", and the wide count and finish with a block of 256 words and the 64 lanes one after the other.  Every
// string lies in an allocation of its own that ENDS where the string ends and begins `alignment` (0 .. 7) bytes in front of it, and
// every counter block in one of exactly its size: a byte read or written outside is the sanitizer's finding.  Behind every string
// the counter block must be all zero again.  The words are compared with a plain restatement of the rule: a histogram, the class of
// every byte by its ranges, and LG written once more.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_measure_core.hpp"

namespace {

constexpr sx::MeasureClg kClg = sx::measure_clg_table();

uint64_t ref_lg(uint64_t x) {
    int e = 0;
    while (x >> (e + 1)) e++;
    uint64_t m = x << (31 - e), f = 0;
    for (int k = 0; k < 16; k++) {
        m = m * m >> 31;
        f <<= 1;
        if (m >= (uint64_t)1 << 32) { f |= 1; m >>= 1; }
    }
    return (uint64_t)e << 16 | f;
}

uint64_t ref(const std::string& in) {
    const uint64_t n = in.size();
    if (!n) return 0;
    uint64_t c[256] = { 0 }, chars = 0, word = 0, distinct = 0, t = n * ref_lg(n);
    for (unsigned char b : in) {
        c[b]++;
        if (b < 0x80 || b > 0xBF) chars++;
        if (b >= 'a' && b <= 'z') word |= SX_MEASURE_LOWER;
        else if (b >= 'A' && b <= 'Z') word |= SX_MEASURE_UPPER;
        else if (b >= '0' && b <= '9') word |= SX_MEASURE_DIGIT;
        else if (b == 0x20 || b == 0x09) word |= SX_MEASURE_SPACE;
        else if (b >= 0x21 && b <= 0x7E) word |= SX_MEASURE_PUNCT;
        else if (b >= 0x80) word |= SX_MEASURE_HIGH;
        else word |= SX_MEASURE_CONTROL;
    }
    for (int b = 0; b < 256; b++)
        if (c[b]) { distinct++; t -= c[b] * ref_lg(c[b]); }
    const uint64_t ent = t / (16 * n) < 65535 ? t / (16 * n) : 65535;
    return word | ent | distinct << SX_MEASURE_DISTINCT_SHIFT | chars << SX_MEASURE_CHARS_SHIFT;
}

uint64_t cases = 0;

// `in` at `alignment`, by the narrow walk if a lane takes it and by the wide lanes in any case; false: a word differs, or counters are left
bool check(const std::string& in, uint32_t alignment) {
    cases++;
    const uint64_t want = ref(in);
    uint8_t* src = (uint8_t*)malloc(alignment + in.size() ? alignment + in.size() : 1);      // (malloc aligns to 16)
    uint8_t* cnt = (uint8_t*)calloc(256, 1);
    uint32_t* cnt32 = (uint32_t*)calloc(256, sizeof(uint32_t));
    if (!src || !cnt || !cnt32) return false;
    uint8_t* s = src + alignment;
    memcpy(s, in.data(), in.size());
    const uint32_t len = (uint32_t)in.size();
    bool ok = true;
    if (len <= sx::kMeasureNarrowMax) {
        const uint64_t got = sx::measure_narrow_string(s, len, cnt, 4, kClg.v);
        for (int b = 0; b < 256; b++) ok = ok && cnt[b] == 0;
        ok = ok && got == want;
    }
    sx::MeasureAcc a{ 0, 0 };
    uint64_t sum = 0;
    uint32_t distinct = 0;
    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) sx::measure_wide_count_lane(s, len, lane, cnt32, &a);
    for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) sx::measure_wide_finish_lane(cnt32, lane, kClg.v, &sum, &distinct);
    for (int b = 0; b < 256; b++) ok = ok && cnt32[b] == 0;
    ok = ok && sx::measure_finish(kClg.v, len, sum, distinct, a) == want && sx::measure_string_host(s, len, kClg.v) == want;
    if (!ok) printf("measure core: a string of %u bytes at alignment %u: want %016llx\n", len, alignment, (unsigned long long)want);
    free(src); free(cnt); free(cnt32);
    return ok;
}

// n bytes over an alphabet of `symbols` values, a function of (n, symbols, k): no random state
std::string made(uint32_t n, uint32_t symbols, uint32_t k) {
    std::string out(n, '\0');
    uint32_t x = n * 2654435761u + symbols * 40503u + k;
    for (uint32_t i = 0; i < n; i++) {
        x = x * 1664525u + 1013904223u;
        out[i] = (char)(symbols == 256 ? x >> 24 : symbols == 64 ? 0x30 + (x >> 24) % 64 : symbols == 16 ? "0123456789abcdef"[(x >> 24) % 16] : symbols == 2 ? "aB"[(x >> 24) % 2] : 0xC3);
    }
    return out;
}

}  // namespace

int main() {
    bool ok = true;
    for (uint32_t b = 0; b < 256; b++) ok = check(std::string(1, (char)b), b % 8) && ok;
    const uint32_t alphabets[] = { 1, 2, 16, 64, 256 };
    for (uint32_t n = 0; n <= 300; n++)
        for (uint32_t a : alphabets)
            for (uint32_t alignment = 0; alignment < 8; alignment++) ok = check(made(n, a, alignment), alignment) && ok;
    for (uint32_t n : { 255u, 256u, 257u }) {
        std::string beside(n, 'x');
        for (uint32_t b = 0; b < 255; b++) beside += (char)(b < 'x' ? b : b + 1);
        ok = check(std::string(n, 'x'), n % 8) && check(beside, (n + 3) % 8) && ok;
    }
    for (uint32_t k : { 1u, 2u, 3u, 255u, 256u, 257u }) {
        std::string all;
        for (uint32_t i = 0; i < k; i++)
            for (uint32_t b = 0; b < 256; b++) all += (char)b;
        ok = check(all, k % 8) && ok;
    }
    for (uint32_t n : { 65535u, 65536u, 65537u, 1u << 20 }) ok = check(made(n, 64, 1), 1) && check(std::string(n, '7'), 5) && ok;
    const struct { const char* s; uint64_t ent, distinct; } known[] = { { "aaaa", 0, 1 }, { "abab", 4096, 2 }, { "0123456789abcdef", 16384, 16 } };
    for (const auto& k : known) {
        const uint64_t w = sx::measure_string_host((const uint8_t*)k.s, (uint32_t)strlen(k.s), kClg.v);
        ok = ok && (w & 0xFFFF) == k.ent && (w >> SX_MEASURE_DISTINCT_SHIFT & 0x1FF) == k.distinct && w >> SX_MEASURE_CHARS_SHIFT == strlen(k.s);
    }
    if (!ok) { printf("measure core: FAILED\n"); return 1; }
    printf("measure core: ok, %llu strings\n", (unsigned long long)cases);
    return 0;
}
