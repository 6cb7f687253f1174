// Test-only program: compiles the lane functions of sx_result_fuzzy_device (sx_fuzzy_core.hpp) and the set's builder
// (sx_fuzzy_build.cpp) as host code and runs them under the address and undefined-behaviour sanitizers (tests/test_fuzzy_core.py builds
// it so).  Every string lies in an allocation of its own that ENDS where the string ends and begins `alignment` (0 .. 7) bytes in
// front of it: a byte read outside is the sanitizer's finding.  Every word is compared with Sellers' table, written out plainly
// below; sets whose patterns have at most 32 bytes run in 32-bit AND in 64-bit words.  The builder's class order and LDS share are
// checked on the tables themselves.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_fuzzy_build.cpp"
#include "../../stringsext_amd/csrc/sx_fuzzy_core.hpp"

namespace {

uint8_t fold(bool nocase, uint8_t x) { return nocase && x >= 'A' && x <= 'Z' ? x | 0x20 : x; }

// min_j D[m][j] of Sellers' table
uint32_t ref_distance(const std::string& p, const std::string& t, bool nocase) {
    const size_t m = p.size();
    std::vector<uint32_t> prev(m + 1), cur(m + 1);
    for (size_t i = 0; i <= m; i++) prev[i] = (uint32_t)i;
    uint32_t best = prev[m];
    for (unsigned char c : t) {
        cur[0] = 0;
        for (size_t i = 1; i <= m; i++)
            cur[i] = std::min({ prev[i - 1] + (fold(nocase, (uint8_t)p[i - 1]) != fold(nocase, c) ? 1u : 0u), prev[i] + 1u, cur[i - 1] + 1u });
        best = std::min(best, cur[m]);
        prev.swap(cur);
    }
    return best;
}

uint64_t cases = 0;

struct Set {
    std::vector<std::string> patterns;
    std::vector<uint8_t> ks;
    bool nocase = false;
    sx::FuzzyTable T;
    bool build() {
        std::vector<sx_pattern> raw;
        for (const std::string& p : patterns) raw.push_back(sx_pattern{ (const uint8_t*)p.data(), (uint32_t)p.size() });
        std::string err;
        return sx::fuzzy_build(raw.data(), ks.data(), (uint32_t)raw.size(), nocase ? SX_SELECT_ASCII_NOCASE : 0, &T, &err) == SX_OK;
    }
    sx::FuzzyDevice dev() const { return sx::FuzzyDevice{ T.map, T.eq.data(), T.lenk, nullptr, nullptr, T.n_patterns, T.classes, T.lds_classes, T.max_len }; }
};

// `in` at `alignment` for the set: the lane functions' word, in every width the set may take, against the table
bool check(const Set& S, const std::string& in, uint32_t alignment) {
    cases++;
    uint64_t want = 0;
    for (size_t p = 0; p < S.patterns.size(); p++)
        if (ref_distance(S.patterns[p], in, S.nocase) <= S.ks[p]) want |= (uint64_t)1 << p;
    uint8_t* src = (uint8_t*)malloc(alignment + in.size() ? alignment + in.size() : 1);      // (malloc aligns to 16)
    if (!src) return false;
    uint8_t* s = src + alignment;
    memcpy(s, in.data(), in.size());
    const sx::FuzzyDevice D = S.dev();
    const uint32_t len = (uint32_t)in.size();
    bool ok = sx::fuzzy_string<uint64_t>(D, D.map, D.eq, s, len) == want && sx::fuzzy_string_host(D, s, len) == want;
    if (S.T.max_len <= 32) ok = ok && sx::fuzzy_string<uint32_t>(D, D.map, D.eq, s, len) == want;
    if (!ok) printf("fuzzy core: %zu patterns, a string of %u bytes at alignment %u: want %016llx, got %016llx\n", S.patterns.size(), len, alignment,
                    (unsigned long long)want, (unsigned long long)sx::fuzzy_string_host(D, s, len));
    free(src);
    return ok;
}

uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

// n bytes over an alphabet of `symbols` values (256: every byte value), a function of (n, symbols, seed)
std::string made(uint32_t n, uint32_t symbols, uint32_t seed) {
    std::string out(n, '\0');
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t x = mix(seed * 1000003u + i * 7u + n) % symbols;
        out[i] = (char)(symbols == 256 ? x : symbols == 26 ? 'a' + x : "acgt"[x]);
    }
    return out;
}

// p with e edits at e different places, the first and the last byte among them where e >= 2: kind 0 another value, 1 a byte put in,
// 2 the byte dropped
std::string edited(const std::string& p, uint32_t e, uint32_t seed, int only = -1) {
    const uint32_t m = (uint32_t)p.size();
    std::vector<bool> at(m, false);
    if (e >= 1) at[seed % 2 && e == 1 ? m - 1 : 0] = true;
    if (e >= 2) at[m - 1] = true;
    for (uint32_t have = e < 2 ? e : 2, j = 0; have < e; j++) {
        const uint32_t x = mix(seed + 31u * j) % m;
        if (!at[x]) { at[x] = true; have++; }
    }
    std::string out;
    for (uint32_t i = 0; i < m; i++) {
        if (!at[i]) { out += p[i]; continue; }
        const uint32_t kind = only >= 0 ? (uint32_t)only : mix(seed + i) % 3;
        const char other = (char)((uint8_t)p[i] + 1u + mix(seed + 5u * i) % 255u);
        if (kind == 0) out += other;
        else if (kind == 1) { if (i + 1 < m) { out += p[i]; out += other; } else { out += other; out += p[i]; } }
    }
    return out;
}

bool one_pattern_cases() {
    bool ok = true;
    const uint32_t lengths[] = { 1, 2, 3, 31, 32, 33, 63, 64 }, alphabets[] = { 2, 4, 26, 256 };
    for (uint32_t m : lengths)
        for (uint32_t a : alphabets)
            for (uint32_t k = 0; k <= SX_FUZZY_MAX_ERRORS && k < m; k++) {
                Set S;
                S.patterns = { made(m, a, m + a) }; S.ks = { (uint8_t)k };
                if (!S.build()) return false;
                const std::string& p = S.patterns[0];
                uint32_t al = m + k;
                // the texts' lengths: 0, len - k - 1, len - k, len, long; prefixes of the pattern and other text
                for (uint32_t n : { 0u, m - k - 1, m - k, m, 300u }) {
                    ok = check(S, p.substr(0, std::min(n, m)) + made(n > m ? n - m : 0, a, n), al++ % 8) && ok;
                    ok = check(S, made(n, a, n + 1), al++ % 8) && ok;
                }
                // variants at k and k + 1 errors (and every kind alone at the first and the last byte) at the head, in the middle, as the tail
                for (uint32_t e : { 0u, 1u, k, k + 1 }) {
                    if (e > m) continue;
                    for (int only = -1; only < (e == 1 ? 3 : 0); only++)
                        for (uint32_t seed = 0; seed < 2; seed++) {
                            const std::string v = edited(p, e, seed + 2 * k, only), fill = made(40, a, seed + e);
                            ok = check(S, v + fill, al++ % 8) && check(S, fill + v + fill, al++ % 8) && check(S, fill + v, al++ % 8) && check(S, v, al++ % 8) && ok;
                        }
                }
            }
    return ok;
}

bool set_cases() {
    bool ok = true;
    // 1, G - 1, G, G + 1 patterns for both groups, and 64: a group's boundary and bit 63; short patterns take the 32-bit words too
    for (uint32_t longest : { 12u, 40u })
        for (uint32_t n : { 1u, sx::kFuzzyGroup64 - 1, sx::kFuzzyGroup64, sx::kFuzzyGroup64 + 1, sx::kFuzzyGroup32 - 1, sx::kFuzzyGroup32, sx::kFuzzyGroup32 + 1, 63u, 64u })
            for (int nocase = 0; nocase < 2; nocase++) {
                Set S;
                S.nocase = nocase != 0;
                for (uint32_t p = 0; p < n; p++) {
                    const uint32_t m = 2 + (p * 7 + n) % (longest - 1);
                    std::string pat = made(m, 26, p + 100 * n);
                    if (nocase && p % 2) for (char& c : pat) c = (char)(c - 0x20);
                    S.patterns.push_back(pat);
                    S.ks.push_back((uint8_t)std::min(m - 1, p % 4));
                }
                if (!S.build()) return false;
                for (uint32_t t = 0; t < 40; t++) {
                    // a few of the set's patterns, edited, in text; every third text in the other case
                    std::string in = made(t % 9, 26, t);
                    for (uint32_t j = 0; j < 1 + t % 3; j++) {
                        const uint32_t p = mix(t * 13 + j) % n;
                        in += edited(S.patterns[p], std::min((uint32_t)S.patterns[p].size(), mix(t + j) % 4), t) + made(3 + j, 26, t + j);
                    }
                    if (t % 3 == 0) for (char& c : in) if (c >= 'a' && c <= 'z') c = (char)(c - 0x20);
                    ok = check(S, in, t % 8) && ok;
                }
                ok = check(S, "", 0) && ok;
            }
    return ok;
}

// The builder's tables: class 0 holds no pattern byte, the others are ordered by how many pattern positions hold them, the masks are
// the patterns', and a set of many distinct bytes keeps only the first classes in LDS
bool table_cases() {
    Set S;
    for (uint32_t p = 0; p < 64; p++) {
        std::string pat(64, '\0');
        for (uint32_t i = 0; i < 64; i++) pat[i] = (char)(1 + (p * 64 + i * 37 + p * p) % 255);
        S.patterns.push_back(pat);
        S.ks.push_back((uint8_t)(p % 9));
    }
    if (!S.build()) return false;
    const sx::FuzzyTable& T = S.T;
    bool ok = T.classes == 256 && T.lds_classes == sx::kSelsetLdsBytes / (64 * 8) && T.lds_classes < T.classes && T.max_len == 64 && T.max_errors == 8 && T.map[0] == 0;
    std::vector<uint32_t> held(T.classes, 0);
    for (uint32_t c = 0; c < T.classes; c++)
        for (uint32_t p = 0; p < 64; p++) held[c] += (uint32_t)__builtin_popcountll(T.eq[c * 64 + p]);
    ok = ok && held[0] == 0;
    for (uint32_t c = 2; c < T.classes; c++) ok = ok && held[c - 1] >= held[c] && held[c] > 0;
    for (uint32_t p = 0; p < 64; p++)
        for (uint32_t i = 0; i < 64; i++) ok = ok && (T.eq[T.map[(uint8_t)S.patterns[p][i]] * 64 + p] >> i & 1);
    uint64_t bits = 0;
    for (uint64_t w : T.eq) bits += (uint64_t)__builtin_popcountll(w);
    ok = ok && bits == 64 * 64;
    // strings that walk the rows beyond the LDS share
    for (uint32_t t = 0; t < 30; t++)
        ok = check(S, made(t, 256, t) + edited(S.patterns[(t * 5) % 64], t % 10, t) + made(t % 7, 256, t + 1), t % 8) && ok;
    // the case union: a letter's two bytes are one class, no other byte is folded
    Set N;
    N.nocase = true; N.patterns = { "aAbZ[" }; N.ks = { 1 };
    if (!N.build()) return false;
    ok = ok && N.T.classes == 5 && N.T.map['a'] == N.T.map['A'] && N.T.map['a'] == 1 && N.T.map['z'] == N.T.map['Z'] && N.T.map['['] != N.T.map['{'] && N.T.map['{'] == 0;
    if (!ok) printf("fuzzy core: the builder's tables\n");
    return ok;
}

}  // namespace

int main() {
    bool ok = one_pattern_cases();
    ok = set_cases() && ok;
    ok = table_cases() && ok;
    if (!ok) { printf("fuzzy core: FAILED\n"); return 1; }
    printf("fuzzy core: ok, %llu strings\n", (unsigned long long)cases);
    return 0;
}
