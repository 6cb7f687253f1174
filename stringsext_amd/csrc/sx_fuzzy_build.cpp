// sx_fuzzy_build.cpp — see sx_fuzzy_build.hpp.  The checks, one count per (folded) byte value, the classes in the order of those
// counts, and a bit per pattern position.
#include "sx_fuzzy_build.hpp"

#include <algorithm>
#include <new>

namespace sx {

namespace {

int fail(std::string* err, const std::string& what) { if (err) *err = what; return SX_E_INVALID; }
uint32_t folded(bool nocase, uint32_t x) { return nocase && x - 'A' < 26u ? x | 0x20u : x; }

}  // namespace

int fuzzy_build(const sx_pattern* patterns, const uint8_t* max_errors, uint32_t n_patterns, uint32_t flags, FuzzyTable* out, std::string* err) {
    if (!patterns || !max_errors || !out) return fail(err, "a NULL pointer");
    if (n_patterns < 1 || n_patterns > SX_FUZZY_MAX_PATTERNS) return fail(err, "n_patterns must be 1..64");
    if (flags & ~(uint32_t)SX_SELECT_ASCII_NOCASE) return fail(err, "a fuzzy set takes SX_SELECT_ASCII_NOCASE and no other flag");
    for (uint32_t p = 0; p < n_patterns; p++) {
        const std::string at = "pattern " + std::to_string(p) + ": ";
        const uint32_t len = patterns[p].len, k = max_errors[p];
        if (len < 1 || !patterns[p].bytes) return fail(err, at + "an empty pattern");
        if (len > SX_FUZZY_MAX_PATTERN_BYTES) return fail(err, at + std::to_string(len) + " bytes, and a pattern has at most 64");
        if (k > SX_FUZZY_MAX_ERRORS) return fail(err, at + std::to_string(k) + " errors, and a budget is at most 8");
        if (k >= len) return fail(err, at + std::to_string(k) + " errors for " + std::to_string(len) + " bytes: the budget must be smaller than the length");
    }
    const bool nocase = (flags & SX_SELECT_ASCII_NOCASE) != 0;
    try {
        FuzzyTable T;
        T.n_patterns = n_patterns; T.nocase = nocase ? 1u : 0u;
        uint32_t held[256] = {};      // pattern positions that hold the (folded) value
        for (uint32_t p = 0; p < n_patterns; p++) {
            for (uint32_t j = 0; j < patterns[p].len; j++) held[folded(nocase, patterns[p].bytes[j])]++;
            T.lenk[p] = patterns[p].len | (uint32_t)max_errors[p] << 8;
            T.max_len = std::max(T.max_len, patterns[p].len);
            T.max_errors = std::max(T.max_errors, (uint32_t)max_errors[p]);
        }
        std::vector<uint32_t> values;
        for (uint32_t x = 0; x < 256; x++) if (held[x]) values.push_back(x);
        std::stable_sort(values.begin(), values.end(), [&](uint32_t a, uint32_t b) { return held[a] > held[b]; });
        T.classes = (uint32_t)values.size() + 1;
        for (uint32_t c = 0; c < values.size(); c++) T.map[values[c]] = (uint16_t)(c + 1);
        for (uint32_t x = 0; x < 256; x++) T.map[x] = T.map[folded(nocase, x)];
        T.lds_classes = std::min(T.classes, kSelsetLdsBytes / (n_patterns * 8u));
        T.eq.assign((size_t)T.classes * n_patterns, 0);
        for (uint32_t p = 0; p < n_patterns; p++)
            for (uint32_t j = 0; j < patterns[p].len; j++) T.eq[(size_t)T.map[patterns[p].bytes[j]] * n_patterns + p] |= (uint64_t)1 << j;
        *out = std::move(T);
    } catch (const std::bad_alloc&) {
        if (err) *err = "no host memory for the fuzzy set's table";
        return SX_E_NOMEM;
    }
    return SX_OK;
}

}  // namespace sx
