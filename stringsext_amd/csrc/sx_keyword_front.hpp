// sx_keyword_front.hpp — what the two keyword builders share (sx_selset_build.cpp: "does a keyword occur in the string";
// sx_seltally_build.cpp: "which keywords occur, how often"), host only and internal to them: the argument checks, the ASCII fold,
// the byte classes and the trie over the (folded) keywords with its children as sibling lists.  Both builders refuse the same
// lists with the same texts because they are these functions; their breadth-first walks over the trie are their own.  No HIP
// header: the test-only harnesses compile it with g++.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"

namespace sx {
namespace kwfront {

struct TrieNode { uint32_t child, sibling; uint8_t cls, ends; };   // child / sibling: 0 = none (the root is nobody's child)

inline int fail(std::string* err, const std::string& what) { if (err) *err = what; return SX_E_INVALID; }

inline uint32_t folded(bool nocase, uint32_t x) { return nocase && x - 'A' < 26u ? x | 0x20u : x; }

// kind: "pattern set" / "tally set", for the one text that names it; *total = the patterns' bytes
inline int check(const char* kind, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, const void* out, uint64_t* total, std::string* err) {
    if (!patterns || !out) return fail(err, "a NULL pointer");
    if (n_patterns < 1 || n_patterns > SX_SELECT_SET_MAX_PATTERNS) return fail(err, "n_patterns must be 1..65536");
    if (flags & ~(uint32_t)SX_SELECT_ASCII_NOCASE) return fail(err, std::string("a ") + kind + " takes SX_SELECT_ASCII_NOCASE and no other flag");
    *total = 0;
    for (uint32_t p = 0; p < n_patterns; p++) {
        if (!patterns[p].bytes || patterns[p].len < 1 || patterns[p].len > SX_SELECT_SET_MAX_PATTERN_BYTES) return fail(err, "a pattern must have 1..255 bytes");
        *total += patterns[p].len;
    }
    if (*total > SX_SELECT_SET_MAX_TOTAL_BYTES) return fail(err, "the patterns' lengths must sum to at most 1 MiB");
    return SX_OK;
}

// The byte classes: one per (folded) byte that occurs in a keyword, class 0 for all the others if there are any; returns their number
inline uint32_t classes(const sx_pattern* patterns, uint32_t n_patterns, bool nocase, uint8_t map[256]) {
    bool used[256] = {};
    for (uint32_t p = 0; p < n_patterns; p++)
        for (uint32_t j = 0; j < patterns[p].len; j++) used[folded(nocase, patterns[p].bytes[j])] = true;
    bool any_unused = false;
    for (uint32_t x = 0; x < 256; x++) any_unused |= !used[folded(nocase, x)];
    uint32_t n = any_unused ? 1u : 0u;
    for (uint32_t x = 0; x < 256; x++) if (used[x]) map[x] = (uint8_t)n++;
    for (uint32_t x = 0; x < 256; x++) if (!used[x]) map[x] = used[folded(nocase, x)] ? map[folded(nocase, x)] : 0;
    return n;
}

// The trie: a node per distinct prefix, node 0 the root.  cut_at_ends: nothing is kept below the end of a keyword (a longer one
// ends where the shorter one does); ends_at: NULL, or per pattern the node it ends in
inline std::vector<TrieNode> trie(const sx_pattern* patterns, uint32_t n_patterns, const uint8_t map[256], uint64_t total, bool cut_at_ends,
                                  std::vector<uint32_t>* ends_at) {
    std::vector<TrieNode> t;
    t.reserve((size_t)total + 1);
    t.push_back(TrieNode{ 0, 0, 0, 0 });
    if (ends_at) ends_at->assign(n_patterns, 0);
    for (uint32_t p = 0; p < n_patterns; p++) {
        uint32_t u = 0;
        for (uint32_t j = 0; j < patterns[p].len && !(cut_at_ends && t[u].ends); j++) {
            const uint8_t c = map[patterns[p].bytes[j]];
            uint32_t v = t[u].child;
            while (v && t[v].cls != c) v = t[v].sibling;
            if (!v) {
                v = (uint32_t)t.size();
                t.push_back(TrieNode{ 0, t[u].child, c, 0 });
                t[u].child = v;
            }
            u = v;
        }
        t[u].ends = 1;
        if (ends_at) (*ends_at)[p] = u;
    }
    return t;
}

}  // namespace kwfront
}  // namespace sx
