// sx_selset_build.hpp — a keyword list compiled into the table that selset_match_kernel walks (sx_select_set_create): Aho-Corasick
// made into a full DFA, built on the host.  No HIP header here or in sx_selset_build.cpp: the test-only harness
// tests/native/selset_core_host.cpp compiles both with g++ (tests/test_selset_core.py).
//
// Only "does any keyword occur in this string" is asked, so every state whose own path or failure chain ends a keyword is ONE
// absorbing state, `matched`, and nothing below such a state exists.  The states are numbered breadth first — the root is 0, the
// shallow states, which most text bytes visit, come first and lie together (the kernel keeps the first lds_states rows in LDS) —
// and `matched` is the last one.  A byte is looked up as its class: the bytes that occur in no keyword share class 0, every other
// byte has a class of its own, and with SX_SELECT_ASCII_NOCASE 'A'..'Z' have the class of 'a'..'z' (the keywords are folded
// first), so the walk folds nothing.  Row layout: next[state * classes + class], 2 bytes an entry while states <= 65536, else 4.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"

namespace sx {

constexpr uint32_t kSelsetLdsBytes = 48 * 1024;   // the rows selset_match_kernel keeps in LDS: three workgroups of it fit a CU's 160 KiB

struct SelsetTable {
    uint32_t n_patterns = 0, states = 0, classes = 0, nocase = 0;
    uint32_t entry_bytes = 0;    // 2 or 4
    uint32_t lds_states = 0;     // min(states, kSelsetLdsBytes / (classes * entry_bytes))
    uint32_t matched = 0;        // == states - 1
    uint8_t map[256] = {};       // byte -> class
    std::vector<uint8_t> next;   // states * classes entries
};

// SX_OK, or SX_E_INVALID with *err said (n_patterns outside 1..SX_SELECT_SET_MAX_PATTERNS, a len outside
// 1..SX_SELECT_SET_MAX_PATTERN_BYTES, a total above SX_SELECT_SET_MAX_TOTAL_BYTES, a NULL pointer, a flag other than
// SX_SELECT_ASCII_NOCASE), or SX_E_NOMEM if the host has no memory for the table.
int selset_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SelsetTable* out, std::string* err);

}  // namespace sx
