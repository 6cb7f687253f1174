// sx_seltally_build.hpp — a keyword list compiled into the tables that seltally_kernel walks (sx_tally_set_create): the Aho-Corasick
// automaton of sx_selset_build.hpp, NOT collapsed and with output links, built on the host.  No HIP header here or in
// sx_seltally_build.cpp: the test-only harness tests/native/seltally_core_host.cpp compiles both with g++ (tests/test_seltally_core.py).
//
// "Which keywords occur, how often, where first" is asked, so nothing is cut below a keyword's end: the states are exactly the
// distinct prefixes of the (folded) keywords, the empty one — the root, state 0 — included.  They are numbered breadth first, so the
// shallow states, which most text bytes visit, come first and lie together (the kernel keeps the first lds_states rows in LDS).  The
// byte classes are sx_selset_build.hpp's: the bytes that occur in no keyword share class 0, every other byte has a class of its own,
// and with SX_SELECT_ASCII_NOCASE 'A'..'Z' have the class of 'a'..'z' (the keywords are folded first), so the walk folds nothing.
//
// Keywords that are equal after the fold are ONE unique keyword; the unique ids are numbered in the order of the states they end in,
// so the short keywords — the ones that can occur often — have the small ids (the kernel counts the ids below kSeltallyLdsIds in LDS).
// Per state: own[state] = the unique id of the keyword that ends exactly there, or kSeltallyNone; dict[state] = the nearest state
// on the failure chain that has an own, or 0 for none (the root ends nothing).  The keywords that end where a walk stands in state t
// are own[t], own[dict[t]], own[dict[dict[t]]], ... until dict gives 0.
// Row layout: next[state * classes + class], an entry = the target state with, in its top bit, "the target or its dictionary chain
// ends a keyword": a step that ends nothing costs one look-up and one test.  2 bytes an entry while states <= 32768, else 4.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"

namespace sx {

// seltally_kernel's LDS, per workgroup: the class map (256 bytes), kSeltallyLdsBytes of rows and kSeltallyLdsIds 32-bit counters —
// 49 408 bytes, so three workgroups fit a CU's 160 KiB.  lds_states is min(states, kSeltallyLdsBytes / (classes * entry_bytes)):
// the rows that fit the kernel's share for ROWS, not the whole budget.
constexpr uint32_t kSeltallyLdsBytes = 32 * 1024;
constexpr uint32_t kSeltallyLdsIds = 4096;
constexpr uint32_t kSeltallyNone = 0xFFFFFFFFu;

struct SeltallyTable {
    uint32_t n_patterns = 0, unique = 0, states = 0, classes = 0, nocase = 0;
    uint32_t entry_bytes = 0;    // 2 or 4
    uint32_t lds_states = 0;
    uint8_t map[256] = {};       // byte -> class
    std::vector<uint8_t> next;   // states * classes entries
    std::vector<uint32_t> own, dict;            // per state
    std::vector<uint32_t> unique_of_pattern;    // per input pattern
};

// SX_OK, or SX_E_INVALID with *err said (the cases of selset_build, word for word), or SX_E_NOMEM if the host has no memory for the tables.
int seltally_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SeltallyTable* out, std::string* err);

}  // namespace sx
