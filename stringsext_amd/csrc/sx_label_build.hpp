// sx_label_build.hpp — a list of byte regular expressions compiled into the table that label_match_kernel walks
// (sx_label_set_create): the regex set's parser, position count and NFA (sx_selre_front.hpp, every pattern with an accept node of
// its own), the subset construction for an unanchored search, minimisation, all on the host.  No HIP header here or in
// sx_label_build.cpp: the test-only harness tests/native/label_core_host.cpp compiles both with g++ (tests/test_label_core.py).
// The language, the refusals, the limits and the error texts are the regex set's (sx_selre_build.hpp); Python's `re` with a bytes
// pattern, `$` read as `\Z`, is the oracle.
//
// What is asked is "WHICH patterns match somewhere in this string", so a state carries two 64-bit masks where the regex set's
// carries two booleans: `here` — the patterns whose accept is reached with the byte that led here, whatever follows — and `end` —
// the patterns whose accept is reached only if the string ends here (`$`).  The root re-enters every pattern in front of every byte
// (without the `^` edges: those are taken in front of the first byte only).  There is no `matched` state: a pattern that has
// matched says nothing about the others, so nothing absorbs — and a label set reaches SX_SELECT_REGEX_MAX_STATES sooner than a regex
// set of the same patterns, whose subsets all collapse into `matched` once any pattern has matched.  `dead` — here == end == 0 and
// every byte leads back to it — exists only where it falls out: every pattern anchored and the walk off all of them.
//
// Numbering: the root is 0, whatever its masks are (root_here holds its `here`); the other states with here == 0 follow breadth
// first (classes in ascending order), so the shallow rows, which most bytes visit, lie first — the kernel keeps the first lds_states
// rows in LDS —; behind them the states with here != 0, breadth first among themselves, so that "this step ended a match" is one
// compare, state >= here_first; `dead`, if there is one and it is not the root, is last.
//   [0, here_first) here == 0 | [here_first, states) here != 0, then dead
// Tables: next[state * classes + class], 2 bytes an entry; here[state - here_first] (dead's entry is 0) and end[state], 64-bit words.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"
#include "sx_selset_build.hpp"

namespace sx {

constexpr uint32_t kLabelNone = 0xFFFFFFFFu;       // `dead` where no state is

struct LabelTable {
    uint32_t n_patterns = 0, states = 0, classes = 0, nocase = 0;
    uint32_t lds_states = 0;     // min(states, kSelsetLdsBytes / (classes * 2))
    uint32_t here_first = 0;     // the first state with here != 0 behind the root (== states: none)
    uint32_t dead = kLabelNone;  // a lane in this state is done
    uint64_t root_here = 0;      // the root's `here`: what a lane's label starts as (`a*`, `^`)
    uint64_t all = 0;            // bits [0, n_patterns)
    uint8_t map[256] = {};       // byte -> class
    std::vector<uint16_t> next;  // states * classes entries
    std::vector<uint64_t> here;  // states - here_first entries
    std::vector<uint64_t> end;   // states entries
};

// SX_OK; SX_E_INVALID with *err said — selre_build's cases with selre_build's texts: a bad count, length, pointer or flag, a refused
// pattern ("pattern P, offset O: why"), or a limit passed: SX_SELECT_REGEX_MAX_REPEAT, _MAX_POSITIONS, _MAX_STATES (the subset
// construction stops at the first state above it; see above for why that comes sooner here), or the bound on the construction's
// memory —; SX_E_NOMEM if the host has no memory for the table.
int label_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, LabelTable* out, std::string* err);

}  // namespace sx
