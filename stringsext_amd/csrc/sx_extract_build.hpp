// sx_extract_build.hpp — a list of byte regular expressions compiled into the table that the extraction kernels walk
// (sx_extract_regex_create): the front end of sx_selre_build.cpp (sx_selre_front.hpp: the same parser, the same count of positions, the
// same NFA — so the same language, refusals, limits and texts), then that header's subset construction with a Rule of its own.  Host only, no HIP header:
// the test-only harness tests/native/extract_core_host.cpp compiles it with g++ (tests/test_extract_core.py).
//
// The question is "where do the matches lie", as `grep -oE` answers it: at an offset o the longest e such that some pattern matches
// exactly s[o, e).  So the automaton is ANCHORED — no pattern is re-entered in front of later bytes; the walk restarts instead — and
// it has two start states: the closure of the NFA's start with the `^` edges (start0: a walk that begins at offset 0) and without
// them (start1: every later offset); they may be one state.  A state says what the bytes read since the start allow:
//   here — a match may end here, whatever follows;
//   end  — a match may end here only if the string ends here (through `$`);
//   dead — no match can end at this or any later byte: the walk from this start is over.  A byte that cannot begin a match leads
//          from the start state to `dead` at once.
// The minimisation begins with the partition none / end / here (`dead` is the one `none` state that every byte leads back to) and
// merges the byte classes whose columns are equal.  Numbering: breadth first from start0, then start1 (classes in ascending order),
// so the shallow rows, which most bytes visit, lie first — the kernels keep the first lds_states rows in LDS —, and the kinds in
// ranges, breadth first among themselves, so that a kind is one compare:
//   [0, end_first) none | [end_first, here_first) end | [here_first, dead_first) here | [dead_first, states) dead (one or none)
// The start states are of the kind none — a match is never empty, so what may end in front of a walk's first byte does not count — and
// have numbers in that range.  Row layout: next[state * classes + class], 2 bytes an entry.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"
#include "sx_selset_build.hpp"

namespace sx {

struct ExtractTable {
    uint32_t n_patterns = 0, states = 0, classes = 0, nocase = 0;
    uint32_t lds_states = 0;     // min(states, kSelsetLdsBytes / (classes * 2))
    uint32_t end_first = 0, here_first = 0, dead_first = 0;
    uint32_t start0 = 0, start1 = 0;
    uint8_t map[256] = {};       // byte -> class
    std::vector<uint16_t> next;  // states * classes entries
};

// SX_OK; SX_E_INVALID with *err said, for what selre_build refuses and in its words — a bad count, length, pointer or flag, a refused
// pattern ("pattern P, offset O: why"), or a limit passed: SX_SELECT_REGEX_MAX_REPEAT, _MAX_POSITIONS, _MAX_STATES (the subset
// construction stops at the first state above it), or the bound on the construction's memory (32 Mi NFA positions in all its states) —;
// SX_E_NOMEM if the host has no memory for the table.
int extract_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, ExtractTable* out, std::string* err);

}  // namespace sx
