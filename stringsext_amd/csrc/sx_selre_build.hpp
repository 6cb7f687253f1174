// sx_selre_build.hpp — a list of byte regular expressions compiled into the table that selre_match_kernel walks
// (sx_select_regex_create): parser, Thompson NFA with the counted repeats unrolled, subset construction for an unanchored search,
// minimisation, all on the host.  No HIP header here or in sx_selre_build.cpp: the test-only harness
// tests/native/selre_core_host.cpp compiles both with g++ (tests/test_selre_core.py).  The pattern language is the one
// include/stringsext_amd.h sets out; Python's `re` with a bytes pattern, `$` read as `\Z`, is its oracle.
//
// Only "does any pattern match somewhere in this string" is asked, so the automaton is the minimal DFA of the language
// { s : some pattern matches in s }: the root re-enters every pattern in front of every byte (without the `^` edges: those are
// taken in front of the first byte only), and a state accepts if the string may END there.  Two kinds of state let a lane stop
// before its string ends, and the minimisation leaves at most one of each: `matched` — accepting, every byte leads back to it:
// whatever follows, the string is selected (a pattern without `$` has matched) — and `dead` — not accepting, every byte leads back
// to it: nothing that follows can match (`^abc` after a mismatch).  Every other accepting state selects a string only if it ends
// there (`$`).
//
// Numbering: the root is 0; the states that neither accept nor are `dead` follow breadth first (classes in ascending order), so
// the shallow rows, which most bytes visit, lie first — the kernel keeps the first lds_states rows in LDS —; behind them the
// end-accepting states, breadth first among themselves, then `dead`, then `matched`, where they exist:
//   [0, end_first) ordinary | [end_first, stop_first) end-accepting | [stop_first, states) dead, matched
// The root keeps number 0 whatever it is; root_end says that it accepts at the end (`^$`), and a root that is `matched` (`a*`) or
// `dead` (`a^b`) is the only state (stop_first == 0).  A byte is looked up as its class: the bytes whose columns are equal in every
// state share one.  Row layout: next[state * classes + class], 2 bytes an entry.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"
#include "sx_selset_build.hpp"

namespace sx {

constexpr uint32_t kSelreNone = 0xFFFFFFFFu;       // `matched` where no state is

struct SelreTable {
    uint32_t n_patterns = 0, states = 0, classes = 0, nocase = 0;
    uint32_t lds_states = 0;     // min(states, kSelsetLdsBytes / (classes * 2))
    uint32_t end_first = 0;      // the first end-accepting state behind the root (== stop_first: none)
    uint32_t stop_first = 0;     // a lane in a state >= stop_first is done
    uint32_t matched = kSelreNone;
    uint32_t root_end = 0;       // the root accepts at the end of the string
    uint32_t end_states = 0;     // stop_first - end_first + root_end
    uint8_t map[256] = {};       // byte -> class
    std::vector<uint16_t> next;  // states * classes entries
};

// SX_OK; SX_E_INVALID with *err said — a bad count, length, pointer or flag, a refused pattern ("pattern P, offset O: why"), or a
// limit passed: SX_SELECT_REGEX_MAX_REPEAT, _MAX_POSITIONS (counted before anything is unrolled), _MAX_STATES (the subset
// construction stops at the first state above it), or the bound on the construction's memory (its states, kept as sorted lists of
// NFA positions, hold more than 32 Mi of them in all: an unanchored a{51000}, whose k-th state holds k) —; SX_E_NOMEM if the host
// has no memory for the table.
int selre_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SelreTable* out, std::string* err);

}  // namespace sx
