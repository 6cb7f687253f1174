// sx_fuzzy_build.hpp — a list of byte strings, each with an error budget, compiled into the masks that fuzzy_match_kernel reads
// (sx_fuzzy_set_create, sx_fuzzy_bytes): all on the host.  No HIP header here or in sx_fuzzy_build.cpp: the test-only harness
// tests/native/fuzzy_core_host.cpp compiles both with g++ (tests/test_fuzzy_core.py).
//
// The byte classes, as the regex builders have them: class 0 is "no pattern holds this byte" — its masks are all zero, the kernel
// does not look them up —; the other classes are the distinct byte values of the patterns, with SX_SELECT_ASCII_NOCASE after 'A'..'Z'
// and 'a'..'z' became one value each (a letter's two bytes map to the same class).  The classes are ordered by how many pattern
// positions hold them, descending (among equals: by the byte's value, a letter's being its lower-case one): the kernel keeps the rows
// of the first lds_classes classes in LDS — kSelsetLdsBytes of them, the label set's budget — and reads the rarest through L2, so no
// set is refused for its size: 64 patterns x 257 classes x 8 bytes = 131 584 bytes at most.
// Tables: map[byte] (2 bytes an entry: there may be 257 classes), eq[class * n_patterns + p] — bit i is set iff byte i of pattern p is
// of that class —, lenk[p] = len_p | k_p << 8.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"
#include "sx_selset_build.hpp"

namespace sx {

struct FuzzyTable {
    uint32_t n_patterns = 0, classes = 0, nocase = 0;
    uint32_t lds_classes = 0;    // min(classes, kSelsetLdsBytes / (n_patterns * 8))
    uint32_t max_len = 0, max_errors = 0;      // the longest pattern, the largest budget
    uint16_t map[256] = {};      // byte -> class
    std::vector<uint64_t> eq;    // classes * n_patterns words
    uint32_t lenk[SX_FUZZY_MAX_PATTERNS] = {};
};

// SX_OK; SX_E_INVALID with *err said: a NULL pointer, "n_patterns must be 1..64", a flag other than SX_SELECT_ASCII_NOCASE, or
// "pattern P: why" — an empty pattern, more than 64 bytes, more than 8 errors, a budget that is not smaller than the length —;
// SX_E_NOMEM if the host has no memory for the table.
int fuzzy_build(const sx_pattern* patterns, const uint8_t* max_errors, uint32_t n_patterns, uint32_t flags, FuzzyTable* out, std::string* err);

}  // namespace sx
