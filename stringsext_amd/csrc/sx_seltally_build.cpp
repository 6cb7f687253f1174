// sx_seltally_build.cpp — see sx_seltally_build.hpp.  The steps of sx_selset_build.cpp, none of which does 256-wide work per state:
// the byte classes; the trie over the (folded) keywords with its children as sibling lists — whole, nothing is cut below a
// keyword's end —; one breadth-first walk that numbers the states, writes a state's row as its failure state's row — complete by
// then: that state is nearer to the root — with the state's own children on top, and gives a new state its output link from its
// failure state's, which is known by then for the same reason.
#include "sx_seltally_build.hpp"

#include <string.h>

#include <new>

namespace sx {

namespace {

struct TallyNode { uint32_t child, sibling; uint8_t cls, ends; };   // child / sibling: 0 = none (the root is nobody's child)

int tally_fail(std::string* err, const char* what) { if (err) *err = what; return SX_E_INVALID; }

}  // namespace

int seltally_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SeltallyTable* out, std::string* err) {
    if (!patterns || !out) return tally_fail(err, "a NULL pointer");
    if (n_patterns < 1 || n_patterns > SX_SELECT_SET_MAX_PATTERNS) return tally_fail(err, "n_patterns must be 1..65536");
    if (flags & ~(uint32_t)SX_SELECT_ASCII_NOCASE) return tally_fail(err, "a tally set takes SX_SELECT_ASCII_NOCASE and no other flag");
    uint64_t total = 0;
    for (uint32_t p = 0; p < n_patterns; p++) {
        if (!patterns[p].bytes || patterns[p].len < 1 || patterns[p].len > SX_SELECT_SET_MAX_PATTERN_BYTES) return tally_fail(err, "a pattern must have 1..255 bytes");
        total += patterns[p].len;
    }
    if (total > SX_SELECT_SET_MAX_TOTAL_BYTES) return tally_fail(err, "the patterns' lengths must sum to at most 1 MiB");
    const bool nocase = (flags & SX_SELECT_ASCII_NOCASE) != 0;
    auto folded = [nocase](uint32_t x) { return nocase && x - 'A' < 26u ? x | 0x20u : x; };
    try {
        SeltallyTable T;
        T.n_patterns = n_patterns; T.nocase = nocase ? 1u : 0u;
        // the classes
        bool used[256] = {};
        for (uint32_t p = 0; p < n_patterns; p++)
            for (uint32_t j = 0; j < patterns[p].len; j++) used[folded(patterns[p].bytes[j])] = true;
        bool any_unused = false;
        for (uint32_t x = 0; x < 256; x++) any_unused |= !used[folded(x)];
        uint32_t classes = any_unused ? 1u : 0u;
        for (uint32_t x = 0; x < 256; x++) if (used[x]) T.map[x] = (uint8_t)classes++;
        for (uint32_t x = 0; x < 256; x++) if (!used[x]) T.map[x] = used[folded(x)] ? T.map[folded(x)] : 0;
        T.classes = classes;
        // the trie: a node per distinct prefix; ends_at[p] = the node pattern p ends in
        std::vector<TallyNode> trie;
        std::vector<uint32_t> ends_at(n_patterns);
        trie.reserve((size_t)total + 1);
        trie.push_back(TallyNode{ 0, 0, 0, 0 });
        for (uint32_t p = 0; p < n_patterns; p++) {
            uint32_t u = 0;
            for (uint32_t j = 0; j < patterns[p].len; j++) {
                const uint8_t c = T.map[patterns[p].bytes[j]];
                uint32_t v = trie[u].child;
                while (v && trie[v].cls != c) v = trie[v].sibling;
                if (!v) {
                    v = (uint32_t)trie.size();
                    trie.push_back(TallyNode{ 0, trie[u].child, c, 0 });
                    trie[u].child = v;
                }
                u = v;
            }
            trie[u].ends = 1;
            ends_at[p] = u;
        }
        // breadth first: state s is the trie node queue[s]; fails[s] its failure state; state_of[node] the other way round
        const size_t states = trie.size();
        std::vector<uint32_t> queue, fails, next, state_of(states, 0);
        queue.reserve(states); fails.reserve(states);
        T.own.assign(states, kSeltallyNone); T.dict.assign(states, 0);
        next.assign(states * classes, 0);
        queue.push_back(0); fails.push_back(0);
        for (size_t s = 0; s < queue.size(); s++) {
            uint32_t* row = next.data() + s * classes;
            if (s) memcpy(row, next.data() + (size_t)fails[s] * classes, classes * sizeof(uint32_t));
            for (uint32_t v = trie[queue[s]].child; v; v = trie[v].sibling) {
                const uint32_t f = row[trie[v].cls];   // where the failure state goes with this class: v's failure state
                const uint32_t t = (uint32_t)queue.size();
                row[trie[v].cls] = t;
                queue.push_back(v); fails.push_back(f);
                state_of[v] = t;
                if (trie[v].ends) T.own[t] = T.unique++;
                T.dict[t] = T.own[f] != kSeltallyNone ? f : T.dict[f];   // (f < t: its link is there; the root's is 0)
            }
        }
        T.states = (uint32_t)states;
        T.unique_of_pattern.resize(n_patterns);
        for (uint32_t p = 0; p < n_patterns; p++) T.unique_of_pattern[p] = T.own[state_of[ends_at[p]]];
        T.entry_bytes = T.states <= 32768u ? 2u : 4u;
        T.lds_states = kSeltallyLdsBytes / (classes * T.entry_bytes);
        if (T.lds_states > T.states) T.lds_states = T.states;
        const size_t entries = states * classes;
        T.next.resize(entries * T.entry_bytes);
        for (size_t i = 0; i < entries; i++) {
            const uint32_t to = next[i], ends = T.own[to] != kSeltallyNone || T.dict[to] ? 1u : 0u;
            if (T.entry_bytes == 2) ((uint16_t*)T.next.data())[i] = (uint16_t)(to | ends << 15);
            else ((uint32_t*)T.next.data())[i] = to | ends << 31;
        }
        *out = std::move(T);
    } catch (const std::bad_alloc&) {
        if (err) *err = "no host memory for the tally set's tables";
        return SX_E_NOMEM;
    }
    return SX_OK;
}

}  // namespace sx
