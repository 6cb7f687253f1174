// sx_seltally_build.cpp — see sx_seltally_build.hpp.  The steps of sx_selset_build.cpp, none of which does 256-wide work per state:
// the byte classes; the trie over the (folded) keywords with its children as sibling lists — whole, nothing is cut below a
// keyword's end —; one breadth-first walk that numbers the states, writes a state's row as its failure state's row — complete by
// then: that state is nearer to the root — with the state's own children on top, and gives a new state its output link from its
// failure state's, which is known by then for the same reason.
#include "sx_seltally_build.hpp"

#include <string.h>

#include <new>

#include "sx_keyword_front.hpp"

namespace sx {

int seltally_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SeltallyTable* out, std::string* err) {
    uint64_t total = 0;
    { const int rc = kwfront::check("tally set", patterns, n_patterns, flags, out, &total, err); if (rc != SX_OK) return rc; }
    const bool nocase = (flags & SX_SELECT_ASCII_NOCASE) != 0;
    try {
        SeltallyTable T;
        T.n_patterns = n_patterns; T.nocase = nocase ? 1u : 0u;
        const uint32_t classes = T.classes = kwfront::classes(patterns, n_patterns, nocase, T.map);
        // whole: a node per distinct prefix; ends_at[p] = the node pattern p ends in
        std::vector<uint32_t> ends_at;
        const std::vector<kwfront::TrieNode> trie = kwfront::trie(patterns, n_patterns, T.map, total, false, &ends_at);
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
