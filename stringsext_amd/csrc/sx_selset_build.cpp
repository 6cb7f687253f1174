// sx_selset_build.cpp — see sx_selset_build.hpp.  Three steps, none of which does 256-wide work per state: the trie over the (folded)
// keywords with its children as sibling lists; the byte classes; one breadth-first walk that numbers the states and writes a
// state's row as its failure state's row — complete by then: that state is nearer to the root — with the state's own children
// on top.
#include "sx_selset_build.hpp"

#include <string.h>

#include <new>

#include "sx_keyword_front.hpp"

namespace sx {

namespace {

constexpr uint32_t kMatchedYet = 0xFFFFFFFFu;                       // `matched` until the number of states is known

}  // namespace

int selset_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SelsetTable* out, std::string* err) {
    uint64_t total = 0;
    { const int rc = kwfront::check("pattern set", patterns, n_patterns, flags, out, &total, err); if (rc != SX_OK) return rc; }
    const bool nocase = (flags & SX_SELECT_ASCII_NOCASE) != 0;
    try {
        SelsetTable T;
        T.n_patterns = n_patterns; T.nocase = nocase ? 1u : 0u;
        const uint32_t classes = T.classes = kwfront::classes(patterns, n_patterns, nocase, T.map);
        // nothing is kept below the end of a keyword (below a shorter keyword's end: that one's, again)
        const std::vector<kwfront::TrieNode> trie = kwfront::trie(patterns, n_patterns, T.map, total, true, nullptr);
        // breadth first: state s is the trie node queue[s]; fails[s] its failure state
        std::vector<uint32_t> queue, fails, next;
        queue.push_back(0); fails.push_back(0);
        for (size_t s = 0; s < queue.size(); s++) {
            next.resize((s + 1) * classes, 0);
            uint32_t* row = next.data() + s * classes;
            if (s) memcpy(row, next.data() + (size_t)fails[s] * classes, classes * sizeof(uint32_t));
            for (uint32_t v = trie[queue[s]].child; v; v = trie[v].sibling) {
                const uint32_t f = row[trie[v].cls];   // where the failure state goes with this class: v's failure state
                if (trie[v].ends || f == kMatchedYet) { row[trie[v].cls] = kMatchedYet; continue; }
                row[trie[v].cls] = (uint32_t)queue.size();
                queue.push_back(v); fails.push_back(f);
            }
        }
        T.states = (uint32_t)queue.size() + 1;
        T.matched = T.states - 1;
        T.entry_bytes = T.states <= 65536u ? 2u : 4u;
        T.lds_states = kSelsetLdsBytes / (classes * T.entry_bytes);
        if (T.lds_states > T.states) T.lds_states = T.states;
        const size_t entries = (size_t)T.states * classes;
        T.next.resize(entries * T.entry_bytes);
        for (size_t i = 0; i < entries; i++) {
            const uint32_t to = i < next.size() && next[i] != kMatchedYet ? next[i] : T.matched;   // (the last row: matched stays matched)
            if (T.entry_bytes == 2) ((uint16_t*)T.next.data())[i] = (uint16_t)to;
            else ((uint32_t*)T.next.data())[i] = to;
        }
        *out = std::move(T);
    } catch (const std::bad_alloc&) {
        if (err) *err = "no host memory for the pattern set's table";
        return SX_E_NOMEM;
    }
    return SX_OK;
}

}  // namespace sx
