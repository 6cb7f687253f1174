// sx_extract_build.cpp — see sx_extract_build.hpp.  The trees, the positions and the NFA are sx_selre_front.hpp's; then the subset
// construction of an anchored automaton with two starts, Hopcroft's minimisation from the partition none / end / here, and the
// numbering.
#include "sx_extract_build.hpp"

#include <string.h>

#include <algorithm>
#include <new>
#include <unordered_map>

#include "sx_selre_front.hpp"

namespace sx {

int extract_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, ExtractTable* out, std::string* err) {
    using namespace refront;
    if (!patterns || !out) return fail(err, "a NULL pointer");
    try {
        Front F;
        { const int rc = front_build(patterns, n_patterns, flags, &F, err); if (rc != SX_OK) return rc; }
        const Nfa& nfa = F.nfa;
        const uint32_t K = F.K;
        // the subsets: a state is the byte nodes it holds and its two flags (in the key: marks behind the nodes).  D[s * K + c];
        // kinds: 0 none, 1 end, 2 here (a match may end here whatever follows: whether it also may at the end no longer counts)
        constexpr uint32_t kHereMark = 0xFFFFFFFEu;
        Closer closer(nfa);
        std::vector<Closure> after(nfa.n.size());      // behind a byte node: closure(its successor), made when first needed
        std::vector<uint8_t> after_made(nfa.n.size(), 0);
        std::unordered_map<std::vector<uint32_t>, uint32_t, KeyHash> ids;
        std::vector<std::vector<uint32_t>> keys;
        std::vector<uint8_t> kinds;
        std::vector<uint32_t> D;
        uint64_t entries = 0;
        auto state_of = [&](std::vector<uint32_t>&& key, bool always, bool at_end) -> uint32_t {
            if (always) key.push_back(kHereMark);
            else if (at_end) key.push_back(kEndMark);
            auto it = ids.find(key);
            if (it != ids.end()) return it->second;
            const uint32_t id = (uint32_t)keys.size();
            entries += key.size();
            ids.emplace(key, id);
            kinds.push_back(always ? 2 : at_end ? 1 : 0);
            keys.push_back(std::move(key));
            return id;
        };
        uint32_t starts[2];
        for (int k = 0; k < 2; k++) {      // with the `^` edges, then without them
            Closure c;
            closer.run(F.start, k == 0, &c);
            starts[k] = state_of(std::move(c.chars), false, false);      // (whether a match may end in front of the first byte never counts: no empty match)
        }
        std::vector<uint32_t> mark(nfa.n.size(), 0);
        uint32_t mark_stamp = 0;
        bool too_many = false;
        for (uint32_t s = 0; s < keys.size() && !too_many; s++) {
            D.resize((size_t)(s + 1) * K);
            const std::vector<uint32_t> key = keys[s];     // (a copy: keys grows)
            for (uint32_t c = 0; c < K; c++) {
                std::vector<uint32_t> to;
                bool always = false, at_end = false;
                mark_stamp++;
                for (uint32_t v : key) {
                    if (v >= kHereMark || !F.sets[nfa.n[v].set].has(F.rep[c])) continue;
                    if (!after_made[v]) { closer.run(nfa.n[v].a, false, &after[v]); after_made[v] = 1; }
                    const Closure& C = after[v];
                    always |= C.always; at_end |= C.at_end;
                    for (uint32_t u : C.chars) if (mark[u] != mark_stamp) { mark[u] = mark_stamp; to.push_back(u); }
                }
                std::sort(to.begin(), to.end());
                D[(size_t)s * K + c] = state_of(std::move(to), always, at_end);
                if (keys.size() > SX_SELECT_REGEX_MAX_STATES || entries > kSubsetEntries) { too_many = true; break; }
            }
        }
        if (too_many)
            return fail(err, keys.size() > SX_SELECT_REGEX_MAX_STATES ? std::string("the patterns need more than SX_SELECT_REGEX_MAX_STATES (65536) states")
                                                                      : "the subset construction was stopped at the bound on its memory: its " + std::to_string(keys.size()) + " states so far hold more than 33554432 NFA positions in all");
        const uint32_t n = (uint32_t)keys.size();
        ids.clear(); keys.clear(); after.clear();
        Quotient Qt;
        minimise(n, K, D, kinds, 3, F.cls, &Qt);
        const std::vector<uint32_t>&Q = Qt.Q, &first_of = Qt.first_of;
        const uint32_t classes = (uint32_t)first_of.size(), none = 0xFFFFFFFFu;
        // breadth first from the two starts; then none | end | here | dead
        std::vector<uint32_t> order, place(Qt.M, none);
        for (int k = 0; k < 2; k++) {
            const uint32_t B = Qt.blk[starts[k]];
            if (place[B] == none) { place[B] = 0; order.push_back(B); }
        }
        for (size_t i = 0; i < order.size(); i++)
            for (uint32_t f = 0; f < classes; f++) {
                const uint32_t to = Q[(size_t)order[i] * K + first_of[f]];
                if (place[to] == none) { place[to] = 0; order.push_back(to); }
            }
        auto absorbing = [&](uint32_t B) { for (uint32_t c = 0; c < K; c++) if (Q[(size_t)B * K + c] != B) return false; return true; };
        ExtractTable T;
        T.n_patterns = n_patterns; T.nocase = (flags & SX_SELECT_ASCII_NOCASE) ? 1u : 0u;
        memcpy(T.map, Qt.map, sizeof T.map);
        T.states = (uint32_t)order.size(); T.classes = classes;
        uint32_t number = 0;
        for (int kind = 0; kind < 4; kind++) {      // 0 none, 1 end, 2 here, 3 dead
            if (kind == 1) T.end_first = number;
            if (kind == 2) T.here_first = number;
            if (kind == 3) T.dead_first = number;
            for (uint32_t B : order) {
                const int is = Qt.kind[B] == 0 && absorbing(B) ? 3 : (int)Qt.kind[B];
                if (is == kind) place[B] = number++;
            }
        }
        T.start0 = place[Qt.blk[starts[0]]]; T.start1 = place[Qt.blk[starts[1]]];
        T.lds_states = std::min(T.states, kSelsetLdsBytes / (classes * 2u));
        T.next.assign((size_t)T.states * classes, 0);
        for (uint32_t B : order)
            for (uint32_t f = 0; f < classes; f++) T.next[(size_t)place[B] * classes + f] = (uint16_t)place[Q[(size_t)B * K + first_of[f]]];
        *out = std::move(T);
    } catch (const std::bad_alloc&) {
        if (err) *err = "no host memory for the extract set's table";
        return SX_E_NOMEM;
    }
    return SX_OK;
}

}  // namespace sx
