// sx_label_build.cpp — see sx_label_build.hpp.  The trees, the positions and the NFA are sx_selre_front.hpp's, with an accept node
// per pattern; then the subset construction of the unanchored automaton with two masks per subset, Hopcroft's minimisation from the
// partition by the pair (here, end), and the numbering.
#include "sx_label_build.hpp"

#include <string.h>

#include <algorithm>
#include <map>
#include <new>
#include <unordered_map>

#include "sx_selre_front.hpp"

namespace sx {

int label_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, LabelTable* out, std::string* err) {
    using namespace refront;
    if (!patterns || !out) return fail(err, "a NULL pointer");
    try {
        Front F;
        F.accept_per_pattern = true;
        { const int rc = front_build(patterns, n_patterns, flags, &F, err); if (rc != SX_OK) return rc; }
        const Nfa& nfa = F.nfa;
        const std::vector<ByteSet>& sets = F.sets;
        const uint32_t start = F.start, K = F.K;
        const uint8_t* rep = F.rep;
        // the subsets.  D[s * K + c]; state 0 is the root.  As in selre_build a subset always holds the re-entry's byte nodes, so its key
        // is what it holds BESIDES them; behind the nodes the key has four words: its two masks.  The patterns that the re-entry accepts
        // without a byte (`a*`) are in every lane's label from the start (they are in the root's `here`): their bits are left out of
        // every subset's masks, where they could only tell apart states that nothing else does.
        Closer closer(nfa);
        std::vector<Closure> after(nfa.n.size());      // behind a byte node: closure(its successor), made when first needed
        std::vector<uint8_t> after_made(nfa.n.size(), 0);
        Closure again;                                  // the re-entry in front of every later byte: no `^` edge
        closer.run(start, false, &again);
        const uint64_t keep = ~again.here;
        std::unordered_map<std::vector<uint32_t>, uint32_t, KeyHash> ids;
        std::vector<std::vector<uint32_t>> keys;
        std::vector<uint32_t> kinds;                                  // subset -> the number of its pair of masks
        std::vector<std::pair<uint64_t, uint64_t>> pairs;             // that number -> (here, end)
        std::map<std::pair<uint64_t, uint64_t>, uint32_t> pair_ids;
        std::vector<uint32_t> D;
        uint64_t entries = 0;
        bool too_many = false;
        auto state_of = [&](std::vector<uint32_t>&& key, uint64_t here, uint64_t end) -> uint32_t {
            here &= keep; end &= keep & ~here;      // (what is reached whatever follows is reached at the end too)
            key.push_back((uint32_t)here); key.push_back((uint32_t)(here >> 32)); key.push_back((uint32_t)end); key.push_back((uint32_t)(end >> 32));
            auto it = ids.find(key);
            if (it != ids.end()) return it->second;
            const uint32_t id = (uint32_t)keys.size();
            entries += key.size();
            ids.emplace(key, id);
            const auto pr = std::make_pair(here, end);
            auto pit = pair_ids.find(pr);
            if (pit == pair_ids.end()) { pit = pair_ids.emplace(pr, (uint32_t)pairs.size()).first; pairs.push_back(pr); }
            kinds.push_back(pit->second);
            keys.push_back(std::move(key));
            return id;
        };
        std::vector<uint8_t> in_again(nfa.n.size(), 0);
        for (uint32_t v : again.chars) in_again[v] = 1;
        std::vector<uint32_t> mark(nfa.n.size(), 0);
        uint32_t mark_stamp = 0;
        auto behind = [&](uint32_t v) -> const Closure& {
            if (!after_made[v]) { closer.run(nfa.n[v].a, false, &after[v]); after_made[v] = 1; }
            return after[v];
        };
        // `to` and the masks joined with what is behind the first `count` nodes of `from` that take a byte of class c
        auto step = [&](const std::vector<uint32_t>& from, size_t count, uint32_t c, std::vector<uint32_t>* to, uint64_t* here, uint64_t* end) {
            for (size_t k = 0; k < count; k++) {
                const uint32_t v = from[k];
                if (!sets[nfa.n[v].set].has(rep[c])) continue;
                const Closure& C = behind(v);
                *here |= C.here; *end |= C.end;
                for (uint32_t u : C.chars) if (!in_again[u] && mark[u] != mark_stamp) { mark[u] = mark_stamp; to->push_back(u); }
            }
        };
        std::vector<Closure> again_to(K);
        for (uint32_t c = 0; c < K; c++) {
            again_to[c].here = again.here; again_to[c].end = again.end;
            mark_stamp++;
            step(again.chars, again.chars.size(), c, &again_to[c].chars, &again_to[c].here, &again_to[c].end);
        }
        uint64_t root_here = 0;
        {
            Closure root;
            closer.run(start, true, &root);
            root_here = root.here;
            std::vector<uint32_t> key;
            for (uint32_t v : root.chars) if (!in_again[v]) key.push_back(v);
            state_of(std::move(key), root.here, root.end);
        }
        for (uint32_t s = 0; s < keys.size() && !too_many; s++) {
            D.resize((size_t)(s + 1) * K);
            const std::vector<uint32_t> key = keys[s];     // (a copy: keys grows)
            for (uint32_t c = 0; c < K; c++) {
                std::vector<uint32_t> to = again_to[c].chars;
                uint64_t here = again_to[c].here, end = again_to[c].end;
                mark_stamp++;
                for (uint32_t v : to) mark[v] = mark_stamp;
                step(key, key.size() - 4, c, &to, &here, &end);
                std::sort(to.begin(), to.end());
                D[(size_t)s * K + c] = state_of(std::move(to), here, end);
                if (keys.size() > SX_SELECT_REGEX_MAX_STATES || entries > kSubsetEntries) { too_many = true; break; }
            }
        }
        if (too_many)
            return fail(err, keys.size() > SX_SELECT_REGEX_MAX_STATES ? std::string("the patterns need more than SX_SELECT_REGEX_MAX_STATES (65536) states")
                                                                      : "the subset construction was stopped at the bound on its memory: its " + std::to_string(keys.size()) + " states so far hold more than 33554432 NFA positions in all");
        const uint32_t n = (uint32_t)keys.size();
        ids.clear(); keys.clear(); after.clear();
        // Hopcroft: blocks of states that no string tells apart, told apart to begin with by their pair of masks
        QuotientOf<uint32_t> Qt;
        minimise(n, K, D, kinds, (uint32_t)pairs.size(), F.cls, &Qt);
        const uint32_t M = Qt.M;
        const std::vector<uint32_t>&Q = Qt.Q, &blk = Qt.blk, &first_of = Qt.first_of;
        LabelTable T;
        T.n_patterns = n_patterns; T.nocase = (flags & SX_SELECT_ASCII_NOCASE) ? 1u : 0u;
        T.root_here = root_here;
        T.all = n_patterns == 64 ? ~(uint64_t)0 : ((uint64_t)1 << n_patterns) - 1u;
        memcpy(T.map, Qt.map, sizeof T.map);
        const uint32_t classes = (uint32_t)first_of.size();
        // breadth first from the root; then: root | here == 0 | here != 0 | dead
        std::vector<uint32_t> order, place(M, kLabelNone);
        order.push_back(blk[0]); place[blk[0]] = 0;
        for (size_t i = 0; i < order.size(); i++)
            for (uint32_t f = 0; f < classes; f++) {
                const uint32_t to = Q[(size_t)order[i] * K + first_of[f]];
                if (place[to] == kLabelNone) { place[to] = 0; order.push_back(to); }
            }
        auto here_of = [&](uint32_t B) { return pairs[Qt.kind[B]].first; };
        auto end_of = [&](uint32_t B) { return pairs[Qt.kind[B]].second; };
        auto is_dead = [&](uint32_t B) {
            if (here_of(B) || end_of(B)) return false;
            for (uint32_t c = 0; c < K; c++) if (Q[(size_t)B * K + c] != B) return false;
            return true;
        };
        const uint32_t root = order[0];
        uint32_t number = 1;
        T.states = (uint32_t)order.size();
        for (int kind = 0; kind < 3; kind++) {      // 0 here == 0, 1 here != 0, 2 dead
            if (kind == 1) T.here_first = number;
            for (size_t i = 1; i < order.size(); i++) {
                const uint32_t B = order[i];
                const int is = is_dead(B) ? 2 : here_of(B) ? 1 : 0;
                if (is != kind) continue;
                if (kind == 2) T.dead = number;
                place[B] = number++;
            }
        }
        place[root] = 0;
        if (is_dead(root)) T.dead = 0;      // (the only state)
        T.classes = classes;
        T.lds_states = std::min(T.states, kSelsetLdsBytes / (classes * 2u));
        T.next.assign((size_t)T.states * classes, 0);
        T.here.assign(T.states - T.here_first, 0);
        T.end.assign(T.states, 0);
        for (uint32_t B : order) {
            for (uint32_t f = 0; f < classes; f++) T.next[(size_t)place[B] * classes + f] = (uint16_t)place[Q[(size_t)B * K + first_of[f]]];
            if (place[B] >= T.here_first) T.here[place[B] - T.here_first] = here_of(B);
            T.end[place[B]] = end_of(B);
        }
        *out = std::move(T);
    } catch (const std::bad_alloc&) {
        if (err) *err = "no host memory for the label set's table";
        return SX_E_NOMEM;
    }
    return SX_OK;
}

}  // namespace sx
