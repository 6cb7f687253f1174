// sx_selre_build.cpp — see sx_selre_build.hpp.  Five steps: the parser, the count of the positions with the repeats unrolled, the
// Thompson NFA (all three in sx_selre_front.hpp, which sx_extract_build.cpp shares), the subset construction over the byte classes
// that the patterns' byte sets tell apart, Hopcroft's minimisation — which also merges the byte classes whose columns have become
// equal and leaves one `matched` and one `dead` state at the most — and the numbering.
#include "sx_selre_build.hpp"

#include <string.h>

#include <algorithm>
#include <new>
#include <unordered_map>

#include "sx_selre_front.hpp"

namespace sx {

int selre_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SelreTable* out, std::string* err) {
    using namespace refront;
    if (!patterns || !out) return fail(err, "a NULL pointer");
    try {
        // 1. to 3. the trees, the positions, the NFA; the byte classes of the construction
        Front F;
        { const int rc = front_build(patterns, n_patterns, flags, &F, err); if (rc != SX_OK) return rc; }
        const Nfa& nfa = F.nfa;
        const std::vector<ByteSet>& sets = F.sets;
        const uint32_t start = F.start, K = F.K;
        const uint8_t* rep = F.rep;
        // 4. the subsets.  D[s * K + c]; state 0 is the root; `matched` is made when first needed
        Closer closer(nfa);
        std::vector<Closure> after(nfa.n.size());      // behind a byte node: closure(its successor), made when first needed
        std::vector<uint8_t> after_made(nfa.n.size(), 0);
        Closure again;                                  // the re-entry in front of every later byte: no `^` edge
        closer.run(start, false, &again);
        std::unordered_map<std::vector<uint32_t>, uint32_t, KeyHash> ids;
        std::vector<std::vector<uint32_t>> keys;
        std::vector<uint8_t> accepts;
        std::vector<uint32_t> D;
        uint32_t matched = kSelreNone;
        uint64_t entries = 0;
        bool too_many = false;
        auto state_of = [&](std::vector<uint32_t>&& key, bool always, bool at_end) -> uint32_t {
            if (always) {
                if (matched == kSelreNone) { matched = (uint32_t)keys.size(); keys.emplace_back(); accepts.push_back(1); }
                return matched;
            }
            if (at_end) key.push_back(kEndMark);
            auto it = ids.find(key);
            if (it != ids.end()) return it->second;
            const uint32_t id = (uint32_t)keys.size();
            entries += key.size();
            ids.emplace(key, id);
            accepts.push_back(at_end ? 1 : 0);
            keys.push_back(std::move(key));
            return id;
        };
        // A subset always holds the re-entry's byte nodes, so its key is what it holds BESIDES them (a keyword list's re-entry has
        // a node per keyword), and what the re-entry's own nodes give with a byte is worked out once per class.
        std::vector<uint8_t> in_again(nfa.n.size(), 0);
        for (uint32_t v : again.chars) in_again[v] = 1;
        std::vector<uint32_t> mark(nfa.n.size(), 0);
        uint32_t mark_stamp = 0;
        auto behind = [&](uint32_t v) -> const Closure& {
            if (!after_made[v]) { closer.run(nfa.n[v].a, false, &after[v]); after_made[v] = 1; }
            return after[v];
        };
        // `to` and the flags joined with what is behind the nodes of `from` that take a byte of class c
        auto step = [&](const std::vector<uint32_t>& from, uint32_t c, std::vector<uint32_t>* to, bool* always, bool* at_end) {
            for (uint32_t v : from) {
                if (v == kEndMark || !sets[nfa.n[v].set].has(rep[c])) continue;
                const Closure& C = behind(v);
                *always |= C.always; *at_end |= C.at_end;
                if (*always) return;
                for (uint32_t u : C.chars) if (!in_again[u] && mark[u] != mark_stamp) { mark[u] = mark_stamp; to->push_back(u); }
            }
        };
        std::vector<Closure> again_to(K);
        for (uint32_t c = 0; c < K; c++) {
            again_to[c].always = again.always; again_to[c].at_end = again.at_end;
            mark_stamp++;
            step(again.chars, c, &again_to[c].chars, &again_to[c].always, &again_to[c].at_end);
        }
        {
            Closure root;
            closer.run(start, true, &root);
            std::vector<uint32_t> key;
            for (uint32_t v : root.chars) if (!in_again[v]) key.push_back(v);
            state_of(std::move(key), root.always, root.at_end);
        }
        for (uint32_t s = 0; s < keys.size() && !too_many; s++) {
            D.resize((size_t)(s + 1) * K);
            if (s == matched) { for (uint32_t c = 0; c < K; c++) D[(size_t)s * K + c] = s; continue; }
            const std::vector<uint32_t> key = keys[s];     // (a copy: keys grows)
            for (uint32_t c = 0; c < K; c++) {
                std::vector<uint32_t> to = again_to[c].chars;
                bool always = again_to[c].always, at_end = again_to[c].at_end;
                mark_stamp++;
                for (uint32_t v : to) mark[v] = mark_stamp;
                if (!always) step(key, c, &to, &always, &at_end);
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
        // 5. Hopcroft: blocks of states that no string tells apart, told apart to begin with by whether they accept
        Quotient Qt;
        minimise(n, K, D, accepts, 2, F.cls, &Qt);
        const uint32_t M = Qt.M;
        const std::vector<uint32_t>&Q = Qt.Q, &blk = Qt.blk, &first_of = Qt.first_of;
        const std::vector<uint8_t>& q_accepts = Qt.kind;
        SelreTable T;
        T.n_patterns = n_patterns; T.nocase = (flags & SX_SELECT_ASCII_NOCASE) ? 1u : 0u;
        memcpy(T.map, Qt.map, sizeof T.map);
        const uint32_t classes = (uint32_t)first_of.size();
        // breadth first from the root; then: root | ordinary | end-accepting | dead | matched
        std::vector<uint32_t> order, place(M, kSelreNone);
        order.push_back(blk[0]); place[blk[0]] = 0;
        for (size_t i = 0; i < order.size(); i++)
            for (uint32_t f = 0; f < classes; f++) {
                const uint32_t to = Q[(size_t)order[i] * K + first_of[f]];
                if (place[to] == kSelreNone) { place[to] = 0; order.push_back(to); }
            }
        auto absorbing = [&](uint32_t B) { for (uint32_t c = 0; c < K; c++) if (Q[(size_t)B * K + c] != B) return false; return true; };
        const uint32_t root = order[0];
        uint32_t number = 1;
        T.states = (uint32_t)order.size();
        for (int kind = 0; kind < 4; kind++) {      // 0 ordinary, 1 end-accepting, 2 dead, 3 matched
            if (kind == 1) T.end_first = number;
            if (kind == 2) T.stop_first = number;
            for (size_t i = 1; i < order.size(); i++) {
                const uint32_t B = order[i];
                const int is = absorbing(B) ? (q_accepts[B] ? 3 : 2) : (q_accepts[B] ? 1 : 0);
                if (is != kind) continue;
                if (kind == 3) T.matched = number;
                place[B] = number++;
            }
        }
        place[root] = 0;
        if (absorbing(root)) { T.end_first = T.stop_first = 0; if (q_accepts[root]) T.matched = 0; }     // (the only state)
        else T.root_end = q_accepts[root];
        T.end_states = T.stop_first - T.end_first + T.root_end;
        T.classes = classes;
        T.lds_states = std::min(T.states, kSelsetLdsBytes / (classes * 2u));
        T.next.assign((size_t)T.states * classes, 0);
        for (uint32_t B : order)
            for (uint32_t f = 0; f < classes; f++) T.next[(size_t)place[B] * classes + f] = (uint16_t)place[Q[(size_t)B * K + first_of[f]]];
        *out = std::move(T);
    } catch (const std::bad_alloc&) {
        if (err) *err = "no host memory for the regex set's table";
        return SX_E_NOMEM;
    }
    return SX_OK;
}

}  // namespace sx
