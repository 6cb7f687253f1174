// sx_label_build.cpp — see sx_label_build.hpp.  Every step is sx_selre_front.hpp's: the trees, the positions, the NFA, with an accept
// node per pattern, the subset construction of the unanchored automaton, Hopcroft's minimisation from the partition by the pair
// (here, end), and the numbering.  Here: the two masks that a subset carries, the ranks, and the fields that only this table has.
#include "sx_label_build.hpp"

#include <map>

#include "sx_selre_front.hpp"

namespace sx {

namespace {
// Behind its nodes a subset's key has four words: its two masks; its kind is the number of that pair.  The patterns that the
// re-entry accepts without a byte (`a*`) are in every lane's label from the start (they are in the root's `here`): their bits are
// left out of every subset's masks (`keep`), where they could only tell apart states that nothing else does.
struct LabelRule {
    static constexpr bool reenter = true;
    uint64_t keep = 0;
    std::vector<std::pair<uint64_t, uint64_t>> pairs;             // kind -> (here, end)
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> pair_ids;
    bool mark(uint64_t& here, uint64_t& end, std::vector<uint32_t>& key) {
        here &= keep; end &= keep & ~here;      // (what is reached whatever follows is reached at the end too)
        key.push_back((uint32_t)here); key.push_back((uint32_t)(here >> 32)); key.push_back((uint32_t)end); key.push_back((uint32_t)(end >> 32));
        return false;      // (nothing absorbs: a pattern that has matched says nothing about the others)
    }
    uint32_t kind(uint64_t here, uint64_t end) {
        const auto at = pair_ids.emplace(std::make_pair(here, end), (uint32_t)pairs.size());
        if (at.second) pairs.push_back(at.first->first);
        return at.first->second;
    }
};
}  // namespace

int label_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, LabelTable* out, std::string* err) {
    using namespace refront;
    return build_table(patterns && out, "label set", err, [&]() -> int {
        Front F;
        F.accept_per_pattern = true;
        { const int rc = front_build(patterns, n_patterns, flags, &F, err); if (rc != SX_OK) return rc; }
        Closure again, root;      // the re-entry in front of every later byte, and the root: with the `^` edges
        { Closer closer(F.nfa); closer.run(F.start, false, &again); closer.run(F.start, true, &root); }
        LabelRule rule;
        rule.keep = ~again.here;
        SubsetDfa S;
        { const int rc = subsets(F, rule, &S, err); if (rc != SX_OK) return rc; }
        Quotient Qt;
        minimise(S, F, &Qt);
        const std::vector<uint32_t> order = bfs_order(Qt, S.starts);
        auto here_of = [&](uint32_t B) { return rule.pairs[Qt.kind[B]].first; };
        auto end_of = [&](uint32_t B) { return rule.pairs[Qt.kind[B]].second; };
        auto is_dead = [&](uint32_t B) { return !here_of(B) && !end_of(B) && absorbing(Qt, B); };
        // root | here == 0 | here != 0 | dead
        const Numbering N = number_by_rank(Qt, order, 3, true, [&](uint32_t B) { return is_dead(B) ? 2u : here_of(B) ? 1u : 0u; });
        LabelTable T;
        write_table(Qt, order, N.place, n_patterns, flags, &T);
        T.root_here = root.here;
        T.all = n_patterns == 64 ? ~(uint64_t)0 : ((uint64_t)1 << n_patterns) - 1u;
        T.here_first = N.first[1];
        if (N.first[2] < N.first[3]) T.dead = N.first[2];
        if (is_dead(order[0])) T.dead = 0;      // (the only state)
        T.here.assign(T.states - T.here_first, 0);
        T.end.assign(T.states, 0);
        for (uint32_t B : order) {
            if (N.place[B] >= T.here_first) T.here[N.place[B] - T.here_first] = here_of(B);
            T.end[N.place[B]] = end_of(B);
        }
        *out = std::move(T);
        return SX_OK;
    });
}

}  // namespace sx
