// sx_extract_build.cpp — see sx_extract_build.hpp.  Every step is sx_selre_front.hpp's: the trees, the positions, the NFA, the subset
// construction — here of an anchored automaton with two starts —, Hopcroft's minimisation from the partition none / end / here, and
// the numbering.  Here: what a subset is, the ranks, and the fields that only this table has.
#include "sx_extract_build.hpp"

#include "sx_selre_front.hpp"

namespace sx {

namespace {
// kinds: 0 none, 1 end, 2 here (a match may end here whatever follows: whether it also may at the end no longer counts)
struct ExtractRule {
    static constexpr bool reenter = false;
    static constexpr uint32_t kHereMark = 0xFFFFFFFEu;      // in a subset's key, as kEndMark
    bool mark(uint64_t& here, uint64_t& end, std::vector<uint32_t>& key) {
        if (here) key.push_back(kHereMark);
        else if (end) key.push_back(refront::kEndMark);
        return false;
    }
    uint32_t kind(uint64_t here, uint64_t end) { return here ? 2u : end ? 1u : 0u; }
};
}  // namespace

int extract_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, ExtractTable* out, std::string* err) {
    using namespace refront;
    return build_table(patterns && out, "extract set", err, [&]() -> int {
        Front F;
        { const int rc = front_build(patterns, n_patterns, flags, &F, err); if (rc != SX_OK) return rc; }
        ExtractRule rule;
        SubsetDfa S;
        { const int rc = subsets(F, rule, &S, err); if (rc != SX_OK) return rc; }
        Quotient Qt;
        minimise(S, F, &Qt);
        const std::vector<uint32_t> order = bfs_order(Qt, S.starts);
        // none | end | here | dead
        const Numbering N = number_by_rank(Qt, order, 4, false, [&](uint32_t B) { return Qt.kind[B] == 0 && absorbing(Qt, B) ? 3u : Qt.kind[B]; });
        ExtractTable T;
        write_table(Qt, order, N.place, n_patterns, flags, &T);
        T.end_first = N.first[1]; T.here_first = N.first[2]; T.dead_first = N.first[3];
        T.start0 = N.place[Qt.blk[S.starts[0]]]; T.start1 = N.place[Qt.blk[S.starts[1]]];
        *out = std::move(T);
        return SX_OK;
    });
}

}  // namespace sx
