// sx_selre_build.cpp — see sx_selre_build.hpp.  Every step is sx_selre_front.hpp's, which sx_extract_build.cpp and
// sx_label_build.cpp share: the parser, the count of the positions with the repeats unrolled, the Thompson NFA, the subset
// construction over the byte classes that the patterns' byte sets tell apart, Hopcroft's minimisation — which also merges the byte
// classes whose columns have become equal and leaves one `matched` and one `dead` state at the most — and the numbering.  Here:
// what a subset of the unanchored search is, the ranks, and the fields that only this table has.
#include "sx_selre_build.hpp"

#include "sx_selre_front.hpp"

namespace sx {

namespace {
// Everything that accepts whatever follows is the one state `matched`; of the others, the kinds are 0 and 1: accepts at the end.
struct SelreRule {
    static constexpr bool reenter = true;
    bool mark(uint64_t& here, uint64_t& end, std::vector<uint32_t>& key) {
        if (!here && end) key.push_back(refront::kEndMark);
        return here != 0;
    }
    uint32_t kind(uint64_t here, uint64_t end) { return here || end ? 1u : 0u; }
};
}  // namespace

int selre_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, SelreTable* out, std::string* err) {
    using namespace refront;
    return build_table(patterns && out, "regex set", err, [&]() -> int {
        Front F;
        { const int rc = front_build(patterns, n_patterns, flags, &F, err); if (rc != SX_OK) return rc; }
        SelreRule rule;
        SubsetDfa S;
        { const int rc = subsets(F, rule, &S, err); if (rc != SX_OK) return rc; }
        Quotient Qt;
        minimise(S, F, &Qt);
        const std::vector<uint32_t> order = bfs_order(Qt, S.starts);
        // root | ordinary | end-accepting | dead | matched
        const Numbering N = number_by_rank(Qt, order, 4, true, [&](uint32_t B) { return (absorbing(Qt, B) ? 2u : 0u) + Qt.kind[B]; });
        SelreTable T;
        write_table(Qt, order, N.place, n_patterns, flags, &T);
        const uint32_t root = order[0];
        T.end_first = N.first[1]; T.stop_first = N.first[2];
        if (N.first[3] < N.first[4]) T.matched = N.first[3];
        if (absorbing(Qt, root)) { T.end_first = T.stop_first = 0; if (Qt.kind[root]) T.matched = 0; }     // (the only state)
        else T.root_end = Qt.kind[root];
        T.end_states = T.stop_first - T.end_first + T.root_end;
        *out = std::move(T);
        return SX_OK;
    });
}

}  // namespace sx
