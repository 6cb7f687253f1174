// Test-only program with a main of its own, for a sanitizer build (tests/test_seen_count_core.py builds it with
// -fsanitize=address,undefined and starts it as a child process): the lane functions of a seen set that counts, as
// seen_count_host.cpp drives them, over a few dozen strings — one result added, one list merged with counts of its own, and the set
// grown into a larger one — with the counts checked against what the strings say.  Prints "ok" and returns 0, or says what differs.
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

#include "seen_count_host.cpp"

static std::vector<std::string> strings_of(int n, int step) {
    std::vector<std::string> out;
    for (int k = 0; k < n; k++) out.push_back("string " + std::to_string(k * step) + std::string((size_t)(k * step % 11), 'x'));
    return out;
}

// {string: count word} by a walk over the table
static std::map<std::string, uint64_t> counts_of(const SxsSeen* S) {
    std::map<std::string, uint64_t> out;
    for (uint64_t s = 0; s < (uint64_t)1 << S->dev.table_log2; s++) {
        const uint64_t word = S->dev.slots[s];
        if (word == sx::kSeenEmpty) continue;
        const uint8_t* e = sx::seen_entry_at(S->dev.arena, word);
        out[std::string((const char*)e + 8, *(const uint32_t*)e)] = S->dev.counts[s];
    }
    return out;
}

static int fail(const char* what) { printf("FAILED: %s\n", what); fflush(stdout); return 1; }

int main() {
    // a result: 40 strings, every fourth of them three times
    const std::vector<std::string> a = strings_of(40, 1), b = strings_of(30, 2);
    std::vector<std::string> flat;
    for (size_t k = 0; k < a.size(); k++)
        for (int r = 0; r < (k % 4 == 0 ? 3 : 1); r++) flat.push_back(a[k]);
    std::string bytes;
    std::vector<sx_finding16> recs;
    for (const std::string& s : flat) {
        recs.push_back(sx_finding16{ 100 + recs.size(), (uint32_t)bytes.size(), (uint16_t)s.size(), 0, 0 });
        bytes += s;
    }
    SxsGuarded arena;
    if (!arena.get(bytes.size())) return fail("no memory");
    memcpy(arena.at, bytes.data(), bytes.size());
    std::vector<uint64_t> labels(flat.size());

    SxsSeen* S = sxs_seen_new(-1, 1, 0, 64, 4096);
    SxcCounts* K = S ? sxc_counts_new(S) : nullptr;
    if (!K) return fail("no set");
    const void* recs_p[1] = { recs.data() };
    const uint8_t* arena_p[1] = { (const uint8_t*)arena.at };
    const uint64_t ns[1] = { flat.size() };
    const int32_t packed[1] = { 1 };
    uint64_t* labels_p[1] = { labels.data() };
    uint64_t info[9];
    if (sxc_seen_call(S, 1, recs_p, arena_p, ns, packed, -1, 2, 0, labels_p, info) != 0) return fail("the result's call");
    std::map<std::string, uint64_t> want;
    for (size_t k = 0; k < a.size(); k++) want[a[k]] = (uint64_t)(k % 4 == 0 ? 3 : 1) << 32 | 1u;
    if (counts_of(S) != want) return fail("the counts behind the result");

    // a list with counts of its own: (2, 5) each; half of it is held
    std::vector<uint8_t> entries;
    std::vector<uint64_t> words, list_counts;
    for (const std::string& s : b) {
        words.push_back(entries.size() / 8);
        list_counts.push_back((uint64_t)5 << 32 | 2u);
        const size_t at = entries.size();
        entries.resize(at + sx::seen_entry_bytes((uint32_t)s.size()), 0);
        *(uint32_t*)(entries.data() + at) = (uint32_t)s.size();
        memcpy(entries.data() + at + 8, s.data(), s.size());
        want[s] = sx::seen_count_sum(want.count(s) ? want[s] : 0, (uint64_t)5 << 32 | 2u);
    }
    SxmList* L = sxm_list_new(words.data(), words.size(), entries.data(), entries.size());
    if (!L) return fail("no list");
    std::vector<uint64_t> held((words.size() + 63) / 64 + 1);
    uint64_t minfo[4];
    if (sxc_merge_list(S, L, list_counts.data(), 2, 0, held.data(), minfo) != 0) return fail("the list's merge");
    sxm_list_free(L);
    if (counts_of(S) != want) return fail("the counts behind the list");

    // growth: everything into a fresh, larger set that counts
    SxsSeen* G = sxs_seen_new(-1, 24, 0, 500, 20000);
    SxcCounts* GK = G ? sxc_counts_new(G) : nullptr;
    if (!GK) return fail("no larger set");
    std::vector<uint64_t> gheld((((uint64_t)1 << S->dev.table_log2) + 63) / 64);
    if (sxc_merge_set(G, S, 1, 0, gheld.data(), minfo) != 0) return fail("the growth");
    if (counts_of(G) != want || G->dev.table_log2 <= S->dev.table_log2) return fail("the counts behind the growth");

    // the counts where the findings lie
    if (sxc_lookup(G, 1, recs_p, arena_p, ns, packed, 2, labels_p) != 0) return fail("the lookup");
    for (size_t i = 0; i < flat.size(); i++)
        if (labels[i] != want[flat[i]]) return fail("a finding's count word");

    sxc_counts_free(G, GK); sxs_seen_free(G);
    sxc_counts_free(S, K); sxs_seen_free(S);
    arena.drop();
    printf("ok\n");
    return 0;
}
