// Test-only program with a main of its own, for a sanitizer build (tests/test_seltally_core.py builds it with
// -fsanitize=address,undefined and starts it as a child process): it compiles the keywords it is given with sx_seltally_build.cpp,
// runs the lane functions of sx_seltally_core.hpp over the strings it is given, twice (the second time with the ordinals behind the
// first's), and prints the counters.  Input: the file argv[1], lines of "case FLAGS LDS_IDS", "p HEX" (a keyword), "s HEX" (a string,
// HEX may be missing: the empty string), "end"; output, per case: "rc CODE TEXT" where the builder refused it, else "hits H0 H1 ..."
// and "first F0 F1 ..." per input keyword.  The strings lie back to back in an allocation of exactly their size, and every table is
// a vector of exactly its size, so a read in front of or behind any of them is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_seltally_build.cpp"
#include "../../stringsext_amd/csrc/sx_seltally_core.hpp"

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    while (s[0] && s[1] && s[0] != '\n') {
        unsigned v = 0;
        sscanf(s, "%2x", &v);
        out.push_back((uint8_t)v);
        s += 2;
    }
    return out;
}

template <class E>
static void walk(const sx::SeltallyParams& P, const sx::SeltallyTable& T, const std::vector<uint8_t>& lds, uint64_t waves) {
    std::vector<uint32_t> counts(P.set.lds_ids ? P.set.lds_ids : 1, 0);
    for (uint64_t w = 0; w < waves; w++)
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            sx::SeltallyLane L = sx::seltally_begin_lane(P, w, lane);
            while (L.active) sx::seltally_step_lane<E>(P, T.map, (const E*)lds.data(), counts.data(), L);
        }
    for (uint32_t c = 0; c < P.set.lds_ids; c++) sx::seltally_flush_lane(P, counts.data(), c);
}

static void run_case(uint32_t flags, uint32_t lds_ids, const std::vector<std::vector<uint8_t>>& pats, const std::vector<std::vector<uint8_t>>& strs) {
    std::vector<sx_pattern> arr;
    for (const auto& p : pats) arr.push_back(sx_pattern{ p.data(), (uint32_t)p.size() });
    sx::SeltallyTable T;
    std::string err;
    const int rc = sx::seltally_build(arr.data(), (uint32_t)arr.size(), flags, &T, &err);
    if (rc != SX_OK) { printf("rc %d %s\n", rc, err.c_str()); return; }
    size_t total = 0;
    for (const auto& s : strs) total += s.size();
    uint8_t* arena = new uint8_t[total ? total : 1];
    std::vector<sx_finding> recs(strs.size());
    size_t off = 0;
    for (size_t i = 0; i < strs.size(); i++) {
        memset(&recs[i], 0, sizeof recs[i]);
        recs[i].str_off = (uint32_t)off; recs[i].str_len = (uint32_t)strs[i].size();
        if (!strs[i].empty()) memcpy(arena + off, strs[i].data(), strs[i].size());
        off += strs[i].size();
    }
    const uint64_t n = strs.size(), waves = (n + sx::kSelectRecs - 1) / sx::kSelectRecs;
    const std::vector<uint8_t> lds(T.next.begin(), T.next.begin() + (ptrdiff_t)((size_t)T.lds_states * T.classes * T.entry_bytes));
    std::vector<uint64_t> hits(T.unique, 0), first(T.unique, UINT64_MAX);
    sx::SeltallyParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs.data(); P.arena = arena; P.n = n; P.packed = 0;
    P.set = sx::SeltallyDevice{ T.map, T.next.data(), T.own.data(), T.dict.data(), hits.data(), first.data(),
                                T.states, T.classes, T.lds_states, T.entry_bytes, T.unique, T.unique < lds_ids ? T.unique : lds_ids };
    for (int pass = 0; pass < 2; pass++) {
        P.ordinal = 100 + pass * n;
        if (T.entry_bytes == 2) walk<uint16_t>(P, T, lds, waves);
        else walk<uint32_t>(P, T, lds, waves);
    }
    printf("hits");
    for (uint32_t p = 0; p < T.n_patterns; p++) printf(" %llu", (unsigned long long)hits[T.unique_of_pattern[p]]);
    printf("\nfirst");
    for (uint32_t p = 0; p < T.n_patterns; p++) printf(" %llu", (unsigned long long)first[T.unique_of_pattern[p]]);
    printf("\n");
    delete[] arena;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: seltally_build_main CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<char> line(1 << 16);
    uint32_t flags = 0, lds_ids = 0;
    std::vector<std::vector<uint8_t>> pats, strs;
    while (fgets(line.data(), (int)line.size(), f)) {
        if (!strncmp(line.data(), "case ", 5)) { pats.clear(); strs.clear(); sscanf(line.data() + 5, "%u %u", &flags, &lds_ids); }
        else if (line[0] == 'p') pats.push_back(unhex(line.data() + (line[1] == ' ' ? 2 : 1)));
        else if (line[0] == 's') strs.push_back(unhex(line.data() + (line[1] == ' ' ? 2 : 1)));
        else if (!strncmp(line.data(), "end", 3)) run_case(flags, lds_ids, pats, strs);
    }
    fclose(f);
    return 0;
}
