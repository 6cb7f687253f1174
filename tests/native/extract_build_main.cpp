// Test-only program with a main of its own, for a sanitizer build (tests/test_extract_core.py builds it with
// -fsanitize=address,undefined and starts it as a child process): it compiles the patterns it is given with sx_extract_build.cpp,
// runs the lane functions of sx_extract_core.hpp over the strings it is given and prints the matches.  Input: the file argv[1], lines
// of "case FLAGS", "p HEX" (a pattern), "s HEX" (a string, HEX may be missing: the empty string), "end"; output, per case:
// "rc CODE TEXT" where the builder refused it, else "m I:FROM-END I:FROM-END ...".  The strings lie back to back in an allocation of
// exactly their size, so a read in front of or behind the arena is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_extract_build.cpp"
#include "../../stringsext_amd/csrc/sx_extract_core.hpp"

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

static void run_case(uint32_t flags, const std::vector<std::vector<uint8_t>>& pats, const std::vector<std::vector<uint8_t>>& strs) {
    std::vector<sx_pattern> arr;
    for (const auto& p : pats) arr.push_back(sx_pattern{ p.data(), (uint32_t)p.size() });
    sx::ExtractTable T;
    std::string err;
    const int rc = sx::extract_build(arr.data(), (uint32_t)arr.size(), flags, &T, &err);
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
    const std::vector<uint16_t> lds(T.next.begin(), T.next.begin() + (ptrdiff_t)((size_t)T.lds_states * T.classes));
    sx::ExtractParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs.data(); P.arena = arena; P.n = n; P.packed = 0;
    P.ex = sx::ExtractDevice{ T.map, T.next.data(), T.states, T.classes, T.lds_states, T.end_first, T.here_first, T.dead_first, T.start0, T.start1 };
    printf("m");
    for (uint64_t w = 0; w <= waves; w++)
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            sx::ExtractLane L = sx::extract_begin_lane(P, w, lane);
            while (L.active) {
                uint32_t from = 0;
                const uint32_t end = sx::extract_step_lane(P, T.map, lds.data(), L, &from);
                if (end) printf(" %llu:%u-%u", (unsigned long long)(w * sx::kSelectRecs + lane), from, end);
            }
        }
    printf("\n");
    delete[] arena;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: extract_build_main CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<char> line(1 << 16);
    uint32_t flags = 0;
    std::vector<std::vector<uint8_t>> pats, strs;
    while (fgets(line.data(), (int)line.size(), f)) {
        if (!strncmp(line.data(), "case ", 5)) { pats.clear(); strs.clear(); sscanf(line.data() + 5, "%u", &flags); }
        else if (line[0] == 'p') pats.push_back(unhex(line.data() + (line[1] == ' ' ? 2 : 1)));
        else if (line[0] == 's') strs.push_back(unhex(line.data() + (line[1] == ' ' ? 2 : 1)));
        else if (!strncmp(line.data(), "end", 3)) run_case(flags, pats, strs);
    }
    fclose(f);
    return 0;
}
