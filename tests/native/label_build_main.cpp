// Test-only program with a main of its own, for a sanitizer build (tests/test_label_core.py builds it with
// -fsanitize=address,undefined and starts it as a child process): it compiles the patterns it is given with sx_label_build.cpp, runs
// the lane functions of sx_label_core.hpp over the strings it is given and prints the labels.  Input: the file argv[1], lines of
// "case FLAGS", "p HEX" (a pattern), "s HEX" (a string, HEX may be missing: the empty string), "end"; output, per case: "rc CODE
// TEXT" where the builder refused it, else "lab L0 L1 ..." (hexadecimal), then "cnt" with findings:first per pattern.  The strings
// lie back to back in an allocation of exactly their size, so a read in front of or behind the arena is an error the sanitizer
// reports.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_label_build.cpp"
#include "../../stringsext_amd/csrc/sx_label_core.hpp"

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
    sx::LabelTable T;
    std::string err;
    const int rc = sx::label_build(arr.data(), (uint32_t)arr.size(), flags, &T, &err);
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
    uint64_t findings[sx::kLabelBits], first[sx::kLabelBits], mins[sx::kLabelBits];
    uint32_t counts[sx::kLabelBits];
    for (uint32_t c = 0; c < sx::kLabelBits; c++) { findings[c] = 0; first[c] = mins[c] = ~(uint64_t)0; counts[c] = 0; }
    sx::LabelParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs.data(); P.arena = arena; P.n = n; P.packed = 0; P.ordinal = 1000;
    P.set = sx::LabelDevice{ T.map, T.next.data(), T.here.data(), T.end.data(), findings, first, T.root_here, T.all,
                             T.states, T.classes, T.lds_states, T.here_first, T.dead, T.n_patterns };
    printf("lab");
    for (uint64_t w = 0; w < waves; w++) {
        uint64_t acc[sx::kSelectRecs], ored = 0;
        for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) {
            sx::LabelLane L = sx::label_begin_lane(P, w, lane);
            while (L.active) sx::label_step_lane(P, T.map, lds.data(), L);
            acc[lane] = L.acc; ored |= L.acc;
            if (w * sx::kSelectRecs + lane < n) printf(" %llx", (unsigned long long)L.acc);
        }
        for (uint64_t m = ored; m; m &= m - 1u) {
            const uint32_t p = (uint32_t)__builtin_ctzll(m);
            uint64_t ballot = 0;
            for (uint32_t lane = 0; lane < sx::kSelectRecs; lane++) ballot |= ((acc[lane] >> p) & 1u) << lane;
            sx::label_count_bit(counts, mins, p, ballot, P.ordinal + w * sx::kSelectRecs);
        }
    }
    for (uint32_t c = 0; c < sx::kLabelBits; c++) sx::label_flush_lane(P, counts, mins, c);
    printf("\ncnt");
    for (uint32_t p = 0; p < T.n_patterns; p++) printf(" %llu:%llu", (unsigned long long)findings[p], (unsigned long long)first[p]);
    printf("\n");
    delete[] arena;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: label_build_main CASES\n"); return 2; }
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
