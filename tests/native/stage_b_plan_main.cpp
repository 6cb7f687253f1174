// The stand-alone program of tests/test_stage_b_plan.py: sx_stage_b_plan.hpp under the address and undefined-behaviour sanitizers.
// Reads a file of cases, a line each — "<function> <u64> <u64> ..." —, and prints each answer as a line of numbers.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "stage_b_plan_host.cpp"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char* line = nullptr;
    size_t cap = 0;
    std::vector<uint64_t> args, out;
    while (getline(&line, &cap, f) > 0) {
        char* at = line;
        while (*at && *at != ' ' && *at != '\n') at++;
        const std::string fn(line, at);
        args.clear();
        for (;;) {
            char* end = nullptr;
            const unsigned long long v = strtoull(at, &end, 10);
            if (end == at) break;
            args.push_back(v); at = end;
        }
        out.assign(4 * args.size() + 16, 0);
        const long n = sbp_eval(fn.c_str(), args.data(), args.size(), out.data(), out.size());
        if (n < 0) { fprintf(stderr, "bad case: %s", line); return 1; }
        for (long i = 0; i < n; i++) printf(i ? " %llu" : "%llu", (unsigned long long)out[i]);
        printf("\n");
    }
    free(line);
    fclose(f);
    return 0;
}
