// Test-only program with a main of its own, for a sanitizer build (tests/test_seen_blob_host.py builds it with
// -fsanitize=address,undefined and starts it as a child process): the host code that checks a saved seen set and builds a source from
// a list of strings (sx_seen_blob.cpp).  Usage:
//   seen_blob_main check FILE...       per file "rc CODE STRINGS BYTES NOCASE WORDS" — the blob lies in an allocation of exactly its size,
//                                      so a read behind it is an error the sanitizer reports
//   seen_blob_main build NOCASE FILE   FILE: a line of hexadecimal per string (an empty line: the empty string); prints "rc CODE", then
//                                      "arena HEX", "words W0 W1 ..." and "kept K0 K1 ..."
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../stringsext_amd/csrc/sx_seen_blob.cpp"

static int check(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return 2; }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* blob = new uint8_t[size ? (size_t)size : 1];
    if (size && fread(blob, 1, (size_t)size, f) != (size_t)size) { fclose(f); delete[] blob; return 2; }
    fclose(f);
    sx_seen_blob_info info{};
    std::vector<uint64_t> words;
    std::string why;
    const int rc = sx::seen_blob_check(size ? blob : nullptr, (uint64_t)size, &info, &words, &why);
    printf("rc %d %llu %llu %u %zu\n", rc, (unsigned long long)info.strings, (unsigned long long)info.bytes, info.nocase, rc == SX_OK ? words.size() : 0);
    delete[] blob;
    return 0;
}

static int build(uint32_t nocase, const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets(1, 0);
    std::vector<char> line(1 << 16);
    while (fgets(line.data(), (int)line.size(), f)) {
        for (const char* s = line.data(); s[0] && s[1] && s[0] != '\n'; s += 2) {
            unsigned v = 0;
            sscanf(s, "%2x", &v);
            bytes.push_back((uint8_t)v);
        }
        offsets.push_back(bytes.size());
    }
    fclose(f);
    uint8_t* exact = new uint8_t[bytes.size() ? bytes.size() : 1];      // (of exactly the strings' size)
    if (!bytes.empty()) memcpy(exact, bytes.data(), bytes.size());
    std::vector<uint8_t> arena;
    std::vector<uint64_t> words;
    std::vector<uint32_t> kept_of;
    std::string why;
    const int rc = sx::seen_entries_build(exact, offsets.data(), offsets.size() - 1, nocase, &arena, &words, &kept_of, &why);
    delete[] exact;
    printf("rc %d\narena ", rc);
    for (uint8_t b : arena) printf("%02x", b);
    printf("\nwords");
    for (uint64_t w : words) printf(" %llu", (unsigned long long)w);
    printf("\nkept");
    for (uint32_t k : kept_of) printf(" %u", k);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "check")) {
        for (int i = 2; i < argc; i++) { const int rc = check(argv[i]); if (rc) return rc; }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "build")) return build((uint32_t)atoi(argv[2]), argv[3]);
    fprintf(stderr, "usage: seen_blob_main check FILE... | build NOCASE FILE\n");
    return 2;
}
