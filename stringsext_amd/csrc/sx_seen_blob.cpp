// sx_seen_blob.cpp — see sx_seen_blob.hpp.  Host C++ only.
#include "sx_seen_blob.hpp"

#include <string.h>

#include <exception>
#include <string_view>
#include <unordered_map>
#include <unordered_set>

namespace sx {

namespace {

const uint8_t kMagic[8] = { 'S', 'X', 'S', 'E', 'E', 'N', 0, 0 };

uint64_t le(const uint8_t* p, int bytes) {
    uint64_t v = 0;
    for (int k = 0; k < bytes; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}
void put_le(uint8_t* p, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; k++) p[k] = (uint8_t)(v >> (8 * k));
}

}  // namespace

uint64_t seen_blob_fnv(const uint8_t* p, uint64_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint64_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

void seen_blob_header(uint8_t* header, uint32_t nocase, uint64_t strings, const uint8_t* area, uint64_t bytes, uint32_t version) {
    memset(header, 0, kSeenBlobHeaderBytes);
    memcpy(header, kMagic, 8);
    put_le(header + 8, version, 4);
    put_le(header + 12, nocase, 4);
    put_le(header + 16, strings, 8);
    put_le(header + 24, bytes, 8);
    put_le(header + 32, seen_blob_fnv(area, bytes + (version == SX_SEEN_BLOB_VERSION_COUNTED ? 8u * strings : 0u)), 8);
}

int seen_blob_check(const void* blob, uint64_t len, sx_seen_blob_info* info, std::vector<uint64_t>* words, std::string* why, std::vector<uint64_t>* counts) {
    const uint8_t* const b = (const uint8_t*)blob;
    if (!b || len < kSeenBlobHeaderBytes) { *why = "shorter than its header"; return SX_E_INVALID; }
    if (memcmp(b, kMagic, 8) != 0) { *why = "no SXSEEN magic"; return SX_E_INVALID; }
    const uint64_t version = le(b + 8, 4), nocase = le(b + 12, 4), strings = le(b + 16, 8), bytes = le(b + 24, 8), sum = le(b + 32, 8);
    if (version != SX_SEEN_BLOB_VERSION && version != SX_SEEN_BLOB_VERSION_COUNTED) { *why = "version " + std::to_string(version); return SX_E_INVALID; }
    if (nocase > 1) { *why = "nocase " + std::to_string(nocase); return SX_E_INVALID; }
    for (uint64_t k = 40; k < kSeenBlobHeaderBytes; k++)
        if (b[k]) { *why = "a header byte behind the checksum is not 0"; return SX_E_INVALID; }
    if (bytes % 8 != 0) { *why = std::to_string(bytes) + " bytes of entries: no multiple of 8"; return SX_E_INVALID; }
    const bool counted = version == SX_SEEN_BLOB_VERSION_COUNTED;
    const uint64_t body = len - kSeenBlobHeaderBytes;
    // (version 2: body = bytes + 8 x strings, said without a sum or a product that could wrap)
    if (counted ? bytes > body || (body - bytes) % 8 != 0 || (body - bytes) / 8 != strings : body != bytes) {
        *why = std::to_string(len) + " bytes, the header says 64 + " + std::to_string(bytes) + (counted ? " + 8 x " + std::to_string(strings) : std::string());
        return SX_E_INVALID;
    }
    const uint8_t* const area = b + kSeenBlobHeaderBytes;
    if (seen_blob_fnv(area, body) != sum) { *why = "the checksum does not match"; return SX_E_INVALID; }
    try {
        std::unordered_set<std::string_view> have;
        if (words) words->clear();
        uint64_t at = 0, count = 0;
        while (at < bytes) {
            const uint64_t n = le(area + at, 4), end = at + SX_SEEN_ENTRY_BYTES(n);
            if (end > bytes) { *why = "the entry at " + std::to_string(at) + " overruns the entries"; return SX_E_INVALID; }
            if (le(area + at + 4, 4) != 0) { *why = "the entry at " + std::to_string(at) + ": its second word is not 0"; return SX_E_INVALID; }
            const uint8_t* s = area + at + 8;
            for (uint64_t k = n; at + 8 + k < end; k++)
                if (s[k]) { *why = "the entry at " + std::to_string(at) + ": its padding is not 0"; return SX_E_INVALID; }
            if (nocase)
                for (uint64_t k = 0; k < n; k++)
                    if (s[k] >= 'A' && s[k] <= 'Z') { *why = "the entry at " + std::to_string(at) + " is not folded"; return SX_E_INVALID; }
            if (!have.insert(std::string_view((const char*)s, n)).second) { *why = "the entry at " + std::to_string(at) + " equals an earlier one"; return SX_E_INVALID; }
            if (words) words->push_back(at / 8u);
            at = end; count++;
        }
        if (count != strings) { *why = std::to_string(count) + " entries, the header says " + std::to_string(strings); return SX_E_INVALID; }
        if (counts) counts->clear();
        for (uint64_t k = 0; counted && k < strings; k++) {
            const uint64_t c = le(area + bytes + 8u * k, 8), results = (c >> SX_SEEN_RESULTS_SHIFT) & 0xFFFFFFFFu, findings = (c >> SX_SEEN_FINDINGS_SHIFT) & 0xFFFFFFFFu;
            if (results == 0 || findings < results) { *why = "count word " + std::to_string(k) + ": " + std::to_string(results) + " results, " + std::to_string(findings) + " findings"; return SX_E_INVALID; }
            if (counts) counts->push_back(c);
        }
    } catch (const std::exception&) {
        *why = "no host memory to check the blob";
        return SX_E_NOMEM;
    }
    if (info) *info = sx_seen_blob_info{ strings, bytes, (uint32_t)nocase, (uint32_t)version };
    return SX_OK;
}

int seen_entries_build(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t nocase, std::vector<uint8_t>* arena, std::vector<uint64_t>* words,
                       std::vector<uint32_t>* kept_of, std::string* why) {
    arena->clear(); words->clear(); kept_of->clear();
    if (n > 0xFFFFFFFFull || (n && !offsets)) { *why = std::to_string(n) + " strings: 2^32 - 1 at most, and their offsets"; return SX_E_INVALID; }
    if (n == 0) return SX_OK;
    uint64_t room = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) { *why = "offsets[" + std::to_string(i + 1) + "] is smaller than the one in front of it"; return SX_E_INVALID; }
        if (offsets[i + 1] - offsets[0] > 0xFFFFFFFFull) { *why = "more than 2^32 - 1 bytes of strings"; return SX_E_INVALID; }
        room += SX_SEEN_ENTRY_BYTES(offsets[i + 1] - offsets[i]);
    }
    if (offsets[n] > offsets[0] && !bytes) { *why = "no bytes"; return SX_E_INVALID; }
    try {
        arena->resize(room);          // (never grown below: the views into it stay where they are)
        kept_of->resize(n);
        std::unordered_map<std::string_view, uint32_t> have;
        uint64_t at = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i], size = SX_SEEN_ENTRY_BYTES(len);
            uint8_t* e = arena->data() + at;
            memset(e, 0, size);
            e[0] = (uint8_t)len; e[1] = (uint8_t)(len >> 8); e[2] = (uint8_t)(len >> 16); e[3] = (uint8_t)(len >> 24);
            const uint8_t* s = bytes + offsets[i];
            for (uint64_t k = 0; k < len; k++) e[8 + k] = nocase && s[k] >= 'A' && s[k] <= 'Z' ? (uint8_t)(s[k] | 0x20) : s[k];
            const auto put = have.emplace(std::string_view((const char*)e + 8, len), (uint32_t)words->size());
            (*kept_of)[i] = put.first->second;
            if (!put.second) continue;                   // (an equal one is kept: this entry's room is written again)
            words->push_back(at / 8u);
            at += size;
        }
        arena->resize(at);
    } catch (const std::exception&) {
        *why = "no host memory for the strings' entries";
        return SX_E_NOMEM;
    }
    return SX_OK;
}

}  // namespace sx
