// sx_seen_blob.hpp — a seen set saved as bytes (sx_seen_set_export, sx_seen_blob_info_get, sx_seen_set_import) and the entries the
// host builds from a list of strings (sx_seen_set_add_strings).  No HIP header here or in sx_seen_blob.cpp: sx_seen_blob_info_get
// works on a machine without a GPU (tests/test_seen_blob_host.py).
//
// The blob: kSeenBlobHeaderBytes of header, little-endian —
//    0  "SXSEEN\0\0"      8  u32 version = 1     12  u32 nocase     16  u64 strings     24  u64 bytes
//   32  u64 FNV-1a-64 over the entry area         40  zeros
// — and then `bytes` bytes of entries as they lie in a set's arena: [u32 len][u32 0][the (folded) bytes, zero-padded to 8], one
// behind the other.  The kernels that take a blob's entries (sx_seen_merge_core.hpp) compare and copy whole words and trust that the
// entries are pairwise different and folded: seen_blob_check is where all of that is made sure of, before anything is allocated.
// A counted set's blob (sx_seen_count_core.hpp) has version = 2 and, behind the entry area, `strings` u64 count words in the order the
// entries lie in the area; its checksum covers the area followed by the count words, and it has 64 + bytes + 8 x strings bytes.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stringsext_amd.h"

namespace sx {

constexpr uint64_t kSeenBlobHeaderBytes = SX_SEEN_BLOB_HEADER_BYTES;

uint64_t seen_blob_fnv(const uint8_t* p, uint64_t n);

// The header of a blob whose entry area is area[0, bytes); version 2: and whose count words lie behind it, area[bytes, bytes + 8 x strings)
void seen_blob_header(uint8_t* header, uint32_t nocase, uint64_t strings, const uint8_t* area, uint64_t bytes, uint32_t version = SX_SEEN_BLOB_VERSION);

// One walk over a blob: SX_OK and *info, or SX_E_INVALID with *why said (wrong magic or version, len other than 64 + bytes, bytes no
// multiple of 8, nocase other than 0 / 1, an entry that overruns the area, a second u32 or padding that is not 0, an entry count other
// than `strings`, a checksum that does not match, two equal entries, with nocase a byte that is not folded), or SX_E_NOMEM if the host
// has no memory for the walk.  words (may be NULL): per entry its offset / 8 in the area, in the area's order — a source's word list.
// Version 2 also: len other than 64 + bytes + 8 x strings, a count word whose results are 0 or whose findings are fewer than its
// results.  counts (may be NULL): the count words, in the words' order; empty for version 1.
int seen_blob_check(const void* blob, uint64_t len, sx_seen_blob_info* info, std::vector<uint64_t>* words, std::string* why, std::vector<uint64_t>* counts = nullptr);

// n strings, string i = bytes[offsets[i], offsets[i + 1]), as a source: folded under `nocase`, the first of every group of equal ones
// kept.  arena: their entries one behind the other; words: per kept string its entry's offset / 8; kept_of[i]: which kept string
// input i equals.  SX_OK, SX_E_INVALID with *why said (n or offsets[n] above 2^32 - 1, offsets that decrease), SX_E_NOMEM.
int seen_entries_build(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t nocase, std::vector<uint8_t>* arena, std::vector<uint64_t>* words,
                       std::vector<uint32_t>* kept_of, std::string* why);

}  // namespace sx
