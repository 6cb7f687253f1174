// Test-only: memory that ends where a page without access begins, for every harness whose arenas must fault on a read or a write
// behind them.  The exported names are what the tests bind.
#pragma once
#include <stdint.h>
#include <sys/mman.h>
#include <unistd.h>

// `bytes` bytes that end where a page without access begins: a read or a write behind them faults.  *region, *region_bytes: what
// sxs_unmap takes
extern "C" void* sxs_guarded(uint64_t bytes, void** region, uint64_t* region_bytes) {
    const uint64_t page = (uint64_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
    uint8_t* p = (uint8_t*)mmap(nullptr, body + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) return nullptr;
    if (mprotect(p + body, page, PROT_NONE) != 0) { munmap(p, body + page); return nullptr; }
    *region = p; *region_bytes = body + page;
    return p + body - bytes;
}
extern "C" void sxs_unmap(void* region, uint64_t region_bytes) { munmap(region, region_bytes); }
