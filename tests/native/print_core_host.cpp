// Test-only harness: compiles the device formatter's core (sx_print_core.hpp) as host code and drives it the way
// sx_print_dev.hip does: pass 1 sums the line bytes of every wavefront's 64 records, an exclusive scan over the sums gives the
// wavefronts' offsets, then wavefront after wavefront — one more than the records need, as the last workgroup's idle wavefronts —
// runs the core's three lane loops on tables that stand for the wavefront's LDS.
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_print_core.hpp"

// tab: 256 x 16 bytes by mission_id (present, label length, label); text + base: where the segment's text begins.
extern "C" int sxp_print_host(const void* recs, uint64_t n, int packed, const uint8_t* arena, int file_id, int n_inputs, int radix,
                              int no_metadata, int n_missions, const uint8_t* tab, uint8_t* text, uint64_t base, uint64_t* text_len) {
    static_assert(sizeof(sx::PrintMission) == 16, "the test builds the Mission table as 16-byte rows");
    sx::PrintParams P;
    memset(&P, 0, sizeof P);
    P.recs = recs; P.arena = arena; P.n = n; P.packed = packed ? 1u : 0u; P.file_id = file_id;
    P.several_inputs = n_inputs > 1; P.radix = (uint32_t)radix; P.no_metadata = no_metadata != 0; P.several_missions = n_missions > 1;
    P.missions = (const sx::PrintMission*)tab;
    const uint64_t waves = (n + sx::kPrintRecs - 1) / sx::kPrintRecs;
    std::vector<uint64_t> wbase(waves + 2, 0);
    uint64_t sum = 0;
    for (uint64_t w = 0; w <= waves; w++) {
        wbase[w] = sum;
        for (uint32_t lane = 0; lane < sx::kPrintRecs; lane++) sum += sx::print_line_len(P, w * sx::kPrintRecs + lane);
    }
    wbase[waves + 1] = sum;
    *text_len = sum;
    P.wbase = wbase.data(); P.text = text; P.base = base;
    for (uint64_t w = 0; w <= waves; w++) {
        uint64_t lens[sx::kPrintRecs], offs[sx::kPrintRecs + 1], srcs[sx::kPrintRecs];
        uint8_t plens[sx::kPrintRecs];
        alignas(16) uint8_t pre[sx::kPrintRecs * sx::kPrintPrefix];
        memset(pre, 0xAA, sizeof pre);
        for (uint32_t lane = 0; lane < sx::kPrintRecs; lane++) sx::print_load_lane(P, w, lane, lens, srcs, plens, pre);
        for (uint32_t lane = 0; lane < sx::kPrintRecs; lane++) sx::print_scan_lane(lane, lens, offs);
        for (uint32_t lane = 0; lane < sx::kPrintRecs; lane++) sx::print_copy_lane(P, w, lane, offs, srcs, plens, pre);
    }
    return 0;
}

// an anonymous region whose untouched pages cost nothing (a text block of more than 4 GiB of which a few pages are written)
extern "C" void* sxp_map(uint64_t bytes) {
    void* p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    return p == MAP_FAILED ? nullptr : p;
}
extern "C" void sxp_unmap(void* p, uint64_t bytes) { munmap(p, bytes); }
