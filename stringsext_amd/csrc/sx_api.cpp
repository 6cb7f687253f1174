// sx_api.cpp — the C-ABI of include/stringsext_amd.h: context and HIP resources, the lower-level
// stages as entry points, results, utilities.  (sx_scan* live in sx_ingest.cpp.)
#include "sx_ctx.hpp"
#include "sx_print_core.hpp"
#include "sx_select_core.hpp"
#include "sx_selset_build.hpp"
#include "sx_selset_core.hpp"
#include "sx_selre_build.hpp"
#include "sx_selre_core.hpp"
#include "sx_extract_build.hpp"
#include "sx_extract_core.hpp"
#include "sx_seltally_build.hpp"
#include "sx_seltally_core.hpp"
#include "sx_label_build.hpp"
#include "sx_label_core.hpp"

using namespace sx;

// sx_select_set_create: a compiled keyword list; `mem` = [the class map][the table], device memory of its own
struct sx_select_set {
    int device = 0;
    uint8_t* mem = nullptr;
    SelsetDevice dev{};
    sx_select_set_info info{};
};

// sx_select_regex_create: compiled regular expressions; `mem` as a set's
struct sx_select_regex {
    int device = 0;
    uint8_t* mem = nullptr;
    SelreDevice dev{};
    sx_select_regex_info info{};
};

// sx_extract_regex_create: regular expressions compiled for the extraction; `mem` as a set's
struct sx_extract_regex {
    int device = 0;
    uint8_t* mem = nullptr;
    ExtractDevice dev{};
    sx_extract_regex_info info{};
};

// sx_tally_set_create: a keyword list compiled for the tally; `mem` = [the class map][the table][own][dict][pattern -> unique id]
// [hits][first], device memory of its own
struct sx_tally_set {
    int device = 0;
    uint8_t* mem = nullptr;
    SeltallyDevice dev{};
    const uint32_t* d_unique_of_pattern = nullptr;
    std::vector<uint32_t> unique_of_pattern;
    sx_tally_set_info info{};
};

// sx_label_set_create: regular expressions compiled for the labels; `mem` = [the class map][the table][here][end][findings][first],
// device memory of its own
struct sx_label_set {
    int device = 0;
    uint8_t* mem = nullptr;
    LabelDevice dev{};
    sx_label_set_info info{};
};

// sx_result_label_device: one result's labels; `mem` = an array per source segment, each 256-byte aligned, device memory of its own.
// Per segment what tells the source apart: where its records lie, how many they are, and the epoch of its block when it was labelled.
struct sx_labels {
    struct Seg {
        const uint64_t* d = nullptr;
        const void* recs = nullptr;
        uint64_t n = 0;
        std::shared_ptr<std::atomic<uint64_t>> epoch_ref;
        uint64_t epoch = 0;
    };
    int device = 0;
    uint8_t* mem = nullptr;
    std::vector<Seg> segs;
};

namespace sx {
PinnedPool::Block PinnedPool::take(size_t bytes) {
    {
        std::lock_guard<std::mutex> g(mu);
        size_t best = free_blocks.size();
        for (size_t i = 0; i < free_blocks.size(); i++)
            if (free_blocks[i].cap >= bytes && (best == free_blocks.size() || free_blocks[i].cap < free_blocks[best].cap)) best = i;
        if (best < free_blocks.size() && free_blocks[best].cap <= 4 * bytes + (4u << 20)) {
            Block b = free_blocks[best];
            free_blocks.erase(free_blocks.begin() + (long)best);
            return b;
        }
    }
    Block b;
    const size_t cap = bytes + bytes / 8 + (1u << 20);
    if (hipHostMalloc(&b.p, cap, hipHostMallocNonCoherent) != hipSuccess) { b.p = nullptr; return b; }
    b.cap = cap;
    return b;
}
void PinnedPool::give(Block b) {
    if (!b.p) return;
    std::lock_guard<std::mutex> g(mu);
    free_blocks.push_back(b);
    if (free_blocks.size() > 40) {  // a result of a large buffer holds one block per piece; beyond that, drop the smallest
        size_t m = 0;
        for (size_t i = 1; i < free_blocks.size(); i++) if (free_blocks[i].cap < free_blocks[m].cap) m = i;
        (void)hipHostFree(free_blocks[m].p);
        free_blocks.erase(free_blocks.begin() + (long)m);
    }
}
PinnedPool::~PinnedPool() { for (Block& b : free_blocks) (void)hipHostFree(b.p); }
}  // namespace sx

namespace {
std::string g_create_error;
}  // namespace

namespace sx {

double g_tl_t0 = 0;
int g_tl_on = 0;

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}


int ensure_pinned(sx_ctx* ctx, uint64_t bytes) {
    if (ctx->h_pin_cap >= bytes) return SX_OK;
    if (ctx->h_pin) HIP_TRY(ctx, hipHostFree(ctx->h_pin));
    ctx->h_pin = nullptr; ctx->h_pin_cap = 0;
    bytes += bytes / 4 + (1u << 20);
    unsigned flags = hipHostMallocNonCoherent;  // CPU-cached: it is only read by the host after a stream sync
    if (ctx->sw.pin_flags >= 0) flags = (unsigned)ctx->sw.pin_flags;
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_pin, bytes, flags));
    ctx->h_pin_cap = bytes;
    return SX_OK;
}
int read_back_async(sx_ctx* ctx, hipStream_t s, void* pinned_dst, const void* dev_src, size_t bytes) {
    if (ctx->sw.small_copy && bytes <= (1u << 20) && ((((uintptr_t)pinned_dst | (uintptr_t)dev_src | bytes) & 3) == 0))
        HIP_TRY(ctx, launch_small_copy(pinned_dst, dev_src, bytes, s));
    else HIP_TRY(ctx, hipMemcpyAsync(pinned_dst, dev_src, bytes, hipMemcpyDeviceToHost, s));
    return SX_OK;
}
int read_back_sync(sx_ctx* ctx, MissionDev& d, hipStream_t s, void* host_dst, const void* dev_src, size_t bytes) {
    if (!ctx->sw.small_copy || bytes > kSmallReadBytes || ((((uintptr_t)dev_src | bytes) & 3) != 0)) {
        HIP_TRY(ctx, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        return SX_OK;
    }
    if (!d.h_small) HIP_TRY(ctx, hipHostMalloc((void**)&d.h_small, kSmallReadBytes, hipHostMallocDefault));
    HIP_TRY(ctx, launch_small_copy(d.h_small, dev_src, bytes, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    memcpy(host_dst, d.h_small, bytes);
    return SX_OK;
}
int ensure_pinned2(sx_ctx* ctx, uint64_t bytes) {
    if (ctx->h_pin2_cap >= bytes) return SX_OK;
    if (ctx->h_pin2) HIP_TRY(ctx, hipHostFree(ctx->h_pin2));
    ctx->h_pin2 = nullptr; ctx->h_pin2_cap = 0;
    bytes += bytes / 4 + (1u << 20);
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_pin2, bytes, hipHostMallocNonCoherent));
    ctx->h_pin2_cap = bytes;
    return SX_OK;
}
int ensure_scratch(sx_ctx* ctx, uint64_t bytes) {
    std::lock_guard<std::recursive_mutex> g(ctx->grow_mu);
    if (ctx->d_scratch_cap >= bytes) return SX_OK;
    if (ctx->merge_async) { const int rc = merge_drain(ctx); if (rc != SX_OK) return rc; }   // (a queued sort may read its cut table here)
    if (ctx->d_scratch) HIP_TRY(ctx, hipFree(ctx->d_scratch));
    ctx->d_scratch = nullptr; ctx->d_scratch_cap = 0;
    bytes += bytes / 4 + (1u << 20);
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_scratch, bytes));
    ctx->d_scratch_cap = bytes;
    return SX_OK;
}

int ensure_capacity(sx_ctx* ctx, ScanSlot& s, uint32_t cap) {
    if (s.capacity >= cap) return SX_OK;
    if (s.d_recs) HIP_TRY(ctx, hipFree(s.d_recs));
    s.d_recs = nullptr; s.capacity = 0;
    HIP_TRY(ctx, hipMalloc((void**)&s.d_recs, (size_t)cap * sizeof(DevRun)));
    s.capacity = cap;
    return SX_OK;
}

// Stage A for a set of missions: launch every mission's kernel on its own stream, then
// collect, growing a record buffer and re-running that mission if it overflowed.
// Pass 1's output cache: one for all missions (their stage B runs one after the other).
int ensure_cache(sx_ctx* ctx, uint64_t bytes) {
    if (ctx->d_cache_cap >= bytes) return SX_OK;
    if (ctx->d_cache) HIP_TRY(ctx, hipFree(ctx->d_cache));
    ctx->d_cache = nullptr; ctx->d_cache_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_cache, bytes));
    ctx->d_cache_cap = bytes;
    return SX_OK;
}
int ensure_rp(sx_ctx* ctx, MissionDev& d, int slot, uint64_t bytes) {
    if (d.d_rp_cap[slot] >= bytes) return SX_OK;   // (a Mission's buffers are its own thread's)
    std::lock_guard<std::recursive_mutex> g(ctx->grow_mu);
    if (ctx->merge_async) { const int rc = merge_drain(ctx); if (rc != SX_OK) return rc; }   // (a queued sort may still read this Mission's findings)
    if (d.d_rp[slot]) HIP_TRY(ctx, hipFree(d.d_rp[slot]));
    d.d_rp[slot] = nullptr; d.d_rp_cap[slot] = 0;
    bytes += bytes / 4 + 4096;
    HIP_TRY(ctx, hipMalloc(&d.d_rp[slot], bytes));
    d.d_rp_cap[slot] = bytes;
    return SX_OK;
}


// CPUs this process may really use: the cgroup quota can be far below the visible cores.
unsigned usable_cpus() {
    unsigned n = std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char a[64] = { 0 };
        unsigned long long period = 0;
        if (fscanf(f, "%63s %llu", a, &period) == 2 && strcmp(a, "max") != 0 && period > 0) {
            const unsigned long long quota = strtoull(a, nullptr, 10);
            const unsigned q = (unsigned)((quota + period - 1) / period);
            if (q >= 1 && q < n) n = q;
        }
        fclose(f);
    }
    return n;
}

unsigned replay_threads(const sx_ctx* ctx) {
    // a few threads per usable CPU smooth out the quota's time slicing (measured: 4x is best)
    unsigned n = ctx->opt.replay_threads ? ctx->opt.replay_threads
                                         : std::min(std::thread::hardware_concurrency(), 4 * usable_cpus());
    if (ctx->sw.replay_threads) n = (unsigned)ctx->sw.replay_threads;
    if (n < 1) n = 1;
    return n > 256 ? 256 : n;
}


void begin_call(sx_ctx* ctx) {
    memset(&ctx->stats, 0, sizeof ctx->stats);
    ctx->err.clear();
    ctx->sharded_call = false;
    ctx->dev_epoch->fetch_add(1);   // (results left on the device by an earlier call — SX_OPT_RESULT_ON_DEVICE — are the context's memory: gone now)
}

// SX_OPT_RESULT_ON_DEVICE: a segment that still lies in HBM comes to the host (the host accessors' first use of it)
static int fetch_to_host(sx_result* r, MissionFindings& s) {
    if (!s.dev_only) return SX_OK;
    if (!s.keep_on_device || !s.dev_epoch_ref || s.dev_epoch_ref->load() != s.dev_epoch) return SX_E_STATE;   // (a later scan has reused the memory)
    const size_t bytes = s.ext_nf * s.rec_size() + s.ext_na;
    PinnedPool::Block blk = r->r.pool ? r->r.pool->take(bytes + 64) : PinnedPool::Block{};
    if (!blk.p) return SX_E_NOMEM;
    if (hipMemcpy(blk.p, s.dev_copy, bytes, hipMemcpyDeviceToHost) != hipSuccess) { r->r.pool->give(blk); return SX_E_HIP; }
    s.ext = blk; s.dev_only = false;
    return SX_OK;
}
static int fetch_all_to_host(const sx_result* r) {
    sx_result* w = const_cast<sx_result*>(r);
    for (auto& s : w->r.segs) { const int rc = fetch_to_host(w, s); if (rc != SX_OK) return rc; }
    return SX_OK;
}


}  // namespace sx

extern "C" {

int sx_abi_version(void) { return SX_ABI_VERSION; }

const uint16_t* sx_decoder_table(uint32_t encoding, uint64_t* n_words) {
    size_t n = 0;
    const uint16_t* t = decoder_table((int)encoding, &n);
    if (n_words) *n_words = n;
    return t;
}

const uint32_t* sx_wave_pair_codes(const sx_mission* mission, uint32_t* out8192) {
    if (!mission || !out8192) return nullptr;
    Mission m;
    std::string err;
    if (Mission::from_c(*mission, false, Switches{}.wave_same, &m, &err) != SX_OK || m.wave_pairs.size() != 8192) return nullptr;
    memcpy(out8192, m.wave_pairs.data(), 8192 * 4);
    return out8192;
}

const uint32_t* sx_wave_pair_codes2(const sx_mission* mission, uint32_t* out4096) {
    if (!mission || !out4096) return nullptr;
    Mission m;
    std::string err;
    if (Mission::from_c(*mission, false, Switches{}.wave_same, &m, &err) != SX_OK || m.wave_pairs2.size() != 4096) return nullptr;
    memcpy(out4096, m.wave_pairs2.data(), 4096 * 4);
    return out4096;
}

int sx_wave_swar(const sx_mission* mission, uint32_t* out26) {
    if (!mission || !out26) return SX_E_INVALID;
    Mission m;
    std::string err;
    const int rc = Mission::from_c(*mission, false, Switches{}.wave_same, &m, &err);
    if (rc != SX_OK) return rc;
    static_assert(sizeof(WvSwar) == 26 * 4, "sx_wave_swar hands the struct out as 26 words");
    memcpy(out26, &m.wave_swar, sizeof(WvSwar));
    return m.wave_ok && m.wave_swar.cls ? 1 : 0;
}

int sx_scan_classifier(const sx_mission* mission, int generic, uint32_t* out20) {
    if (!mission || !out20) return SX_E_INVALID;
    Mission m;
    std::string err;
    const int rc = Mission::from_c(*mission, generic != 0, Switches{}.wave_same, &m, &err);
    if (rc != SX_OK) return rc;
    const ScanParams& p = m.proto;
    const uint32_t head[7] = { p.a_lo, p.a_hi, p.u_lo, p.u_hi, p.l3_lo, p.l3_hi, p.n_ranges };
    memcpy(out20, head, sizeof head);
    memcpy(out20 + 7, p.rng_c1, 6 * sizeof(uint32_t));
    memcpy(out20 + 13, p.rng_c2, 6 * sizeof(uint32_t));
    out20[19] = 0;
    return (int)m.kind;
}

int sx_wave_classes(const sx_mission* mission, uint8_t* classes) {
    if (!mission || !classes) return SX_E_INVALID;
    Mission m;
    std::string err;
    const int rc = Mission::from_c(*mission, false, Switches{}.wave_same, &m, &err);
    if (rc != SX_OK) return rc;
    if (!m.wave_ok || m.wave_lead_check || (m.wave_lut.size() != 256 && !(m.wave_family == 2 && m.wave_lut.size() == 512))) return 0;   // (wave_lead_check: -r, covered per buffer only)
    memcpy(classes, m.wave_lut.data(), m.wave_lut.size());   // (UTF-16: 512 bytes)
    return 1 + (int)m.wave_family;
}

int sx_create(sx_ctx** out, const sx_mission* missions, int n_missions, int hip_device, const sx_options* opt) {
    if (!out || !missions || n_missions <= 0 || n_missions > 26) { g_create_error = "bad arguments"; return SX_E_INVALID; }
    sx_ctx* ctx = new sx_ctx();
    ctx->sw = Switches::from_env();   // the one reading of the environment: everything below the C-ABI asks ctx->sw
    if (opt) ctx->opt = *opt;
    if (ctx->sw.result_on_device) ctx->opt.flags |= SX_OPT_RESULT_ON_DEVICE;   // (tests / fuzz: the flag through the environment)
    ctx->missions.resize((size_t)n_missions);
    ctx->states.resize((size_t)n_missions);
    for (int k = 0; k < n_missions; k++) {
        std::string err;
        int rc = Mission::from_c(missions[k], (ctx->opt.flags & SX_OPT_GENERIC_KERNELS) != 0, ctx->sw.wave_same, &ctx->missions[(size_t)k], &err);
        if (rc != SX_OK) { g_create_error = "mission " + std::to_string(k) + ": " + err; delete ctx; return rc; }
        ctx->states[(size_t)k].reset(ctx->missions[(size_t)k]);
    }
    if (hip_device == SX_HOST_ONLY) { ctx->host_only = true; *out = ctx; return SX_OK; }

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0 || hip_device < 0 || hip_device >= n_dev) {
        g_create_error = std::string("no usable HIP device (hipGetDeviceCount: ")
                         + (e == hipSuccess ? "ok" : hipGetErrorString(e)) + ", devices=" + std::to_string(n_dev)
                         + ", requested=" + std::to_string(hip_device) + "); the scan only runs on the GPU";
        delete ctx;
        return SX_E_NO_DEVICE;
    }
    ctx->device = hip_device;
    auto fail = [&](const char* what, hipError_t err) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(err);
        sx_destroy(ctx);
        return SX_E_HIP;
    };
    if ((e = hipSetDevice(hip_device)) != hipSuccess) return fail("hipSetDevice", e);
    ctx->dev.resize((size_t)n_missions);
    const uint32_t cap = ctx->opt.record_capacity ? ctx->opt.record_capacity : (1u << 20);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, hip_device) == hipSuccess && cus > 0) ctx->n_cus = (unsigned)cus;
        if (ctx->sw.scan_blocks_per_cu >= 0) ctx->scan_blocks_per_cu = (unsigned)ctx->sw.scan_blocks_per_cu;
        if (ctx->sw.region_cap >= 0) ctx->region_cap = (uint32_t)ctx->sw.region_cap;
        if (ctx->sw.scan_cus) ctx->n_cus = (unsigned)ctx->sw.scan_cus;  // tests: persistent grid on small inputs
    }
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);  // numerically lower = higher priority
    if (ctx->sw.prio_n >= 0) {
        if (ctx->sw.prio_n >= 1) prio_lo = ctx->sw.prio_scan;
        if (ctx->sw.prio_n >= 2) prio_hi = ctx->sw.prio_post;
        fprintf(stderr, "[sx] stream priorities: scan %d, post %d\n", prio_lo, prio_hi);
    }
    // Two streams for the whole context: the scan kernels of all missions queue up in one (a
    // kernel alone already fills the device, and HIP multiplexes streams onto few hardware
    // queues: more streams only alias), everything else runs in a second, higher-priority one
    // so that it overlaps the scans of the next piece.  SX_OPT_MISSION_STREAMS: a scan stream per mission.
    const bool per_mission = (ctx->opt.flags & SX_OPT_MISSION_STREAMS) || ctx->sw.mission_streams;
    if ((e = hipStreamCreateWithPriority(&ctx->post_stream, hipStreamNonBlocking, prio_hi)) != hipSuccess) return fail("hipStreamCreate", e);
    if (!per_mission && (e = hipStreamCreateWithPriority(&ctx->scan_stream, hipStreamNonBlocking, prio_lo)) != hipSuccess)
        return fail("hipStreamCreate", e);
    for (auto& d : ctx->dev) {
        d.stream_b = ctx->post_stream;
        if (per_mission) {
            if ((e = hipStreamCreateWithPriority(&d.stream, hipStreamNonBlocking, prio_lo)) != hipSuccess) return fail("hipStreamCreate", e);
        } else d.stream = ctx->scan_stream;
        for (ScanSlot& s : d.slot) {
            if ((e = hipEventCreate(&s.ev0)) != hipSuccess) return fail("hipEventCreate", e);
            if ((e = hipEventCreate(&s.ev1)) != hipSuccess) return fail("hipEventCreate", e);
            if ((e = hipEventCreateWithFlags(&s.ev_free, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
            if ((e = hipMalloc((void**)&s.d_counters, kCounterWords * sizeof(uint32_t))) != hipSuccess) return fail("hipMalloc", e);
            if ((e = hipMalloc((void**)&s.d_recs, (size_t)cap * sizeof(DevRun))) != hipSuccess) return fail("hipMalloc", e);
            s.capacity = cap;
        }
    }
    for (size_t k = 0; k < ctx->dev.size(); k++) {
        size_t n_words = 0;
        if (const uint16_t* t = decoder_table(ctx->missions[k].c.encoding, &n_words)) {
            if ((e = hipMalloc((void**)&ctx->dev[k].d_table, n_words * 2)) != hipSuccess) return fail("hipMalloc", e);
            if ((e = hipMemcpy(ctx->dev[k].d_table, t, n_words * 2, hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy", e);
        }
        const std::vector<uint32_t>& pl = ctx->missions[k].pair_lut;
        if (!pl.empty()) {
            if ((e = hipMalloc((void**)&ctx->dev[k].d_pair_lut, pl.size() * 4)) != hipSuccess) return fail("hipMalloc", e);
            if ((e = hipMemcpy(ctx->dev[k].d_pair_lut, pl.data(), pl.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy", e);
        }
    }
    *out = ctx;
    return SX_OK;
}

void sx_destroy(sx_ctx* ctx) {
    if (!ctx) return;
    // results may outlive the context (they share the pinned pool and the epoch word): what they left in HBM is freed below, so the
    // accessors must answer SX_E_STATE from here on
    ctx->dev_epoch->fetch_add(1);
    for (auto& e : ctx->select_epoch) e->fetch_add(1);
    if (!ctx->host_only && ctx->device >= 0) {
        (void)hipSetDevice(ctx->device);
        for (auto& d : ctx->dev) {
            if (d.stream) (void)hipStreamSynchronize(d.stream);
            if (d.stream_b) (void)hipStreamSynchronize(d.stream_b);
            for (ScanSlot& s : d.slot) {
                if (s.d_recs) (void)hipFree(s.d_recs);
                if (s.d_cnt) (void)hipFree(s.d_cnt);
                if (s.d_grid) (void)hipFree(s.d_grid);
                if (s.d_packed) (void)hipFree(s.d_packed);
                if (s.d_counters) (void)hipFree(s.d_counters);
                if (s.ev0) (void)hipEventDestroy(s.ev0);
                if (s.ev1) (void)hipEventDestroy(s.ev1);
                if (s.ev_free) (void)hipEventDestroy(s.ev_free);
            }
            if (d.d_table) (void)hipFree(d.d_table);
            if (d.d_pair_lut) (void)hipFree(d.d_pair_lut);
            if (d.d_wave_lut) (void)hipFree(d.d_wave_lut);
            if (d.d_wave_pairs) (void)hipFree(d.d_wave_pairs);
            if (d.d_wave_pairs2) (void)hipFree(d.d_wave_pairs2);
            for (void* q : d.d_rp) if (q) (void)hipFree(q);
            if (d.h_runs) (void)hipHostFree(d.h_runs);
            if (d.ev_runs) (void)hipEventDestroy(d.ev_runs);
            if (d.stream_w) (void)hipStreamDestroy(d.stream_w);
            if (d.h_tot) (void)hipHostFree(d.h_tot);
            if (d.h_small) (void)hipHostFree(d.h_small);
            for (hipEvent_t e : d.wave_ev) if (e) (void)hipEventDestroy(e);
            if (d.stream && d.stream != ctx->scan_stream) (void)hipStreamDestroy(d.stream);
        }
        for (int i = 0; i < 2; i++) {
            if (ctx->ing_pin[i]) (void)hipHostFree(ctx->ing_pin[i]);
            if (ctx->ing_dev[i]) (void)hipFree(ctx->ing_dev[i]);
        }
        if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
        if (ctx->d2h_stream) (void)hipStreamDestroy(ctx->d2h_stream);
        if (ctx->scan_stream) (void)hipStreamDestroy(ctx->scan_stream);
        if (ctx->d_cache) (void)hipFree(ctx->d_cache);
        if (ctx->post_stream) (void)hipStreamDestroy(ctx->post_stream);
        if (ctx->merge_copy_stream) (void)hipStreamDestroy(ctx->merge_copy_stream);
        if (ctx->d_merge) (void)hipFree(ctx->d_merge);
        if (ctx->d_result) (void)hipFree(ctx->d_result);
        if (ctx->d_result_up) (void)hipFree(ctx->d_result_up);
        if (ctx->d_text) (void)hipFree(ctx->d_text);
        if (ctx->d_print_scratch) (void)hipFree(ctx->d_print_scratch);
        if (ctx->d_print_missions) (void)hipFree(ctx->d_print_missions);
        for (uint8_t* p : ctx->d_select) if (p) (void)hipFree(p);
        if (ctx->d_select_scratch) (void)hipFree(ctx->d_select_scratch);
        if (ctx->d_select_scratch2) (void)hipFree(ctx->d_select_scratch2);
        for (hipEvent_t e : ctx->merge_ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ctx->slab_ev) if (e) (void)hipEventDestroy(e);
        if (ctx->ev_interleaved) (void)hipEventDestroy(ctx->ev_interleaved);
        if (ctx->d_input) (void)hipFree(ctx->d_input);
        if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
        if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
        if (ctx->h_pin2) (void)hipHostFree(ctx->h_pin2);
    }
    delete ctx;
}

const char* sx_last_error(const sx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int sx_reset(sx_ctx* ctx) {
    if (!ctx) return SX_E_INVALID;
    for (size_t k = 0; k < ctx->missions.size(); k++) ctx->states[k].reset(ctx->missions[k]);
    ctx->shard_runs_valid = false;
    return SX_OK;
}

// Device-resident input: download only the byte ranges the replay will look at.

int sx_device_runs(sx_ctx* ctx, int mission_index, const void* device_bytes, uint64_t len, int stream_parity,
                   uint64_t min_chars, sx_run** runs, uint64_t* n_runs) {
    if (!ctx || !runs || !n_runs || mission_index < 0 || (size_t)mission_index >= ctx->missions.size()) return SX_E_INVALID;
    begin_call(ctx);
    ctx->sw.scan_warm = Switches::from_env().scan_warm;   // (the one switch read after sx_create, sx_switches.hpp: measurements set it around this call on a live context)
    if (ctx->host_only) { ctx->err = "host-only context: no device scan"; return SX_E_STATE; }
    if ((uintptr_t)device_bytes & 15) { ctx->err = "device_bytes must be 16-byte aligned"; return SX_E_INVALID; }
    if (ctx->missions[(size_t)mission_index].host_sequential()) { ctx->err = "an ISO-2022-JP mission has no stage A (one sequential pass on the host)"; return SX_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<RunList> out;
    ctx->shard_runs_valid = false;  // the mission's device-side run list is about to be replaced
    int rc = device_runs(ctx, { mission_index }, (const uint8_t*)device_bytes, len, { (uint32_t)(stream_parity & 1) },
                         { min_chars }, &out);
    if (rc != SX_OK) return rc;
    HIP_TRY(ctx, out[0].wait());
    *n_runs = out[0].size();
    *runs = (sx_run*)malloc(sizeof(sx_run) * (out[0].size() ? out[0].size() : 1));
    if (!*runs) return SX_E_NOMEM;
    memcpy(*runs, out[0].data(), sizeof(sx_run) * out[0].size());
    return SX_OK;
}

int sx_device_runs_multi(sx_ctx* ctx, const int* mission_indices, int n, const void* device_bytes, uint64_t len, int stream_parity,
                         const uint64_t* min_chars, sx_run** runs, uint64_t* n_runs) {
    if (!ctx || !mission_indices || n <= 0 || !min_chars || !runs || !n_runs) return SX_E_INVALID;
    begin_call(ctx);
    if (ctx->host_only) { ctx->err = "host-only context: no device scan"; return SX_E_STATE; }
    if ((uintptr_t)device_bytes & 15) { ctx->err = "device_bytes must be 16-byte aligned"; return SX_E_INVALID; }
    std::vector<int> which; std::vector<uint32_t> par; std::vector<uint64_t> mc;
    for (int i = 0; i < n; i++) {
        const int k = mission_indices[i];
        if (k < 0 || (size_t)k >= ctx->missions.size() || std::find(which.begin(), which.end(), k) != which.end()) { ctx->err = "bad mission index"; return SX_E_INVALID; }
        if (ctx->missions[(size_t)k].host_sequential()) { ctx->err = "an ISO-2022-JP mission has no stage A (one sequential pass on the host)"; return SX_E_INVALID; }
        which.push_back(k); par.push_back((uint32_t)(stream_parity & 1)); mc.push_back(min_chars[i]);
        runs[i] = nullptr; n_runs[i] = 0;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<RunList> out;
    ctx->shard_runs_valid = false;
    int rc = device_runs(ctx, which, (const uint8_t*)device_bytes, len, par, mc, &out);
    if (rc != SX_OK) return rc;
    for (int i = 0; i < n; i++) {
        if (!out[(size_t)i].own.empty()) out[(size_t)i].use_own();
        HIP_TRY(ctx, out[(size_t)i].wait());
        n_runs[i] = out[(size_t)i].size();
        runs[i] = (sx_run*)malloc(sizeof(sx_run) * (n_runs[i] ? n_runs[i] : 1));
        if (!runs[i]) { for (int j = 0; j < i; j++) { free(runs[j]); runs[j] = nullptr; } return SX_E_NOMEM; }
        memcpy(runs[i], out[(size_t)i].data(), sizeof(sx_run) * n_runs[i]);
    }
    return SX_OK;
}

int sx_replay_runs(sx_ctx* ctx, const uint8_t* bytes, uint64_t len, int input_file_id, int is_last_input_buffer,
                   const sx_run* const* runs, const uint64_t* n_runs, sx_result** out) {
    if (!ctx || !out || (!bytes && len) || !runs || !n_runs) return SX_E_INVALID;
    begin_call(ctx);
    std::vector<RunList> r(ctx->missions.size());
    for (size_t k = 0; k < r.size(); k++) r[k].assign(runs[k], runs[k] + n_runs[k]);
    HostBytes view(bytes ? bytes : (const uint8_t*)"");
    ResultHolder res;
    std::vector<uint32_t> entry;
    int rc = set_entry_params(ctx, true, bytes, nullptr, len, 0, &entry);
    if (rc != SX_OK) return rc;
    rc = replay_all(ctx, view, whole_chunk_job(ctx, len, input_file_id, is_last_input_buffer != 0), r, &res.r->r, nullptr);
    if (rc == SX_OK) *out = res.release();
    return rc;
}


int sx_scan_shard_device(sx_ctx* ctx, const void* device_bytes, uint64_t buf_off, uint64_t buf_len, uint64_t own_lo,
                         uint64_t own_hi, const uint64_t* start_at, uint64_t file_stream_off, int input_file_id,
                         int reuse_runs, sx_result** out, uint64_t* end_pos) {
    if (!ctx || (!device_bytes && buf_len)) return SX_E_INVALID;
    begin_call(ctx);
    if (ctx->host_only) { ctx->err = "host-only context: no device scan"; return SX_E_STATE; }
    if ((uintptr_t)device_bytes & 15) { ctx->err = "device_bytes must be 16-byte aligned"; return SX_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return shard_common(ctx, nullptr, (const uint8_t*)device_bytes, nullptr, nullptr, buf_off, buf_len, own_lo, own_hi, start_at,
                        file_stream_off, input_file_id, reuse_runs, out, end_pos);
}

int sx_scan_shard(sx_ctx* ctx, const uint8_t* bytes, uint64_t buf_off, uint64_t buf_len, uint64_t own_lo, uint64_t own_hi,
                  const uint64_t* start_at, uint64_t file_stream_off, int input_file_id, int reuse_runs, sx_result** out,
                  uint64_t* end_pos) {
    if (!ctx || (!bytes && buf_len)) return SX_E_INVALID;
    begin_call(ctx);
    if (ctx->host_only) { ctx->err = "host-only context: no device scan"; return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (sx_scan_shard uploads into the context's own staging buffer: the runs of the previous call belong to the same
    //  host bytes only if offset, length and pointer agree — shard_common checks that again on its side)
    if (!(reuse_runs && ctx->shard_runs_valid && ctx->shard_runs_off == buf_off && ctx->shard_runs_len == buf_len && ctx->shard_runs_ptr == (const void*)ctx->d_input)) {
        if (buf_len > ctx->d_input_cap) {
            if (ctx->d_input) HIP_TRY(ctx, hipFree(ctx->d_input));
            ctx->d_input = nullptr; ctx->d_input_cap = 0;
            HIP_TRY(ctx, hipMalloc((void**)&ctx->d_input, buf_len));
            ctx->d_input_cap = buf_len;
        }
        if (buf_len) HIP_TRY(ctx, hipMemcpy(ctx->d_input, bytes, buf_len, hipMemcpyHostToDevice));
    }
    return shard_common(ctx, bytes ? bytes : (const uint8_t*)"", ctx->d_input, nullptr, nullptr, buf_off, buf_len, own_lo, own_hi,
                        start_at, file_stream_off, input_file_id, reuse_runs, out, end_pos);
}

int sx_replay_shard_runs(sx_ctx* ctx, const uint8_t* bytes, uint64_t buf_off, uint64_t buf_len, uint64_t own_lo,
                         uint64_t own_hi, const uint64_t* start_at, uint64_t file_stream_off, int input_file_id,
                         const sx_run* const* runs, const uint64_t* n_runs, sx_result** out, uint64_t* end_pos) {
    if (!ctx || (!bytes && buf_len) || !runs || !n_runs) return SX_E_INVALID;
    begin_call(ctx);
    return shard_common(ctx, bytes ? bytes : (const uint8_t*)"", nullptr, runs, n_runs, buf_off, buf_len, own_lo, own_hi, start_at,
                        file_stream_off, input_file_id, 0, out, end_pos);
}

uint64_t sx_result_count(const sx_result* r) { return r ? r->r.count() : 0; }
uint64_t sx_result_segments(const sx_result* r) { return r ? r->r.segs.size() : 0; }
int sx_result_segment(const sx_result* r, uint64_t i, const sx_finding** findings, uint64_t* n_findings,
                      const uint8_t** arena, uint64_t* arena_len) {
    if (!r || i >= r->r.segs.size()) return SX_E_INVALID;
    { const int rc = fetch_to_host(const_cast<sx_result*>(r), const_cast<sx_result*>(r)->r.segs[(size_t)i]); if (rc != SX_OK) return rc; }
    const MissionFindings& s = r->r.segs[(size_t)i];
    if (findings) *findings = s.data();
    if (n_findings) *n_findings = s.count();
    if (arena) *arena = (const uint8_t*)s.strings();
    if (arena_len) *arena_len = s.strings_len();
    return SX_OK;
}
int sx_result_segment_packed(const sx_result* r, uint64_t i, const void** findings, uint64_t* n_findings, const uint8_t** arena,
                             uint64_t* arena_len, int* packed, sx_segment_info* info) {
    if (!r || i >= r->r.segs.size()) return SX_E_INVALID;
    { const int rc = fetch_to_host(const_cast<sx_result*>(r), const_cast<sx_result*>(r)->r.segs[(size_t)i]); if (rc != SX_OK) return rc; }
    const MissionFindings& s = r->r.segs[(size_t)i];
    if (findings) *findings = s.packed ? (const void*)s.data16() : (const void*)s.data();
    if (n_findings) *n_findings = s.count();
    if (arena) *arena = (const uint8_t*)s.strings();
    if (arena_len) *arena_len = s.strings_len();
    if (packed) *packed = s.packed ? 1 : 0;
    if (info) {
        memset(info, 0, sizeof *info);
        info->packed = s.packed ? 1 : 0;
        info->input_file_id = -1;
        if (s.packed && s.info) {
            info->input_file_id = s.info->file_id; info->slice_base = s.info->slice_base;
            memcpy(info->position0, s.info->pos0, sizeof info->position0);
        }
    }
    return SX_OK;
}
int sx_result_segment_device(const sx_result* r, uint64_t i, const void** d_records, uint64_t* n_findings, const uint8_t** d_arena,
                             uint64_t* arena_len, int* packed, sx_segment_info* info) {
    if (!r || i >= r->r.segs.size()) return SX_E_INVALID;
    const MissionFindings& s = r->r.segs[(size_t)i];
    if (d_records) *d_records = nullptr;
    if (d_arena) *d_arena = nullptr;
    if (n_findings) *n_findings = s.count();
    if (arena_len) *arena_len = s.strings_len();
    if (packed) *packed = s.packed ? 1 : 0;
    if (info) {
        memset(info, 0, sizeof *info);
        info->packed = s.packed ? 1 : 0;
        info->input_file_id = -1;
        if (s.packed && s.info) {
            info->input_file_id = s.info->file_id; info->slice_base = s.info->slice_base;
            memcpy(info->position0, s.info->pos0, sizeof info->position0);
        }
    }
    if (!s.dev_only) return SX_OK;   // (in host memory: the host accessors)
    if (!s.keep_on_device || !s.dev_epoch_ref || s.dev_epoch_ref->load() != s.dev_epoch) return SX_E_STATE;
    if (d_records) *d_records = s.dev_copy;
    if (d_arena) *d_arena = (const uint8_t*)s.dev_copy + s.ext_nf * s.rec_size();
    return SX_OK;
}
// The contiguous view: joins the segments on first use (a copy; none if there is one segment).
const sx_finding* sx_result_findings(const sx_result* r) {
    if (!r || fetch_all_to_host(r) != SX_OK || !const_cast<sx_result*>(r)->r.flatten(nullptr) || r->r.segs.empty()) return nullptr;
    return r->r.segs[0].data();
}
const uint8_t* sx_result_arena(const sx_result* r, uint64_t* len) {
    if (len) *len = 0;
    if (!r || fetch_all_to_host(r) != SX_OK || !const_cast<sx_result*>(r)->r.flatten(nullptr) || r->r.segs.empty()) return nullptr;
    if (len) *len = r->r.segs[0].strings_len();
    return (const uint8_t*)r->r.segs[0].strings();
}
void sx_result_free(sx_result* r) { delete r; }

int sx_print_findings(const sx_ctx* ctx, const sx_result* r, int n_inputs, int radix, int no_metadata, uint8_t** out,
                      uint64_t* out_len) {
    if (!ctx || !r || !out || !out_len) return SX_E_INVALID;
    if (radix != 0 && radix != 'x' && radix != 'd' && radix != 'o') return SX_E_INVALID;
    { const int rc = fetch_all_to_host(r); if (rc != SX_OK) return rc; }
    std::string s;
    print_findings(ctx->missions, r->r, n_inputs, radix, no_metadata != 0, &s);
    *out = (uint8_t*)malloc(s.size() ? s.size() : 1);
    if (!*out) return SX_E_NOMEM;
    memcpy(*out, s.data(), s.size());
    *out_len = s.size();
    return SX_OK;
}

// What sx_print_findings_device and sx_result_select_device ask of a result: every segment in HBM, in memory of this context — the result
// block of the last scan call or one of the two selection blocks — that has not been written again since.
static int result_on_device(sx_ctx* ctx, const sx_result* r, const char* host_call) {
    const std::string in_host = std::string("the result is in host memory: ") + host_call;
    if (r->r.segs.empty()) { ctx->set_err(in_host); return SX_E_STATE; }
    for (const MissionFindings& s : r->r.segs) {
        if (!s.dev_only || !s.keep_on_device || s.ext_nf == 0) { ctx->set_err(in_host); return SX_E_STATE; }
        const bool ours = s.dev_epoch_ref && (s.dev_epoch_ref == ctx->dev_epoch || s.dev_epoch_ref == ctx->select_epoch[0] || s.dev_epoch_ref == ctx->select_epoch[1]);
        if (!ours || s.dev_epoch_ref->load() != s.dev_epoch) {
            ctx->set_err("a later scan or selection has reused the result's device memory");
            return SX_E_STATE;
        }
    }
    return SX_OK;
}

// Finding::print where the findings lie (sx_print_dev.hip): pass 1 of every segment, one wait for the segments' text bytes, the text
// block, pass 2 of every segment at its 64-bit base, one more wait.  The result is read, never moved.
int sx_print_findings_device(sx_ctx* ctx, const sx_result* r, int n_inputs, int radix, int no_metadata, const uint8_t** d_text,
                             uint64_t* text_len) {
    if (d_text) *d_text = nullptr;
    if (text_len) *text_len = 0;
    if (!ctx || !r || !d_text || !text_len) return SX_E_INVALID;
    if (radix != 0 && radix != 'x' && radix != 'd' && radix != 'o') { ctx->set_err("radix must be 0, 'x', 'd' or 'o'"); return SX_E_INVALID; }
    if (ctx->host_only) { ctx->set_err("host-only context: no device print"); return SX_E_STATE; }
    { const int rc = result_on_device(ctx, r, "sx_print_findings"); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    if (!ctx->d_print_missions) {
        std::vector<PrintMission> tab(256);
        memset(tab.data(), 0, tab.size() * sizeof(PrintMission));
        for (size_t k = ctx->missions.size(); k-- > 0;) {   // (print_findings takes the first Mission of an id)
            const Mission& m = ctx->missions[k];
            const char* name = m.c.print_encoding_as_ascii ? "ascii" : m.encoding_name();
            const std::string label = name ? name : "";
            PrintMission& t = tab[m.c.mission_id];
            if (label.size() > sizeof t.label) { ctx->set_err("encoding label longer than 14 bytes"); return SX_E_STATE; }
            t.present = 1; t.len = (uint8_t)label.size();
            memcpy(t.label, label.data(), label.size());
        }
        uint8_t* p = nullptr;
        if (hipMalloc((void**)&p, tab.size() * sizeof(PrintMission)) != hipSuccess) { (void)hipGetLastError(); ctx->set_err("device print: no memory for the Mission table"); return SX_E_NOMEM; }
        const hipError_t e = hipMemcpy(p, tab.data(), tab.size() * sizeof(PrintMission), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); ctx->set_err(std::string("hipMemcpy: ") + hipGetErrorString(e)); return SX_E_HIP; }
        ctx->d_print_missions = p;
    }
    const size_t ns = r->r.segs.size();
    uint64_t scratch = 0;
    for (const MissionFindings& s : r->r.segs) scratch += print_scratch_bytes(s.ext_nf);
    if (scratch > ctx->d_print_scratch_cap) {
        if (ctx->d_print_scratch) (void)hipFree(ctx->d_print_scratch);
        ctx->d_print_scratch = nullptr; ctx->d_print_scratch_cap = 0;
        if (hipMalloc((void**)&ctx->d_print_scratch, scratch) != hipSuccess) { (void)hipGetLastError(); ctx->d_print_scratch = nullptr; ctx->set_err("device print: no memory for the offsets"); return SX_E_NOMEM; }
        ctx->d_print_scratch_cap = scratch;
    }
    std::vector<PrintParams> P(ns);
    std::vector<const uint64_t*> d_total(ns);
    uint64_t at = 0;
    for (size_t i = 0; i < ns; i++) {
        const MissionFindings& s = r->r.segs[i];
        PrintParams& p = P[i];
        memset(&p, 0, sizeof p);
        p.recs = s.dev_copy; p.arena = (const uint8_t*)s.dev_copy + s.ext_nf * s.rec_size(); p.n = s.ext_nf; p.packed = s.packed ? 1u : 0u;
        p.file_id = s.packed && s.info ? s.info->file_id : -1;
        p.several_inputs = n_inputs > 1; p.radix = (uint32_t)radix; p.no_metadata = no_metadata != 0; p.several_missions = ctx->missions.size() > 1;
        p.missions = (const PrintMission*)ctx->d_print_missions;
        const size_t bytes = print_scratch_bytes(s.ext_nf);
        HIP_TRY(ctx, print_measure(p, ctx->d_print_scratch + at, bytes, st, &p.wbase, &d_total[i]));
        at += bytes;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    uint64_t total = 0;
    for (size_t i = 0; i < ns; i++) {
        uint64_t t = 0;
        HIP_TRY(ctx, hipMemcpy(&t, d_total[i], sizeof t, hipMemcpyDeviceToHost));
        P[i].base = total;
        total += t;
    }
    if (total > ctx->d_text_cap) {
        if (ctx->d_text) (void)hipFree(ctx->d_text);
        ctx->d_text = nullptr; ctx->d_text_cap = 0;
        if (hipMalloc((void**)&ctx->d_text, total) != hipSuccess) {
            (void)hipGetLastError();
            ctx->d_text = nullptr;
            ctx->set_err("device print: no memory for " + std::to_string(total) + " bytes of text");
            return SX_E_NOMEM;
        }
        ctx->d_text_cap = total;
    }
    for (size_t i = 0; i < ns; i++) {
        P[i].text = ctx->d_text;
        HIP_TRY(ctx, print_write(P[i], st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *d_text = ctx->d_text;
    *text_len = total;
    return SX_OK;
}

// (a grow-only device buffer of the selection: SX_E_NOMEM leaves it empty)
static int grow_device(sx_ctx* ctx, uint8_t** p, uint64_t* cap, uint64_t bytes, const char* what) {
    if (bytes <= *cap) return SX_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc((void**)p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        ctx->set_err(std::string("device select: no memory for ") + std::to_string(bytes) + " bytes of " + what);
        return SX_E_NOMEM;
    }
    *cap = bytes;
    return SX_OK;
}

// grep where the findings lie (sx_select_dev.hip), for the three entry points, whose arguments are checked: pass 1 of every segment —
// select_match_kernel with `patterns`, selset_match_kernel with the compiled `set`, or selre_match_kernel with the compiled `re` —, one wait for the segments' totals, the
// selection block, pass 2 of every segment that has selected findings, one more wait.  The source is read, never moved.
// grep -o (sx_extract_dev.hip), for the fourth: with the compiled `ex` the two passes are extract_measure and extract_place, an output
// record is a match, not a finding, and a segment may get more records than it had; the blocks, their turns and the epochs are the same.
// By label (sx_label_dev.hip), for the fifth: with `labels` (made from r: checked here) and masks = { any, all, none } pass 1 is
// label_pick_kernel, which reads no string byte; everything behind it is the selection's.
static int select_on_device(sx_ctx* ctx, const sx_result* r, const sx_pattern* patterns, int n_patterns, const SelsetDevice* set, const SelreDevice* re, const ExtractDevice* ex, uint32_t flags, sx_result** out,
                            const sx_labels* labels = nullptr, const uint64_t* masks = nullptr) {
    if (ctx->host_only) { ctx->set_err("host-only context: no device selection"); return SX_E_STATE; }
    { const int rc = result_on_device(ctx, r, "filter on the host"); if (rc != SX_OK) return rc; }
    if (labels) {
        bool same = labels->segs.size() == r->r.segs.size();
        for (size_t i = 0; same && i < labels->segs.size(); i++) {
            const sx_labels::Seg& l = labels->segs[i];
            const MissionFindings& s = r->r.segs[i];
            same = l.recs == s.dev_copy && l.n == s.ext_nf && l.epoch_ref == s.dev_epoch_ref && l.epoch == s.dev_epoch;
        }
        if (!same) { ctx->set_err("the labels were not made from this result"); return SX_E_INVALID; }
    }
    // the block this call writes: a source that lies there was made two selections ago
    const int slot = (int)(ctx->select_calls & 1u);
    for (const MissionFindings& s : r->r.segs)
        if (s.dev_epoch_ref == ctx->select_epoch[slot]) { ctx->set_err("this selection reuses the source's device memory: it was selected two calls ago"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    const size_t ns = r->r.segs.size();
    uint64_t scratch = 0;
    for (const MissionFindings& s : r->r.segs) scratch += ex ? extract_scratch_bytes(s.ext_nf) : select_scratch_bytes(s.ext_nf);
    { const int rc = grow_device(ctx, &ctx->d_select_scratch, &ctx->d_select_scratch_cap, scratch, "wavefront tables"); if (rc != SX_OK) return rc; }
    std::vector<SelectParams> P(ex ? 0 : ns);
    std::vector<ExtractParams> X(ex ? ns : 0);
    std::vector<const uint32_t*> d_count(ns);
    std::vector<const uint64_t*> d_count64(ns), d_bytes(ns);
    uint64_t at = 0;
    for (size_t i = 0; i < ns; i++) {
        const MissionFindings& s = r->r.segs[i];
        if (ex) {
            ExtractParams& x = X[i];
            memset(&x, 0, sizeof x);
            x.recs = s.dev_copy; x.arena = (const uint8_t*)s.dev_copy + s.ext_nf * s.rec_size(); x.n = s.ext_nf; x.packed = s.packed ? 1u : 0u;
            x.ex = *ex;
            const size_t bytes = extract_scratch_bytes(s.ext_nf);
            HIP_TRY(ctx, extract_measure(&x, ctx->d_select_scratch + at, bytes, st, &d_count64[i], &d_bytes[i]));
            at += bytes;
            continue;
        }
        SelectParams& p = P[i];
        memset(&p, 0, sizeof p);
        p.recs = s.dev_copy; p.arena = (const uint8_t*)s.dev_copy + s.ext_nf * s.rec_size(); p.n = s.ext_nf; p.packed = s.packed ? 1u : 0u;
        if (set || re) p.pat.invert = (flags & SX_SELECT_INVERT) ? 1u : 0u;
        else select_fill_patterns(&p.pat, patterns, n_patterns, flags);
        const size_t bytes = select_scratch_bytes(s.ext_nf);
        LabelPick pick{ nullptr, 0, 0, 0 };
        if (labels) pick = LabelPick{ labels->segs[i].d, masks[0], masks[1], masks[2] };
        HIP_TRY(ctx, select_measure(&p, set, re, ctx->d_select_scratch + at, bytes, st, &d_count[i], &d_bytes[i], labels ? &pick : nullptr));
        at += bytes;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::vector<uint64_t> n_sel(ns), b_sel(ns), base(ns);
    uint64_t block = 0, scratch2 = 0;
    for (size_t i = 0; i < ns; i++) {
        uint64_t c = 0;
        if (ex) HIP_TRY(ctx, hipMemcpy(&c, d_count64[i], sizeof c, hipMemcpyDeviceToHost));
        else { uint32_t c32 = 0; HIP_TRY(ctx, hipMemcpy(&c32, d_count[i], sizeof c32, hipMemcpyDeviceToHost)); c = c32; }
        HIP_TRY(ctx, hipMemcpy(&b_sel[i], d_bytes[i], sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (c >= 0xFFFFFFFFull) {      // (an extraction: a selection has no more records than its source)
            ctx->set_err("segment " + std::to_string(i) + " has " + std::to_string(c) + " matches: more than the 32-bit counters of a segment hold");
            return SX_E_INVALID;
        }
        n_sel[i] = c;
        if (!c) continue;
        base[i] = block;
        block += (c * r->r.segs[i].rec_size() + b_sel[i] + 255) / 256 * 256;
        scratch2 = std::max<uint64_t>(scratch2, ex ? extract_place_scratch_bytes(c) : select_place_scratch_bytes(c));
    }
    // from here on the call counts: the block of the selection before the last one is written again
    ctx->select_epoch[slot]->fetch_add(1);
    ctx->select_calls++;
    ResultHolder res;
    res.r->r.pool = ctx->pool;
    if (block) {
        { const int rc = grow_device(ctx, &ctx->d_select[slot], &ctx->d_select_cap[slot], block, "selected findings"); if (rc != SX_OK) return rc; }
        { const int rc = grow_device(ctx, &ctx->d_select_scratch2, &ctx->d_select_scratch2_cap, scratch2, "string offsets"); if (rc != SX_OK) return rc; }
        for (size_t i = 0; i < ns; i++) {
            if (!n_sel[i]) continue;
            const MissionFindings& s = r->r.segs[i];
            uint8_t* recs = ctx->d_select[slot] + base[i];
            if (ex) HIP_TRY(ctx, extract_place(X[i], recs, n_sel[i], recs + n_sel[i] * s.rec_size(), ctx->d_select_scratch2, extract_place_scratch_bytes(n_sel[i]), st));
            else HIP_TRY(ctx, select_place(P[i], recs, n_sel[i], recs + n_sel[i] * s.rec_size(), ctx->d_select_scratch2, select_place_scratch_bytes(n_sel[i]), st));
            MissionFindings o;
            o.ext_nf = n_sel[i]; o.ext_na = b_sel[i]; o.dev_copy = recs; o.dev_only = true; o.keep_on_device = true;
            o.dev_epoch_ref = ctx->select_epoch[slot]; o.dev_epoch = ctx->select_epoch[slot]->load();
            o.packed = s.packed; o.info = s.info;
            res.r->r.segs.push_back(std::move(o));
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    *out = res.release();
    return SX_OK;
}

int sx_result_select_device(sx_ctx* ctx, const sx_result* r, const sx_pattern* patterns, int n_patterns, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !patterns || !out) return SX_E_INVALID;
    if (n_patterns < 1 || n_patterns > SX_SELECT_MAX_PATTERNS) { ctx->set_err("n_patterns must be 1..16"); return SX_E_INVALID; }
    if (flags & ~(uint32_t)(SX_SELECT_ASCII_NOCASE | SX_SELECT_INVERT)) { ctx->set_err("unknown selection flags"); return SX_E_INVALID; }
    for (int p = 0; p < n_patterns; p++)
        if (!patterns[p].bytes || patterns[p].len < 1 || patterns[p].len > SX_SELECT_MAX_PATTERN_BYTES) { ctx->set_err("a pattern must have 1..64 bytes"); return SX_E_INVALID; }
    return select_on_device(ctx, r, patterns, n_patterns, nullptr, nullptr, nullptr, flags, out);
}

int sx_select_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_select_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    SelsetTable T;
    std::string err;
    { const int rc = selset_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("pattern set: " + err); return rc; } }
    if (ctx->host_only) { ctx->set_err("host-only context: no device for the pattern set"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t table = (T.next.size() + 15) / 16 * 16;   // (selset_match_kernel copies the LDS rows in 16-byte chunks)
    uint8_t* mem = nullptr;
    if (hipMalloc((void**)&mem, sizeof T.map + table) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_err("pattern set: no device memory for " + std::to_string(sizeof T.map + table) + " bytes of table");
        return SX_E_NOMEM;
    }
    hipError_t e = hipMemcpy(mem, T.map, sizeof T.map, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + sizeof T.map, T.next.data(), T.next.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(mem); ctx->set_err(std::string("hipMemcpy: ") + hipGetErrorString(e)); return SX_E_HIP; }
    sx_select_set* set = new (std::nothrow) sx_select_set;
    if (!set) { (void)hipFree(mem); return SX_E_NOMEM; }
    set->device = ctx->device; set->mem = mem;
    set->dev = SelsetDevice{ mem, mem + sizeof T.map, T.states, T.classes, T.lds_states, T.matched, T.entry_bytes, 0 };
    set->info = sx_select_set_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)T.next.size(), T.lds_states, 0 };
    *out = set;
    return SX_OK;
}

int sx_select_set_info_get(const sx_select_set* set, sx_select_set_info* out) {
    if (!set || !out) return SX_E_INVALID;
    *out = set->info;
    return SX_OK;
}

void sx_select_set_free(sx_select_set* set) {
    if (!set) return;
    (void)hipFree(set->mem);
    delete set;
}

int sx_result_select_set_device(sx_ctx* ctx, const sx_result* r, const sx_select_set* set, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !set || !out) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SELECT_INVERT) { ctx->set_err("a pattern set is selected with SX_SELECT_INVERT or no flag: the fold is compiled into the set"); return SX_E_INVALID; }
    if (ctx->host_only) { ctx->set_err("host-only context: no device selection"); return SX_E_STATE; }
    if (set->device != ctx->device) { ctx->set_err("the pattern set lies on another device"); return SX_E_INVALID; }
    return select_on_device(ctx, r, nullptr, 0, &set->dev, nullptr, nullptr, flags, out);
}

int sx_select_regex_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_select_regex** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    SelreTable T;
    std::string err;
    { const int rc = selre_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("regex set: " + err); return rc; } }
    if (ctx->host_only) { ctx->set_err("host-only context: no device for the regex set"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = T.next.size() * sizeof(uint16_t), table = (bytes + 15) / 16 * 16;   // (selre_match_kernel copies the LDS rows in 16-byte chunks)
    uint8_t* mem = nullptr;
    if (hipMalloc((void**)&mem, sizeof T.map + table) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_err("regex set: no device memory for " + std::to_string(sizeof T.map + table) + " bytes of table");
        return SX_E_NOMEM;
    }
    hipError_t e = hipMemcpy(mem, T.map, sizeof T.map, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + sizeof T.map, T.next.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(mem); ctx->set_err(std::string("hipMemcpy: ") + hipGetErrorString(e)); return SX_E_HIP; }
    sx_select_regex* re = new (std::nothrow) sx_select_regex;
    if (!re) { (void)hipFree(mem); return SX_E_NOMEM; }
    re->device = ctx->device; re->mem = mem;
    re->dev = SelreDevice{ mem, (const uint16_t*)(mem + sizeof T.map), T.states, T.classes, T.lds_states, T.end_first, T.stop_first, T.matched, T.root_end, 0 };
    re->info = sx_select_regex_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)bytes, T.lds_states, T.end_states };
    *out = re;
    return SX_OK;
}

int sx_select_regex_info_get(const sx_select_regex* re, sx_select_regex_info* out) {
    if (!re || !out) return SX_E_INVALID;
    *out = re->info;
    return SX_OK;
}

void sx_select_regex_free(sx_select_regex* re) {
    if (!re) return;
    (void)hipFree(re->mem);
    delete re;
}

int sx_result_select_regex_device(sx_ctx* ctx, const sx_result* r, const sx_select_regex* re, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !re || !out) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SELECT_INVERT) { ctx->set_err("a regex set is selected with SX_SELECT_INVERT or no flag: the fold is compiled into the set"); return SX_E_INVALID; }
    if (ctx->host_only) { ctx->set_err("host-only context: no device selection"); return SX_E_STATE; }
    if (re->device != ctx->device) { ctx->set_err("the regex set lies on another device"); return SX_E_INVALID; }
    return select_on_device(ctx, r, nullptr, 0, nullptr, &re->dev, nullptr, flags, out);
}

int sx_extract_regex_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_extract_regex** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    ExtractTable T;
    std::string err;
    { const int rc = extract_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("extract set: " + err); return rc; } }
    if (ctx->host_only) { ctx->set_err("host-only context: no device for the extract set"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = T.next.size() * sizeof(uint16_t), table = (bytes + 15) / 16 * 16;   // (the kernels copy the LDS rows in 16-byte chunks)
    uint8_t* mem = nullptr;
    if (hipMalloc((void**)&mem, sizeof T.map + table) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_err("extract set: no device memory for " + std::to_string(sizeof T.map + table) + " bytes of table");
        return SX_E_NOMEM;
    }
    hipError_t e = hipMemcpy(mem, T.map, sizeof T.map, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + sizeof T.map, T.next.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(mem); ctx->set_err(std::string("hipMemcpy: ") + hipGetErrorString(e)); return SX_E_HIP; }
    sx_extract_regex* ex = new (std::nothrow) sx_extract_regex;
    if (!ex) { (void)hipFree(mem); return SX_E_NOMEM; }
    ex->device = ctx->device; ex->mem = mem;
    ex->dev = ExtractDevice{ mem, (const uint16_t*)(mem + sizeof T.map), T.states, T.classes, T.lds_states, T.end_first, T.here_first, T.dead_first, T.start0, T.start1 };
    ex->info = sx_extract_regex_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)bytes, T.lds_states, 0 };
    *out = ex;
    return SX_OK;
}

int sx_extract_regex_info_get(const sx_extract_regex* ex, sx_extract_regex_info* out) {
    if (!ex || !out) return SX_E_INVALID;
    *out = ex->info;
    return SX_OK;
}

void sx_extract_regex_free(sx_extract_regex* ex) {
    if (!ex) return;
    (void)hipFree(ex->mem);
    delete ex;
}

int sx_result_extract_regex_device(sx_ctx* ctx, const sx_result* r, const sx_extract_regex* ex, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !ex || !out) return SX_E_INVALID;
    if (flags) { ctx->set_err("an extraction takes no flag: the fold is compiled into the set"); return SX_E_INVALID; }
    if (ctx->host_only) { ctx->set_err("host-only context: no device extraction"); return SX_E_STATE; }
    if (ex->device != ctx->device) { ctx->set_err("the extract set lies on another device"); return SX_E_INVALID; }
    return select_on_device(ctx, r, nullptr, 0, nullptr, nullptr, &ex->dev, flags, out);
}

int sx_tally_set_reset(sx_tally_set* set) {
    if (!set) return SX_E_INVALID;
    if (hipSetDevice(set->device) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    hipError_t e = hipMemset(set->dev.hits, 0, (size_t)set->dev.unique * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemset(set->dev.first, 0xFF, (size_t)set->dev.unique * sizeof(uint64_t));   // SX_TALLY_NEVER
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (a device memset may return before it is done, and the tally runs on a stream that does not wait for this one)
    if (e != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    return SX_OK;
}

int sx_tally_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_tally_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    SeltallyTable T;
    std::string err;
    { const int rc = seltally_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("tally set: " + err); return rc; } }
    if (ctx->host_only) { ctx->set_err("host-only context: no device for the tally set"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t table = (T.next.size() + 15) / 16 * 16;   // (seltally_kernel copies the LDS rows in 16-byte chunks)
    const size_t per_state = (size_t)T.states * sizeof(uint32_t), map_words = (((size_t)T.n_patterns + 1) & ~(size_t)1) * sizeof(uint32_t);
    const size_t counters = (size_t)T.unique * sizeof(uint64_t);
    const size_t at_own = sizeof T.map + table, at_dict = at_own + per_state, at_map = at_dict + per_state;
    const size_t at_hits = (at_map + map_words + 7) / 8 * 8, bytes = at_hits + 2 * counters;
    uint8_t* mem = nullptr;
    if (hipMalloc((void**)&mem, bytes) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_err("tally set: no device memory for " + std::to_string(bytes) + " bytes of tables and counters");
        return SX_E_NOMEM;
    }
    hipError_t e = hipMemcpy(mem, T.map, sizeof T.map, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + sizeof T.map, T.next.data(), T.next.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + at_own, T.own.data(), per_state, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + at_dict, T.dict.data(), per_state, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + at_map, T.unique_of_pattern.data(), (size_t)T.n_patterns * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(mem); ctx->set_err(std::string("hipMemcpy: ") + hipGetErrorString(e)); return SX_E_HIP; }
    sx_tally_set* set = new (std::nothrow) sx_tally_set;
    if (!set) { (void)hipFree(mem); return SX_E_NOMEM; }
    set->device = ctx->device; set->mem = mem;
    set->dev = SeltallyDevice{ mem, mem + sizeof T.map, (const uint32_t*)(mem + at_own), (const uint32_t*)(mem + at_dict),
                               (uint64_t*)(mem + at_hits), (uint64_t*)(mem + at_hits + counters),
                               T.states, T.classes, T.lds_states, T.entry_bytes, T.unique, T.unique < kSeltallyLdsIds ? T.unique : kSeltallyLdsIds };
    set->d_unique_of_pattern = (const uint32_t*)(mem + at_map);
    set->info = sx_tally_set_info{ T.n_patterns, T.unique, T.states, T.classes, T.nocase, T.entry_bytes,
                                   (uint64_t)(sizeof T.map + T.next.size() + 2 * per_state + (size_t)T.n_patterns * sizeof(uint32_t)), T.lds_states, 0 };
    set->unique_of_pattern = std::move(T.unique_of_pattern);
    if (sx_tally_set_reset(set) != SX_OK) { ctx->set_err("tally set: the counters could not be reset"); sx_tally_set_free(set); return SX_E_HIP; }
    *out = set;
    return SX_OK;
}

int sx_tally_set_info_get(const sx_tally_set* set, sx_tally_set_info* out) {
    if (!set || !out) return SX_E_INVALID;
    *out = set->info;
    return SX_OK;
}

void sx_tally_set_free(sx_tally_set* set) {
    if (!set) return;
    (void)hipFree(set->mem);
    delete set;
}

// The tally where the findings lie (sx_seltally_dev.hip): the source is checked as a whole, then one kernel per segment, each with the
// ordinal of its first record, on the selections' stream, and one wait.  Only the set's counters are written.
int sx_result_tally_device(sx_ctx* ctx, const sx_result* r, sx_tally_set* set, uint64_t ordinal_base, uint64_t* n_findings) {
    if (n_findings) *n_findings = 0;
    if (!ctx || !r || !set) return SX_E_INVALID;
    if (ctx->host_only) { ctx->set_err("host-only context: no device tally"); return SX_E_STATE; }
    if (set->device != ctx->device) { ctx->set_err("the tally set lies on another device"); return SX_E_INVALID; }
    { const int rc = result_on_device(ctx, r, "count on the host"); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    uint64_t walked = 0;
    for (const MissionFindings& s : r->r.segs) {
        SeltallyParams p;
        memset(&p, 0, sizeof p);
        p.recs = s.dev_copy; p.arena = (const uint8_t*)s.dev_copy + s.ext_nf * s.rec_size(); p.n = s.ext_nf; p.packed = s.packed ? 1u : 0u;
        p.ordinal = ordinal_base + walked;
        p.set = set->dev;
        HIP_TRY(ctx, seltally_launch(p, st));
        walked += s.ext_nf;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (n_findings) *n_findings = walked;
    return SX_OK;
}

int sx_tally_set_read(const sx_tally_set* set, uint64_t* hits, uint64_t* first, uint32_t n_patterns) {
    if (!set || n_patterns != set->info.n_patterns) return SX_E_INVALID;
    if (hipSetDevice(set->device) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    std::vector<uint64_t> u(set->dev.unique);
    for (int k = 0; k < 2; k++) {
        uint64_t* out = k ? first : hits;
        if (!out) continue;
        if (hipMemcpy(u.data(), k ? set->dev.first : set->dev.hits, u.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
        for (uint32_t p = 0; p < n_patterns; p++) out[p] = u[set->unique_of_pattern[p]];
    }
    return SX_OK;
}

int sx_tally_set_counters_device(const sx_tally_set* set, const uint64_t** d_hits, const uint64_t** d_first,
                                 const uint32_t** d_unique_of_pattern, uint32_t* unique) {
    if (!set) return SX_E_INVALID;
    if (d_hits) *d_hits = set->dev.hits;
    if (d_first) *d_first = set->dev.first;
    if (d_unique_of_pattern) *d_unique_of_pattern = set->d_unique_of_pattern;
    if (unique) *unique = set->dev.unique;
    return SX_OK;
}

int sx_label_set_reset(sx_label_set* set) {
    if (!set) return SX_E_INVALID;
    if (hipSetDevice(set->device) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    hipError_t e = hipMemset(set->dev.findings, 0, kLabelBits * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemset(set->dev.first, 0xFF, kLabelBits * sizeof(uint64_t));   // SX_LABEL_NEVER
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (as sx_tally_set_reset: the labelling runs on a stream that does not wait for this one)
    if (e != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    return SX_OK;
}

int sx_label_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_label_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    LabelTable T;
    std::string err;
    { const int rc = label_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("label set: " + err); return rc; } }
    if (ctx->host_only) { ctx->set_err("host-only context: no device for the label set"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t next_bytes = T.next.size() * sizeof(uint16_t), table = (next_bytes + 15) / 16 * 16;   // (label_match_kernel copies the LDS rows in 16-byte chunks)
    const size_t here_bytes = T.here.size() * sizeof(uint64_t), end_bytes = T.end.size() * sizeof(uint64_t), counters = kLabelBits * sizeof(uint64_t);
    const size_t at_here = sizeof T.map + table, at_end = at_here + here_bytes, at_findings = at_end + end_bytes, bytes = at_findings + 2 * counters;
    uint8_t* mem = nullptr;
    if (hipMalloc((void**)&mem, bytes) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_err("label set: no device memory for " + std::to_string(bytes) + " bytes of tables and counters");
        return SX_E_NOMEM;
    }
    hipError_t e = hipMemcpy(mem, T.map, sizeof T.map, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + sizeof T.map, T.next.data(), next_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && here_bytes) e = hipMemcpy(mem + at_here, T.here.data(), here_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mem + at_end, T.end.data(), end_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(mem); ctx->set_err(std::string("hipMemcpy: ") + hipGetErrorString(e)); return SX_E_HIP; }
    sx_label_set* set = new (std::nothrow) sx_label_set;
    if (!set) { (void)hipFree(mem); return SX_E_NOMEM; }
    set->device = ctx->device; set->mem = mem;
    set->dev = LabelDevice{ mem, (const uint16_t*)(mem + sizeof T.map), (const uint64_t*)(mem + at_here), (const uint64_t*)(mem + at_end),
                            (uint64_t*)(mem + at_findings), (uint64_t*)(mem + at_findings + counters), T.root_here, T.all,
                            T.states, T.classes, T.lds_states, T.here_first, T.dead, T.n_patterns };
    set->info = sx_label_set_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)(sizeof T.map + next_bytes + here_bytes + end_bytes), T.lds_states, (uint32_t)T.here.size() };
    if (sx_label_set_reset(set) != SX_OK) { ctx->set_err("label set: the counters could not be reset"); sx_label_set_free(set); return SX_E_HIP; }
    *out = set;
    return SX_OK;
}

int sx_label_set_info_get(const sx_label_set* set, sx_label_set_info* out) {
    if (!set || !out) return SX_E_INVALID;
    *out = set->info;
    return SX_OK;
}

void sx_label_set_free(sx_label_set* set) {
    if (!set) return;
    (void)hipFree(set->mem);
    delete set;
}

int sx_label_set_read(const sx_label_set* set, uint64_t* findings, uint64_t* first, uint32_t n_patterns) {
    if (!set || n_patterns != set->info.n_patterns) return SX_E_INVALID;
    if (hipSetDevice(set->device) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    for (int k = 0; k < 2; k++) {
        uint64_t* out = k ? first : findings;
        if (!out) continue;
        if (hipMemcpy(out, k ? set->dev.first : set->dev.findings, (size_t)n_patterns * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    }
    return SX_OK;
}

int sx_label_set_counters_device(const sx_label_set* set, const uint64_t** d_findings, const uint64_t** d_first) {
    if (!set) return SX_E_INVALID;
    if (d_findings) *d_findings = set->dev.findings;
    if (d_first) *d_first = set->dev.first;
    return SX_OK;
}

// The labels where the findings lie (sx_label_dev.hip): the source is checked as a whole, the labels' memory is had, then one kernel per
// segment, each with the ordinal of its first record, on the selections' stream, and one wait.  Only the labels and the set's counters
// are written.
int sx_result_label_device(sx_ctx* ctx, const sx_result* r, sx_label_set* set, uint64_t ordinal_base, sx_labels** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !set || !out) return SX_E_INVALID;
    if (ctx->host_only) { ctx->set_err("host-only context: no device labels"); return SX_E_STATE; }
    if (set->device != ctx->device) { ctx->set_err("the label set lies on another device"); return SX_E_INVALID; }
    { const int rc = result_on_device(ctx, r, "label on the host"); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    sx_labels* lab = new (std::nothrow) sx_labels;
    if (!lab) return SX_E_NOMEM;
    lab->device = ctx->device;
    uint64_t bytes = 0;
    for (const MissionFindings& s : r->r.segs) bytes += ((uint64_t)s.ext_nf * sizeof(uint64_t) + 255) / 256 * 256;
    if (hipMalloc((void**)&lab->mem, bytes ? bytes : 256) != hipSuccess) {
        (void)hipGetLastError();
        delete lab;
        ctx->set_err("device labels: no memory for " + std::to_string(bytes) + " bytes of labels");
        return SX_E_NOMEM;
    }
    uint64_t walked = 0, at = 0;
    hipError_t e = hipSuccess;
    for (const MissionFindings& s : r->r.segs) {
        sx_labels::Seg seg;
        seg.d = (const uint64_t*)(lab->mem + at); seg.recs = s.dev_copy; seg.n = s.ext_nf; seg.epoch_ref = s.dev_epoch_ref; seg.epoch = s.dev_epoch;
        lab->segs.push_back(seg);
        LabelParams p;
        memset(&p, 0, sizeof p);
        p.recs = s.dev_copy; p.arena = (const uint8_t*)s.dev_copy + s.ext_nf * s.rec_size(); p.n = s.ext_nf; p.packed = s.packed ? 1u : 0u;
        p.ordinal = ordinal_base + walked;
        p.labels = (uint64_t*)(lab->mem + at);
        p.set = set->dev;
        e = label_launch(p, st);
        if (e != hipSuccess) break;
        walked += s.ext_nf;
        at += ((uint64_t)s.ext_nf * sizeof(uint64_t) + 255) / 256 * 256;
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        sx_labels_free(lab);
        ctx->set_err(std::string("device labels: ") + hipGetErrorString(e));
        return SX_E_HIP;
    }
    *out = lab;
    return SX_OK;
}

uint64_t sx_labels_segments(const sx_labels* labels) { return labels ? labels->segs.size() : 0; }

int sx_labels_segment_device(const sx_labels* labels, uint64_t segment, const uint64_t** d_labels, uint64_t* n_findings) {
    if (d_labels) *d_labels = nullptr;
    if (n_findings) *n_findings = 0;
    if (!labels || segment >= labels->segs.size()) return SX_E_INVALID;
    if (d_labels) *d_labels = labels->segs[segment].d;
    if (n_findings) *n_findings = labels->segs[segment].n;
    return SX_OK;
}

void sx_labels_free(sx_labels* labels) {
    if (!labels) return;
    (void)hipFree(labels->mem);
    delete labels;
}

int sx_result_select_labels_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels, uint64_t any, uint64_t all, uint64_t none, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !labels || !out) return SX_E_INVALID;
    if (ctx->host_only) { ctx->set_err("host-only context: no device selection"); return SX_E_STATE; }
    if (labels->device != ctx->device) { ctx->set_err("the labels lie on another device"); return SX_E_INVALID; }
    const uint64_t masks[3] = { any, all, none };
    return select_on_device(ctx, r, nullptr, 0, nullptr, nullptr, nullptr, 0, out, labels, masks);
}

int sx_get_stats(const sx_ctx* ctx, sx_stats* out) {
    if (!ctx || !out) return SX_E_INVALID;
    *out = ctx->stats;
    return SX_OK;
}

void sx_free(void* p) { free(p); }

int sx_fill_background_device(sx_ctx* ctx, void* device_bytes, uint64_t first_byte_index, uint64_t len, uint64_t seed) {
    if (!ctx || ctx->host_only) return SX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_fill_background((uint8_t*)device_bytes, first_byte_index, len, seed, ctx->dev[0].stream_b));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->dev[0].stream_b));
    return SX_OK;
}

int sx_device_alloc(sx_ctx* ctx, uint64_t bytes, void** device_ptr) {
    if (!ctx || ctx->host_only || !device_ptr) return SX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc(device_ptr, bytes ? bytes : 1));
    return SX_OK;
}
int sx_device_free(sx_ctx* ctx, void* device_ptr) {
    if (!ctx || ctx->host_only) return SX_E_STATE;
    HIP_TRY(ctx, hipFree(device_ptr));
    return SX_OK;
}
int sx_device_upload(sx_ctx* ctx, void* device_dst, const void* host_src, uint64_t bytes) {
    if (!ctx || ctx->host_only) return SX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(device_dst, host_src, bytes, hipMemcpyHostToDevice));
    return SX_OK;
}
int sx_device_download(sx_ctx* ctx, void* host_dst, const void* device_src, uint64_t bytes) {
    if (!ctx || ctx->host_only) return SX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(host_dst, device_src, bytes, hipMemcpyDeviceToHost));
    return SX_OK;
}

int sx_device_read_bandwidth(sx_ctx* ctx, const void* device_bytes, uint64_t len, int repeats, double* gbytes_per_s) {
    if (!ctx || ctx->host_only || !gbytes_per_s || repeats == 0) return SX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MissionDev& d = ctx->dev[0];
    uint64_t* d_out = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d_out, 8));
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, 8, d.stream));
    // repeats < 0: probe with the scan kernels' traversal (private sub-chunk per wavefront) instead of grid-stride
    const uint32_t sub = repeats < 0 ? (ctx->opt.subchunk_bytes ? ctx->opt.subchunk_bytes : 256u * 1024u) : 0u;
    if (repeats < 0) repeats = -repeats;
    HIP_TRY(ctx, launch_read_sum((const uint8_t*)device_bytes, len, d_out, d.stream, sub, ctx->sw.probe_rot));  // warm-up
    float best = 1e30f;
    for (int i = 0; i < repeats; i++) {
        HIP_TRY(ctx, hipEventRecord(d.slot[0].ev0, d.stream));
        HIP_TRY(ctx, launch_read_sum((const uint8_t*)device_bytes, len, d_out, d.stream, sub, ctx->sw.probe_rot));
        HIP_TRY(ctx, hipEventRecord(d.slot[0].ev1, d.stream));
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
        float ms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, d.slot[0].ev0, d.slot[0].ev1));
        if (ms < best) best = ms;
    }
    (void)hipFree(d_out);
    *gbytes_per_s = (double)(len / 16 * 16) / (best * 1e-3) / 1e9;
    return SX_OK;
}

}  // extern "C"
