// sx_stage_b.cpp — stage B: the exact replay of FindingCollection::from around long runs, on the
// device (regions, which of them stand, output offsets) and on the host (entry/exit of every buffer,
// missions with few runs, regions the device gives back).  The Missions' findings are interleaved by
// sx_merge.cpp; the drivers' arithmetic is sx_stage_b_plan.hpp's.
#include "sx_ctx.hpp"

using namespace sx;

namespace sx {

static_assert(plan::kBufLen == kInputBufLen, "sx_stage_b_plan.hpp counts windows from the input buffers' grid");
using plan::win_start_h;

bool device_replay_wanted(const sx_ctx* ctx, const ReplayJob& job, size_t k, size_t n_runs) {
    if (!job.d_bytes || ctx->host_only || job.is_last || ctx->missions[k].host_sequential()) return false;
    if (ctx->opt.flags & SX_OPT_HOST_REPLAY) return false;
    if (ctx->missions[k].q > 255) return false;   // (64 < q <= 255: the replay kernels' QBIG instantiations, round 4)
    // -n 0: SplitStr's exit 4 (helper.rs:317) then fires on a rejected char with nothing collected, which ends the
    // iteration for the whole decoder call (helper.rs:343) — accepted chars behind it are never carried, so the
    // rule "the last accepted char in front of a window start is the leftover" (derive_at) does not hold.  Such a
    // mission is replayed by ONE exact sequential pass on the host: no derived states, no speculation.
    if (ctx->missions[k].c.chars_min_nb == 0) return false;
    if (ctx->sw.host_replay) return false;
    if (wave_replay_wanted(ctx, job, k, n_runs)) return true;
    return (ctx->opt.flags & SX_OPT_DEVICE_REPLAY) || ctx->sw.device_replay || n_runs >= 4096;
}

// ---- a slab's output (the contract: sx_ctx.hpp)
int slab_strings_limit(sx_ctx* ctx, uint64_t string_bytes) {
    if (string_bytes <= 0xFFFFFFFFull) return SX_OK;
    ctx->set_err("more than 4 GiB of strings in one chunk");
    return SX_E_NOMEM;
}

// the slab's output buffer, large enough and free: a copy of an earlier slab may still read it — the stream waits, or the host if
// the buffer must grow
int slab_out_reserve(sx_ctx* ctx, MissionDev& d, const SlabOutPath& p, const plan::SlabOut& lay, uint8_t** d_all) {
    if (p.reuse_after) {
        if (d.d_rp_cap[p.slot] < lay.bytes + 64) HIP_TRY(ctx, hipEventSynchronize(p.reuse_after));
        else HIP_TRY(ctx, hipStreamWaitEvent(p.stream, p.reuse_after, 0));
    }
    const int rc = ensure_rp(ctx, d, p.slot, lay.bytes + 64); if (rc) return rc;
    *d_all = (uint8_t*)d.d_rp[p.slot];
    return SX_OK;
}

// the host's entry part (a few findings) goes in front of what the device writes: the missions can be interleaved on the device
int slab_out_upload_entry(sx_ctx* ctx, const SlabOutPath& p, const plan::SlabOut& lay, uint8_t* d_all, const void* recs, const void* strings) {
    if (!lay.nfh) return SX_OK;
    HIP_TRY(ctx, hipMemcpyAsync(d_all, recs, lay.nfh * lay.rec, hipMemcpyHostToDevice, p.stream));
    if (lay.nbh) HIP_TRY(ctx, hipMemcpyAsync(d_all + lay.host_s, strings, lay.nbh, hipMemcpyHostToDevice, p.stream));
    return SX_OK;
}

int slab_out_deliver(sx_ctx* ctx, const SlabOutPath& p, const plan::SlabOut& lay, SlabDest dest, const uint8_t* d_all, PinnedPool::Block* blk) {
    if (dest != SlabDest::Pinned) return SX_OK;
    *blk = ctx->pool->take(lay.bytes + 64);
    if (!blk->p) { ctx->set_err("hipHostMalloc failed"); return SX_E_NOMEM; }
    if (p.async_copy) {   // on the copy stream: the next slab's kernels run meanwhile
        if (p.leaves_copy_running) ctx->slab_copy_pending = true;   // (from here on the block must not go back to the pool before slab_copy_drain)
        HIP_TRY(ctx, hipEventRecord(p.written, p.stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->merge_copy_stream, p.written, 0));
        HIP_TRY(ctx, hipMemcpyAsync(blk->p, d_all, lay.bytes, hipMemcpyDeviceToHost, ctx->merge_copy_stream));
        HIP_TRY(ctx, hipEventRecord(p.copied, ctx->merge_copy_stream));
    } else {
        // (experiments, SX_REPLAY_COPY_WGS=n: the copy as a kernel of n workgroups instead of the runtime's blit, which slows every
        // kernel next to it — here: the last Mission's scan launch, DESIGN.md section 2 "Schedule")
        if (p.copy_wgs > 0 && lay.bytes >= (1u << 20)) HIP_TRY(ctx, launch_copy_bytes(blk->p, d_all, lay.bytes, (uint32_t)p.copy_wgs, p.stream, ctx->sw.merge_copy_threads, ctx->sw.merge_copy_nt != 0));
        else HIP_TRY(ctx, hipMemcpyAsync(blk->p, d_all, lay.bytes, hipMemcpyDeviceToHost, p.stream));
    }
    return SX_OK;
}

int slab_out_settle(sx_ctx* ctx, const SlabOutPath& p, const plan::SlabOut& lay) {
    if (!p.async_copy || lay.nfh) HIP_TRY(ctx, hipStreamSynchronize(p.stream));
    return SX_OK;
}

void slab_out_describe(const sx_ctx* ctx, const SlabOutPath& p, const plan::SlabOut& lay, SlabDest dest, const PinnedPool::Block& blk,
                       const uint8_t* d_all, MissionFindings* seg) {
    seg->ext_nf = lay.findings(); seg->ext_na = lay.strings();
    if (dest == SlabDest::Pinned) { seg->ext = blk; seg->dev_copy = p.async_copy ? nullptr : d_all; return; }
    seg->dev_only = true; seg->dev_copy = d_all;
    if (dest == SlabDest::Keep) keep_on_device(*seg, ctx);
}

// Stage B of one mission on the device (sx_replay_dev.hip) + the little the host keeps:
// the chunk's strict entry region, regions the device gave back, the exact exit state.
// One slab = the runs [i0, i1) of the list (all of them unless the mission is replayed in slabs, see device_replay_mission):
// its regions begin in [job.lo, job.hi); what it writes goes to the host on the copy stream, behind `copied`.
struct Slab {
    size_t i0 = 0, i1 = 0;
    bool first = true, last = true;   // first: the host's entry part belongs to it; last: the exit state
    SlabOutPath out;                  // its output buffer (two in turn), and whether the copy to the host is left running
    // one of several Missions: what this slab may write at most — from there on the Mission's output could reach the deferral
    // threshold, which only the whole-list path knows (SX_RETRY_WHOLE); 0: no bound
    uint64_t out_budget = 0;
    // the mission's own start in this buffer (the job's lo / entry_exact are the slab's): the exit state is replayed from the
    // last region's start, which may lie in an earlier slab
    uint64_t lo0 = 0;
    bool entry_exact0 = false;
};
struct SlabCarry {                    // from slab to slab: where the replay stands
    uint64_t last_start = 0;
    bool last_is_entry = false, any = false;
};
constexpr int SX_RETRY_WHOLE = 1000;  // (internal) a slab met something only the whole-list path handles
constexpr size_t kEdgeRuns = 8192;    // the part of a list the host may read without the whole copy: [0, kEdgeRuns) and [n - kEdgeRuns, n)

// One slab's replay: what device_replay_slab's steps hand on to each other.
struct SlabReplay {
    sx_ctx* ctx; const size_t k; ByteView& view; const ReplayJob& job; const RunList& runs; const Slab& sl; MissionFindings* out;
    const Mission& m; MissionDev& d;
    const size_t n_all, n, W;         // n: the runs this slab's kernels visit (lookups may go on to the list's end)
    const bool slabbed;
    // pass 1
    ReplayParams P{};
    uint64_t* h_tot = nullptr;        // kTotCount totals; words 32, 33: the fast pre-pass' statistics
    ReplayRegionOut* ro = nullptr;    // the regions' records, when the host decides what stands
    bool dev_stitch, fast_pass = false;
    // where the replay stands
    uint64_t E, last_start;           // last_start: start of the last region of any kind (for the exit state)
    bool last_is_entry;
    std::deque<ReplayPart> host_parts;
    struct Seg { int host_part; size_t v0, v1; };  // host_part >= 0, or device regions [v0, v1) of `valid`
    std::vector<Seg> segs;
    // what stands
    std::vector<uint64_t> valid, fbase, abase;
    uint64_t nf = 0, nb = 0, n_standing = 0;
    // pass 2
    plan::SlabOut lay; SlabOutPath path; SlabDest dest = SlabDest::Pinned;
    PinnedPool::Block blk{};
    uint8_t* d_all = nullptr;
    bool entry_only = false;
    const MissionFindings* hf0 = nullptr;   // the host's entry part, if it is all the host has
    std::vector<sx_finding> entry_f;

    SlabReplay(sx_ctx* ctx, size_t k, ByteView& view, const ReplayJob& job, const RunList& runs, const Slab& sl, const SlabCarry& carry, MissionFindings* out)
        : ctx(ctx), k(k), view(view), job(job), runs(runs), sl(sl), out(out), m(ctx->missions[k]), d(ctx->dev[k]), n_all(runs.size()),
          n(sl.i1 - sl.i0), W(m.window), slabbed(!(sl.first && sl.last)), dev_stitch(n > 0 && !ctx->sw.host_stitch),
          E(std::min(job.lo[k], job.hi)), last_start(carry.any ? carry.last_start : E), last_is_entry(carry.any ? carry.last_is_entry : false) {}

    // the steps, in device_replay_slab's order
    int pinned_totals(bool with_regions), queue_pass1(), host_entry_part(), finish_stitch(), retry_or_give_back(), what_stands();
    int pass2_and_deliver(uint64_t defer_min_bytes), exit_state(uint64_t* end_pos);
    void splice();
};

// (the regions' records only travel to the host when it decides what stands: 24 bytes per run, 6 GB for C5's floods)
int SlabReplay::pinned_totals(bool with_regions) {
    const int rc = ensure_pinned2(ctx, (with_regions ? n * sizeof(ReplayRegionOut) : 0) + 512);
    if (rc != SX_OK) return rc;
    h_tot = (uint64_t*)ctx->h_pin2;
    ro = (ReplayRegionOut*)(ctx->h_pin2 + 384);
    return SX_OK;
}

// ---- pass 1 on the device: every region's extent and output size; then (still on the
// device) which regions stand and where each writes.  The host keeps its own version of
// that step for buffers with regions the device gave back (kRegionTooLong).
int SlabReplay::queue_pass1() {
    int rc = pinned_totals(!dev_stitch);
    if (rc != SX_OK) return rc;
    if (!n) return SX_OK;
    rc = ensure_rp(ctx, d, kRpRuns, n * sizeof(sx_run)); if (rc) return rc;
    rc = ensure_rp(ctx, d, kRpRegionOut, n * sizeof(ReplayRegionOut)); if (rc) return rc;
    rc = ensure_rp(ctx, d, kRpIdx, n * 8); if (rc) return rc;
    rc = ensure_rp(ctx, d, kRpFbase, (n + 1) * 8); if (rc) return rc;
    rc = ensure_rp(ctx, d, kRpAbase, (n + 1) * 8); if (rc) return rc;
    rc = ensure_rp(ctx, d, kRpStitchBlocks, stitch_blocks_bytes(n, ctx->sw.stitch_block)); if (rc) return rc;
    rc = ensure_rp(ctx, d, kRpTotals, kTotCount * 8); if (rc) return rc;
    rc = ensure_scratch(ctx, stitch_scratch_bytes(n)); if (rc) return rc;
    ReplayRegionOut* d_ro = (ReplayRegionOut*)d.d_rp[kRpRegionOut];
    if (!runs.on_device)   // (never slabbed)
        HIP_TRY(ctx, hipMemcpyAsync(d.d_rp[kRpRuns], runs.data(), n * sizeof(sx_run), hipMemcpyHostToDevice, d.stream_b));
    P.data = job.d_bytes; P.len = job.len; P.runs = (runs.on_device ? runs.dev_ptr : (const sx_run*)d.d_rp[kRpRuns]) + sl.i0; P.n_runs = n;
    P.n_look = n_all - sl.i0;
    P.lo = job.lo[k]; P.hi = job.hi; P.consumed0 = job.consumed0[k]; P.stream0 = job.stream0[k];
    P.slice_base = job.slice_base; P.encoding = m.c.encoding; P.table = d.d_table;
    P.chars_min_nb = m.c.chars_min_nb; P.same_block = m.c.require_same_unicode_block; P.q = (uint32_t)m.q;
    P.W = (uint32_t)W; P.long_run = m.long_run; P.skip = ctx->sw.no_replay_skip ? 0u : 1u; P.grep_char = m.c.grep_char; P.mission_id = m.c.mission_id;
    P.file_id = job.file_id; P.af_lo = m.c.af_lo; P.af_hi = m.c.af_hi; P.ubf = m.c.ubf;
    P.max_windows = kMaxRegionWindowsDefault;
    P.entry_skip = m.buf_entry_skip;
    P.grid_flags = nullptr; P.grid_sub = 0;
    // (not for gb18030 / GBK — ADVICE round 5: the scan kernel publishes the hang-over of the TWO-byte grammar; a four-byte token that
    //  straddles a sub-chunk start followed by lead / digit bytes only would start the walk two bytes off and never resynchronise)
    if (d.grid_of_scan && d.grid_data == job.d_bytes && d.grid_len == job.len && !ctx->sw.no_grid_bound && !enc_is_gb(m.c.encoding)) { P.grid_flags = d.grid_of_scan; P.grid_sub = d.grid_sub; }
    if (ctx->sw.max_region_windows) P.max_windows = ctx->sw.max_region_windows;
    // pass-1 output cache: one arena for all replaying regions (slot = arena / their number, on the device)
    if (dev_stitch && !ctx->sw.no_replay_cache) {
        // (plan::cache_arena_bytes: a flood of runs gets slots of the minimum size for as many regions as possible — a region
        // without slot is replayed twice)
        uint64_t free_plus_held = 0;
        if (plan::cache_arena_asks_free(n)) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) == hipSuccess) free_plus_held = (uint64_t)fr + ctx->d_cache_cap;
        }
        uint64_t arena = plan::cache_arena_bytes(n, free_plus_held, ctx->sw.replay_cache_mib);
        const uint64_t lists = (uint64_t)(3 * n + 8) * 4 + 512;   // slot_of, n_heads, head_list; (round 5) n_hard, hard_list
        rc = ensure_cache(ctx, arena + lists);
        while (rc != SX_OK && arena > (64ull << 20)) {   // the device is short of memory: a smaller arena (more regions are replayed twice)
            (void)hipGetLastError();
            arena /= 2;
            rc = ensure_cache(ctx, arena + lists);
        }
        if (rc) return rc;
        rc = ensure_scratch(ctx, std::max(stitch_scratch_bytes(n), replay_heads_scratch_bytes(n))); if (rc) return rc;
        uint8_t* base = ctx->d_cache;
        P.cache_arena = base; P.arena_bytes = arena & ~255ull;
        uint32_t* slot_of = (uint32_t*)(base + plan::up256(arena));
        P.slot_of = slot_of; P.n_heads = slot_of + n + 1; P.head_list = slot_of + n + 2;
        HIP_TRY(ctx, launch_replay_heads(P, slot_of, slot_of + n + 1, slot_of + n + 2, d_ro, ctx->d_scratch, ctx->d_scratch_cap, d.stream_b));
        // (round 5) the fast pre-pass settles the regions that are one run inside one window; the general kernel gets the rest
        P.n_hard = slot_of + 2 * n + 4; P.hard_list = slot_of + 2 * n + 5;
        if (replay_fast_covers(P) && ctx->sw.fast_replay) {
            HIP_TRY(ctx, hipMemsetAsync(P.n_hard, 0, 4, d.stream_b));
            HIP_TRY(ctx, launch_replay_fast(P, d_ro, d.stream_b));
            fast_pass = true;
        } else { P.n_hard = nullptr; P.hard_list = nullptr; }
    }
    HIP_TRY(ctx, launch_replay_count(P, d_ro, d.stream_b, ctx->sw.count_waves));
    if (fast_pass) {   // (statistics: how many regions each pass took; read with the totals below)
        h_tot[32] = 0; h_tot[33] = 0;
        rc = read_back_async(ctx, d.stream_b, h_tot + 32, P.n_hard, 4);
        if (rc == SX_OK) rc = read_back_async(ctx, d.stream_b, h_tot + 33, P.n_heads, 4);
        if (rc != SX_OK) return rc;
    }
    // The host's copy of a device-joined run list: its share of this replay (the buffer's entry region, the exit state)
    // reads only the list's two ends — a large list is not copied whole (68 MB for the headline's 2.8 M runs, 1.2 ms on
    // the critical path when nothing else runs); the rest follows on demand (regions the device gives back).
    if (runs.size() * sizeof(sx_run) <= (4u << 20)) HIP_TRY(ctx, runs.start_copy());
    if (dev_stitch) {
        HIP_TRY(ctx, hipMemsetAsync(d.d_rp[kRpTotals], 0, kTotCount * 8, d.stream_b));
        HIP_TRY(ctx, launch_stitch_blocks(P, d_ro, (uint8_t*)d.d_rp[kRpIdx], d.d_rp[kRpStitchBlocks], (uint64_t*)d.d_rp[kRpTotals], d.stream_b, ctx->sw.stitch_block));
    } else
        HIP_TRY(ctx, hipMemcpyAsync(ro, d_ro, n * sizeof(ReplayRegionOut), hipMemcpyDeviceToHost, d.stream_b));
    return SX_OK;
}

// ---- meanwhile on the host: the strict entry region (exact carried state), if any
int SlabReplay::host_entry_part() {
    if (dev_stitch) HIP_TRY(ctx, runs.fetch_edges(kEdgeRuns)); else HIP_TRY(ctx, runs.wait());   // (the host's stitch walks the whole list)
    if (!job.entry_exact[k]) return SX_OK;
    const size_t head_n = runs.full() ? n_all : kEdgeRuns;
    // The chunk's first window belongs to the host: only it has the exact carried state
    // (leftover, cut flag, and the decoder's pending bytes, which cannot be re-derived here).
    host_parts.emplace_back();
    replay_part(m, ctx->states[k], job.consumed0[k], job.stream0[k], view, job.len, job.file_id, false, runs.data(), head_n,
                job.lo[k], job.lo[k] + 1, true, &host_parts.back());
    if (head_n < n_all && host_parts.back().end_pos >= runs[head_n - 1].start) {   // it ran into what was not copied: the whole list
        HIP_TRY(ctx, runs.wait());
        host_parts.pop_back();
        host_parts.emplace_back();
        replay_part(m, ctx->states[k], job.consumed0[k], job.stream0[k], view, job.len, job.file_id, false, runs.data(), n_all,
                    job.lo[k], job.lo[k] + 1, true, &host_parts.back());
    }
    if (host_parts.back().regions.empty()) host_parts.pop_back();
    else { segs.push_back({ (int)host_parts.size() - 1, 0, 0 }); last_is_entry = true; E = std::max(E, host_parts.back().end_pos); }
    E = std::max(E, job.lo[k] + 1);
    return SX_OK;
}

// the stitch from where the entry part ended, the totals' way back, and the one wait of pass 1
int SlabReplay::finish_stitch() {
    if (dev_stitch) {
        HIP_TRY(ctx, launch_stitch_finish(P, (const ReplayRegionOut*)d.d_rp[kRpRegionOut], (uint8_t*)d.d_rp[kRpIdx], d.d_rp[kRpStitchBlocks], E,
                                          (uint64_t*)d.d_rp[kRpFbase], (uint64_t*)d.d_rp[kRpAbase], (uint64_t*)d.d_rp[kRpTotals], ctx->d_scratch,
                                          ctx->d_scratch_cap, d.stream_b, ctx->sw.stitch_block));
        { const int rb = read_back_async(ctx, d.stream_b, h_tot, d.d_rp[kRpTotals], kTotCount * 8); if (rb != SX_OK) return rb; }
    }
    SX_TL("  replay: pass 1 + stitch queued, host entry part done");
    if (n) HIP_TRY(ctx, hipStreamSynchronize(d.stream_b));
    SX_TL("  replay: pass 1 + stitch done");
    return SX_OK;
}

// SX_RETRY_WHOLE: a slab with regions for the host, or one that would take the Mission's output to the deferral threshold.
// Regions for the host in a whole list: it also decides what stands.
int SlabReplay::retry_or_give_back() {
    if (dev_stitch && h_tot[kTotTooLong] && slabbed) return SX_RETRY_WHOLE;
    if (dev_stitch && slabbed && sl.out_budget && h_tot[kTotFindings] * sizeof(sx_finding) + h_tot[kTotBytes] >= sl.out_budget) return SX_RETRY_WHOLE;
    if (dev_stitch && h_tot[kTotTooLong]) {
        dev_stitch = false;
        HIP_TRY(ctx, runs.wait());
        const uint64_t keep32 = h_tot[32], keep33 = h_tot[33];
        const int rc = pinned_totals(true);   // (the totals' values are not read again)
        if (rc != SX_OK) return rc;
        h_tot[32] = keep32; h_tot[33] = keep33;
        HIP_TRY(ctx, hipMemcpyAsync(ro, d.d_rp[kRpRegionOut], n * sizeof(ReplayRegionOut), hipMemcpyDeviceToHost, d.stream_b));
        HIP_TRY(ctx, hipStreamSynchronize(d.stream_b));
    }
    return SX_OK;
}

// the device's totals, or the host's walk: a region is void if an earlier one ran over its start
int SlabReplay::what_stands() {
    if (fast_pass && n) {
        std::lock_guard<std::mutex> g(ctx->mu);
        ctx->stats.fast_regions += (uint32_t)h_tot[33] - (uint32_t)h_tot[32];
        ctx->stats.general_regions += (uint32_t)h_tot[32];
    }
    if (dev_stitch) {
        nf = h_tot[kTotFindings]; nb = h_tot[kTotBytes]; n_standing = h_tot[kTotStanding];
        out->replay_bytes += h_tot[kTotReplayBytes];
        if (h_tot[kTotLast] != ~0ull) {
            E = std::max(E, h_tot[kTotEnd]);
            last_start = h_tot[kTotLastStart];
            last_is_entry = false;
        }
    } else {
        valid.reserve(n); fbase.reserve(n + 1); abase.reserve(n + 1);
        for (size_t i = 0; i < n; i++) {
            const uint32_t st = ro[i].status;
            if (st == kRegionChained || st == kRegionNotMine) continue;
            const uint64_t want = win_start_h(runs[i].start, W);
            if (want >= job.hi) break;
            if (want < E) continue;
            if (st == kRegionTooLong) {  // given back: the host replays it (and whatever it runs into)
                host_parts.emplace_back();
                replay_part(m, ctx->states[k], job.consumed0[k], job.stream0[k], view, job.len, job.file_id, false, runs.data(),
                            n, want, want + 1, false, &host_parts.back());
                segs.push_back({ (int)host_parts.size() - 1, 0, 0 });
                E = std::max(E, host_parts.back().end_pos);
            } else {
                if (segs.empty() || segs.back().host_part >= 0) segs.push_back({ -1, valid.size(), valid.size() });
                valid.push_back(i); fbase.push_back(nf); abase.push_back(nb);
                segs.back().v1 = valid.size();
                nf += ro[i].n_find; nb += ro[i].n_bytes;
                E = std::max(E, ro[i].end);
            }
            last_start = want; last_is_entry = false;
        }
        fbase.push_back(nf); abase.push_back(nb);
        n_standing = valid.size();
        for (uint64_t v : valid) out->replay_bytes += ro[v].end - win_start_h(runs[v].start, W);
    }
    return slab_strings_limit(ctx, nb);
}

// ---- pass 2: the standing regions write findings and strings, in order; the D2H lands in a
// pinned block that becomes the result's storage (no copy).  The host's entry part (the chunk's first
// region, replayed from the exact carried state) goes in front of it in the same block: the device writes
// its str_off already shifted by that part's strings.  Only regions the device gave back to the host
// (somewhere in the middle) need the finding-by-finding splice.
int SlabReplay::pass2_and_deliver(uint64_t defer_min_bytes) {
    entry_only = dev_stitch && host_parts.size() == 1;
    hf0 = entry_only ? &host_parts[0].findings : nullptr;
    lay = plan::slab_out_layout(hf0 ? hf0->v.size() : 0, nf, hf0 ? hf0->arena.size() : 0, nb, sizeof(sx_finding));
    int rc = slab_strings_limit(ctx, lay.strings()); if (rc) return rc;
    if (!n_standing) return SX_OK;
    path = sl.out; path.stream = d.stream_b; path.copy_wgs = ctx->sw.replay_copy_wgs;
    rc = slab_out_reserve(ctx, d, path, lay, &d_all); if (rc) return rc;
    sx_finding* d_f = (sx_finding*)(d_all + lay.dev_f);
    uint8_t* d_a = d_all + lay.dev_s;
    if (dev_stitch) {
        P.str_off_base = (uint32_t)lay.nbh;
        HIP_TRY(ctx, launch_replay_write_flagged(P, (const ReplayRegionOut*)d.d_rp[kRpRegionOut], (const uint8_t*)d.d_rp[kRpIdx],
                                                 (const uint64_t*)d.d_rp[kRpFbase], (const uint64_t*)d.d_rp[kRpAbase], d_f, d_a,
                                                 (nf * sizeof(sx_finding) + nb) / std::max<uint64_t>(1, n_standing), d.stream_b));
        if (lay.nfh) {
            entry_f.assign(hf0->v.begin(), hf0->v.end());
            for (sx_finding& f : entry_f) f.slice_index += job.slice_base;
            rc = slab_out_upload_entry(ctx, path, lay, d_all, entry_f.data(), hf0->arena.data()); if (rc) return rc;
        }
    } else {
        const size_t nv = valid.size();
        HIP_TRY(ctx, hipMemcpyAsync(d.d_rp[kRpIdx], valid.data(), nv * 8, hipMemcpyHostToDevice, d.stream_b));
        HIP_TRY(ctx, hipMemcpyAsync(d.d_rp[kRpFbase], fbase.data(), (nv + 1) * 8, hipMemcpyHostToDevice, d.stream_b));
        HIP_TRY(ctx, hipMemcpyAsync(d.d_rp[kRpAbase], abase.data(), (nv + 1) * 8, hipMemcpyHostToDevice, d.stream_b));
        HIP_TRY(ctx, launch_replay_write(P, (const uint64_t*)d.d_rp[kRpIdx], (const uint64_t*)d.d_rp[kRpFbase],
                                         (const uint64_t*)d.d_rp[kRpAbase], nv, d_f, d_a, d.stream_b));
    }
    const bool nothing_to_splice = dev_stitch && (host_parts.empty() || entry_only);
    // a large output of one of several missions: the caller interleaves the missions on the device first, one copy instead of two
    if (defer_min_bytes && nf * sizeof(sx_finding) + nb >= defer_min_bytes && nothing_to_splice) dest = SlabDest::Defer;
    // SX_OPT_RESULT_ON_DEVICE (round 5): one Mission, the whole buffer in this one slab, nothing the host has to splice in — it stays here
    if (single_result_stays_on_device(ctx, job, defer_min_bytes) && sl.first && sl.last && !sl.out.async_copy && nothing_to_splice) dest = SlabDest::Keep;
    rc = slab_out_deliver(ctx, path, lay, dest, d_all, &blk); if (rc) return rc;
    SX_TL("  replay: pass 2 + copy queued (%llu bytes%s)", (unsigned long long)lay.bytes, dest != SlabDest::Pinned ? ", stays on the device" : "");
    rc = slab_out_settle(ctx, path, lay); if (rc) return rc;
    SX_TL("  replay: pass 2 + copy done");
    return SX_OK;
}

// ---- splice (almost always: device findings only, or the entry part in front of them)
void SlabReplay::splice() {
    const bool on_device = dest != SlabDest::Pinned;
    if (host_parts.empty() || (entry_only && (blk.p || on_device))) {
        if (on_device || blk.p) slab_out_describe(ctx, path, lay, dest, blk, d_all, out);
        if (hf0) out->replay_bytes += hf0->replay_bytes;
        return;
    }
    const sx_finding* dev_f = (const sx_finding*)blk.p;
    const char* dev_a = blk.p ? (const char*)blk.p + nf * sizeof(sx_finding) : nullptr;
    if (dev_stitch) {  // only the entry part can be here; everything the device wrote follows it
        fbase.assign({ 0, nf }); abase.assign({ 0, nb });
        if (n_standing) segs.push_back({ -1, 0, 1 });
    }
    for (const Seg& g : segs) {
        if (g.host_part >= 0) {
            const MissionFindings& hf = host_parts[(size_t)g.host_part].findings;
            const uint32_t base = (uint32_t)out->arena.size();
            out->arena += hf.arena;
            for (sx_finding f : hf.v) { f.str_off += base; f.slice_index += job.slice_base; out->v.push_back(f); }
            out->replay_bytes += hf.replay_bytes;
        } else if (g.v1 > g.v0) {
            const uint64_t f0 = fbase[g.v0], f1 = fbase[g.v1], a0 = abase[g.v0], a1 = abase[g.v1];
            const uint32_t base = (uint32_t)out->arena.size();
            out->arena.append(dev_a + a0, a1 - a0);
            for (uint64_t j = f0; j < f1; j++) { sx_finding f = dev_f[j]; f.str_off = f.str_off - (uint32_t)a0 + base; out->v.push_back(f); }
        }
    }
    ctx->pool->give(blk);
}

// ---- the state handed to the next chunk: replay the last region and the tail once more
// on the host, only for its final state (RangeReplay's tail rule makes it exact)
int SlabReplay::exit_state(uint64_t* end_pos) {
    if (job.commit_state) {
        const uint64_t lo0 = slabbed ? sl.lo0 : job.lo[k];
        const bool exact0 = slabbed ? sl.entry_exact0 : job.entry_exact[k] != 0;
        const uint64_t from = plan::exit_replay_from(job.len, W, lo0, E, last_start, last_is_entry);
        ReplayPart fin;
        const sx_run* fr = runs.data();
        size_t fn = n_all;
        if (!runs.full()) {   // the list's tail is enough if it begins in front of `from`
            if (n_all > kEdgeRuns && runs[n_all - kEdgeRuns].start <= from) { fr = runs.data() + (n_all - kEdgeRuns); fn = kEdgeRuns; }
            else HIP_TRY(ctx, runs.wait());
        }
        replay_part(m, ctx->states[k], job.consumed0[k], job.stream0[k], view, job.len, job.file_id, false, fr, fn,
                    from, job.len, exact0 && from == lo0, &fin);
        ctx->states[k] = fin.state;
        ctx->states[k].consumed_bytes = job.consumed0[k] + job.len;
        ctx->states[k].stream_bytes = job.stream0[k] + job.len;
        E = job.len;
    }
    if (end_pos) *end_pos = std::max(E, std::min(job.hi, job.len));
    return SX_OK;
}

static int device_replay_slab(sx_ctx* ctx, size_t k, ByteView& view, const ReplayJob& job, const RunList& runs, const Slab& sl,
                              SlabCarry& carry, MissionFindings* out, uint64_t* end_pos, uint64_t defer_min_bytes) {
    const double t0 = now_ms();
    SlabReplay r(ctx, k, view, job, runs, sl, carry, out);
    int rc = r.queue_pass1();               if (rc != SX_OK) return rc;
    rc = r.host_entry_part();               if (rc != SX_OK) return rc;
    rc = r.finish_stitch();                 if (rc != SX_OK) return rc;
    rc = r.retry_or_give_back();            if (rc != SX_OK) return rc;
    const double t1 = now_ms();
    rc = r.what_stands();                   if (rc != SX_OK) return rc;
    const double t2 = now_ms();
    rc = r.pass2_and_deliver(defer_min_bytes); if (rc != SX_OK) return rc;
    const double t3 = now_ms();
    r.splice();
    rc = r.exit_state(end_pos);             if (rc != SX_OK) return rc;
    carry.last_start = r.last_start; carry.last_is_entry = r.last_is_entry; carry.any = true;
    if (ctx->sw.timing)
        fprintf(stderr, "[sx] device replay mission %zu: %zu runs, pass1+entry %.2f ms, validity %.2f ms (%zu standing, %zu host parts), "
                        "pass2+d2h %.2f ms (%llu findings), splice+state %.2f ms\n", k, r.n, t1 - t0, t2 - t1, (size_t)r.n_standing,
                r.host_parts.size(), t3 - t2, (unsigned long long)r.nf, now_ms() - t3);
    return SX_OK;
}

// The stream of the result copies (slabs, merge parts).
int ensure_copy_stream(sx_ctx* ctx) {
    if (ctx->merge_copy_stream) return SX_OK;
    HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->merge_copy_stream, hipStreamNonBlocking, 0));
    for (hipEvent_t& e : ctx->merge_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (hipEvent_t& e : ctx->slab_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return SX_OK;
}

// The last slab's copy is left running when device_replay_mission returns (the other Missions' stage A is collected, the host's
// share of stage B replayed meanwhile): whoever reads a slab's block, or gives one back to the pool, calls this first.
int slab_copy_drain(sx_ctx* ctx) {
    if (!ctx->slab_copy_pending.exchange(false)) return SX_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->merge_copy_stream));
    return SX_OK;
}

// Stage B of one mission on the device.  A mission with a long run list is replayed in slabs (a third of the list each, next to
// other Missions half of it, cut where a region begins): a slab's findings travel to the host while the next slab is replayed, and the last slab's copy is left
// running for the caller (slab_copy_drain) — the other Missions' stage A is collected and the host's share of stage B replayed
// under it.  Slab j begins where slab j-1 stopped — its last region may run past the cut —, with the state derived there as at a
// shard start.  The Mission's findings then are several blocks (MissionFindings::more), which merge_findings interleaves with
// the other Missions' on the host.  So, with several Missions, slabs are for the busy one among quiet ones:
//  * every other Mission has too few runs for the device by ctx->last_runs: that is this buffer's count for the Missions replayed
//    before this one, and the last buffer's for those that follow (their findings are on the host, the merge is the host's whatever
//    this Mission does) — two busy Missions are interleaved by device_merge, which wants each list in one piece.  A later Mission
//    that was quiet then and is busy now still comes out right: it is replayed whole, in one block, and the host merges;
//  * the output stays below the deferral threshold (defer_min_bytes: from there on it waits in HBM for device_merge).  It is
//    estimated from the last buffer's bytes per run, with a factor of two; and it is checked: every slab knows after pass 1 what
//    it will write, and the slab that would take the sum to the threshold hands the Mission to the whole-list path, which defers;
//  * the result goes to the host, and the buffer is not one of a sequence whose merged parts are still being copied (merge_async).
static bool slabs_next_to_others(const sx_ctx* ctx, size_t k, const ReplayJob& job) {
    if (ctx->missions.size() < 2 || (ctx->opt.flags & SX_OPT_RESULT_ON_DEVICE) || ctx->merge_async || ctx->sharded_call) return false;
    if (ctx->last_runs.size() != ctx->missions.size()) return false;
    for (size_t o = 0; o < ctx->missions.size(); o++)
        if (o != k && (ctx->missions[o].host_sequential() || device_replay_wanted(ctx, job, o, ctx->last_runs[o]))) return false;
    return true;
}

// how many slabs Mission k's list is cut into, at most
static size_t slabs_wanted(const sx_ctx* ctx, size_t k, const ReplayJob& job, const RunList& runs, uint64_t defer_min_bytes) {
    const size_t n = runs.size();
    const MissionDev& d = ctx->dev[k];
    size_t K = 1;
    const bool alone = ctx->missions.size() == 1 && defer_min_bytes == 0;
    const bool beside = !alone && slabs_next_to_others(ctx, k, job);
    const bool can = (alone || beside) && runs.on_device && !ctx->sw.host_stitch;
    const bool keep_dev_wanted = single_result_stays_on_device(ctx, job, defer_min_bytes);   // (one slab then: one block of the context's)
    // (measured on string-dense and text-like input, one Mission: 3 beats 2, 4 and 6.  Next to other Missions, on the headline — 1.4 M runs
    // and 60 MB of findings per half —: 2 beats 1, and 3 and 4 lose to 1: a slab costs two host waits, and the half that is replayed first
    // does so next to the following half's scan, where every kernel and wait takes longer)
    if (can && n >= (1u << 20) && !keep_dev_wanted) {
        K = beside ? 2 : 3;
        // (next to other Missions: only with a buffer behind this one — what the others yield, what this one writes per run)
        if (beside && (!d.last_out_runs || (defer_min_bytes && 2.0 * (double)n * (double)d.last_out_bytes / (double)d.last_out_runs >= (double)defer_min_bytes))) K = 1;
    }
    if (ctx->sw.slabs) { K = (size_t)ctx->sw.slabs; if (!can || n < 8 * K) K = 1; }
    return K;
}

// where to cut: idx = the slabs' first runs, closed with n; his[j] = where slab j's first region begins
static int cut_slabs(sx_ctx* ctx, size_t k, const ReplayJob& job, const RunList& runs, size_t K, std::vector<uint64_t>* idx, std::vector<uint64_t>* his) {
    const size_t n = runs.size();
    idx->assign(1, 0); his->assign(1, 0);
    if (K > 1) {
        MissionDev& d = ctx->dev[k];
        int rc = ensure_copy_stream(ctx); if (rc != SX_OK) return rc;
        rc = ensure_scratch(ctx, 4096); if (rc != SX_OK) return rc;
        rc = ensure_pinned2(ctx, 4096); if (rc != SX_OK) return rc;
        ReplayParams P{};
        P.runs = runs.dev_ptr; P.n_runs = n; P.W = (uint32_t)ctx->missions[k].window; P.grep_char = ctx->missions[k].c.grep_char;
        uint64_t* d_cut = (uint64_t*)ctx->d_scratch;
        HIP_TRY(ctx, launch_slab_cuts(P, (uint32_t)K, d_cut, d_cut + 64, d.stream_b));
        { const int rb = read_back_async(ctx, d.stream_b, ctx->h_pin2, d_cut, 128 * 8); if (rb != SX_OK) return rb; }
        HIP_TRY(ctx, hipStreamSynchronize(d.stream_b));
        const uint64_t* h = (const uint64_t*)ctx->h_pin2;
        plan::accept_slab_cuts(h, h + 64, K, n, job.hi, idx, his);
    }
    idx->push_back(n);
    return SX_OK;
}

static void note_output(MissionDev& d, size_t n_runs, const MissionFindings& out) {   // for the next buffer's estimate
    uint64_t bytes = out.count() * sizeof(sx_finding) + out.strings_len();
    for (const MissionFindings& m : out.more) bytes += m.count() * sizeof(sx_finding) + m.strings_len();
    d.last_out_runs = n_runs; d.last_out_bytes = bytes;
}

// The slabs one after the other.  SX_RETRY_WHOLE: nothing was produced and nothing is in flight — the whole-list path takes the Mission.
static int replay_in_slabs(sx_ctx* ctx, size_t k, ByteView& view, const ReplayJob& job, const RunList& runs, const std::vector<uint64_t>& idx,
                           const std::vector<uint64_t>& his, MissionFindings* out, uint64_t* end_pos, uint64_t defer_min_bytes) {
    MissionDev& d = ctx->dev[k];
    const size_t ns = idx.size() - 1;
    std::vector<MissionFindings> got;
    SlabCarry carry;
    hipEvent_t copied[2] = { ctx->slab_ev[1], ctx->slab_ev[2] };
    uint64_t e_prev = 0, written = 0;
    uint64_t fast0 = 0, general0 = 0;   // (a Mission handed to the whole-list path is counted once)
    { std::lock_guard<std::mutex> g(ctx->mu); fast0 = ctx->stats.fast_regions; general0 = ctx->stats.general_regions; }
    int rc = SX_OK;
    for (size_t j = 0; j < ns && rc == SX_OK; j++) {
        ReplayJob sj = job;
        sj.hi = j + 1 < ns ? std::min(job.hi, his[j + 1]) : job.hi;
        if (j > 0) { sj.lo[k] = std::max(job.lo[k], e_prev); sj.entry_exact[k] = 0; }
        sj.commit_state = job.commit_state && j + 1 == ns;
        Slab sl;
        sl.i0 = idx[j]; sl.i1 = idx[j + 1]; sl.first = j == 0; sl.last = j + 1 == ns;
        sl.out.slot = rp_out_slot(j); sl.out.async_copy = true; sl.out.leaves_copy_running = true;
        sl.out.reuse_after = j >= 2 ? copied[j & 1] : nullptr; sl.out.copied = copied[j & 1]; sl.out.written = ctx->slab_ev[0];
        sl.lo0 = job.lo[k]; sl.entry_exact0 = job.entry_exact[k] != 0;
        if (defer_min_bytes) {
            if (written >= defer_min_bytes) { rc = SX_RETRY_WHOLE; break; }
            sl.out_budget = defer_min_bytes - written;
        }
        MissionFindings mf;
        uint64_t e_now = 0;
        rc = device_replay_slab(ctx, k, view, sj, runs, sl, carry, &mf, &e_now, 0);
        e_prev = std::max(e_prev, e_now);
        if (rc == SX_OK) {
            out->replay_bytes += mf.replay_bytes; mf.replay_bytes = 0;
            written += mf.count() * sizeof(sx_finding) + mf.strings_len();
            if (mf.count()) got.push_back(std::move(mf));
        } else if (mf.ext.p) got.push_back(std::move(mf));
    }
    // On success neither stream is waited for here.  The last slab's copy runs on (slab_copy_drain).  So may the tail of its pass 2
    // on stream_b, while the caller queues the next Mission's stage A or device replay: that is in order only because every
    // Mission's stream_b is the one ctx->post_stream (sx_api.cpp) — what is queued next runs behind it —, and because d_cache and
    // d_scratch grow through hipFree, which waits for the device.  A Mission with a stream of its own would need the wait back.
    if (rc == SX_OK) {
        fold_slabs(out, got);
        if (end_pos) *end_pos = e_prev;
        return SX_OK;
    }
    (void)hipStreamSynchronize(ctx->merge_copy_stream);
    (void)hipStreamSynchronize(d.stream_b);
    ctx->slab_copy_pending = false;
    for (auto& g : got) if (g.ext.p) ctx->pool->give(g.ext);
    out->replay_bytes = 0;
    if (rc == SX_RETRY_WHOLE) { std::lock_guard<std::mutex> g(ctx->mu); ctx->stats.fast_regions = fast0; ctx->stats.general_regions = general0; }
    return rc;
}

int device_replay_mission(sx_ctx* ctx, size_t k, ByteView& view, const ReplayJob& job, const RunList& runs,
                          MissionFindings* out, uint64_t* end_pos, uint64_t defer_min_bytes) {
    const size_t n = runs.size();
    MissionDev& d = ctx->dev[k];
    if (wave_replay_wanted(ctx, job, k, n)) {   // string-dense: a lane per window instead of a lane per region (sx_wave.cpp)
        const int rc = wave_replay_mission(ctx, k, view, job, out, end_pos, defer_min_bytes);
        if (rc != SX_WAVE_FALLBACK) return rc;
        if (k < ctx->wave_off.size()) ctx->wave_off[k] = 1;
        if (k < ctx->wave_pred.size()) ctx->wave_pred[k] = 0;
    }
    if (runs.skipped) return SX_NEED_RUNS;
    std::vector<uint64_t> idx, his;
    int rc = cut_slabs(ctx, k, job, runs, slabs_wanted(ctx, k, job, runs, defer_min_bytes), &idx, &his);
    if (rc != SX_OK) return rc;
    if (idx.size() > 2) {
        rc = replay_in_slabs(ctx, k, view, job, runs, idx, his, out, end_pos, defer_min_bytes);
        if (rc == SX_OK) note_output(d, n, *out);
        if (rc != SX_RETRY_WHOLE) return rc;
    }
    Slab sl;
    sl.i1 = n;
    SlabCarry carry;
    rc = device_replay_slab(ctx, k, view, job, runs, sl, carry, out, end_pos, defer_min_bytes);
    if (rc == SX_OK) note_output(d, n, *out);
    return rc;
}

// A Mission whose decoder state cannot be derived from the bytes near a position (ISO-2022-JP): FindingCollection::from over every
// window of the buffer, in order, from the carried state — no stage A, no regions.  Device-resident input comes to the host in pieces.
static int host_sequential_mission(sx_ctx* ctx, size_t k, ByteView& bytes, const ReplayJob& job, MissionFindings* out) {
    const Mission& m = ctx->missions[k];
    ScannerState st = ctx->states[k];
    if (bytes.all_on_host() || !job.d_bytes) {
        replay_exact_windows(m, st, job.consumed0[k], job.stream0[k], bytes, job.len, job.file_id, 0, job.len, out, job.is_last);
    } else {
        struct Piece : ByteView {
            std::vector<uint8_t> buf; uint64_t base = 0;
            const uint8_t* span(uint64_t off, size_t, size_t*) override { return buf.data() + (off - base); }
        } piece;
        const uint64_t step = 64ull << 20;
        for (uint64_t at = 0; at < job.len; at += step) {
            const uint64_t n = std::min(step, job.len - at);
            piece.buf.resize(n); piece.base = at;
            HIP_TRY(ctx, hipMemcpy(piece.buf.data(), job.d_bytes + at, n, hipMemcpyDeviceToHost));
            replay_exact_windows(m, st, job.consumed0[k], job.stream0[k], piece, job.len, job.file_id, at, at + n, out, job.is_last);
        }
    }
    out->replay_bytes += job.len;
    if (job.slice_base) for (auto& f : out->v) f.slice_index += job.slice_base;
    if (job.commit_state) {
        st.consumed_bytes = job.consumed0[k] + job.len;
        st.stream_bytes = job.stream0[k] + job.len;
        ctx->states[k] = st;
    }
    return SX_OK;
}

// parts are speculative restarts: worth a thread each only if they hold real work
unsigned host_parts_wanted(const sx_ctx* ctx, size_t k, size_t n_runs) {
    if (ctx->missions[k].c.chars_min_nb == 0) return 1;  // no speculative restarts (see device_replay_wanted)
    return (unsigned)std::min<uint64_t>(replay_threads(ctx), std::max<uint64_t>(1, n_runs / 512));
}

// Stage B for all missions: every (mission, part) pair is one task for a small thread pool;
// part 0 of a mission starts from its entry state, the others speculate, and the per-mission
// stitch verifies/repairs them serially.
int replay_all(sx_ctx* ctx, ByteView& bytes, const ReplayJob& job, const std::vector<RunList>& runs,
               Result* into, uint64_t* end_pos, PreReplayed* pre) {
    const double t0 = now_ms();
    const size_t nm = ctx->missions.size();
    const unsigned nthreads = replay_threads(ctx);
    // (leaving early: no slab's copy may still be writing into a block that goes back to the pool)
    struct SlabDrain { sx_ctx* ctx; ~SlabDrain() { (void)slab_copy_drain(ctx); } } slab_drain{ ctx };
    std::vector<std::vector<uint64_t>> bounds(nm);
    std::vector<std::vector<ReplayPart>> parts(nm);
    std::vector<std::pair<size_t, size_t>> tasks;
    std::vector<char> on_device(nm, 0);
    uint64_t host_runs = 0;
    for (size_t k = 0; k < nm; k++)
        on_device[k] = (pre && pre->done[k]) ? 2 : ctx->missions[k].host_sequential() ? 3 : (device_replay_wanted(ctx, job, k, runs[k].size()) ? 1 : 0);
    for (size_t k = 0; k < nm; k++) {
        if (on_device[k]) continue;
        HIP_TRY(ctx, runs[k].wait());
        host_runs += runs[k].size();
        replay_plan_range(std::min(job.lo[k], job.hi), job.hi, host_parts_wanted(ctx, k, runs[k].size()), &bounds[k]);
        parts[k].resize(bounds[k].size() - 1);
        for (size_t p = 0; p + 1 < bounds[k].size(); p++) tasks.emplace_back(k, p);
    }
    std::atomic<size_t> next{ 0 };
    std::vector<double> task_ms(tasks.size(), 0.0);
    auto worker = [&]() {
        for (;;) {
            const size_t t = next.fetch_add(1);
            if (t >= tasks.size()) break;
            const size_t k = tasks[t].first, p = tasks[t].second;
            const double tt0 = now_ms();
            replay_part(ctx->missions[k], ctx->states[k], job.consumed0[k], job.stream0[k], bytes, job.len, job.file_id,
                        job.is_last, runs[k].data(), runs[k].size(), bounds[k][p], bounds[k][p + 1],
                        p == 0 && job.entry_exact[k], &parts[k][p]);
            task_ms[t] = now_ms() - tt0;
        }
    };
    const size_t nw = host_runs < 2048 ? 1 : std::min<size_t>(nthreads, tasks.size());
    if (nw <= 1) worker();
    else {
        std::vector<std::thread> th;
        for (size_t i = 0; i < nw; i++) th.emplace_back(worker);
        for (auto& t : th) t.join();
    }
    const double t_parts = now_ms();
    std::vector<MissionFindings> per(nm);
    std::vector<uint64_t> ends(nm, 0);
    for (size_t k = 0; k < nm; k++) {
        if (on_device[k] == 2) { per[k] = std::move(pre->per[k]); pre->per[k].ext = {}; ends[k] = pre->ends[k]; }
        else if (on_device[k] == 3) {
            int rc = host_sequential_mission(ctx, k, bytes, job, &per[k]);
            if (rc != SX_OK) return rc;
            ends[k] = job.len;
        } else if (on_device[k]) {
            int rc = device_replay_mission(ctx, k, bytes, job, runs[k], &per[k], &ends[k], 0);
            if (rc != SX_OK) return rc;
        }
    }
    auto stitch = [&](size_t k) {
        if (on_device[k]) return;
        ScannerState st = ctx->states[k];
        replay_stitch(ctx->missions[k], st, job.consumed0[k], job.stream0[k], bytes, job.len, job.file_id, job.is_last,
                      runs[k].data(), runs[k].size(), parts[k], &per[k], nthreads, &ends[k]);
        if (job.commit_state) ctx->states[k] = st;
        if (job.slice_base) for (auto& f : per[k].v) f.slice_index += job.slice_base;
    };
    if (nm == 1) stitch(0);
    else {
        std::vector<std::thread> th;
        for (size_t k = 0; k < nm; k++) th.emplace_back(stitch, k);
        for (auto& t : th) t.join();
    }
    if (end_pos) for (size_t k = 0; k < nm; k++) end_pos[k] = ends[k];
    const double t_stitch = now_ms();
    SX_TL("replay_all: host parts + stitch done");
    const size_t count_before = into->count();
    {   // from here on the findings are read: a Mission's last slab may still be on its way (device_replay_mission)
        int rc = slab_copy_drain(ctx);
        if (rc != SX_OK) return rc;
    }
    SX_TL("replay_all: slab copies done");
    {   // several missions with findings that are all still on the device: interleave them there
        // (a stable radix sort by position) instead of finding by finding on the host
        int rc = device_merge(ctx, job, per, into);
        if (rc != SX_OK) return rc;
    }
    SX_TL("replay_all: device_merge done");
    merge_findings(per, ctx->pool, into, ctx->sw.host_merge_seg_bytes);
    SX_TL("replay_all: merge_findings done");
    if (ctx->sw.timing) {
        double mx = 0, sum = 0;
        for (double v : task_ms) { sum += v; mx = std::max(mx, v); }
        fprintf(stderr, "[sx] replay: parts %.2f ms (%zu tasks, %zu workers; task sum %.1f max %.1f ms), stitch %.2f ms, merge %.2f ms, "
                        "on-demand fetches so far %llu\n", t_parts - t0, tasks.size(), nw, sum, mx, t_stitch - t_parts,
                now_ms() - t_stitch, (unsigned long long)ctx->ondemand_fetches);
    }
    for (auto& mf : per) ctx->stats.replay_bytes += mf.replay_bytes;
    ctx->stats.findings += into->count() - count_before;
    ctx->stats.replay_ms += now_ms() - t0;
    return SX_OK;
}

ReplayJob whole_chunk_job(sx_ctx* ctx, uint64_t len, int file_id, bool is_last) {
    ReplayJob j;
    const size_t nm = ctx->missions.size();
    j.len = len; j.file_id = file_id; j.is_last = is_last; j.hi = len;
    j.lo.assign(nm, 0); j.entry_exact.assign(nm, 1);
    for (size_t k = 0; k < nm; k++) { j.consumed0.push_back(ctx->states[k].consumed_bytes); j.stream0.push_back(ctx->states[k].stream_bytes); }
    return j;
}


// Downloads what the host part of stage B reads: the buffer's first and last 64 KiB ("base",
// entry and exit of every mission) and the replay ranges of the missions the host replays.
// runs == nullptr: the base only, copied into the view.  skip: missions not to plan for; if the
// plan then holds nothing beyond the base and `base_view` already has it, nothing is done and
// *used_base is set.
int download_for_replay(sx_ctx* ctx, const uint8_t* d_bytes, uint64_t len,
                               const std::vector<RunList>* runs_opt, SparseDeviceBytes* view,
                               const ReplayJob& job, const std::vector<char>* skip, bool* used_base) {
    const size_t nm = runs_opt ? ctx->missions.size() : 0;
    static const std::vector<RunList> no_runs;
    const std::vector<RunList>& runs = runs_opt ? *runs_opt : no_runs;
    if (used_base) *used_base = false;
    const double t0 = now_ms();
    std::vector<std::pair<uint64_t, uint64_t>> rg;
    // what the host always looks at: the chunk's first windows and its tail
    rg.emplace_back(0, std::min<uint64_t>(len, 64 * 1024));
    if (len > 64 * 1024) rg.emplace_back(len - 64 * 1024, len);
    for (size_t k = 0; k < nm; k++) {
        if ((skip && (*skip)[k]) || ctx->missions[k].host_sequential() || device_replay_wanted(ctx, job, k, runs[k].size())) continue;  // stage B of this mission runs on the device (or fetches its bytes itself)
        HIP_TRY(ctx, runs[k].wait());
        const size_t before = rg.size();
        replay_ranges(ctx->missions[k], ctx->states[k], len, runs[k].data(), runs[k].size(), host_parts_wanted(ctx, k, runs[k].size()), &rg);
        // a mission's ranges come out almost sorted (runs are); fix up, then merge the sorted lists
        if (!std::is_sorted(rg.begin() + before, rg.end())) std::sort(rg.begin() + before, rg.end());
        std::inplace_merge(rg.begin(), rg.begin() + before, rg.end());
    }
    const double t_rg = now_ms();
    std::vector<std::pair<uint64_t, uint64_t>> mg;
    mg.reserve(rg.size());
    for (auto& r : rg) {
        if (!mg.empty() && r.first <= mg.back().second) mg.back().second = std::max(mg.back().second, r.second);
        else mg.push_back(r);
    }
    if (used_base) {  // nothing beyond the base (already in the caller's view)?
        bool inside = true;
        for (auto& r : mg)
            inside = inside && (r.second <= std::min<uint64_t>(len, 64 * 1024) || (len > 64 * 1024 && r.first >= len - 64 * 1024));
        if (inside) { *used_base = true; return SX_OK; }
    }
    // split long ranges so that one gather wavefront never copies more than 64 KiB
    std::vector<uint64_t> seg_src, seg_dst;
    std::vector<uint32_t> seg_len;
    uint64_t total = 0;
    for (auto& r : mg)
        for (uint64_t a = r.first; a < r.second; a += 65536) {
            const uint64_t n = std::min<uint64_t>(65536, r.second - a);
            seg_src.push_back(a); seg_dst.push_back(total); seg_len.push_back((uint32_t)n);
            total += n;
        }
    const double t_seg = now_ms();
    if (total) {
        hipStream_t s = ctx->dev[0].stream_b;
        const size_t ns = seg_src.size();
        const uint64_t seg_bytes = ns * (8 + 8 + 4) + 64;
        int rc2 = ensure_pinned(ctx, total + 64);
        if (rc2 != SX_OK) return rc2;
        rc2 = ensure_scratch(ctx, total + seg_bytes + 256);
        if (rc2 != SX_OK) return rc2;
        uint8_t* d_out = ctx->d_scratch;
        uint64_t* d_src = (uint64_t*)(ctx->d_scratch + plan::up256(total));
        uint64_t* d_dst = d_src + ns;
        uint32_t* d_len = (uint32_t*)(d_dst + ns);
        HIP_TRY(ctx, hipMemcpyAsync(d_src, seg_src.data(), ns * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_dst, seg_dst.data(), ns * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_len, seg_len.data(), ns * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, launch_gather(d_bytes, d_out, d_src, d_dst, d_len, (uint32_t)ns, s));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pin, d_out, total, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        uint64_t off = 0;
        for (auto& r : mg) {
            if (runs_opt) view->add(r.first, r.second, ctx->h_pin + off);
            else view->add_copy(r.first, r.second, ctx->h_pin + off);
            off += r.second - r.first;
        }
    }
    ctx->stats.d2h_ms += now_ms() - t0;
    if (ctx->sw.timing)
        fprintf(stderr, "[sx] sparse download: ranges %.2f ms, sort+merge+segments %.2f ms (%zu ranges, %zu segs), gather+d2h %.2f ms (%.1f MB)\n",
                t_rg - t0, t_seg - t_rg, mg.size(), seg_src.size(), now_ms() - t_seg, total / 1e6);
    return SX_OK;
}

}  // namespace sx
