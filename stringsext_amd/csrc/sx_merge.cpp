// sx_merge.cpp — the merger (src/main.rs:118-136) on the device, its host driver: device_merge plans the parts (merge_plan; the
// arithmetic is sx_stage_b_plan.hpp's), then emits them (emit_kept, emit_to_host).
#include "sx_ctx.hpp"

using namespace sx;

namespace sx {

// A block of the context's that is replaced, not kept, when it is too small.  SX_E_NOMEM without an error text: no memory — the
// block is gone and the result goes to the host.
static int regrow_quietly(sx_ctx* ctx, uint8_t** p, uint64_t* cap, uint64_t need) {
    if (*p) HIP_TRY(ctx, hipFree(*p));
    *p = nullptr; *cap = 0;
    if (hipMalloc((void**)p, need) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return SX_E_NOMEM; }
    *cap = need;
    return SX_OK;
}

// A mission's findings that were left on the device (dev_only) come to the host after all.
static int fetch_deferred(sx_ctx* ctx, MissionFindings& mf) {
    if (!mf.dev_only) return SX_OK;
    const size_t bytes = mf.ext_nf * sizeof(sx_finding) + mf.ext_na;
    PinnedPool::Block blk = ctx->pool->take(bytes + 64);
    if (!blk.p) { ctx->err = "hipHostMalloc failed"; return SX_E_NOMEM; }
    HIP_TRY(ctx, hipMemcpyAsync(blk.p, mf.dev_copy, bytes, hipMemcpyDeviceToHost, ctx->post_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->post_stream));
    mf.ext = blk; mf.dev_only = false;
    return SX_OK;
}

// SX_OPT_RESULT_ON_DEVICE with several Missions: does this call's merged result stay in HBM?  (What only shows later — no findings,
// Missions that count from different origins, no memory for the block — is device_merge's to see.)
bool result_stays_on_device(const sx_ctx* ctx, const ReplayJob& job) {
    return (ctx->opt.flags & SX_OPT_RESULT_ON_DEVICE) && ctx->missions.size() >= 2 && merge_part_can_pack(1, (int)ctx->missions.size()) && !ctx->host_only &&
           job.d_bytes && job.commit_state && !ctx->sharded_call && ctx->single_piece && !ctx->sw.host_merge;
}

// ... then a Mission's list that exists on the host only (few runs: the host replayed it; ISO-2022-JP's sequential pass; regions the device
// gave back) joins the merge as a device list: [records][strings] of all such lists through one pinned block, one copy, into memory of
// the context's.  SX_E_NOMEM without an error text: no memory for it, the result goes to the host.
static int upload_host_lists(sx_ctx* ctx, std::vector<MissionFindings>& per, std::vector<char>& uploaded) {
    uint64_t need = 0;
    for (auto& mf : per) {
        if (!mf.count() || mf.dev_copy) continue;
        if (!mf.more.empty() || mf.packed) return SX_E_NOMEM;   // (a single Mission's forms)
        need += plan::up256(mf.count() * sizeof(sx_finding) + mf.strings_len());
    }
    if (!need) return SX_OK;
    if (ctx->d_result_up_cap < need) { const int rc = regrow_quietly(ctx, &ctx->d_result_up, &ctx->d_result_up_cap, need); if (rc != SX_OK) return rc; }
    PinnedPool::Block blk = ctx->pool->take(need);
    if (!blk.p) return SX_E_NOMEM;
    uint64_t at = 0;
    for (size_t k = 0; k < per.size(); k++) {
        MissionFindings& mf = per[k];
        if (!mf.count() || mf.dev_copy) continue;
        const uint64_t fb = mf.count() * sizeof(sx_finding);
        memcpy((uint8_t*)blk.p + at, mf.data(), fb);
        memcpy((uint8_t*)blk.p + at + fb, mf.strings(), mf.strings_len());
        mf.dev_copy = ctx->d_result_up + at; uploaded[k] = 1;
        at += plan::up256(fb + mf.strings_len());
    }
    hipError_t e = hipMemcpyAsync(ctx->d_result_up, blk.p, need, hipMemcpyHostToDevice, ctx->post_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->post_stream);
    ctx->pool->give(blk);
    if (e != hipSuccess) {
        for (size_t k = 0; k < per.size(); k++) if (uploaded[k]) { per[k].dev_copy = nullptr; uploaded[k] = 0; }
        HIP_TRY(ctx, e);
    }
    return SX_OK;
}

int merge_drain(sx_ctx* ctx) {
    std::lock_guard<std::recursive_mutex> g(ctx->grow_mu);   // (a wave Mission's thread may get here through ensure_rp)
    if (ctx->post_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->post_stream));
    if (ctx->merge_copy_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->merge_copy_stream));
    ctx->merge_copy_pending[0] = ctx->merge_copy_pending[1] = false;
    ctx->slab_copy_pending = false;
    ctx->interleave_pending = false;
    return SX_OK;
}

// What device_merge decided before it writes anything: K parts cut at slice boundaries, per Mission the K + 1 finding indices and
// string offsets, each part's size over all Missions.
struct MergePlan {
    uint64_t K = 1;
    std::vector<std::vector<uint64_t>> idx, off;
    std::vector<plan::PartSize> parts;
    bool gave_up = false;   // no K fits: the host merges
    uint64_t max_out = 0, max_n = 0;   // the largest part: bytes as 32-byte records + strings, findings
};

// str_off has 32 bits and the place table 32-bit indices: from the first K (the switches' part sizes) the cuts are looked up on the
// device and K is doubled until every part fits — eight times at most, and no finer than a slice per part.
static int merge_plan(sx_ctx* ctx, const ReplayJob& job, const std::vector<MissionFindings>& per, uint64_t total, uint64_t bytes, MergePlan* mp) {
    const size_t nm = per.size();
    const plan::MergeLimits lim = plan::merge_limits(ctx->sw.merge_part_mib, ctx->sw.merge_part_findings);
    uint64_t K = plan::merge_first_k(bytes, total, lim);
    hipStream_t s = ctx->post_stream;
    const uint64_t n_slices = (job.len + kInputBufLen - 1) / kInputBufLen;
    std::vector<std::vector<uint64_t>>& idx = mp->idx;
    std::vector<std::vector<uint64_t>>& off = mp->off;
    idx.assign(nm, {}); off.assign(nm, {});
    for (int attempt = 0;; attempt++) {
        K = plan::merge_clamp_k(K, n_slices);
        for (size_t k = 0; k < nm; k++) { idx[k].assign(K + 1, 0); off[k].assign(K + 1, 0); idx[k][K] = per[k].count(); off[k][K] = per[k].strings_len(); }
        if (K > 1) {
            std::vector<uint64_t> cuts(K - 1);
            for (uint64_t j = 1; j < K; j++) cuts[j - 1] = job.consumed0[0] + (n_slices * j / K) * kInputBufLen;
            const size_t row = (K - 1) * 8;
            int rc = ensure_scratch(ctx, row * (1 + 2 * nm) + 256);
            if (rc != SX_OK) return rc;
            rc = ensure_pinned2(ctx, row * 2 * nm + 256);
            if (rc != SX_OK) return rc;
            uint64_t* d_cuts = (uint64_t*)ctx->d_scratch;
            HIP_TRY(ctx, hipMemcpyAsync(d_cuts, cuts.data(), row, hipMemcpyHostToDevice, s));
            for (size_t k = 0; k < nm; k++)
                if (per[k].count())
                    HIP_TRY(ctx, launch_merge_cuts((const sx_finding*)per[k].dev_copy, per[k].count(), per[k].strings_len(), d_cuts,
                                                   (uint32_t)(K - 1), d_cuts + (K - 1) * (1 + 2 * k), d_cuts + (K - 1) * (2 + 2 * k), s));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pin2, d_cuts + (K - 1), row * 2 * nm, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            const uint64_t* h = (const uint64_t*)ctx->h_pin2;
            for (size_t k = 0; k < nm; k++)
                if (per[k].count())
                    for (uint64_t j = 1; j < K; j++) { idx[k][j] = h[(K - 1) * 2 * k + (j - 1)]; off[k][j] = h[(K - 1) * (2 * k + 1) + (j - 1)]; }
                else
                    for (uint64_t j = 1; j < K; j++) { idx[k][j] = 0; off[k][j] = 0; }
        }
        plan::merge_part_sizes(idx, off, K, &mp->parts);
        if (plan::merge_parts_fit(mp->parts, lim.part_findings, K, n_slices)) break;
        if (attempt >= 8 || K >= n_slices) { mp->gave_up = true; return SX_OK; }   // (one slice alone with more than 4 GiB of strings cannot be)
        K *= 2;
    }
    mp->K = K;
    for (const plan::PartSize& p : mp->parts) { mp->max_out = std::max(mp->max_out, p.pf * sizeof(sx_finding) + p.pb); mp->max_n = std::max(mp->max_n, p.pf); }
    return SX_OK;
}

// part j of every Mission's list, as merge_findings_device_part takes them
struct PartSources {
    std::vector<const sx_finding*> fp;
    std::vector<const uint8_t*> ap;
    std::vector<uint64_t> pnf, pnb;
    std::vector<uint32_t> off0;
    explicit PartSources(size_t nm) : fp(nm), ap(nm), pnf(nm), pnb(nm), off0(nm) {}
    void of(const std::vector<MissionFindings>& per, const MergePlan& mp, uint64_t j) {
        for (size_t k = 0; k < per.size(); k++) {
            const sx_finding* f0 = (const sx_finding*)per[k].dev_copy;
            const uint8_t* a0 = (const uint8_t*)per[k].dev_copy + per[k].count() * sizeof(sx_finding);
            fp[k] = f0 ? f0 + mp.idx[k][j] : nullptr; ap[k] = f0 ? a0 + mp.off[k][j] : nullptr;
            pnf[k] = mp.idx[k][j + 1] - mp.idx[k][j]; pnb[k] = mp.off[k][j + 1] - mp.off[k][j]; off0[k] = (uint32_t)mp.off[k][j];
        }
    }
};

// SX_OPT_RESULT_ON_DEVICE: room for every part's [records][strings], 256-byte aligned, in the context's result block; the merger's
// scratch is the context's.  *keep = false: a part the one-pass merger does not take (the radix sort's arena is grouped by Mission),
// or no memory — to the host as ever.
static int reserve_kept(sx_ctx* ctx, const MergePlan& mp, size_t nm, bool pack, bool* keep) {
    uint64_t need = 0;
    for (const plan::PartSize& p : mp.parts) {
        if (!*keep) break;
        if (!p.pf) continue;
        *keep = merge_part_can_pack(p.pf, (int)nm);
        need += plan::merge_part_room(p.pf, pack ? sizeof(sx_finding16) : sizeof(sx_finding), p.pb);
    }
    if (*keep) { const int rc = ensure_scratch(ctx, merge_findings_scratch_bytes(mp.max_n, (int)nm, 1) + 512); if (rc != SX_OK) return rc; }
    if (*keep && ctx->d_result_cap < need) {   // (what it held went with the epoch)
        const int rc = regrow_quietly(ctx, &ctx->d_result, &ctx->d_result_cap, need);
        if (rc == SX_E_NOMEM) *keep = false;   // no room: the host result
        else if (rc != SX_OK) return rc;
    }
    return SX_OK;
}

// the parts one behind the other in the result block; each becomes a segment the caller reads through sx_result_segment_device
static int emit_kept(sx_ctx* ctx, const std::vector<MissionFindings>& per, const MergePlan& mp, bool pack, const std::shared_ptr<SegInfo>& seg_info,
                     std::vector<MissionFindings>* outs) {
    const size_t nm = per.size();
    hipStream_t s = ctx->post_stream;
    PartSources src(nm);
    uint64_t result_at = 0;
    for (uint64_t j = 0; j < mp.K; j++) {
        const plan::PartSize& p = mp.parts[j];
        if (!p.pf) continue;
        src.of(per, mp, j);
        uint8_t* d_part = ctx->d_result + result_at;   // (merge_part_can_pack: checked by reserve_kept)
        HIP_TRY(ctx, merge_findings_device_part(src.fp.data(), src.ap.data(), src.pnf.data(), src.pnb.data(), src.off0.data(), (int)nm, d_part, ctx->d_scratch, ctx->d_scratch_cap, s, pack ? 1 : 0, 1));
        result_at += plan::merge_part_room(p.pf, pack ? sizeof(sx_finding16) : sizeof(sx_finding), p.pb);
        outs->emplace_back();
        MissionFindings& o = outs->back();
        keep_on_device(o, ctx);
        o.ext_nf = p.pf; o.ext_na = p.pb; o.dev_copy = d_part;
        if (pack) { o.packed = true; o.info = seg_info; }
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));   // (the pointers may be read from any stream once the call returns)
    return SX_OK;
}

// device_merge's own memory: n_out output buffers of out_room bytes, then the sort's scratch
static int reserve_merge_buffers(sx_ctx* ctx, const MergePlan& mp, size_t nm) {
    const size_t out_room = plan::up256(mp.max_out + 256);
    const size_t n_out = (mp.K > 1 || ctx->merge_async) ? 2 : 1;
    const size_t tmp_need = merge_findings_scratch_bytes(mp.max_n, (int)nm) + 512;
    if (!(ctx->merge_out_room < out_room || ctx->merge_n_out < n_out || ctx->d_merge_cap < ctx->merge_n_out * ctx->merge_out_room + tmp_need)) return SX_OK;
    // (the copy of an earlier call's last part may still read the buffers that are about to go)
    int rc = merge_drain(ctx);
    if (rc != SX_OK) return rc;
    if (ctx->d_merge) HIP_TRY(ctx, hipFree(ctx->d_merge));
    ctx->d_merge = nullptr; ctx->d_merge_cap = 0; ctx->merge_out_room = 0; ctx->merge_n_out = 0;
    // pieces of one buffer are alike but not equal: a quarter more than this one needs
    const size_t room = ctx->merge_async ? plan::up256(out_room + out_room / 4 + 256) : out_room;
    const size_t tmp = ctx->merge_async ? tmp_need + tmp_need / 4 : tmp_need;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_merge, n_out * room + tmp));
    ctx->d_merge_cap = n_out * room + tmp; ctx->merge_out_room = room; ctx->merge_n_out = n_out;
    return SX_OK;
}

// the parts through the two output buffers in turn: the copy of one (on merge_copy_stream) runs while the next is sorted
static int emit_to_host(sx_ctx* ctx, const std::vector<MissionFindings>& per, const MergePlan& mp, bool pack, const std::shared_ptr<SegInfo>& seg_info,
                        std::vector<MissionFindings>* outs) {
    const size_t nm = per.size();
    hipStream_t s = ctx->post_stream, cs = ctx->merge_copy_stream;
    uint8_t* d_tmp = ctx->d_merge + ctx->merge_n_out * ctx->merge_out_room;
    const size_t tmp_bytes = ctx->d_merge_cap - ctx->merge_n_out * ctx->merge_out_room;
    hipEvent_t ev_sorted = ctx->merge_ev[0], ev_copied[2] = { ctx->merge_ev[1], ctx->merge_ev[2] };
    PartSources src(nm);
    for (uint64_t j = 0; j < mp.K; j++) {
        const plan::PartSize& p = mp.parts[j];
        if (!p.pf) continue;
        src.of(per, mp, j);
        const unsigned ob = ctx->merge_n_out == 2 ? (unsigned)(ctx->merge_parts & 1) : 0u;   // (parts of all calls in turn: merge_async)
        ctx->merge_parts++;
        uint8_t* d_out = ctx->d_merge + ob * ctx->merge_out_room;
        if (ctx->merge_copy_pending[ob]) HIP_TRY(ctx, hipStreamWaitEvent(s, ev_copied[ob], 0));   // the buffer is free again
        const bool pack_part = pack && merge_part_can_pack(p.pf, (int)nm);
        HIP_TRY(ctx, merge_findings_device_part(src.fp.data(), src.ap.data(), src.pnf.data(), src.pnb.data(), src.off0.data(), (int)nm, d_out, d_tmp, tmp_bytes, s, pack_part ? 1 : 0));
        HIP_TRY(ctx, hipEventRecord(ev_sorted, s));
        const size_t out_bytes = p.pf * (pack_part ? sizeof(sx_finding16) : sizeof(sx_finding)) + p.pb;
        PinnedPool::Block blk = ctx->pool->take(out_bytes + 64);
        if (!blk.p) { ctx->err = "hipHostMalloc failed"; return SX_E_NOMEM; }
        HIP_TRY(ctx, hipStreamWaitEvent(cs, ev_sorted, 0));
        {
            // Next to the kernels of the following piece (merge_async) the copy is a kernel of two workgroups, each writing one
            // contiguous half into the pinned block: measured on the MI355X (BASELINE config 5, 2.3 GB per piece), hipMemcpyAsync
            // — a blit kernel that fills the chip with wavefronts waiting on PCIe — delays every kernel next to it until it is done
            // (a 6 ms scan takes 45), eight workgroups slow the count passes by half, one does not fill the link; two copy at
            // ~45 GB/s and cost the count passes 8 %.  With nothing next to it the runtime's copy is the faster one (53 GB/s).
            const int copy_wgs = ctx->sw.merge_copy_wgs >= 0 ? ctx->sw.merge_copy_wgs : (ctx->merge_async ? 2 : 0);
            if (copy_wgs > 0) HIP_TRY(ctx, launch_copy_bytes(blk.p, d_out, out_bytes, (uint32_t)copy_wgs, cs, ctx->sw.merge_copy_threads, ctx->sw.merge_copy_nt != 0));
            else HIP_TRY(ctx, hipMemcpyAsync(blk.p, d_out, out_bytes, hipMemcpyDeviceToHost, cs));
        }
        HIP_TRY(ctx, hipEventRecord(ev_copied[ob], cs));
        ctx->merge_copy_pending[ob] = true;
        ctx->merged_out_bytes += out_bytes;
        outs->emplace_back();
        outs->back().ext = blk; outs->back().ext_nf = p.pf; outs->back().ext_na = p.pb;
        if (pack_part) { outs->back().packed = true; outs->back().info = seg_info; }
    }
    return SX_OK;
}

// The missions' findings, each ordered by position and still in HBM, are interleaved there (sx_sort.hip: every finding's place follows
// from short searches in the other missions' lists) and arrive on the host as they will be printed.  A large output is cut at slice
// boundaries into parts (each at most SX_MERGE_PART_MIB of strings and SX_MERGE_PART_FINDINGS findings) that become one segment of
// the result each; the copy of part j runs while part j+1 is interleaved.  If the conditions do not hold the host merges (merge_findings).
// SX_OPT_RESULT_ON_DEVICE (result_stays_on_device): the parts are written one behind the other, each 256-byte aligned, into the context's
// result block and stay there — no pinned block, no copy.  Their strings lie back to back in record order (merge_findings_device_part's
// `ordered`).  Small results and a single Mission with findings among several take this way too, lists on the host are uploaded
// first; all segments of a result are on the device or none is.
int device_merge(sx_ctx* ctx, const ReplayJob& job, std::vector<MissionFindings>& per, Result* into) {
    const size_t nm = per.size();
    size_t with = 0, on_dev = 0, deferred = 0;
    uint64_t total = 0, bytes = 0;
    bool same_origin = true;
    for (size_t k = 0; k < nm; k++) {
        if (!per[k].count()) continue;
        with++;
        if ((per[k].ext.p || per[k].dev_only) && per[k].dev_copy) on_dev++;
        if (per[k].dev_only) deferred++;
        total += per[k].count(); bytes += per[k].strings_len();
        same_origin = same_origin && job.consumed0[k] == job.consumed0[0];
    }
    std::vector<char> uploaded(nm, 0);
    auto give_up = [&]() -> int {
        for (size_t k = 0; k < nm; k++) if (uploaded[k]) { per[k].dev_copy = nullptr; uploaded[k] = 0; }   // (the host's copy is the list again)
        for (auto& mf : per) { if (mf.keep_on_device) continue; int rc = fetch_deferred(ctx, mf); if (rc != SX_OK) return rc; }   // (SX_OPT_RESULT_ON_DEVICE: it stays)
        return SX_OK;
    };
    bool keep = result_stays_on_device(ctx, job) && total > 0 && same_origin;
    if (keep && on_dev != with) {
        const int rc = upload_host_lists(ctx, per, uploaded);
        if (rc == SX_E_NOMEM) keep = false;
        else if (rc != SX_OK) return rc;
        else on_dev = with;
    }
    // (the way to the host: worth it for two lists or more of some size, all of them still in HBM)
    auto host_way_ok = [&]() { return with >= 2 && on_dev == with && same_origin && total >= 4096 && !ctx->sw.host_merge; };
    if (!keep && !host_way_ok()) return give_up();
    const double tm0 = now_ms();
    // The records cross PCIe as sx_finding16 (include/stringsext_amd.h): half the bytes of what bounds this path.  Not with lines of
    // more than 16 000 chars (str_len has 16 bits there), nor where the one-pass merger does not apply (SX_PACKED=0: tests).
    bool pack = ctx->sw.packed;
    for (size_t k = 0; k < nm; k++) pack = pack && ctx->missions[k].q <= 16000;
    std::shared_ptr<SegInfo> seg_info;
    if (pack) seg_info = make_seg_info(ctx, job, 0, nm);
    MergePlan mp;
    { const int rc = merge_plan(ctx, job, per, total, bytes, &mp); if (rc != SX_OK) return rc; }
    if (mp.gave_up) return give_up();
    if (keep) {
        const int rc = reserve_kept(ctx, mp, nm, pack, &keep);
        if (rc != SX_OK) return rc;
        if (!keep && !host_way_ok()) return give_up();
    }
    { int rc = ensure_copy_stream(ctx); if (rc != SX_OK) return rc; }
    if (!keep) { const int rc = reserve_merge_buffers(ctx, mp, nm); if (rc != SX_OK) return rc; }
    std::vector<MissionFindings> outs;
    // leaving early (a HIP error, no pinned memory): no copy may still be writing into a block that goes back to the pool
    struct Guard {
        sx_ctx* ctx; std::vector<MissionFindings>* outs; bool done = false;
        ~Guard() {
            if (done) return;
            (void)merge_drain(ctx);
            for (auto& o : *outs) if (o.ext.p) ctx->pool->give(o.ext);
            outs->clear();
        }
    } guard{ ctx, &outs };
    uint64_t rb = 0;
    for (size_t k = 0; k < nm; k++) rb += per[k].replay_bytes;
    { const int rc = keep ? emit_kept(ctx, per, mp, pack, seg_info, &outs) : emit_to_host(ctx, per, mp, pack, seg_info, &outs); if (rc != SX_OK) return rc; }
    if (ctx->merge_async) {   // a Mission whose stage B writes on a stream of its own waits for this before it overwrites its findings
        if (!ctx->ev_interleaved) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_interleaved, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_interleaved, ctx->post_stream));
        ctx->interleave_pending = true;
    }
    // (merge_async: the last copies run on while the caller scans the next piece of the buffer; the sorts are in order with
    // everything else stage B does — post_stream —, so the missions' findings and the scratch may be reused at once)
    if (!ctx->merge_async) { int rc = merge_drain(ctx); if (rc != SX_OK) return rc; }
    guard.done = true;
    for (size_t k = 0; k < nm; k++) {
        if (per[k].ext.p) ctx->pool->give(per[k].ext);
        per[k] = MissionFindings{};
    }
    if (!outs.empty()) outs[0].replay_bytes = rb; else per[0].replay_bytes = rb;
    into->pool = ctx->pool;
    for (auto& o : outs) { ctx->stats.replay_bytes += o.replay_bytes; into->segs.push_back(std::move(o)); o.ext = {}; }
    if (ctx->sw.timing)
        fprintf(stderr, "[sx] device merge of %zu missions (%zu held back on the device): %llu findings, %llu parts, %.2f ms\n", with, deferred,
                (unsigned long long)total, (unsigned long long)mp.K, now_ms() - tm0);
    return SX_OK;
}

}  // namespace sx
