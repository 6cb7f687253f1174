// sx_result_api.cpp — the C-ABI of include/stringsext_amd.h for a result that stays in HBM (SX_OPT_RESULT_ON_DEVICE): the print, the
// selections, the extraction, the Unicode case fold, the decoding of encoded strings, what the strings look like, the tally, the labels and their rebinding, the approximate match, the duplicate strings and the seen set — with its merge, growth, blob and string
// lists, and its counts —, and the compiled sets they take.  What the operations share is here once — the view of a segment, a set's upload, a
// handle's device and memory, the counters' reset, a buffer that grows, a result's labels, the two passes of whatever writes a new
// result, the mark and add passes of whatever goes into a seen set —; what tells them apart is in their lane functions
// (sx_*_core.hpp) and kernels (sx_*_dev.hip).
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
#include "sx_distinct_core.hpp"
#include "sx_order_core.hpp"
#include "sx_fold_core.hpp"
#include "sx_decode_core.hpp"
#include "sx_measure_core.hpp"
#include "sx_fuzzy_build.hpp"
#include "sx_fuzzy_core.hpp"
#include "sx_seen_core.hpp"
#include "sx_seen_merge_core.hpp"
#include "sx_seen_count_core.hpp"
#include "sx_seen_blob.hpp"

using namespace sx;

// What every handle of this file has: device memory of its own, `mem`, on `device`
struct sx_device_handle {
    int device = 0;
    uint8_t* mem = nullptr;
};

// sx_select_set_create: a compiled keyword list; `mem` = [the class map][the table]
struct sx_select_set : sx_device_handle {
    SelsetDevice dev{};
    sx_select_set_info info{};
};

// sx_select_regex_create: compiled regular expressions; `mem` as a set's
struct sx_select_regex : sx_device_handle {
    SelreDevice dev{};
    sx_select_regex_info info{};
};

// sx_extract_regex_create: regular expressions compiled for the extraction; `mem` as a set's
struct sx_extract_regex : sx_device_handle {
    ExtractDevice dev{};
    sx_extract_regex_info info{};
};

// sx_tally_set_create: a keyword list compiled for the tally; `mem` = [the class map][the table][own][dict][pattern -> unique id]
// [hits][first]
struct sx_tally_set : sx_device_handle {
    SeltallyDevice dev{};
    const uint32_t* d_unique_of_pattern = nullptr;
    std::vector<uint32_t> unique_of_pattern;
    sx_tally_set_info info{};
};

// sx_label_set_create: regular expressions compiled for the labels; `mem` = [the class map][the table][here][end][findings][first]
struct sx_label_set : sx_device_handle {
    LabelDevice dev{};
    sx_label_set_info info{};
};

// sx_fuzzy_set_create: keywords with error budgets compiled for the approximate match; `mem` = [the class map][the masks][len and k]
// [findings][first]
struct sx_fuzzy_set : sx_device_handle {
    FuzzyDevice dev{};
    sx_fuzzy_set_info info{};
};

// sx_result_label_device: one result's labels; `mem` = an array per source segment, each 256-byte aligned.
// Per segment what tells the source apart: where its records lie, how many they are, and the epoch of its block when it was labelled.
struct sx_labels : sx_device_handle {
    struct Seg {
        const uint64_t* d = nullptr;
        const void* recs = nullptr;
        uint64_t n = 0;
        std::shared_ptr<std::atomic<uint64_t>> epoch_ref;
        uint64_t epoch = 0;
    };
    std::vector<Seg> segs;
};

// sx_seen_set_create: strings remembered from result to result; `mem` = [the cursors and a call's totals: kSeenHeadBytes][the slots]
// [the entries][a counted set's count words], each 256-byte aligned.  info's strings and bytes are not kept here: the cursors say
struct sx_seen_set : sx_device_handle {
    SeenSet dev{};
    sx_seen_set_info info{};
};

namespace {

constexpr uint64_t kSeenHeadBytes = 256, kSeenMaxCapacity = (uint64_t)1 << 40;

// A segment where it lies in HBM: what every kernel's parameters begin with
struct SegRef {
    const void* recs;
    const uint8_t* arena;
    uint64_t n;
    uint32_t packed;
};
SegRef seg_ref(const MissionFindings& s) {
    return SegRef{ s.dev_copy, (const uint8_t*)s.dev_copy + s.ext_nf * s.rec_size(), s.ext_nf, s.packed ? 1u : 0u };
}
// (P: PrintParams, SelectParams, ExtractParams, SeltallyParams, LabelParams)
template <class P>
P params_of(const SegRef& v) {
    P p;
    memset(&p, 0, sizeof p);
    p.recs = v.recs; p.arena = v.arena; p.n = v.n; p.packed = v.packed;
    return p;
}

bool host_only(sx_ctx* ctx, const char* no_device_what) {
    if (ctx->host_only) ctx->set_err(std::string("host-only context: no device ") + no_device_what);
    return ctx->host_only;
}
// (what_lies: "the pattern set lies", "the labels lie")
bool on_another_device(sx_ctx* ctx, const sx_device_handle& h, const char* what_lies) {
    if (h.device != ctx->device) ctx->set_err(std::string(what_lies) + " on another device");
    return h.device != ctx->device;
}
template <class H>
void handle_free(H* h) {
    if (!h) return;
    (void)hipFree(h->mem);
    delete h;
}
template <class H, class Info>
int handle_info(const H* h, Info* out) {
    if (!h || !out) return SX_E_INVALID;
    *out = h->info;
    return SX_OK;
}

// One piece of a set's device memory: `bytes` from `src`, in a place of `bytes` rounded up to a multiple of `round`
struct SetPiece {
    const void* src;
    size_t bytes, round;
};
// A compiled set's memory on the context's device: the pieces one behind the other, then `counter_bytes` of counters (not written).
// at[i]: the offset of piece i, at[n_pieces]: the counters'.  kind: the set's name in the messages.
int upload_set(sx_ctx* ctx, const char* kind, const std::vector<SetPiece>& pieces, size_t counter_bytes, uint8_t** mem, size_t* at) {
    if (host_only(ctx, (std::string("for the ") + kind).c_str())) return SX_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t bytes = 0;
    for (size_t i = 0; i < pieces.size(); i++) { at[i] = bytes; bytes += (pieces[i].bytes + pieces[i].round - 1) / pieces[i].round * pieces[i].round; }
    at[pieces.size()] = bytes;
    bytes += counter_bytes;
    if (hipMalloc((void**)mem, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *mem = nullptr;
        ctx->set_err(std::string(kind) + ": no device memory for " + std::to_string(bytes) + " bytes of " + (counter_bytes ? "tables and counters" : "table"));
        return SX_E_NOMEM;
    }
    hipError_t e = hipSuccess;
    for (size_t i = 0; e == hipSuccess && i < pieces.size(); i++)
        if (pieces[i].bytes) e = hipMemcpy(*mem + at[i], pieces[i].src, pieces[i].bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(*mem); *mem = nullptr; ctx->set_err(std::string("hipMemcpy: ") + hipGetErrorString(e)); return SX_E_HIP; }
    return SX_OK;
}
// (the handle of an uploaded set; NULL: no host memory, and `mem` is freed)
template <class H>
H* new_handle(const sx_ctx* ctx, uint8_t* mem) {
    H* h = new (std::nothrow) H;
    if (!h) { (void)hipFree(mem); return nullptr; }
    h->device = ctx->device; h->mem = mem;
    return h;
}

// A set's two counter arrays of n words as they are before the first call: `zeros` 0, `never` all ones (SX_TALLY_NEVER, SX_LABEL_NEVER)
int reset_counters(int device, uint64_t* zeros, uint64_t* never, size_t n) {
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    hipError_t e = hipMemset(zeros, 0, n * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemset(never, 0xFF, n * sizeof(uint64_t));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (a device memset may return before it is done, and the kernels run on a stream that does not wait for this one)
    if (e != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    return SX_OK;
}
// n words of a set's counters to the host (out: NULL = not asked for)
int read_counters(int device, const uint64_t* d, uint64_t* out, size_t n) {
    if (!out) return SX_OK;
    if (hipSetDevice(device) != hipSuccess || hipMemcpy(out, d, n * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    return SX_OK;
}

// What the device operations ask of a result: every segment in HBM, in memory of this context — the result block of the last scan call
// or one of the two selection blocks — that has not been written again since.
int result_on_device(sx_ctx* ctx, const sx_result* r, const char* host_call) {
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

// A grow-only device buffer of the context holds `bytes`.  false: the allocation failed and the buffer is empty; the caller says so in
// its own words
bool device_room(uint8_t** p, uint64_t* cap, uint64_t bytes) {
    if (bytes <= *cap) return true;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc((void**)p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
    *cap = bytes;
    return true;
}
// (a buffer of the selection)
int grow_device(sx_ctx* ctx, uint8_t** p, uint64_t* cap, uint64_t bytes, const char* what) {
    if (device_room(p, cap, bytes)) return SX_OK;
    ctx->set_err(std::string("device select: no memory for ") + std::to_string(bytes) + " bytes of " + what);
    return SX_E_NOMEM;
}

// The labels of a result whose segments lie in HBM: the handle, an array of a word per record for every segment — each 256-byte aligned
// in ONE allocation of *bytes bytes, not written here — and per segment what tells the source apart.  NULL: no memory for them
sx_labels* labels_of(const sx_ctx* ctx, const sx_result* r, uint64_t* bytes) {
    *bytes = 0;
    for (const MissionFindings& s : r->r.segs) *bytes += up256(s.ext_nf * sizeof(uint64_t));
    uint8_t* mem = nullptr;
    if (hipMalloc((void**)&mem, *bytes ? *bytes : 256) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    sx_labels* lab = new_handle<sx_labels>(ctx, mem);
    uint64_t at = 0;
    for (size_t i = 0; lab && i < r->r.segs.size(); i++) {
        const MissionFindings& s = r->r.segs[i];
        sx_labels::Seg seg;
        seg.d = (const uint64_t*)(mem + at); seg.recs = s.dev_copy; seg.n = s.ext_nf; seg.epoch_ref = s.dev_epoch_ref; seg.epoch = s.dev_epoch;
        lab->segs.push_back(seg);
        at += up256(s.ext_nf * sizeof(uint64_t));
    }
    return lab;
}

// The words of a compiled set where the findings lie — the labels (sx_label_dev.hip), the approximate matches (sx_fuzzy_dev.hip) —: the
// source is checked as a whole, the words' memory is had, then one kernel per segment, each with the ordinal of its first record, on
// the selections' stream, and one wait.  Only the words and the set's counters are written.  what: the call's nouns for the messages —
// { no device ..., ... on another device, ... on the host, device ...: , bytes of ... }; launch: P (Params) with the segment, the
// ordinal, the words' place and the set's tables
struct SetWordsWhat { const char *no_device, *set_lies, *host_call, *device, *words; };
template <class Params, class Set, class Launch>
int set_words_on_device(sx_ctx* ctx, const sx_result* r, Set* set, uint64_t ordinal_base, sx_labels** out, const SetWordsWhat& what, Launch launch) {
    if (out) *out = nullptr;
    if (!ctx || !r || !set || !out) return SX_E_INVALID;
    if (host_only(ctx, what.no_device)) return SX_E_STATE;
    if (on_another_device(ctx, *set, what.set_lies)) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, r, what.host_call); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    uint64_t bytes = 0;
    sx_labels* lab = labels_of(ctx, r, &bytes);
    if (!lab) {
        ctx->set_err(std::string("device ") + what.device + ": no memory for " + std::to_string(bytes) + " bytes of " + what.words);
        return SX_E_NOMEM;
    }
    uint64_t walked = 0;
    hipError_t e = hipSuccess;
    for (size_t i = 0; e == hipSuccess && i < lab->segs.size(); i++) {
        Params p = params_of<Params>(seg_ref(r->r.segs[i]));
        p.ordinal = ordinal_base + walked;
        p.labels = (uint64_t*)lab->segs[i].d;
        p.set = set->dev;
        e = launch(p, st);
        walked += lab->segs[i].n;
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        sx_labels_free(lab);
        ctx->set_err(std::string("device ") + what.device + ": " + hipGetErrorString(e));
        return SX_E_HIP;
    }
    *out = lab;
    return SX_OK;
}

// The two passes of an operation that writes a new result, a segment at a time, as select_on_device drives them.  measure: pass 1
// of segment i inside `scratch` (scratch_bytes(seg.n), 256-aligned); *count and *bytes = the device words that will hold the output's
// records — a word of count_bytes() bytes — and string bytes.  place: pass 2 of segment i, its c records to `recs`, their strings to
// `arena` (scratch: place_scratch_bytes(c)).  settle: between the passes, once per segment and in segment order, with what measure left of
// segment i: SX_OK, or the code — and in *why the message — that ends the call before a block is written or aged.  A selection and an
// extraction have nothing to settle; the fold reads its totals there (SX_E_HIP if it cannot), judges them (SX_E_INVALID) and keeps them.
struct TwoPass {
    virtual ~TwoPass() = default;
    virtual size_t count_bytes() const = 0;
    virtual size_t scratch_bytes(uint64_t n) const = 0;
    virtual hipError_t measure(size_t i, const SegRef& seg, void* scratch, size_t bytes, hipStream_t st, const void** count, const uint64_t** nbytes) = 0;
    virtual size_t place_scratch_bytes(uint64_t c) const = 0;
    virtual hipError_t place(size_t i, void* recs, uint64_t c, uint8_t* arena, void* scratch, size_t bytes, hipStream_t st) = 0;
    virtual int settle(size_t i, uint64_t c, uint64_t bytes, std::string* why) { return SX_OK; }
};

// grep (sx_select_dev.hip): pass 1 by `by.kind` — the patterns of `pat`, a compiled keyword set, a compiled regex set (of `pat` they
// read `invert`), `labels` with masks = { any, all, none }, or `labels` with the field and bounds of `range`, neither of which reads a
// string byte —, pass 2 the same for all five
struct Selection final : TwoPass {
    SelectBy by;
    SelectPatterns pat{};
    const sx_labels* labels = nullptr;
    uint64_t masks[3] = { 0, 0, 0 };
    LabelRange range{};
    std::vector<SelectParams> P;
    explicit Selection(size_t ns) : P(ns) {}
    size_t count_bytes() const override { return sizeof(uint32_t); }
    size_t scratch_bytes(uint64_t n) const override { return select_scratch_bytes(n); }
    hipError_t measure(size_t i, const SegRef& seg, void* scratch, size_t bytes, hipStream_t st, const void** count, const uint64_t** nbytes) override {
        P[i] = params_of<SelectParams>(seg);
        P[i].pat = pat;
        SelectBy b = by;
        LabelPick pick{ nullptr, masks[0], masks[1], masks[2] };
        if (by.kind == SelectBy::kLabels) { pick.labels = labels->segs[i].d; b.pick = &pick; }
        LabelRange field = range;
        if (by.kind == SelectBy::kLabelRange) { field.labels = labels->segs[i].d; b.range = &field; }
        return select_measure(&P[i], b, scratch, bytes, st, (const uint32_t**)count, nbytes);
    }
    size_t place_scratch_bytes(uint64_t c) const override { return select_place_scratch_bytes(c); }
    hipError_t place(size_t i, void* recs, uint64_t c, uint8_t* arena, void* scratch, size_t bytes, hipStream_t st) override {
        return select_place(P[i], recs, c, arena, scratch, bytes, st);
    }
};

// grep -o (sx_extract_dev.hip): an output record is a match, not a finding, and a segment may get more records than it had
struct Extraction final : TwoPass {
    const ExtractDevice& ex;
    std::vector<ExtractParams> X;
    Extraction(const ExtractDevice& e, size_t ns) : ex(e), X(ns) {}
    size_t count_bytes() const override { return sizeof(uint64_t); }
    size_t scratch_bytes(uint64_t n) const override { return extract_scratch_bytes(n); }
    hipError_t measure(size_t i, const SegRef& seg, void* scratch, size_t bytes, hipStream_t st, const void** count, const uint64_t** nbytes) override {
        X[i] = params_of<ExtractParams>(seg);
        X[i].ex = ex;
        return extract_measure(&X[i], scratch, bytes, st, (const uint64_t**)count, nbytes);
    }
    size_t place_scratch_bytes(uint64_t c) const override { return extract_place_scratch_bytes(c); }
    hipError_t place(size_t i, void* recs, uint64_t c, uint8_t* arena, void* scratch, size_t bytes, hipStream_t st) override {
        return extract_place(X[i], recs, c, arena, scratch, bytes, st);
    }
};

// casefold (sx_fold_dev.hip): an output record is its source record with another string, so segment i of the output is segment i of
// the source record for record; the folded strings may have more bytes than the source's
struct Fold final : TwoPass {
    std::vector<FoldParams> F;
    std::vector<const uint64_t*> d_totals;
    sx_fold_info info{ 0, 0, 0, 0 };
    explicit Fold(size_t ns) : F(ns), d_totals(ns) {}
    size_t count_bytes() const override { return sizeof(uint64_t); }
    size_t scratch_bytes(uint64_t n) const override { return fold_scratch_bytes(n); }
    hipError_t measure(size_t i, const SegRef& seg, void* scratch, size_t bytes, hipStream_t st, const void** count, const uint64_t** nbytes) override {
        F[i] = params_of<FoldParams>(seg);
        return fold_measure(&F[i], scratch, bytes, st, (const uint64_t**)count, nbytes, &d_totals[i]);
    }
    size_t place_scratch_bytes(uint64_t c) const override { return 0; }
    hipError_t place(size_t i, void* recs, uint64_t c, uint8_t* arena, void* scratch, size_t bytes, hipStream_t st) override {
        return c == F[i].n ? fold_place(F[i], recs, arena, st) : hipErrorInvalidValue;
    }
    int settle(size_t i, uint64_t c, uint64_t bytes, std::string* why) override {
        uint64_t tot[kFoldTotals] = { 0 };
        const hipError_t e = hipMemcpy(tot, d_totals[i], sizeof tot, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { (void)hipGetLastError(); *why = "device fold: segment " + std::to_string(i) + "'s totals: " + hipGetErrorString(e); return SX_E_HIP; }
        const FoldFit fit = fold_segment_fits(F[i].packed, bytes, tot[kFoldLongest]);
        if (fit == kFoldTooManyBytes) { *why = "fold: segment " + std::to_string(i) + " has " + std::to_string(bytes) + " bytes of folded strings: a 32-bit str_off holds less than 2^32"; return SX_E_INVALID; }
        if (fit == kFoldPackedTooLong) { *why = "fold: a string of the packed segment " + std::to_string(i) + " has " + std::to_string(tot[kFoldLongest]) + " bytes when it is folded: the 16-bit str_len of sx_finding16 holds 65535"; return SX_E_INVALID; }
        info.findings += c; info.bytes_in += tot[kFoldBytesIn]; info.bytes_out += bytes; info.changed += tot[kFoldChanged];
        return SX_OK;
    }
};

// decode (sx_decode_dev.hip): the fold's shape — an output record is its source record with another string —, and pass 1 leaves the
// call's words in `lab`, which the driver has made for the source
struct Decode final : TwoPass {
    const uint32_t kind, flags;
    const sx_labels* lab;
    std::vector<DecodeParams> D;
    std::vector<const uint64_t*> d_totals;
    sx_decode_info info{ 0, 0, 0, 0, 0, 0 };
    Decode(size_t ns, uint32_t k, uint32_t f, const sx_labels* l) : kind(k), flags(f), lab(l), D(ns), d_totals(ns) {}
    size_t count_bytes() const override { return sizeof(uint64_t); }
    size_t scratch_bytes(uint64_t n) const override { return decode_scratch_bytes(n); }
    hipError_t measure(size_t i, const SegRef& seg, void* scratch, size_t bytes, hipStream_t st, const void** count, const uint64_t** nbytes) override {
        D[i] = params_of<DecodeParams>(seg);
        D[i].kind = kind; D[i].flags = flags; D[i].words = (uint64_t*)lab->segs[i].d;
        return decode_measure(&D[i], scratch, bytes, st, (const uint64_t**)count, nbytes, &d_totals[i]);
    }
    size_t place_scratch_bytes(uint64_t c) const override { return 0; }
    hipError_t place(size_t i, void* recs, uint64_t c, uint8_t* arena, void* scratch, size_t bytes, hipStream_t st) override {
        return c == D[i].n ? decode_place(D[i], recs, arena, st) : hipErrorInvalidValue;
    }
    int settle(size_t i, uint64_t c, uint64_t bytes, std::string* why) override {
        uint64_t tot[kDecodeTotals] = { 0 };
        const hipError_t e = hipMemcpy(tot, d_totals[i], sizeof tot, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { (void)hipGetLastError(); *why = "device decode: segment " + std::to_string(i) + "'s totals: " + hipGetErrorString(e); return SX_E_HIP; }
        const DecodeFit fit = decode_segment_fits(D[i].packed, bytes, tot[kDecodeLongest]);
        if (fit == kDecodeTooManyBytes) { *why = "decode: segment " + std::to_string(i) + " has " + std::to_string(bytes) + " bytes of output strings: a 32-bit str_off holds less than 2^32"; return SX_E_INVALID; }
        if (fit == kDecodePackedTooLong) { *why = "decode: a string of the packed segment " + std::to_string(i) + " has " + std::to_string(tot[kDecodeLongest]) + " bytes when it is decoded: the 16-bit str_len of sx_finding16 holds 65535"; return SX_E_INVALID; }
        info.findings += c; info.decoded += tot[kDecodeDecoded]; info.text += tot[kDecodeText]; info.wide += tot[kDecodeWide];
        info.bytes_in += tot[kDecodeBytesIn]; info.bytes_out += bytes;
        return SX_OK;
    }
};

// A new result out of one in HBM, for the eight entry points, whose arguments are checked: pass 1 of every segment, one wait for the
// segments' totals, the selection block, pass 2 of every segment that has output records, one more wait.  The source is read, never
// moved.  The blocks take turns: the one this call writes held the selection before the last one.
int select_on_device(sx_ctx* ctx, const sx_result* r, TwoPass& pass, sx_result** out) {
    // the block this call writes: a source that lies there was made two selections ago
    const int slot = (int)(ctx->select_calls & 1u);
    for (const MissionFindings& s : r->r.segs)
        if (s.dev_epoch_ref == ctx->select_epoch[slot]) { ctx->set_err("this selection reuses the source's device memory: it was selected two calls ago"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    const size_t ns = r->r.segs.size();
    uint64_t scratch = 0;
    for (const MissionFindings& s : r->r.segs) scratch += pass.scratch_bytes(s.ext_nf);
    { const int rc = grow_device(ctx, &ctx->d_select_scratch, &ctx->d_select_scratch_cap, scratch, "wavefront tables"); if (rc != SX_OK) return rc; }
    std::vector<const void*> d_count(ns);
    std::vector<const uint64_t*> d_bytes(ns);
    uint64_t at = 0;
    for (size_t i = 0; i < ns; i++) {
        const size_t bytes = pass.scratch_bytes(r->r.segs[i].ext_nf);
        HIP_TRY(ctx, pass.measure(i, seg_ref(r->r.segs[i]), ctx->d_select_scratch + at, bytes, st, &d_count[i], &d_bytes[i]));
        at += bytes;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::vector<uint64_t> n_sel(ns), b_sel(ns), base(ns);
    uint64_t block = 0, scratch2 = 0;
    for (size_t i = 0; i < ns; i++) {
        uint64_t c = 0;      // (little-endian: a 32-bit word fills its low half)
        HIP_TRY(ctx, hipMemcpy(&c, d_count[i], pass.count_bytes(), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(&b_sel[i], d_bytes[i], sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (c >= 0xFFFFFFFFull) {      // (an extraction: a selection has no more records than its source)
            ctx->set_err("segment " + std::to_string(i) + " has " + std::to_string(c) + " matches: more than the 32-bit counters of a segment hold");
            return SX_E_INVALID;
        }
        std::string why;
        { const int rc = pass.settle(i, c, b_sel[i], &why); if (rc != SX_OK) { ctx->set_err(why); return rc; } }
        n_sel[i] = c;
        if (!c) continue;
        base[i] = block;
        block += up256(c * r->r.segs[i].rec_size() + b_sel[i]);
        scratch2 = std::max<uint64_t>(scratch2, pass.place_scratch_bytes(c));
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
            HIP_TRY(ctx, pass.place(i, recs, n_sel[i], recs + n_sel[i] * s.rec_size(), ctx->d_select_scratch2, pass.place_scratch_bytes(n_sel[i]), st));
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

// The duplicate strings where the findings lie (sx_distinct_dev.hip): the source is checked as a whole, the words' memory is had as the
// labels' is, then the call's own tables — [the segments][the counter and the totals][rep][count][the table], each 256-byte aligned, in
// sx_ctx::d_distinct, which grows on demand and is no selection block —, then the rounds on the selections' stream: the table emptied,
// every segment's claim, every segment's resolve, and one read of the counter, until it is 0; a round that does not lower it is an
// error.  Then every segment's finalize and one read of the totals.  Only the words and the tables are written.
// This is the body of sx_result_distinct_device and the first part of sx_result_seen_device, whose arguments are checked (what:
// "distinct", "seen" — the call's name in the messages; nocase: 0 / 1).  *segs_out (may be NULL): the segments as the kernels took them.
int distinct_on_device(sx_ctx* ctx, const sx_result* r, uint32_t nocase, const char* what, sx_labels** out, sx_distinct_info* info,
                       std::vector<DistinctSeg>* segs_out) {
    *out = nullptr;
    if (host_only(ctx, what)) return SX_E_STATE;
    { const int rc = result_on_device(ctx, r, "compare the strings on the host"); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    const size_t n_segs = r->r.segs.size();
    std::vector<DistinctSeg> segs;
    uint64_t findings = 0, label_bytes = 0;
    for (const MissionFindings& s : r->r.segs) {
        const SegRef v = seg_ref(s);
        if (v.n >> 32 || n_segs >> 31) { ctx->set_err(std::string(what) + ": a segment of 2^32 findings or more"); return SX_E_INVALID; }
        segs.push_back(DistinctSeg{ v.recs, v.arena, v.n, v.packed, 0u, findings });
        findings += v.n;
    }
    uint32_t table_log2 = 1;
    if (ctx->sw.distinct_table_log2 >= 0) table_log2 = (uint32_t)ctx->sw.distinct_table_log2;
    else while (((uint64_t)1 << table_log2) < 2 * findings) table_log2++;
    const uint64_t at_words = up256(n_segs * sizeof(DistinctSeg)), at_rep = at_words + 256, at_count = at_rep + up256(findings * sizeof(uint64_t)),
                   at_table = at_count + up256(findings * sizeof(uint64_t)), table_bytes = sizeof(uint64_t) << table_log2;
    // (the words; then the tables: grown on demand, SX_E_NOMEM leaves them empty)
    sx_labels* lab = labels_of(ctx, r, &label_bytes);
    if (!lab || !device_room(&ctx->d_distinct, &ctx->d_distinct_cap, at_table + table_bytes)) {
        ctx->set_err("device distinct: no memory for " + std::to_string(label_bytes) + " bytes of words and " + std::to_string(at_table + table_bytes) + " bytes of tables");
        sx_labels_free(lab);
        return SX_E_NOMEM;
    }
    uint8_t* const tab = ctx->d_distinct;
    DistinctParams base;
    memset(&base, 0, sizeof base);
    base.segs = (const DistinctSeg*)tab; base.n_segs = (uint32_t)n_segs; base.nocase = nocase; base.table_log2 = table_log2;
    base.unresolved = (uint64_t*)(tab + at_words); base.totals = base.unresolved + 1;
    base.rep = (uint64_t*)(tab + at_rep); base.count = (uint64_t*)(tab + at_count); base.table = (uint64_t*)(tab + at_table);
    // one phase over every segment, in order
    auto phase = [&](int which, uint32_t round) {
        for (size_t i = 0; i < n_segs; i++) {
            DistinctParams p = base;
            p.recs = segs[i].recs; p.arena = segs[i].arena; p.n = segs[i].n; p.packed = segs[i].packed; p.seg = (uint32_t)i; p.base = segs[i].base;
            p.round = round; p.labels = (uint64_t*)lab->segs[i].d;
            const hipError_t pe = distinct_launch(p, which, st);
            if (pe != hipSuccess) return pe;
        }
        return hipSuccess;
    };
    hipError_t e = hipMemcpy(tab, segs.data(), n_segs * sizeof(DistinctSeg), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(tab + at_words, 0, 256, st);
    if (e == hipSuccess) e = hipMemsetAsync(base.rep, 0xFF, findings * sizeof(uint64_t), st);          // (the top bit: no class yet)
    if (e == hipSuccess) e = hipMemsetAsync(base.count, 0, findings * sizeof(uint64_t), st);
    uint64_t left = findings, words[3] = { 0, 0, 0 };
    uint32_t rounds = 0;
    bool stuck = false;
    while (e == hipSuccess && left != 0) {
        const uint64_t before = left;
        e = hipMemsetAsync(base.table, 0xFF, table_bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(base.unresolved, 0, sizeof(uint64_t), st);
        if (e == hipSuccess) e = phase(kDistinctClaim, rounds);
        if (e == hipSuccess) e = phase(kDistinctResolve, rounds);
        if (e == hipSuccess) e = hipMemcpyAsync(&left, base.unresolved, sizeof left, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        rounds++;
        if (ctx->sw.timing) fprintf(stderr, "[sx] distinct round %u: %llu of %llu findings left, 2^%u slots\n", rounds - 1, (unsigned long long)left, (unsigned long long)findings, table_log2);
        if (left >= before) { stuck = true; break; }      // (every round resolves its winners' classes: this is an error, not a reason to go on)
    }
    if (e == hipSuccess && !stuck) e = phase(kDistinctFinalize, rounds);
    if (e == hipSuccess && !stuck) e = hipMemcpyAsync(words, base.unresolved, sizeof words, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess || stuck) {
        (void)hipGetLastError();
        sx_labels_free(lab);
        ctx->set_err(stuck ? "device distinct: round " + std::to_string(rounds - 1) + " left " + std::to_string(left) + " findings without a class, no fewer than the round before"
                           : std::string("device distinct: ") + hipGetErrorString(e));
        return SX_E_HIP;
    }
    if (info) *info = sx_distinct_info{ findings, words[1], words[2], rounds, table_log2 };
    if (segs_out) *segs_out = std::move(segs);
    *out = lab;
    return SX_OK;
}

// The findings in sorted order where they lie (sx_order_dev.hip), for sx_result_order_device, whose arguments are checked.  The pick's
// tables — per wavefront of the call — go into the selections' wavefront tables, the sort's into sx_ctx::d_distinct, which grows on
// demand and is no selection block.  On the selections' stream: every segment's pick, one scan, ONE read of the totals — how many
// take part, their bytes, the longest string: the 32-bit limits are decided here, before anything else is written —; every segment's
// number; then the label key's one sort, or the rounds of the string key with ONE read each — the scan's total: the slots still
// undecided and their groups —, at most longest / 8 + 2 of them (one more is an error, never a reason to go on); measure and one
// read — the kept findings' bytes and ties —; the block whose turn it is, gather, order_part_strings, one wait.  The call takes its
// turn only when both blocks are had: an error in front of that ages nothing.
int order_on_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels, const sx_order_spec& spec, sx_result** out, sx_order_info* info) {
    const int slot = (int)(ctx->select_calls & 1u);
    for (const MissionFindings& s : r->r.segs)
        if (s.dev_epoch_ref == ctx->select_epoch[slot]) { ctx->set_err("this order reuses the source's device memory: it was selected two calls ago"); return SX_E_STATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    const size_t ns = r->r.segs.size();
    const bool by_field = spec.by == SX_ORDER_BY_LABEL_FIELD;
    const uint32_t descending = spec.flags & SX_ORDER_DESCENDING ? 1u : 0u, nocase = spec.flags & SX_ORDER_NOCASE ? 1u : 0u;
    std::vector<OrderSeg> segs;
    std::vector<uint64_t> pos0;
    std::vector<size_t> pos0_of(ns, 0);
    uint64_t waves = 0, n_packed = 0;
    for (size_t i = 0; i < ns; i++) {
        const MissionFindings& s = r->r.segs[i];
        const SegRef v = seg_ref(s);
        if (v.n >> 32 || ns >> 31) { ctx->set_err("order: a segment of 2^32 findings or more"); return SX_E_INVALID; }
        OrderSeg g;
        memset(&g, 0, sizeof g);
        g.recs = v.recs; g.arena = v.arena; g.n = v.n; g.packed = v.packed; g.file_id = -1;
        g.labels = labels ? labels->segs[i].d : nullptr; g.wave0 = waves;
        if (v.packed) {
            pos0_of[i] = n_packed++;
            pos0.resize(n_packed * 256, 0);
            if (s.info) { g.file_id = s.info->file_id; g.slice_base = s.info->slice_base; memcpy(&pos0[pos0_of[i] * 256], s.info->pos0, 256 * sizeof(uint64_t)); }
        }
        segs.push_back(g);
        waves += (v.n + kSelectRecs - 1) / kSelectRecs;
    }
    { const int rc = grow_device(ctx, &ctx->d_select_scratch, &ctx->d_select_scratch_cap, order_pick_tables(nullptr, ns, n_packed, waves, nullptr), "wavefront tables"); if (rc != SX_OK) return rc; }
    OrderPickTables PT;
    (void)order_pick_tables(ctx->d_select_scratch, ns, n_packed, waves, &PT);
    for (size_t i = 0; i < ns; i++)
        if (segs[i].packed) segs[i].pos0 = PT.pos0 + pos0_of[i] * 256;
    OrderPick pick;
    memset(&pick, 0, sizeof pick);
    pick.filter = (spec.any | spec.all | spec.none) != 0 ? 1u : 0u; pick.any = spec.any; pick.all = spec.all; pick.none = spec.none;
    pick.wmask = PT.wmask; pick.wcount = PT.wcount; pick.wbase = PT.wbase; pick.totals = PT.totals;
    pick.shift = spec.shift; pick.descending = descending; pick.mask = spec.bits >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << spec.bits) - 1u;
    uint64_t tot[kOrderTotals] = { 0 };
    hipError_t e = hipMemcpy(PT.segs, segs.data(), ns * sizeof(OrderSeg), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_packed) e = hipMemcpy(PT.pos0, pos0.data(), pos0.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(PT.totals, 0, kOrderTotals * sizeof(uint64_t), st);
    for (size_t i = 0; e == hipSuccess && i < ns; i++) { pick.seg = segs[i]; pick.seg_index = (uint32_t)i; e = order_launch_pick(pick, st); }
    if (e == hipSuccess) e = order_scan_picks(PT, waves, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tot, PT.totals, sizeof tot, hipMemcpyDeviceToHost, st);
    { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    auto failed = [&](const std::string& what) {
        (void)hipGetLastError();
        ctx->set_err("device order: " + what);
        return SX_E_HIP;
    };
    if (e != hipSuccess) return failed(hipGetErrorString(e));
    const uint64_t m = tot[kOrderCount];
    if (m > 0xFFFFFFFEull || tot[kOrderBytes] >> 32) {
        ctx->set_err("order: " + std::to_string(m) + " findings with " + std::to_string(tot[kOrderBytes]) + " bytes of strings take part: one segment holds 2^32 - 2 findings and less than 2^32 bytes");
        return SX_E_INVALID;
    }
    ResultHolder res;
    res.r->r.pool = ctx->pool;
    if (m == 0) {      // (as a selection that selects nothing: the call counts, the result has no segment)
        ctx->select_epoch[slot]->fetch_add(1);
        ctx->select_calls++;
        if (info) *info = sx_order_info{ 0, 0, 0, 0, 0 };
        *out = res.release();
        return SX_OK;
    }
    const uint64_t sort_bytes = order_sort_tables(nullptr, m, nullptr);
    if (!device_room(&ctx->d_distinct, &ctx->d_distinct_cap, sort_bytes)) {
        ctx->set_err("device order: no memory for " + std::to_string(sort_bytes) + " bytes of tables");
        return SX_E_NOMEM;
    }
    OrderSortTables ST;
    (void)order_sort_tables(ctx->d_distinct, m, &ST);
    pick.ikey = ST.ikey[0]; pick.slotpos = ST.slotpos[0]; pick.slotgrp = ST.slotgrp[0]; pick.field = by_field ? ST.wkey : nullptr;
    for (size_t i = 0; e == hipSuccess && i < ns; i++) { pick.seg = segs[i]; pick.seg_index = (uint32_t)i; e = order_launch_number(pick, st); }
    uint64_t rounds = 0;
    if (by_field) {
        if (e == hipSuccess) e = order_by_field(ST, m, spec.bits, st);
    } else {
        const uint64_t most = tot[kOrderLongest] / 8 + 2;
        uint64_t left = m, groups = 1;
        int cur = 0;
        while (e == hipSuccess && left != 0) {
            if (rounds >= most) return failed("round " + std::to_string(rounds) + " would look behind the longest string's end, and " + std::to_string(left) + " findings are not yet in order");
            uint64_t word = 0;
            e = order_round(ST, PT.segs, cur, left, groups, (uint32_t)rounds, nocase, descending, st);
            if (e == hipSuccess) e = hipMemcpyAsync(&word, ST.scan + left, sizeof word, hipMemcpyDeviceToHost, st);
            { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
            if (e != hipSuccess) break;
            rounds++;
            if (ctx->sw.timing) fprintf(stderr, "[sx] order round %llu: %llu of %llu findings left in %llu groups\n", (unsigned long long)(rounds - 1), (unsigned long long)(word & 0xFFFFFFFFu), (unsigned long long)m, (unsigned long long)(word >> 32));
            if ((word & 0xFFFFFFFFu) > left) return failed("round " + std::to_string(rounds - 1) + " left more findings undecided than it began with");
            left = word & 0xFFFFFFFFu; groups = word >> 32; cur ^= 1;
        }
    }
    const uint64_t kept = spec.limit && spec.limit < m ? spec.limit : m;
    OrderOut O;
    memset(&O, 0, sizeof O);
    O.segs = PT.segs; O.order = ST.order; O.classhead = ST.classhead; O.kept = kept; O.totals = PT.totals;
    if (e == hipSuccess) e = order_launch_measure(O, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tot, PT.totals, sizeof tot, hipMemcpyDeviceToHost, st);
    { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) return failed(hipGetErrorString(e));
    // the two blocks; where the output's block is had anew, what lay there is gone whether or not the call goes on
    const uint64_t kept_bytes = tot[kOrderKeptBytes], block = up256(kept * sizeof(sx_finding) + kept_bytes), src_bytes = up256(kept * sizeof(uint64_t)),
                   scratch2 = src_bytes + order_strings_scratch_bytes(kept);
    if (!device_room(&ctx->d_select[slot], &ctx->d_select_cap[slot], block)) {
        ctx->select_epoch[slot]->fetch_add(1);
        ctx->set_err("device order: no memory for " + std::to_string(block) + " bytes of ordered findings");
        return SX_E_NOMEM;
    }
    { const int rc = grow_device(ctx, &ctx->d_select_scratch2, &ctx->d_select_scratch2_cap, scratch2, "string offsets"); if (rc != SX_OK) return rc; }
    ctx->select_epoch[slot]->fetch_add(1);
    ctx->select_calls++;
    uint8_t* recs = ctx->d_select[slot];
    O.out = (sx_finding*)recs; O.out_src = (uint64_t*)ctx->d_select_scratch2;
    e = order_launch_gather(O, st);
    if (e == hipSuccess) e = order_part_strings(recs, kept, 0, O.out_src, recs + kept * sizeof(sx_finding), ctx->d_select_scratch2 + src_bytes, scratch2 - src_bytes, st);
    { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) return failed(hipGetErrorString(e));
    MissionFindings o;
    o.ext_nf = kept; o.ext_na = kept_bytes; o.dev_copy = recs; o.dev_only = true; o.keep_on_device = true;
    o.dev_epoch_ref = ctx->select_epoch[slot]; o.dev_epoch = ctx->select_epoch[slot]->load();
    res.r->r.segs.push_back(std::move(o));
    if (info) *info = sx_order_info{ m, kept, rounds, tot[kOrderTied], rounds ? rounds - 1 : 0 };
    *out = res.release();
    return SX_OK;
}

// THE mark/add protocol of a seen set, for a result's records (sx_seen_dev.hip) and for a source of entries (sx_seen_merge_dev.hip),
// on the selections' stream: the totals zeroed; the caller's mark launches; ONE read — the set's cursors and the call's totals, which
// lie side by side, and in the same wait held[] where the caller wants it (d_held -> *held, sized by the caller) —; the host decides
// `lost` (a lookup walked every slot), then `full` (what is new does not fit: SX_E_NOMEM BEFORE the add pass, the set is as it was);
// the caller's add launches, only if adding and something is new; the same read again behind them: the error total — an adder that
// found no slot — and the cursors, which have to be the sums.  launch(phase): the caller's launches of one pass, kSeenMark / kSeenAdd.
// A destination that COUNTS (dst.counts) has a third phase, kSeenCount, only when adding: behind the add launches — or in their place
// when nothing is new but something was held —, in front of that read: every class of the call (held + new) adds to its slot's count
// word, and the counted total, the word behind the totals, has to be their number.  A plain destination launches what it always did.
// what: the call's name in a refusal ("seen set", "seen set merge"), err_what: in an error.  tot: the totals as mark left them.
template <class Launch>
int seen_mark_add(sx_ctx* ctx, const std::string& what, const std::string& err_what, const SeenSet& dst, uint64_t capacity_strings, uint64_t capacity_bytes,
                  bool add, Launch launch, uint64_t tot[kSeenTotals], const uint64_t* d_held, std::vector<uint64_t>* held) {
    hipStream_t st = ctx->post_stream;
    const bool counts = add && dst.counts != nullptr;
    const size_t n_words = 2 + kSeenTotals + (counts ? 1u : 0u);      // the cursors, the totals, a counting call's counted total
    uint64_t words[2 + kSeenTotals + 1] = { 0 };
    auto read_back = [&] { return hipMemcpyAsync(words, dst.cursors, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, st); };
    hipError_t e = hipMemsetAsync(dst.cursors + 2, 0, (n_words - 2) * sizeof(uint64_t), st);
    if (e == hipSuccess) e = launch(kSeenMark);
    if (e == hipSuccess) e = read_back();
    if (e == hipSuccess && held && !held->empty()) e = hipMemcpyAsync(held->data(), d_held, held->size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    memcpy(tot, words + 2, kSeenTotals * sizeof(uint64_t));
    const uint64_t had[2] = { words[0], words[1] }, fresh = tot[kSeenNewClasses], fresh_bytes = tot[kSeenNewBytes], classes = tot[kSeenClasses] + fresh;
    bool lost = e == hipSuccess && tot[kSeenError] != 0, added = false;
    const bool full = e == hipSuccess && !lost && add && (had[0] + fresh > capacity_strings || had[1] + fresh_bytes > capacity_bytes);
    const bool count = counts && classes != 0;
    if (e == hipSuccess && !lost && !full && add && (fresh || count)) {
        added = true;
        if (fresh) e = launch(kSeenAdd);
        if (e == hipSuccess && count) e = launch(kSeenCount);
        if (e == hipSuccess) e = read_back();
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
        lost = e == hipSuccess && (words[2 + kSeenError] != 0 || words[0] != had[0] + fresh || words[1] != had[1] + fresh_bytes || (count && words[2 + kSeenCounted] != classes));
    }
    if (e == hipSuccess && !lost && !full) return SX_OK;
    (void)hipGetLastError();
    if (full)
        ctx->set_err(what + ": " + std::to_string(had[0]) + " + " + std::to_string(fresh) + " strings of " + std::to_string(capacity_strings) + ", "
                     + std::to_string(had[1]) + " + " + std::to_string(fresh_bytes) + " bytes of " + std::to_string(capacity_bytes) + ": the set is as it was, sx_seen_set_grow gives it room");
    else if (lost)
        ctx->set_err(err_what + (added ? ": an adder walked every slot of the set and met no empty one, the cursors are not the sums, or not every string was counted"
                                       : ": a probe walked every slot of the set and met no empty one"));
    else
        ctx->set_err(err_what + ": " + hipGetErrorString(e));
    return full ? SX_E_NOMEM : SX_E_HIP;
}

}  // namespace

extern "C" {

int sx_result_segment_device(const sx_result* r, uint64_t i, const void** d_records, uint64_t* n_findings, const uint8_t** d_arena,
                             uint64_t* arena_len, int* packed, sx_segment_info* info) {
    if (!r || i >= r->r.segs.size()) return SX_E_INVALID;
    const MissionFindings& s = r->r.segs[(size_t)i];
    if (d_records) *d_records = nullptr;
    if (d_arena) *d_arena = nullptr;
    if (n_findings) *n_findings = s.count();
    if (arena_len) *arena_len = s.strings_len();
    if (packed) *packed = s.packed ? 1 : 0;
    if (info) fill_segment_info(s, info);
    if (!s.dev_only) return SX_OK;   // (in host memory: the host accessors)
    if (!s.keep_on_device || !s.dev_epoch_ref || s.dev_epoch_ref->load() != s.dev_epoch) return SX_E_STATE;
    const SegRef v = seg_ref(s);
    if (d_records) *d_records = v.recs;
    if (d_arena) *d_arena = v.arena;
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
    if (host_only(ctx, "print")) return SX_E_STATE;
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
    if (!device_room(&ctx->d_print_scratch, &ctx->d_print_scratch_cap, scratch)) { ctx->set_err("device print: no memory for the offsets"); return SX_E_NOMEM; }
    std::vector<PrintParams> P(ns);
    std::vector<const uint64_t*> d_total(ns);
    uint64_t at = 0;
    for (size_t i = 0; i < ns; i++) {
        const MissionFindings& s = r->r.segs[i];
        PrintParams& p = P[i];
        p = params_of<PrintParams>(seg_ref(s));
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
    if (!device_room(&ctx->d_text, &ctx->d_text_cap, total)) { ctx->set_err("device print: no memory for " + std::to_string(total) + " bytes of text"); return SX_E_NOMEM; }
    for (size_t i = 0; i < ns; i++) {
        P[i].text = ctx->d_text;
        HIP_TRY(ctx, print_write(P[i], st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *d_text = ctx->d_text;
    *text_len = total;
    return SX_OK;
}

int sx_result_select_device(sx_ctx* ctx, const sx_result* r, const sx_pattern* patterns, int n_patterns, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !patterns || !out) return SX_E_INVALID;
    if (n_patterns < 1 || n_patterns > SX_SELECT_MAX_PATTERNS) { ctx->set_err("n_patterns must be 1..16"); return SX_E_INVALID; }
    if (flags & ~(uint32_t)(SX_SELECT_ASCII_NOCASE | SX_SELECT_INVERT)) { ctx->set_err("unknown selection flags"); return SX_E_INVALID; }
    for (int p = 0; p < n_patterns; p++)
        if (!patterns[p].bytes || patterns[p].len < 1 || patterns[p].len > SX_SELECT_MAX_PATTERN_BYTES) { ctx->set_err("a pattern must have 1..64 bytes"); return SX_E_INVALID; }
    if (host_only(ctx, "selection")) return SX_E_STATE;
    { const int rc = result_on_device(ctx, r, "filter on the host"); if (rc != SX_OK) return rc; }
    Selection sel(r->r.segs.size());
    select_fill_patterns(&sel.pat, patterns, n_patterns, flags);
    return select_on_device(ctx, r, sel, out);
}

int sx_select_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_select_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    SelsetTable T;
    std::string err;
    { const int rc = selset_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("pattern set: " + err); return rc; } }
    uint8_t* mem = nullptr;
    size_t at[3];
    // (the kernels copy the LDS rows in 16-byte chunks: every set's table ends on one)
    { const int rc = upload_set(ctx, "pattern set", { { T.map, sizeof T.map, 1 }, { T.next.data(), T.next.size(), 16 } }, 0, &mem, at); if (rc != SX_OK) return rc; }
    sx_select_set* set = new_handle<sx_select_set>(ctx, mem);
    if (!set) return SX_E_NOMEM;
    set->dev = SelsetDevice{ mem, mem + at[1], T.states, T.classes, T.lds_states, T.matched, T.entry_bytes, 0 };
    set->info = sx_select_set_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)T.next.size(), T.lds_states, 0 };
    *out = set;
    return SX_OK;
}
int sx_select_set_info_get(const sx_select_set* set, sx_select_set_info* out) { return handle_info(set, out); }
void sx_select_set_free(sx_select_set* set) { handle_free(set); }

int sx_result_select_set_device(sx_ctx* ctx, const sx_result* r, const sx_select_set* set, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !set || !out) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SELECT_INVERT) { ctx->set_err("a pattern set is selected with SX_SELECT_INVERT or no flag: the fold is compiled into the set"); return SX_E_INVALID; }
    if (host_only(ctx, "selection")) return SX_E_STATE;
    if (on_another_device(ctx, *set, "the pattern set lies")) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, r, "filter on the host"); if (rc != SX_OK) return rc; }
    Selection sel(r->r.segs.size());
    sel.by.kind = SelectBy::kSet; sel.by.set = &set->dev;
    sel.pat.invert = (flags & SX_SELECT_INVERT) ? 1u : 0u;
    return select_on_device(ctx, r, sel, out);
}

int sx_select_regex_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_select_regex** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    SelreTable T;
    std::string err;
    { const int rc = selre_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("regex set: " + err); return rc; } }
    const size_t bytes = T.next.size() * sizeof(uint16_t);
    uint8_t* mem = nullptr;
    size_t at[3];
    { const int rc = upload_set(ctx, "regex set", { { T.map, sizeof T.map, 1 }, { T.next.data(), bytes, 16 } }, 0, &mem, at); if (rc != SX_OK) return rc; }
    sx_select_regex* re = new_handle<sx_select_regex>(ctx, mem);
    if (!re) return SX_E_NOMEM;
    re->dev = SelreDevice{ mem, (const uint16_t*)(mem + at[1]), T.states, T.classes, T.lds_states, T.end_first, T.stop_first, T.matched, T.root_end, 0 };
    re->info = sx_select_regex_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)bytes, T.lds_states, T.end_states };
    *out = re;
    return SX_OK;
}
int sx_select_regex_info_get(const sx_select_regex* re, sx_select_regex_info* out) { return handle_info(re, out); }
void sx_select_regex_free(sx_select_regex* re) { handle_free(re); }

int sx_result_select_regex_device(sx_ctx* ctx, const sx_result* r, const sx_select_regex* re, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !re || !out) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SELECT_INVERT) { ctx->set_err("a regex set is selected with SX_SELECT_INVERT or no flag: the fold is compiled into the set"); return SX_E_INVALID; }
    if (host_only(ctx, "selection")) return SX_E_STATE;
    if (on_another_device(ctx, *re, "the regex set lies")) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, r, "filter on the host"); if (rc != SX_OK) return rc; }
    Selection sel(r->r.segs.size());
    sel.by.kind = SelectBy::kRegex; sel.by.re = &re->dev;
    sel.pat.invert = (flags & SX_SELECT_INVERT) ? 1u : 0u;
    return select_on_device(ctx, r, sel, out);
}

int sx_extract_regex_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_extract_regex** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    ExtractTable T;
    std::string err;
    { const int rc = extract_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("extract set: " + err); return rc; } }
    const size_t bytes = T.next.size() * sizeof(uint16_t);
    uint8_t* mem = nullptr;
    size_t at[3];
    { const int rc = upload_set(ctx, "extract set", { { T.map, sizeof T.map, 1 }, { T.next.data(), bytes, 16 } }, 0, &mem, at); if (rc != SX_OK) return rc; }
    sx_extract_regex* ex = new_handle<sx_extract_regex>(ctx, mem);
    if (!ex) return SX_E_NOMEM;
    ex->dev = ExtractDevice{ mem, (const uint16_t*)(mem + at[1]), T.states, T.classes, T.lds_states, T.end_first, T.here_first, T.dead_first, T.start0, T.start1 };
    ex->info = sx_extract_regex_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)bytes, T.lds_states, 0 };
    *out = ex;
    return SX_OK;
}
int sx_extract_regex_info_get(const sx_extract_regex* ex, sx_extract_regex_info* out) { return handle_info(ex, out); }
void sx_extract_regex_free(sx_extract_regex* ex) { handle_free(ex); }

int sx_result_extract_regex_device(sx_ctx* ctx, const sx_result* r, const sx_extract_regex* ex, uint32_t flags, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !ex || !out) return SX_E_INVALID;
    if (flags) { ctx->set_err("an extraction takes no flag: the fold is compiled into the set"); return SX_E_INVALID; }
    if (host_only(ctx, "extraction")) return SX_E_STATE;
    if (on_another_device(ctx, *ex, "the extract set lies")) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, r, "filter on the host"); if (rc != SX_OK) return rc; }
    Extraction x(ex->dev, r->r.segs.size());
    return select_on_device(ctx, r, x, out);
}

int sx_tally_set_reset(sx_tally_set* set) {
    if (!set) return SX_E_INVALID;
    return reset_counters(set->device, set->dev.hits, set->dev.first, set->dev.unique);
}

int sx_tally_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_tally_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    SeltallyTable T;
    std::string err;
    { const int rc = seltally_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("tally set: " + err); return rc; } }
    const size_t per_state = (size_t)T.states * sizeof(uint32_t), map_bytes = (size_t)T.n_patterns * sizeof(uint32_t), counters = (size_t)T.unique * sizeof(uint64_t);
    uint8_t* mem = nullptr;
    size_t at[6];
    // (the counters are 64-bit words: the pattern -> unique id map in front of them ends on 8 bytes)
    { const int rc = upload_set(ctx, "tally set", { { T.map, sizeof T.map, 1 }, { T.next.data(), T.next.size(), 16 }, { T.own.data(), per_state, 1 }, { T.dict.data(), per_state, 1 },
                                                    { T.unique_of_pattern.data(), map_bytes, 8 } }, 2 * counters, &mem, at); if (rc != SX_OK) return rc; }
    sx_tally_set* set = new_handle<sx_tally_set>(ctx, mem);
    if (!set) return SX_E_NOMEM;
    set->dev = SeltallyDevice{ mem, mem + at[1], (const uint32_t*)(mem + at[2]), (const uint32_t*)(mem + at[3]),
                               (uint64_t*)(mem + at[5]), (uint64_t*)(mem + at[5] + counters),
                               T.states, T.classes, T.lds_states, T.entry_bytes, T.unique, T.unique < kSeltallyLdsIds ? T.unique : kSeltallyLdsIds };
    set->d_unique_of_pattern = (const uint32_t*)(mem + at[4]);
    set->info = sx_tally_set_info{ T.n_patterns, T.unique, T.states, T.classes, T.nocase, T.entry_bytes,
                                   (uint64_t)(sizeof T.map + T.next.size() + 2 * per_state + map_bytes), T.lds_states, 0 };
    set->unique_of_pattern = std::move(T.unique_of_pattern);
    if (sx_tally_set_reset(set) != SX_OK) { ctx->set_err("tally set: the counters could not be reset"); sx_tally_set_free(set); return SX_E_HIP; }
    *out = set;
    return SX_OK;
}
int sx_tally_set_info_get(const sx_tally_set* set, sx_tally_set_info* out) { return handle_info(set, out); }
void sx_tally_set_free(sx_tally_set* set) { handle_free(set); }

// The tally where the findings lie (sx_seltally_dev.hip): the source is checked as a whole, then one kernel per segment, each with the
// ordinal of its first record, on the selections' stream, and one wait.  Only the set's counters are written.
int sx_result_tally_device(sx_ctx* ctx, const sx_result* r, sx_tally_set* set, uint64_t ordinal_base, uint64_t* n_findings) {
    if (n_findings) *n_findings = 0;
    if (!ctx || !r || !set) return SX_E_INVALID;
    if (host_only(ctx, "tally")) return SX_E_STATE;
    if (on_another_device(ctx, *set, "the tally set lies")) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, r, "count on the host"); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    uint64_t walked = 0;
    for (const MissionFindings& s : r->r.segs) {
        SeltallyParams p = params_of<SeltallyParams>(seg_ref(s));
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
    std::vector<uint64_t> u(set->dev.unique);
    for (int k = 0; k < 2; k++) {
        uint64_t* out = k ? first : hits;
        if (!out) continue;
        { const int rc = read_counters(set->device, k ? set->dev.first : set->dev.hits, u.data(), u.size()); if (rc != SX_OK) return rc; }
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
    return reset_counters(set->device, set->dev.findings, set->dev.first, kLabelBits);
}

int sx_label_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_label_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !out) return SX_E_INVALID;
    LabelTable T;
    std::string err;
    { const int rc = label_build(patterns, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("label set: " + err); return rc; } }
    const size_t next_bytes = T.next.size() * sizeof(uint16_t), here_bytes = T.here.size() * sizeof(uint64_t), end_bytes = T.end.size() * sizeof(uint64_t);
    const size_t counters = kLabelBits * sizeof(uint64_t);
    uint8_t* mem = nullptr;
    size_t at[5];
    { const int rc = upload_set(ctx, "label set", { { T.map, sizeof T.map, 1 }, { T.next.data(), next_bytes, 16 }, { T.here.data(), here_bytes, 1 }, { T.end.data(), end_bytes, 1 } },
                                2 * counters, &mem, at); if (rc != SX_OK) return rc; }
    sx_label_set* set = new_handle<sx_label_set>(ctx, mem);
    if (!set) return SX_E_NOMEM;
    set->dev = LabelDevice{ mem, (const uint16_t*)(mem + at[1]), (const uint64_t*)(mem + at[2]), (const uint64_t*)(mem + at[3]),
                            (uint64_t*)(mem + at[4]), (uint64_t*)(mem + at[4] + counters), T.root_here, T.all,
                            T.states, T.classes, T.lds_states, T.here_first, T.dead, T.n_patterns };
    set->info = sx_label_set_info{ T.n_patterns, T.states, T.classes, T.nocase, (uint64_t)(sizeof T.map + next_bytes + here_bytes + end_bytes), T.lds_states, (uint32_t)T.here.size() };
    if (sx_label_set_reset(set) != SX_OK) { ctx->set_err("label set: the counters could not be reset"); sx_label_set_free(set); return SX_E_HIP; }
    *out = set;
    return SX_OK;
}
int sx_label_set_info_get(const sx_label_set* set, sx_label_set_info* out) { return handle_info(set, out); }
void sx_label_set_free(sx_label_set* set) { handle_free(set); }

int sx_label_set_read(const sx_label_set* set, uint64_t* findings, uint64_t* first, uint32_t n_patterns) {
    if (!set || n_patterns != set->info.n_patterns) return SX_E_INVALID;
    const int rc = read_counters(set->device, set->dev.findings, findings, n_patterns);
    return rc != SX_OK ? rc : read_counters(set->device, set->dev.first, first, n_patterns);
}

int sx_label_set_counters_device(const sx_label_set* set, const uint64_t** d_findings, const uint64_t** d_first) {
    if (!set) return SX_E_INVALID;
    if (d_findings) *d_findings = set->dev.findings;
    if (d_first) *d_first = set->dev.first;
    return SX_OK;
}

int sx_result_label_device(sx_ctx* ctx, const sx_result* r, sx_label_set* set, uint64_t ordinal_base, sx_labels** out) {
    return set_words_on_device<LabelParams>(ctx, r, set, ordinal_base, out, { "labels", "the label set lies", "label on the host", "labels", "labels" }, label_launch);
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

void sx_labels_free(sx_labels* labels) { handle_free(labels); }

// What both selections by labels ask, the pointers checked: a device, a result in HBM, and labels made from it
static int labels_of_result(sx_ctx* ctx, const sx_result* r, const sx_labels* labels) {
    if (host_only(ctx, "selection")) return SX_E_STATE;
    if (on_another_device(ctx, *labels, "the labels lie")) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, r, "filter on the host"); if (rc != SX_OK) return rc; }
    // the labels are this result's: segment by segment the same records, in a block that has not been written since
    bool same = labels->segs.size() == r->r.segs.size();
    for (size_t i = 0; same && i < labels->segs.size(); i++) {
        const sx_labels::Seg& l = labels->segs[i];
        const MissionFindings& s = r->r.segs[i];
        same = l.recs == s.dev_copy && l.n == s.ext_nf && l.epoch_ref == s.dev_epoch_ref && l.epoch == s.dev_epoch;
    }
    if (!same) { ctx->set_err("the labels were not made from this result"); return SX_E_INVALID; }
    return SX_OK;
}

int sx_result_select_labels_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels, uint64_t any, uint64_t all, uint64_t none, sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !labels || !out) return SX_E_INVALID;
    { const int rc = labels_of_result(ctx, r, labels); if (rc != SX_OK) return rc; }
    Selection sel(r->r.segs.size());
    sel.by.kind = SelectBy::kLabels;
    sel.labels = labels;
    sel.masks[0] = any; sel.masks[1] = all; sel.masks[2] = none;
    return select_on_device(ctx, r, sel, out);
}

int sx_result_select_labels_range_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels, uint32_t shift, uint32_t bits, uint64_t lo, uint64_t hi,
                                         sx_result** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !labels || !out) return SX_E_INVALID;
    if (bits < 1 || bits > 64 || shift > 64 - bits) {
        ctx->set_err("select by range: a field of " + std::to_string(bits) + " bits at bit " + std::to_string(shift) + ": 1 to 64 bits that end at bit 64 at most");
        return SX_E_INVALID;
    }
    { const int rc = labels_of_result(ctx, r, labels); if (rc != SX_OK) return rc; }
    Selection sel(r->r.segs.size());
    sel.by.kind = SelectBy::kLabelRange;
    sel.labels = labels;
    sel.range = LabelRange{ nullptr, lo, hi, shift, bits };
    return select_on_device(ctx, r, sel, out);
}

int sx_result_order_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels, const sx_order_spec* spec, sx_result** out, sx_order_info* info) {
    if (out) *out = nullptr;
    if (!ctx || !r || !spec || !out) return SX_E_INVALID;
    if (spec->by != SX_ORDER_BY_STRING && spec->by != SX_ORDER_BY_LABEL_FIELD) { ctx->set_err("order: `by` is neither SX_ORDER_BY_STRING nor SX_ORDER_BY_LABEL_FIELD"); return SX_E_INVALID; }
    if (spec->flags & ~(uint32_t)(SX_ORDER_DESCENDING | SX_ORDER_NOCASE)) { ctx->set_err("order: flags other than SX_ORDER_DESCENDING and SX_ORDER_NOCASE"); return SX_E_INVALID; }
    const bool by_field = spec->by == SX_ORDER_BY_LABEL_FIELD;
    if (by_field && (spec->flags & SX_ORDER_NOCASE)) { ctx->set_err("order: SX_ORDER_NOCASE folds strings, and the key is a label field"); return SX_E_INVALID; }
    if (by_field && (spec->bits < 1 || spec->bits > 64 || spec->shift > 64 - spec->bits)) {
        ctx->set_err("order: a field of " + std::to_string(spec->bits) + " bits at bit " + std::to_string(spec->shift) + ": 1 to 64 bits that end at bit 64 at most");
        return SX_E_INVALID;
    }
    if (!labels && (by_field || spec->any || spec->all || spec->none)) {
        ctx->set_err(by_field ? "order: the key is a label field, and there are no labels" : "order: the masks any, all and none pick by labels, and there are none");
        return SX_E_INVALID;
    }
    if (labels) { const int rc = labels_of_result(ctx, r, labels); if (rc != SX_OK) return rc; }
    else {
        if (host_only(ctx, "order")) return SX_E_STATE;
        { const int rc = result_on_device(ctx, r, "sort on the host"); if (rc != SX_OK) return rc; }
    }
    return order_on_device(ctx, r, labels, *spec, out, info);
}

static const FoldTable kFoldHost{ kFoldIndex, kFoldPages };

int sx_fold_utf8(const uint8_t* in, uint64_t len, uint32_t flags, uint8_t* out, uint64_t cap, uint64_t* written) {
    if (written) *written = 0;
    if ((!in && len) || !written || flags != SX_FOLD_SIMPLE) return SX_E_INVALID;
    bool changed;
    const uint64_t need = fold_measure_string(kFoldHost, in, len, &changed);
    *written = need;
    if (!out) return SX_OK;            // (the size was asked for)
    if (need > cap) return SX_E_INVALID;
    (void)fold_place_string(kFoldHost, in, len, out);
    return SX_OK;
}

int sx_result_fold_device(sx_ctx* ctx, const sx_result* r, uint32_t flags, sx_result** out, sx_fold_info* info) {
    if (out) *out = nullptr;
    if (!ctx || !r || !out) return SX_E_INVALID;
    if (flags != SX_FOLD_SIMPLE) { ctx->set_err("fold: flags other than SX_FOLD_SIMPLE"); return SX_E_INVALID; }
    if (host_only(ctx, "fold")) return SX_E_STATE;
    { const int rc = result_on_device(ctx, r, "fold on the host, with sx_fold_utf8"); if (rc != SX_OK) return rc; }
    Fold fold(r->r.segs.size());
    const int rc = select_on_device(ctx, r, fold, out);
    if (rc == SX_OK && info) *info = fold.info;
    return rc;
}

static bool decode_args_ok(uint32_t kind, uint32_t flags) {
    return kind >= SX_DECODE_BASE64 && kind <= SX_DECODE_PERCENT && !(flags & ~(uint32_t)SX_DECODE_UTF16LE);
}

int sx_decode_bytes(uint32_t kind, uint32_t flags, const uint8_t* in, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* written, uint64_t* word) {
    if (written) *written = 0;
    if (word) *word = 0;
    if ((!in && len) || !written || !decode_args_ok(kind, flags) || len >> 32) return SX_E_INVALID;
    uint64_t need = 0;
    const uint64_t w = decode_measure_string(kind, flags, in, (uint32_t)len, &need);
    *written = need;
    if (word) *word = w;
    if (!out) return SX_OK;            // (the size was asked for)
    if (need > cap) return SX_E_INVALID;
    decode_place_string(kind, flags, w, in, (uint32_t)len, out);
    return SX_OK;
}

// The words' memory is had as sx_result_measure_device has it, then the fold's two passes: pass 1 writes the words
int sx_result_decode_device(sx_ctx* ctx, const sx_result* r, uint32_t kind, uint32_t flags, sx_result** out, sx_labels** words, sx_decode_info* info) {
    if (out) *out = nullptr;
    if (words) *words = nullptr;
    if (!ctx || !r || !out) return SX_E_INVALID;
    if (!decode_args_ok(kind, flags)) { ctx->set_err("decode: a kind other than SX_DECODE_BASE64, SX_DECODE_HEX, SX_DECODE_PERCENT, or a flag other than SX_DECODE_UTF16LE"); return SX_E_INVALID; }
    if (host_only(ctx, "decode")) return SX_E_STATE;
    { const int rc = result_on_device(ctx, r, "decode on the host, with sx_decode_bytes"); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint64_t bytes = 0;
    sx_labels* lab = labels_of(ctx, r, &bytes);
    if (!lab) { ctx->set_err("device decode: no memory for " + std::to_string(bytes) + " bytes of words"); return SX_E_NOMEM; }
    Decode decode(r->r.segs.size(), kind, flags, lab);
    const int rc = select_on_device(ctx, r, decode, out);
    if (rc != SX_OK || !words) sx_labels_free(lab);
    else *words = lab;
    if (rc == SX_OK && info) *info = decode.info;
    return rc;
}

static constexpr MeasureClg kMeasureClgHost = measure_clg_table();

int sx_measure_bytes(const uint8_t* s, uint64_t len, uint32_t flags, uint64_t* word) {
    if (word) *word = 0;
    if ((!s && len) || !word || flags != 0 || len >> 32) return SX_E_INVALID;
    *word = measure_string_host(s, (uint32_t)len, kMeasureClgHost.v);
    return SX_OK;
}

// What the strings look like, where the findings lie (sx_measure_dev.hip): the words' memory is had as the labels' is, then the call's
// own tables — [the totals and the cursor: 256 bytes][the list of the longest segment's records] in sx_ctx::d_distinct, which grows on
// demand and is no selection block —, then one launch per segment on the selections' stream, the list used by one segment after the
// other, and one read of the totals.
int sx_result_measure_device(sx_ctx* ctx, const sx_result* r, uint32_t flags, sx_labels** out, sx_measure_info* info) {
    if (out) *out = nullptr;
    if (!ctx || !r || !out) return SX_E_INVALID;
    if (flags != 0) { ctx->set_err("measure: no flag is defined yet"); return SX_E_INVALID; }
    if (host_only(ctx, "measure")) return SX_E_STATE;
    { const int rc = result_on_device(ctx, r, "measure on the host, with sx_measure_bytes"); if (rc != SX_OK) return rc; }
    uint64_t longest = 0;
    for (const MissionFindings& s : r->r.segs) {
        if (s.ext_nf >> 32) { ctx->set_err("measure: a segment of 2^32 findings or more"); return SX_E_INVALID; }
        longest = s.ext_nf > longest ? s.ext_nf : longest;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    uint64_t bytes = 0, tot[kMeasureTotals] = { 0, 0, 0, 0, 0 };
    const uint64_t table_bytes = 256 + up256(longest * sizeof(uint32_t));
    sx_labels* lab = labels_of(ctx, r, &bytes);
    if (!lab || !device_room(&ctx->d_distinct, &ctx->d_distinct_cap, table_bytes)) {
        ctx->set_err("device measure: no memory for " + std::to_string(bytes) + " bytes of words and " + std::to_string(table_bytes) + " bytes of tables");
        sx_labels_free(lab);
        return SX_E_NOMEM;
    }
    uint8_t* const tab = ctx->d_distinct;
    hipError_t e = hipMemsetAsync(tab, 0, 256, st);
    for (size_t i = 0; e == hipSuccess && i < lab->segs.size(); i++) {
        MeasureParams p = params_of<MeasureParams>(seg_ref(r->r.segs[i]));
        p.labels = (uint64_t*)lab->segs[i].d; p.totals = (uint64_t*)tab; p.cursor = (uint64_t*)tab + kMeasureTotals; p.list = (uint32_t*)(tab + 256);
        e = measure_launch(p, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(tot, tab, sizeof tot, hipMemcpyDeviceToHost, st);
    { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sx_labels_free(lab);
        ctx->set_err(std::string("device measure: ") + hipGetErrorString(e));
        return SX_E_HIP;
    }
    if (info) *info = sx_measure_info{ tot[kMeasureFindings], tot[kMeasureBytes], tot[kMeasureChars], tot[kMeasureWide], tot[kMeasureAscii] };
    *out = lab;
    return SX_OK;
}

// The approximate match (sx_fuzzy_build.hpp, sx_fuzzy_core.hpp, sx_fuzzy_dev.hip): the set, its counters, the words of a result, and
// the same lane code for one string on the host
int sx_fuzzy_set_reset(sx_fuzzy_set* set) {
    if (!set) return SX_E_INVALID;
    return reset_counters(set->device, set->dev.findings, set->dev.first, kLabelBits);
}

int sx_fuzzy_set_create(sx_ctx* ctx, const sx_pattern* patterns, const uint8_t* max_errors, uint32_t n_patterns, uint32_t flags, sx_fuzzy_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !patterns || !max_errors || !out) return SX_E_INVALID;
    FuzzyTable T;
    std::string err;
    { const int rc = fuzzy_build(patterns, max_errors, n_patterns, flags, &T, &err); if (rc != SX_OK) { ctx->set_err("fuzzy set: " + err); return rc; } }
    const size_t eq_bytes = T.eq.size() * sizeof(uint64_t), lenk_bytes = n_patterns * sizeof(uint32_t), counters = kLabelBits * sizeof(uint64_t);
    uint8_t* mem = nullptr;
    size_t at[4];
    { const int rc = upload_set(ctx, "fuzzy set", { { T.map, sizeof T.map, 16 }, { T.eq.data(), eq_bytes, 16 }, { T.lenk, lenk_bytes, 8 } }, 2 * counters, &mem, at);
      if (rc != SX_OK) return rc; }
    sx_fuzzy_set* set = new_handle<sx_fuzzy_set>(ctx, mem);
    if (!set) return SX_E_NOMEM;
    set->dev = FuzzyDevice{ (const uint16_t*)mem, (const uint64_t*)(mem + at[1]), (const uint32_t*)(mem + at[2]), (uint64_t*)(mem + at[3]),
                            (uint64_t*)(mem + at[3] + counters), T.n_patterns, T.classes, T.lds_classes, T.max_len };
    set->info = sx_fuzzy_set_info{ T.n_patterns, T.classes, T.lds_classes, T.nocase, (uint64_t)(sizeof T.map + eq_bytes + lenk_bytes), T.max_len, T.max_errors };
    if (sx_fuzzy_set_reset(set) != SX_OK) { ctx->set_err("fuzzy set: the counters could not be reset"); sx_fuzzy_set_free(set); return SX_E_HIP; }
    *out = set;
    return SX_OK;
}
int sx_fuzzy_set_info_get(const sx_fuzzy_set* set, sx_fuzzy_set_info* out) { return handle_info(set, out); }
void sx_fuzzy_set_free(sx_fuzzy_set* set) { handle_free(set); }

int sx_fuzzy_set_read(const sx_fuzzy_set* set, uint64_t* findings, uint64_t* first, uint32_t n_patterns) {
    if (!set || n_patterns != set->info.n_patterns) return SX_E_INVALID;
    const int rc = read_counters(set->device, set->dev.findings, findings, n_patterns);
    return rc != SX_OK ? rc : read_counters(set->device, set->dev.first, first, n_patterns);
}

int sx_fuzzy_set_counters_device(const sx_fuzzy_set* set, const uint64_t** d_findings, const uint64_t** d_first) {
    if (!set) return SX_E_INVALID;
    if (d_findings) *d_findings = set->dev.findings;
    if (d_first) *d_first = set->dev.first;
    return SX_OK;
}

int sx_result_fuzzy_device(sx_ctx* ctx, const sx_result* r, sx_fuzzy_set* set, uint64_t ordinal_base, sx_labels** out) {
    return set_words_on_device<FuzzyParams>(ctx, r, set, ordinal_base, out, { "approximate match", "the fuzzy set lies", "match on the host", "fuzzy", "words" }, fuzzy_launch);
}

int sx_fuzzy_bytes(const sx_pattern* patterns, const uint8_t* max_errors, uint32_t n_patterns, uint32_t flags, const uint8_t* s, uint64_t len, uint64_t* word) {
    if (word) *word = 0;
    if ((!s && len) || !word || len >> 32) return SX_E_INVALID;
    FuzzyTable T;
    { const int rc = fuzzy_build(patterns, max_errors, n_patterns, flags, &T, nullptr); if (rc != SX_OK) return rc; }
    const FuzzyDevice dev{ T.map, T.eq.data(), T.lenk, nullptr, nullptr, T.n_patterns, T.classes, T.lds_classes, T.max_len };
    *word = fuzzy_string_host(dev, s, (uint32_t)len);
    return SX_OK;
}

int sx_labels_rebind(sx_ctx* ctx, const sx_labels* labels, const sx_result* to, sx_labels** out) {
    if (out) *out = nullptr;
    if (!ctx || !labels || !to || !out) return SX_E_INVALID;
    if (host_only(ctx, "labels")) return SX_E_STATE;
    if (on_another_device(ctx, *labels, "the labels lie")) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, to, "label on the host"); if (rc != SX_OK) return rc; }
    bool same = labels->segs.size() == to->r.segs.size();
    for (size_t i = 0; same && i < labels->segs.size(); i++) same = labels->segs[i].n == to->r.segs[i].ext_nf;
    if (!same) { ctx->set_err("rebind: the result has other segments or other record counts than the labels' source"); return SX_E_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    uint64_t bytes = 0;
    sx_labels* lab = labels_of(ctx, to, &bytes);
    if (!lab) {
        ctx->set_err("rebind: no memory for " + std::to_string(bytes) + " bytes of labels");
        return SX_E_NOMEM;
    }
    // (the same record counts: the same layout, an array per segment, each 256-byte aligned)
    hipError_t e = bytes ? hipMemcpyAsync(lab->mem, labels->mem, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        sx_labels_free(lab);
        ctx->set_err(std::string("rebind: ") + hipGetErrorString(e));
        return SX_E_HIP;
    }
    *out = lab;
    return SX_OK;
}

int sx_result_distinct_device(sx_ctx* ctx, const sx_result* r, uint32_t flags, sx_labels** out, sx_distinct_info* info) {
    if (out) *out = nullptr;
    if (!ctx || !r || !out) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SELECT_ASCII_NOCASE) { ctx->set_err("distinct: flags other than SX_SELECT_ASCII_NOCASE"); return SX_E_INVALID; }
    return distinct_on_device(ctx, r, flags & SX_SELECT_ASCII_NOCASE ? 1u : 0u, "distinct", out, info, nullptr);
}

int sx_seen_set_reset(sx_seen_set* set) {
    if (!set) return SX_E_INVALID;
    if (hipSetDevice(set->device) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    hipError_t e = hipMemset(set->mem, 0, kSeenHeadBytes);                                  // the cursors (and the totals of a call)
    if (e == hipSuccess) e = hipMemset(set->dev.slots, 0xFF, sizeof(uint64_t) << set->dev.table_log2);
    if (e == hipSuccess && set->dev.counts) e = hipMemset(set->dev.counts, 0, sizeof(uint64_t) << set->dev.table_log2);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (as reset_counters: the kernels run on a stream that does not wait for this one)
    if (e != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    return SX_OK;
}

// (what sx_seen_set_create, _grow and _import ask of a set's capacities)
static bool seen_capacity_refused(sx_ctx* ctx, uint64_t capacity_strings, uint64_t capacity_bytes) {
    if (capacity_strings != 0 && capacity_strings <= kSeenMaxCapacity && capacity_bytes <= kSeenMaxCapacity) return false;
    ctx->set_err("seen set: a capacity of " + std::to_string(capacity_strings) + " strings and " + std::to_string(capacity_bytes) + " bytes: at least one string, 2^40 of either at most");
    return true;
}

// An empty set of checked capacities on the context's device (nocase: 0 / 1; counted: it gets count words)
static int seen_set_make(sx_ctx* ctx, uint64_t capacity_strings, uint64_t capacity_bytes, uint32_t nocase, uint32_t tag_bits, bool counted, sx_seen_set** out) {
    uint32_t table_log2 = 1;
    while (((uint64_t)1 << table_log2) < 2 * capacity_strings) table_log2++;
    const uint64_t table_bytes = sizeof(uint64_t) << table_log2, at_arena = kSeenHeadBytes + up256(table_bytes), at_counts = at_arena + up256(capacity_bytes ? capacity_bytes : 1),
                   bytes = at_counts + (counted ? up256(table_bytes) : 0u);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint8_t* mem = nullptr;
    if (hipMalloc((void**)&mem, bytes) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_err("seen set: no device memory for " + std::to_string(bytes) + " bytes of slots and entries");
        return SX_E_NOMEM;
    }
    sx_seen_set* set = new_handle<sx_seen_set>(ctx, mem);
    if (!set) return SX_E_NOMEM;
    set->dev = SeenSet{ (uint64_t*)(mem + kSeenHeadBytes), mem + at_arena, (uint64_t*)mem, table_log2, tag_bits, nocase, 0u, counted ? (uint64_t*)(mem + at_counts) : nullptr };
    set->info = sx_seen_set_info{ 0, 0, capacity_strings, capacity_bytes, table_log2, set->dev.nocase, set->dev.tag_bits, counted ? 1u : 0u };
    if (sx_seen_set_reset(set) != SX_OK) { ctx->set_err("seen set: the slots could not be emptied"); sx_seen_set_free(set); return SX_E_HIP; }
    *out = set;
    return SX_OK;
}

int sx_seen_set_create(sx_ctx* ctx, uint64_t capacity_strings, uint64_t capacity_bytes, uint32_t flags, sx_seen_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return SX_E_INVALID;
    if (flags & ~(uint32_t)(SX_SELECT_ASCII_NOCASE | SX_SEEN_COUNTED)) { ctx->set_err("seen set: flags other than SX_SELECT_ASCII_NOCASE and SX_SEEN_COUNTED"); return SX_E_INVALID; }
    if (seen_capacity_refused(ctx, capacity_strings, capacity_bytes)) return SX_E_INVALID;
    if (host_only(ctx, "for the seen set")) return SX_E_STATE;
    return seen_set_make(ctx, capacity_strings, capacity_bytes, flags & SX_SELECT_ASCII_NOCASE ? 1u : 0u, (uint32_t)ctx->sw.seen_tag_bits, (flags & SX_SEEN_COUNTED) != 0, out);
}

// (strings and bytes are the cursors, read where they lie)
int sx_seen_set_info_get(const sx_seen_set* set, sx_seen_set_info* out) {
    if (!set || !out) return SX_E_INVALID;
    uint64_t cursors[2];
    { const int rc = read_counters(set->device, set->dev.cursors, cursors, 2); if (rc != SX_OK) return rc; }
    *out = set->info;
    out->strings = cursors[0]; out->bytes = cursors[1];
    return SX_OK;
}
void sx_seen_set_free(sx_seen_set* set) { handle_free(set); }

// The seen set where the findings lie: the distinct pass under the set's fold, as sx_result_distinct_device runs it; then seen_mark_add
// with every segment's mark, every segment's add and, for a set that counts, every segment's count.  On any refusal or error the
// labels are freed.
int sx_result_seen_device(sx_ctx* ctx, const sx_result* r, sx_seen_set* set, uint32_t flags, sx_labels** out, sx_seen_info* info) {
    if (out) *out = nullptr;
    if (!ctx || !r || !set || !out) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SEEN_LOOKUP_ONLY) { ctx->set_err("seen: flags other than SX_SEEN_LOOKUP_ONLY"); return SX_E_INVALID; }
    if (host_only(ctx, "seen")) return SX_E_STATE;
    if (on_another_device(ctx, *set, "the seen set lies")) return SX_E_INVALID;
    sx_labels* lab = nullptr;
    sx_distinct_info di{};
    std::vector<DistinctSeg> segs;
    { const int rc = distinct_on_device(ctx, r, set->dev.nocase, "seen", &lab, &di, &segs); if (rc != SX_OK) return rc; }
    auto pass = [&](int which) {
        for (size_t i = 0; i < segs.size(); i++) {
            SeenParams p;
            memset(&p, 0, sizeof p);
            p.recs = segs[i].recs; p.arena = segs[i].arena; p.n = segs[i].n; p.packed = segs[i].packed;
            p.labels = (uint64_t*)lab->segs[i].d; p.totals = set->dev.cursors + 2; p.set = set->dev;
            const hipError_t pe = which == kSeenCount ? seen_count_launch(p, which, ctx->post_stream) : seen_launch(p, which, ctx->post_stream);
            if (pe != hipSuccess) return pe;
        }
        return hipSuccess;
    };
    const bool add = !(flags & SX_SEEN_LOOKUP_ONLY);
    uint64_t tot[kSeenTotals];
    const int rc = seen_mark_add(ctx, "seen set", "device seen", set->dev, set->info.capacity_strings, set->info.capacity_bytes, add, pass, tot, nullptr, nullptr);
    if (rc != SX_OK) { sx_labels_free(lab); return rc; }
    if (add && set->dev.counts && tot[kSeenClasses] + tot[kSeenNewClasses] != di.distinct) {      // (what the count pass was checked against)
        sx_labels_free(lab);
        ctx->set_err("device seen: " + std::to_string(tot[kSeenClasses] + tot[kSeenNewClasses]) + " classes were counted, the distinct pass found " + std::to_string(di.distinct));
        return SX_E_HIP;
    }
    if (info)
        *info = sx_seen_info{ di.findings, di.distinct, di.repeated, tot[kSeenFindings], tot[kSeenClasses], add ? tot[kSeenNewClasses] : 0u, add ? tot[kSeenNewBytes] : 0u,
                              di.rounds, di.table_log2 };
    *out = lab;
    return SX_OK;
}

// The counts where the findings lie: the words' memory as the labels' is had, then one lookup launch per segment and one read of the
// error total.  No distinct pass: a word depends on its own record and the set alone.
int sx_result_seen_counts_device(sx_ctx* ctx, const sx_result* r, sx_seen_set* set, sx_labels** out) {
    if (out) *out = nullptr;
    if (!ctx || !r || !set || !out) return SX_E_INVALID;
    if (!set->dev.counts) { ctx->set_err("seen counts: the set was made without SX_SEEN_COUNTED"); return SX_E_INVALID; }
    if (host_only(ctx, "seen counts")) return SX_E_STATE;
    if (on_another_device(ctx, *set, "the seen set lies")) return SX_E_INVALID;
    { const int rc = result_on_device(ctx, r, "compare the strings on the host"); if (rc != SX_OK) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->post_stream;
    uint64_t bytes = 0, lost = 0;
    sx_labels* lab = labels_of(ctx, r, &bytes);
    if (!lab) { ctx->set_err("seen counts: no memory for " + std::to_string(bytes) + " bytes of words"); return SX_E_NOMEM; }
    hipError_t e = hipMemsetAsync(set->dev.cursors + 2, 0, kSeenTotals * sizeof(uint64_t), st);
    for (size_t i = 0; e == hipSuccess && i < lab->segs.size(); i++) {
        SeenParams p = params_of<SeenParams>(seg_ref(r->r.segs[i]));
        p.labels = (uint64_t*)lab->segs[i].d; p.totals = set->dev.cursors + 2; p.set = set->dev;
        e = seen_count_launch(p, kSeenCountsLookup, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&lost, set->dev.cursors + 2 + kSeenError, sizeof lost, hipMemcpyDeviceToHost, st);
    { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess || lost) {
        (void)hipGetLastError();
        sx_labels_free(lab);
        ctx->set_err(e != hipSuccess ? std::string("seen counts: ") + hipGetErrorString(e) : std::string("seen counts: a probe walked every slot of the set and met no empty one"));
        return SX_E_HIP;
    }
    *out = lab;
    return SX_OK;
}

// A source of the merge kernels where it lies in HBM (sx_seen_merge_core.hpp)
struct SeenSource {
    const uint64_t* words;
    const uint8_t* arena;
    uint64_t n;
    const uint64_t* counts;      // a count word per source word, or NULL: every entry counts (1, 1).  Read only by a destination that counts
};

// A source into a set: seen_mark_add with the source's one mark launch, one add launch and, into a set that counts, one count launch.  dst, capacity_*: the destination; d_held:
// ceil(src.n / 64) words of scratch; what: the call's name in the messages; held (may be NULL): held[] as mark left it.  *info is
// written for a refused call too: what would have been added.
static int seen_merge_run(sx_ctx* ctx, const char* what, const SeenSet& dst, uint64_t capacity_strings, uint64_t capacity_bytes, const SeenSource& src,
                          uint64_t* d_held, bool add, sx_seen_merge_info* info, std::vector<uint64_t>* held) {
    SeenMergeParams p;
    memset(&p, 0, sizeof p);
    p.words = src.words; p.src_arena = src.arena; p.n = src.n; p.held = d_held; p.totals = dst.cursors + 2; p.set = dst;
    if (held) held->assign((src.n + kSelectRecs - 1) / kSelectRecs, 0);
    uint64_t tot[kSeenTotals];
    const std::string name = std::string("seen set ") + what;
    const int rc = seen_mark_add(ctx, name, name, dst, capacity_strings, capacity_bytes, add, [&](int which) {
        return which == kSeenCount ? seen_merge_count_launch(SeenMergeCountParams{ p, src.counts }, ctx->post_stream) : seen_merge_launch(p, which, ctx->post_stream);
    }, tot, d_held, held);
    if (info) *info = sx_seen_merge_info{ tot[kSeenMergeOccupied], tot[kSeenMergeHeld], add ? tot[kSeenNewClasses] : 0u, add ? tot[kSeenNewBytes] : 0u };
    return rc;
}

// (the scratch of a merge: `bytes` of sx_ctx::d_distinct, which is no selection block)
static int seen_merge_room(sx_ctx* ctx, const char* what, uint64_t bytes) {
    if (device_room(&ctx->d_distinct, &ctx->d_distinct_cap, bytes)) return SX_OK;
    ctx->set_err(std::string("seen set ") + what + ": no device memory for " + std::to_string(bytes) + " bytes of scratch");
    return SX_E_NOMEM;
}

// A source the host built — n words, and the arena_bytes of entries they point into — uploaded behind held[] and put into `set`.
// counts (may be NULL: (1, 1) each): n count words, uploaded behind the entries if the set counts
static int seen_merge_list(sx_ctx* ctx, const char* what, sx_seen_set* set, const uint64_t* words, uint64_t n, const uint8_t* arena, uint64_t arena_bytes,
                           const uint64_t* counts, bool add, sx_seen_merge_info* info, std::vector<uint64_t>* held) {
    if (info) *info = sx_seen_merge_info{ 0, 0, 0, 0 };
    if (held) held->clear();
    if (n == 0) return SX_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t at_words = up256((n + kSelectRecs - 1) / kSelectRecs * sizeof(uint64_t)), at_arena = at_words + up256(n * sizeof(uint64_t));
    if (!set->dev.counts || !add) counts = nullptr;
    const uint64_t at_counts = at_arena + up256(arena_bytes);
    { const int rc = seen_merge_room(ctx, what, at_counts + (counts ? up256(n * sizeof(uint64_t)) : 0u)); if (rc != SX_OK) return rc; }
    uint8_t* const d = ctx->d_distinct;
    HIP_TRY(ctx, hipMemcpy(d + at_words, words, n * sizeof(uint64_t), hipMemcpyHostToDevice));      // (done when they return: the kernels' stream need not wait)
    HIP_TRY(ctx, hipMemcpy(d + at_arena, arena, arena_bytes, hipMemcpyHostToDevice));
    if (counts) HIP_TRY(ctx, hipMemcpy(d + at_counts, counts, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    return seen_merge_run(ctx, what, set->dev, set->info.capacity_strings, set->info.capacity_bytes,
                          SeenSource{ (const uint64_t*)(d + at_words), d + at_arena, n, counts ? (const uint64_t*)(d + at_counts) : nullptr }, (uint64_t*)d, add, info, held);
}

// A set's slot table as the source
static int seen_merge_set(sx_ctx* ctx, const char* what, const SeenSet& dst, uint64_t capacity_strings, uint64_t capacity_bytes, const sx_seen_set* src, bool add,
                          sx_seen_merge_info* info) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t n = (uint64_t)1 << src->dev.table_log2;
    { const int rc = seen_merge_room(ctx, what, up256((n + kSelectRecs - 1) / kSelectRecs * sizeof(uint64_t))); if (rc != SX_OK) return rc; }
    return seen_merge_run(ctx, what, dst, capacity_strings, capacity_bytes, SeenSource{ src->dev.slots, src->dev.arena, n, src->dev.counts }, (uint64_t*)ctx->d_distinct, add, info, nullptr);
}

int sx_seen_set_merge(sx_ctx* ctx, sx_seen_set* dst, const sx_seen_set* src, uint32_t flags, sx_seen_merge_info* info) {
    if (!ctx || !dst || !src) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SEEN_LOOKUP_ONLY) { ctx->set_err("seen set merge: flags other than SX_SEEN_LOOKUP_ONLY"); return SX_E_INVALID; }
    if (dst == src) { ctx->set_err("seen set merge: a set into itself"); return SX_E_INVALID; }
    if (dst->dev.nocase != src->dev.nocase) { ctx->set_err("seen set merge: the sets fold differently"); return SX_E_INVALID; }
    if (host_only(ctx, "for a seen set's merge")) return SX_E_STATE;
    if (on_another_device(ctx, *dst, "the seen set lies") || on_another_device(ctx, *src, "the source set lies")) return SX_E_INVALID;
    return seen_merge_set(ctx, "merge", dst->dev, dst->info.capacity_strings, dst->info.capacity_bytes, src, !(flags & SX_SEEN_LOOKUP_ONLY), info);
}

int sx_seen_set_grow(sx_ctx* ctx, sx_seen_set* set, uint64_t capacity_strings, uint64_t capacity_bytes) {
    if (!ctx || !set) return SX_E_INVALID;
    if (seen_capacity_refused(ctx, capacity_strings, capacity_bytes)) return SX_E_INVALID;
    if (host_only(ctx, "for a seen set's growth")) return SX_E_STATE;
    if (on_another_device(ctx, *set, "the seen set lies")) return SX_E_INVALID;
    uint64_t cursors[2];
    { const int rc = read_counters(set->device, set->dev.cursors, cursors, 2); if (rc != SX_OK) { ctx->set_err("seen set grow: the cursors could not be read"); return rc; } }
    if (cursors[0] > capacity_strings || cursors[1] > capacity_bytes) {
        ctx->set_err("seen set grow: the set holds " + std::to_string(cursors[0]) + " strings and " + std::to_string(cursors[1]) + " bytes, more than the new capacity of "
                     + std::to_string(capacity_strings) + " and " + std::to_string(capacity_bytes));
        return SX_E_INVALID;
    }
    sx_seen_set* fresh = nullptr;
    { const int rc = seen_set_make(ctx, capacity_strings, capacity_bytes, set->dev.nocase, set->dev.tag_bits, set->dev.counts != nullptr, &fresh); if (rc != SX_OK) return rc; }
    sx_seen_merge_info mi{};
    int rc = seen_merge_set(ctx, "grow", fresh->dev, capacity_strings, capacity_bytes, set, true, &mi);
    if (rc == SX_OK && (mi.source_strings != cursors[0] || mi.added_strings != cursors[0] || mi.added_bytes != cursors[1])) {
        ctx->set_err("seen set grow: the set's table holds " + std::to_string(mi.source_strings) + " entries, its cursors say " + std::to_string(cursors[0]));
        rc = SX_E_HIP;
    }
    if (rc != SX_OK) { sx_seen_set_free(fresh); return rc; }
    std::swap(set->mem, fresh->mem);
    set->dev = fresh->dev; set->info = fresh->info;
    sx_seen_set_free(fresh);       // (the old memory)
    return SX_OK;
}

int sx_seen_set_export_size(const sx_seen_set* set, uint64_t* bytes) {
    if (!set || !bytes) return SX_E_INVALID;
    uint64_t cursors[2];
    { const int rc = read_counters(set->device, set->dev.cursors, cursors, 2); if (rc != SX_OK) return rc; }
    *bytes = kSeenBlobHeaderBytes + cursors[1] + (set->dev.counts ? 8u * cursors[0] : 0u);
    return SX_OK;
}

int sx_seen_set_export(const sx_seen_set* set, void* buf, uint64_t cap, uint64_t* written) {
    if (written) *written = 0;
    if (!set || !buf || !written) return SX_E_INVALID;
    uint64_t cursors[2];
    { const int rc = read_counters(set->device, set->dev.cursors, cursors, 2); if (rc != SX_OK) return rc; }
    const bool counted = set->dev.counts != nullptr;
    const uint64_t size = kSeenBlobHeaderBytes + cursors[1] + (counted ? 8u * cursors[0] : 0u);
    if (cap < size) return SX_E_INVALID;
    uint8_t* const area = (uint8_t*)buf + kSeenBlobHeaderBytes;
    if (cursors[1] && hipMemcpy(area, set->dev.arena, cursors[1], hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
    if (counted) {
        // the count words in the order the entries lie in the area: the slot and count tables as they lie, the occupied slots' (entry
        // offset, count) pairs sorted by offset on the host
        try {
            const uint64_t slots = (uint64_t)1 << set->dev.table_log2;
            std::vector<uint64_t> words(slots), counts(slots);
            if (hipMemcpy(words.data(), set->dev.slots, slots * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess
                || hipMemcpy(counts.data(), set->dev.counts, slots * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return SX_E_HIP; }
            std::vector<std::pair<uint64_t, uint64_t>> by_offset;
            for (uint64_t k = 0; k < slots; k++)
                if (words[k] != kSeenEmpty) by_offset.emplace_back(words[k] & (((uint64_t)1 << kSeenOffsetBits) - 1u), counts[k]);
            if (by_offset.size() != cursors[0]) return SX_E_HIP;      // (the table holds what the cursor says)
            std::sort(by_offset.begin(), by_offset.end());
            for (uint64_t k = 0; k < by_offset.size(); k++) memcpy(area + cursors[1] + 8u * k, &by_offset[k].second, 8);      // (little-endian hosts, as everywhere here)
        } catch (const std::exception&) {
            return SX_E_NOMEM;
        }
    }
    seen_blob_header((uint8_t*)buf, set->dev.nocase, cursors[0], area, cursors[1], counted ? SX_SEEN_BLOB_VERSION_COUNTED : SX_SEEN_BLOB_VERSION);
    *written = size;
    return SX_OK;
}

int sx_seen_blob_info_get(const void* blob, uint64_t len, sx_seen_blob_info* out) {
    if (!blob || !out) return SX_E_INVALID;
    std::string why;
    return seen_blob_check(blob, len, out, nullptr, &why);
}

int sx_seen_set_import(sx_ctx* ctx, const void* blob, uint64_t len, uint64_t capacity_strings, uint64_t capacity_bytes, sx_seen_set** out) {
    if (out) *out = nullptr;
    if (!ctx || !blob || !out) return SX_E_INVALID;
    if (host_only(ctx, "for the seen set")) return SX_E_STATE;
    sx_seen_blob_info bi{};
    std::vector<uint64_t> words, counts;
    std::string why;
    { const int rc = seen_blob_check(blob, len, &bi, &words, &why, &counts); if (rc != SX_OK) { ctx->set_err("seen set import: " + why); return rc; } }
    if (capacity_strings == 0) capacity_strings = bi.strings ? bi.strings : 1;
    if (capacity_bytes == 0) capacity_bytes = bi.bytes;
    if (capacity_strings < bi.strings || capacity_bytes < bi.bytes) {
        ctx->set_err("seen set import: the blob holds " + std::to_string(bi.strings) + " strings and " + std::to_string(bi.bytes) + " bytes, more than the capacity of "
                     + std::to_string(capacity_strings) + " and " + std::to_string(capacity_bytes));
        return SX_E_INVALID;
    }
    if (seen_capacity_refused(ctx, capacity_strings, capacity_bytes)) return SX_E_INVALID;
    sx_seen_set* set = nullptr;
    const bool counted = bi.version == SX_SEEN_BLOB_VERSION_COUNTED;
    { const int rc = seen_set_make(ctx, capacity_strings, capacity_bytes, bi.nocase, (uint32_t)ctx->sw.seen_tag_bits, counted, &set); if (rc != SX_OK) return rc; }
    sx_seen_merge_info mi{};
    int rc = seen_merge_list(ctx, "import", set, words.data(), words.size(), (const uint8_t*)blob + kSeenBlobHeaderBytes, bi.bytes, counted ? counts.data() : nullptr, true, &mi, nullptr);
    if (rc == SX_OK && (mi.added_strings != bi.strings || mi.added_bytes != bi.bytes)) { ctx->set_err("seen set import: not every entry of the blob was added"); rc = SX_E_HIP; }
    if (rc != SX_OK) { sx_seen_set_free(set); return rc; }
    *out = set;
    return SX_OK;
}

int sx_seen_set_add_strings(sx_ctx* ctx, sx_seen_set* set, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t flags, uint8_t* held_out,
                            sx_seen_merge_info* info) {
    if (!ctx || !set) return SX_E_INVALID;
    if (flags & ~(uint32_t)SX_SEEN_LOOKUP_ONLY) { ctx->set_err("seen set add_strings: flags other than SX_SEEN_LOOKUP_ONLY"); return SX_E_INVALID; }
    if (host_only(ctx, "for a seen set's strings")) return SX_E_STATE;
    if (on_another_device(ctx, *set, "the seen set lies")) return SX_E_INVALID;
    std::vector<uint8_t> arena;
    std::vector<uint64_t> words, held;
    std::vector<uint32_t> kept_of;
    std::string why;
    { const int rc = seen_entries_build(bytes, offsets, n, set->dev.nocase, &arena, &words, &kept_of, &why); if (rc != SX_OK) { ctx->set_err("seen set add_strings: " + why); return rc; } }
    // (into a set that counts the list is one result: a kept string was in 1 result, as often as the list has it)
    std::vector<uint64_t> counts;
    if (set->dev.counts && !(flags & SX_SEEN_LOOKUP_ONLY)) {
        try { counts.assign(words.size(), (uint64_t)1 << SX_SEEN_RESULTS_SHIFT); } catch (const std::exception&) { ctx->set_err("seen set add_strings: no host memory for the counts"); return SX_E_NOMEM; }
        for (uint64_t i = 0; i < n; i++) counts[kept_of[i]] = seen_count_sum(counts[kept_of[i]], (uint64_t)1 << SX_SEEN_FINDINGS_SHIFT);
    }
    const int rc = seen_merge_list(ctx, "add_strings", set, words.data(), words.size(), arena.data(), arena.size(), counts.empty() ? nullptr : counts.data(),
                                   !(flags & SX_SEEN_LOOKUP_ONLY), info, held_out ? &held : nullptr);
    if (rc != SX_OK) return rc;
    if (held_out)
        for (uint64_t i = 0; i < n; i++) held_out[i] = (uint8_t)((held[kept_of[i] / kSelectRecs] >> (kept_of[i] % kSelectRecs)) & 1u);
    return SX_OK;
}

}  // extern "C"
