// sx_switches.cpp — the environment, read once: one line per switch, each with the parse it always had (sx_switches.hpp says what they do).
#include "sx_switches.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

namespace sx {

static bool present(const char* name) { return getenv(name) != nullptr; }
static bool on_unless_0(const char* name) { const char* e = getenv(name); return !(e && !atoi(e)); }
static bool on_if_nonzero(const char* name) { const char* e = getenv(name); return e && atoi(e); }
static int int_or(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
static int64_t i64_or(const char* name, int64_t unset) { const char* e = getenv(name); return e ? (int64_t)atoll(e) : unset; }
static int clamped_or(const char* name, int lo, int hi, int unset) { const char* e = getenv(name); return e ? std::max(lo, std::min(hi, atoi(e))) : unset; }
static uint64_t u64_at_least(const char* name, uint64_t lo, uint64_t unset) { const char* e = getenv(name); return e ? std::max<uint64_t>(lo, (uint64_t)atoll(e)) : unset; }

Switches Switches::from_env() {
    Switches s;
    if (const char* e = getenv("SX_PIN_FLAGS")) s.pin_flags = (int64_t)(unsigned)strtoul(e, nullptr, 0);
    s.small_copy = on_unless_0("SX_SMALL_COPY");
    if (const char* e = getenv("SX_REPLAY_THREADS")) s.replay_threads = (int)std::max(1u, std::min(256u, (unsigned)atoi(e)));
    s.result_on_device = on_if_nonzero("SX_RESULT_ON_DEVICE");
    s.scan_blocks_per_cu = int_or("SX_SCAN_BLOCKS_PER_CU", s.scan_blocks_per_cu);
    if (const char* e = getenv("SX_REGION_CAP")) s.region_cap = (int64_t)(uint32_t)atoi(e);
    s.scan_cus = clamped_or("SX_SCAN_CUS", 1, INT32_MAX, s.scan_cus);
    if (const char* e = getenv("SX_PRIO")) s.prio_n = std::max(0, sscanf(e, "%d,%d", &s.prio_scan, &s.prio_post));
    s.mission_streams = present("SX_MISSION_STREAMS");
    s.scan_prio = (uint32_t)int_or("SX_SCAN_PRIO", (int)s.scan_prio);
    s.fused = on_unless_0("SX_FUSED");
    s.fused_prefilter = int_or("SX_FUSED_PREFILTER", s.fused_prefilter);
    s.scan_warm = clamped_or("SX_SCAN_WARM", 0, INT32_MAX, s.scan_warm);
    s.no_large_regions = present("SX_NO_LARGE_REGIONS");
    s.device_join_min = (uint32_t)int_or("SX_DEVICE_JOIN_MIN", (int)s.device_join_min);
    s.no_pieces = present("SX_NO_PIECES");
    s.probe_rot = (uint32_t)int_or("SX_PROBE_ROT", (int)s.probe_rot);
    s.host_replay = present("SX_HOST_REPLAY");
    s.device_replay = present("SX_DEVICE_REPLAY");
    s.host_stitch = present("SX_HOST_STITCH");
    s.no_replay_skip = present("SX_NO_REPLAY_SKIP");
    s.no_grid_bound = present("SX_NO_GRID_BOUND");
    s.no_replay_cache = present("SX_NO_REPLAY_CACHE");
    s.max_region_windows = (uint32_t)clamped_or("SX_MAX_REGION_WINDOWS", 1, INT32_MAX, (int)s.max_region_windows);
    s.replay_cache_mib = i64_or("SX_REPLAY_CACHE_MIB", s.replay_cache_mib);
    s.fast_replay = on_unless_0("SX_FAST_REPLAY");
    s.count_waves = int_or("SX_COUNT_WAVES", s.count_waves);
    s.stitch_block = clamped_or("SX_STITCH_BLOCK", 0, INT32_MAX, s.stitch_block);
    s.slabs = clamped_or("SX_SLABS", 1, 64, s.slabs);
    s.replay_copy_wgs = int_or("SX_REPLAY_COPY_WGS", s.replay_copy_wgs);
    s.host_merge = present("SX_HOST_MERGE");
    s.packed = on_unless_0("SX_PACKED");
    s.merge_part_mib = u64_at_least("SX_MERGE_PART_MIB", 1, s.merge_part_mib);
    s.merge_part_findings = u64_at_least("SX_MERGE_PART_FINDINGS", 1024, s.merge_part_findings);
    s.merge_copy_wgs = int_or("SX_MERGE_COPY_WGS", s.merge_copy_wgs);
    s.merge_copy_nt = int_or("SX_MERGE_COPY_NT", s.merge_copy_nt);
    s.merge_copy_threads = clamped_or("SX_MERGE_COPY_THREADS", 64, 1024, s.merge_copy_threads);
    s.host_merge_seg_bytes = u64_at_least("SX_HOST_MERGE_SEG_BYTES", 1, s.host_merge_seg_bytes);
    s.splice_seg_bytes = u64_at_least("SX_SPLICE_SEG_BYTES", 1, s.splice_seg_bytes);
    s.piece_mib = i64_or("SX_PIECE_MIB", s.piece_mib);
    s.seq_piece_kib = i64_or("SX_SEQ_PIECE_KIB", s.seq_piece_kib);
    s.seq_piece_mib = i64_or("SX_SEQ_PIECE_MIB", s.seq_piece_mib);
    s.debug_entry = present("SX_DEBUG_ENTRY");
    s.busiest_last = int_or("SX_BUSIEST_LAST", s.busiest_last);
    if (const char* e = getenv("SX_DEFER_MIN_BYTES")) s.defer_min_bytes = (uint64_t)atoll(e);
    s.wave_threads = on_unless_0("SX_WAVE_THREADS");
    s.timeline = int_or("SX_TIMELINE", s.timeline);
    s.timing = present("SX_TIMING");
    s.timing2 = present("SX_TIMING2");
    if (const char* e = getenv("SX_WAVE_REPLAY")) s.wave_replay = atoi(e) != 0;
    s.wave_keep_scan = present("SX_WAVE_KEEP_SCAN");
    if (const char* e = getenv("SX_WAVE_BYTES_PER_RUN")) s.wave_bytes_per_run = (uint64_t)atoll(e);
    s.wave_stream_prio = int_or("SX_WAVE_STREAM_PRIO", s.wave_stream_prio);
    s.wave_batches = clamped_or("SX_WAVE_BATCHES", 1, 64, s.wave_batches);
    s.wave_slabs = clamped_or("SX_WAVE_SLABS", 1, 64, s.wave_slabs);
    s.wave_lut = on_if_nonzero("SX_WAVE_LUT");
    s.wave_desc = on_unless_0("SX_WAVE_DESC");
    s.wave_desc_cap = clamped_or("SX_WAVE_DESC_CAP", 1, INT32_MAX, s.wave_desc_cap);
    s.wave_fail = present("SX_WAVE_FAIL");
    if (const char* e = getenv("SX_WAVE_REPAIR")) s.wave_repair = atoi(e) ? std::max(1, atoi(e)) : 0;
    s.wave_same = on_unless_0("SX_WAVE_SAME");
    s.distinct_table_log2 = clamped_or("SX_DISTINCT_TABLE_LOG2", 0, 40, s.distinct_table_log2);
    s.seen_tag_bits = clamped_or("SX_SEEN_TAG_BITS", 0, 24, s.seen_tag_bits);
    if (const char* e = getenv("SX_SCAN_STREAM_MIB")) s.scan_stream_mib = (uint64_t)atoll(e);
    s.ingest_mmap = present("SX_INGEST_MMAP");
    return s;
}

}  // namespace sx
