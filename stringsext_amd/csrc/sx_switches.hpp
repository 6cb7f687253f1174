// sx_switches.hpp — every SX_* environment switch of the library: one field per switch, initialised to its default.
//
// Switches::from_env() (sx_switches.cpp) is the only code in this directory that reads the environment.  sx_create calls it once
// and keeps the result in sx_ctx::sw: a switch set or removed AFTER the context exists does nothing (one exception: SX_SCAN_WARM).
// The one entry point without a context that has a switch (sx_shard_splice_segs) calls from_env() itself.
//
// Conventions, as they grew (this table records them, it does not tidy them):
//   presence  the variable's existence switches, its value is not looked at (SX_MISSION_STREAMS=0 turns per-Mission streams ON)
//   on / off  on by default, off only by a value that atoi() reads as 0 (SX_FUSED=0); one that is off by default says so
//   -1 / 0    "unset" where the code tells unset from a value; from_env() applies each switch's own clamp, so a field that is
//             not "unset" holds the value the code uses
// Users: (tests) tests/ and tools/fuzz_case.py set it to reach a code path; (measurements) bench.py / tools/ set it;
// (experiments) nothing in the repository sets it — a knob kept for measuring by hand.
#pragma once
#include <stdint.h>

namespace sx {

struct Switches {
    // ---- context and streams (sx_api.cpp)
    int64_t pin_flags = -1;            // SX_PIN_FLAGS=flags (strtoul, any base): hipHostMalloc flags of sx_ctx::h_pin; -1 unset: hipHostMallocNonCoherent (experiments)
    bool small_copy = true;            // SX_SMALL_COPY on / off: small read-backs by a one-wavefront kernel, not the runtime's blit (experiments)
    int replay_threads = 0;            // SX_REPLAY_THREADS=n (1 .. 256): host threads of stage B, over sx_options::replay_threads; 0 unset (experiments)
    bool result_on_device = false;     // SX_RESULT_ON_DEVICE=1, off by default: sets SX_OPT_RESULT_ON_DEVICE (tests: the flag through the environment)
    int scan_blocks_per_cu = -1;       // SX_SCAN_BLOCKS_PER_CU=n: 1 .. 7 = persistent scan grid of n blocks per CU; -1 unset: 8, every wave slot (tests)
    int64_t region_cap = -1;           // SX_REGION_CAP=n: record slots per sub-chunk in region mode, 0 = never region mode; -1 unset: 64 (tests)
    int scan_cus = 0;                  // SX_SCAN_CUS=n (>= 1): CUs the persistent grid is sized for; 0 unset: the device's (tests: small inputs)
    int prio_n = -1, prio_scan = 0, prio_post = 0;   // SX_PRIO=scan,post: stream priorities; prio_n = fields given (-1 unset: the device's range) (experiments)
    bool mission_streams = false;      // SX_MISSION_STREAMS presence: a scan stream per Mission, as SX_OPT_MISSION_STREAMS; no fused launch (tests, measurements)
    // ---- stage A (sx_stage_a.cpp, sx_fused.hip, sx_kernels.hip)
    uint32_t scan_prio = 0;            // SX_SCAN_PRIO=1: ScanParams::wave_prio, the scan wavefronts raise their issue priority (experiments)
    bool fused = true;                 // SX_FUSED on / off: the Missions the fused kernel holds share one launch (tests)
    int fused_prefilter = -1;          // SX_FUSED_PREFILTER=0 / 2: the fused kernel's prefilter off / on pairs only; anything else: its own choice (tests)
    int scan_warm = -1;                // SX_SCAN_WARM=n: n identical launches in front of each unfused scan launch, and no fused launch; -1 unset.  Two sites,
                                       // presence and count: both are "set, n >= 0".  THE ONE SWITCH READ AFTER sx_create: sx_device_runs refreshes it at its entry
                                       // (and the context keeps that value until the next sx_device_runs), because bench.py sets it on a live context (measurements)
    bool no_large_regions = false;     // SX_NO_LARGE_REGIONS presence: dense input goes to the shared record pool, never to large regions (tests)
    uint32_t device_join_min = 65536;  // SX_DEVICE_JOIN_MIN=n: records from which they are sorted and joined on the device (tests)
    bool no_pieces = false;            // SX_NO_PIECES presence: long runs are not cut into a piece per window (tests)
    uint32_t probe_rot = 0;            // SX_PROBE_ROT=n: sx_device_read_bandwidth's sub-chunk probe starts wavefront w at tile w * n (experiments)
    // ---- stage B, lane per region (sx_stage_b.cpp, sx_replay_dev.hip, sx_sort.hip)
    bool host_replay = false;          // SX_HOST_REPLAY presence: stage B on the host (experiments)
    bool device_replay = false;        // SX_DEVICE_REPLAY presence: stage B on the device whatever the number of runs, as SX_OPT_DEVICE_REPLAY (experiments)
    bool host_stitch = false;          // SX_HOST_STITCH presence: the host decides which regions stand (tests)
    bool no_replay_skip = false;       // SX_NO_REPLAY_SKIP presence: the replay kernels decode every byte, ReplayParams::skip = 0 (tests)
    bool no_grid_bound = false;        // SX_NO_GRID_BOUND presence: the replay does not use stage A's token grid (experiments)
    bool no_replay_cache = false;      // SX_NO_REPLAY_CACHE presence: no pass-1 output cache (tests)
    uint32_t max_region_windows = 0;   // SX_MAX_REGION_WINDOWS=n (>= 1): longer regions go back to the host; 0 unset: kMaxRegionWindowsDefault (tests)
    int64_t replay_cache_mib = -1;     // SX_REPLAY_CACHE_MIB=n: budget of the pass-1 cache; -1 unset: 8 GiB, more for floods of runs (tests)
    bool fast_replay = true;           // SX_FAST_REPLAY on / off: the fast pre-pass of pass 1 (tests)
    int count_waves = 4;               // SX_COUNT_WAVES=4 / 6 / 8: wavefronts per SIMD the cached count kernel is built for (experiments)
    int stitch_block = 0;              // SX_STITCH_BLOCK=n (> 0): runs per block of the stitch; 0 unset: 128, 512 from 2^20 runs on (tests)
    int slabs = 0;                     // SX_SLABS=n (1 .. 64): slabs of the device replay of a Mission that may have them (alone, or busy among quiet ones: sx_stage_b.cpp); 0 unset: from 2^20 runs on 3 for a single Mission, 2 next to other Missions (tests)
    int replay_copy_wgs = 0;           // SX_REPLAY_COPY_WGS=n (> 0): the result copy as a kernel of n workgroups, not the runtime's blit (experiments)
    // ---- the Missions' findings interleaved (sx_merge.cpp device_merge, sx_sort.hip, sx_replay.cpp)
    bool host_merge = false;           // SX_HOST_MERGE presence: interleave on the host (tests)
    bool packed = true;                // SX_PACKED on / off: findings cross PCIe as sx_finding16 (tests)
    uint64_t merge_part_mib = 0;       // SX_MERGE_PART_MIB=n (>= 1): string bytes per part of the device merge; 0 unset: 2048 (tests)
    uint64_t merge_part_findings = 0;  // SX_MERGE_PART_FINDINGS=n (>= 1024): findings per part; 0 unset: 96 Mi (tests)
    int merge_copy_wgs = -1;           // SX_MERGE_COPY_WGS=n: workgroups of a part's copy kernel, 0 = the runtime's blit; -1 unset: 2 when copies overlap kernels (experiments)
    int merge_copy_nt = 1;             // SX_MERGE_COPY_NT=0: the copy kernel's stores are not non-temporal (experiments)
    int merge_copy_threads = 512;      // SX_MERGE_COPY_THREADS=n (64 .. 1024): its block size (experiments)
    uint64_t host_merge_seg_bytes = 0; // SX_HOST_MERGE_SEG_BYTES=n (>= 1): string bytes per segment of the host's interleave; 0 unset: 4 GiB - 16 (tests)
    uint64_t splice_seg_bytes = 0;     // SX_SPLICE_SEG_BYTES=n (>= 1): the same for sx_shard_splice_segs, which has no context and reads it per call; 0 unset: 2 GiB (tests)
    // ---- schedule (sx_schedule.cpp)
    int64_t piece_mib = -1;            // SX_PIECE_MIB=n: a large buffer is scanned in pieces of n MiB, 0 = in one go; -1 unset: two halves from 16 GiB on (tests, measurements)
    int64_t seq_piece_kib = -1;        // SX_SEQ_PIECE_KIB=n: pieces scanned one after the other, n KiB each, 0 = never; wins over _MIB; -1 unset (tests)
    int64_t seq_piece_mib = -1;        // SX_SEQ_PIECE_MIB=n: the same in MiB; -1 unset: sized from the last buffer's output (tests)
    bool debug_entry = false;          // SX_DEBUG_ENTRY presence: prints a double-byte Mission's entry state per buffer (experiments)
    int busiest_last = 0;              // SX_BUSIEST_LAST=1 / 2: the busiest Mission's scan is queued last / second to last (tests)
    uint64_t defer_min_bytes = 256ull << 20;   // SX_DEFER_MIN_BYTES=n: with several Missions, an output from n bytes on stays on the device for the merge (every output does when the merged result is to stay in HBM: SX_OPT_RESULT_ON_DEVICE).  Two
                                       // sites, one meaning: "nm >= 2 ? n : 0" (tests)
    bool wave_threads = true;          // SX_WAVE_THREADS on / off: unscanned string-dense Missions replay on a host thread and stream each (tests)
    int timeline = 0;                  // SX_TIMELINE=1: host-side marks on stderr, g_tl_on (measurements)
    bool timing = false;               // SX_TIMING presence: a line per stage on stderr (measurements)
    bool timing2 = false;              // SX_TIMING2 presence: finer lines, with stream syncs in between (experiments)
    // ---- stage B, wave-cooperative (sx_wave.cpp, sx_mission.cpp)
    int wave_replay = -1;              // SX_WAVE_REPLAY=0 / 1: never / always the wave kernels where they apply; -1 unset: by density (tests)
    bool wave_keep_scan = false;       // SX_WAVE_KEEP_SCAN presence: a Mission on the wave path keeps its stage A (tests)
    uint64_t wave_bytes_per_run = 0;   // SX_WAVE_BYTES_PER_RUN=n: bytes per run below which a buffer counts as dense; 0 unset: per family (experiments)
    int wave_stream_prio = -1;         // SX_WAVE_STREAM_PRIO=0 / 1: a threaded Mission's stream at the lowest / middle priority; anything else: the highest (experiments)
    int wave_batches = 0;              // SX_WAVE_BATCHES=n (1 .. 64): batches of 64 windows per wavefront; 0 unset: by size, 1 .. 8 (tests)
    int wave_slabs = 0;                // SX_WAVE_SLABS=n (1 .. 64): slabs of a single Mission's wave replay; 0 unset: one per 32 MiB, 8 at most (tests)
    bool wave_lut = false;             // SX_WAVE_LUT=1, off by default: the class table also where ranges would do (tests)
    bool wave_desc = true;             // SX_WAVE_DESC on / off: descriptors for the lane-per-finding writer (tests)
    int wave_desc_cap = 0;             // SX_WAVE_DESC_CAP=n (>= 1): descriptors per wavefront, and no "too dense" shortcut; 0 unset (tests)
    bool wave_fail = false;            // SX_WAVE_FAIL presence: the wave replay gives every buffer back (tests of the way back)
    int wave_repair = -1;              // SX_WAVE_REPAIR=0 / n: no repair launches / n at most (>= 1); -1 unset: 48 (tests)
    bool wave_same = true;             // SX_WAVE_SAME on / off: -r inside the wave kernels, Mission::wave_same (tests)
    // ---- device-resident results (sx_result_api.cpp)
    int distinct_table_log2 = -1;      // SX_DISTINCT_TABLE_LOG2=n (0 .. 40): sx_result_distinct_device's table has 2^n slots, 0 = one slot and a round per distinct string; -1 unset: the power of two >= 2 x findings (tests)
    int seen_tag_bits = 24;            // SX_SEEN_TAG_BITS=n (0 .. 24): the tag bits of a slot of a seen set made by this context (sx_seen_set_create), 0 = every occupied slot on a probe's way is compared byte for byte (tests)
    // ---- ingest (sx_ingest.cpp)
    uint64_t scan_stream_mib = 0;      // SX_SCAN_STREAM_MIB=n: sx_scan of >= 2n MiB goes through the chunked ingest pipeline; 0: never (tests)
    bool ingest_mmap = false;          // SX_INGEST_MMAP presence: sx_scan_file maps the file instead of reading it (tests)

    static Switches from_env();
};

}  // namespace sx
