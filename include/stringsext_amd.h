/*
 * stringsext_amd.h — C-ABI of the MI355X-native replacement for stringsext's
 * per-Mission byte-stream scan.
 *
 * The reference (getreu/stringsext v2.3.5, Rust) has no FFI layer; its seam is
 *
 *     FindingCollection::from(ss: &mut ScannerState, input_file_id: Option<u8>,
 *                             input_buffer: &[u8], is_last_input_buffer: bool)
 *         -> Pin<Box<FindingCollection>>                 src/finding_collection.rs:84-89
 *
 * called once per Mission per 4096-byte slice from the loop in
 * src/main.rs:153-168 and drained by the merger in src/main.rs:118-136.  A
 * 4 KiB call is useless for a GPU, so this library replaces that LOOP for one
 * large chunk of one input file: sx_scan() returns exactly the findings the
 * loop would have pushed to the merger for the chunk's slices, already in the
 * merger's order, and carries the same state between calls that ScannerState
 * carries between slices (src/scanner.rs:40-69).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative SX_E_* code, with text from sx_last_error(); the
 * caller owns inputs, the library owns sx_result until sx_result_free(); a
 * context is bound to ONE HIP device and is not thread-safe; internally the
 * Missions are scanned by ONE fused kernel that reads the buffer once where
 * their classifiers allow (round 6, csrc/sx_fused.hip; else their scan kernels
 * queue up in one HIP stream) and everything after them
 * (records -> runs, the exact replay, copies) runs in a second one
 * (SX_OPT_MISSION_STREAMS: a scan stream per Mission, the reference's one
 * thread per Mission, src/main.rs:97,151).  There is no CPU fallback: without
 * a HIP device sx_create() fails with SX_E_NO_DEVICE.
 */
#ifndef STRINGSEXT_AMD_H
#define STRINGSEXT_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct of this header changes size or layout or an enum value changes meaning (2: sx_stats grew by the wave /
 * re-scan / piece fields in round 3, SX_ENC_ISO_2022_JP was added; packed findings, round 4; 4: sx_stats grew by the fused scan's fields,
 * round 6).  A consumer compares it with
 * sx_abi_version() before it hands the library a struct to fill. */
#define SX_ABI_VERSION 4

enum {
    SX_OK = 0,
    SX_E_INVALID = -1,     /* bad argument / unsupported mission */
    SX_E_NO_DEVICE = -2,   /* no usable HIP device: the product never runs on the CPU */
    SX_E_HIP = -3,         /* a HIP call failed */
    SX_E_NOMEM = -4,
    SX_E_STATE = -5,       /* call not valid for this context (e.g. device scan on a host-only ctx) */
    SX_E_HALO = -6         /* sx_scan_shard*: the buffer must begin further in front of own_lo (Big5 / EUC-JP: no byte outside
                              the lead range lies between the buffer start and own_lo, so its token grid is unknown) */
};

/* Encoding ids == `Encoding::name()` of encoding_rs as used at src/mission.rs:681,
 * src/finding.rs:147.  "ascii" is x-user-defined + print_encoding_as_ascii
 * (src/mission.rs:675-679). */
enum {
    SX_ENC_X_USER_DEFINED = 0, SX_ENC_UTF8 = 1, SX_ENC_UTF16LE = 2, SX_ENC_UTF16BE = 3,
    SX_ENC_KOI8_R = 16, SX_ENC_IBM866 = 17, SX_ENC_ISO_8859_2 = 18, SX_ENC_ISO_8859_5 = 19,
    SX_ENC_ISO_8859_15 = 20, SX_ENC_WINDOWS_1251 = 21, SX_ENC_WINDOWS_1252 = 22,
    /* the rest of the WHATWG single-byte set (tables: csrc/gen_tables.py; parity unpinned) */
    SX_ENC_ISO_8859_3 = 23, SX_ENC_ISO_8859_4 = 24, SX_ENC_ISO_8859_6 = 25, SX_ENC_ISO_8859_7 = 26,
    SX_ENC_ISO_8859_8 = 27, SX_ENC_ISO_8859_8_I = 28, SX_ENC_ISO_8859_10 = 29,
    SX_ENC_ISO_8859_13 = 30, SX_ENC_ISO_8859_14 = 31, SX_ENC_ISO_8859_16 = 32, SX_ENC_KOI8_U = 33,
    SX_ENC_MACINTOSH = 34, SX_ENC_WINDOWS_874 = 35, SX_ENC_WINDOWS_1250 = 36,
    SX_ENC_WINDOWS_1253 = 37, SX_ENC_WINDOWS_1254 = 38, SX_ENC_WINDOWS_1255 = 39,
    SX_ENC_WINDOWS_1256 = 40, SX_ENC_WINDOWS_1257 = 41, SX_ENC_WINDOWS_1258 = 42,
    SX_ENC_X_MAC_CYRILLIC = 43,
    /* legacy multi-byte (tables: csrc/gen_tables.py; parity unpinned): a pending lead byte is the decoder state */
    SX_ENC_BIG5 = 64, SX_ENC_EUC_JP = 65, SX_ENC_SHIFT_JIS = 66, SX_ENC_EUC_KR = 67,
    SX_ENC_GB18030 = 68, SX_ENC_GBK = 69,   /* one decoder (four-byte tokens too), two names */
    /* the "replacement" encoding (ISO-2022-KR, ISO-2022-CN, HZ-GB-2312): its decoder reports one error and nothing else */
    SX_ENC_REPLACEMENT = 70,
    /* ISO-2022-JP: escape sequences select the character set, so the meaning of a byte depends on unbounded history: a Mission
     * with it is ONE sequential pass on the host (never on the device, never sharded) */
    SX_ENC_ISO_2022_JP = 71
};

/* `Precision` — src/finding.rs:34-46 */
enum { SX_PRECISION_BEFORE = 0, SX_PRECISION_EXACT = 1, SX_PRECISION_AFTER = 2 };

/* The fields of `Mission` the scan reads — src/mission.rs:382-421; `filter` is
 * `Utf8Filter{af: u128, ubf: u64, grep_char: Option<u8>}` (src/mission.rs:307-327). */
typedef struct sx_mission {
    uint8_t  mission_id;
    uint8_t  encoding;                   /* SX_ENC_* */
    uint8_t  chars_min_nb;
    uint8_t  require_same_unicode_block;
    int16_t  grep_char;                  /* -1 = None */
    uint8_t  print_encoding_as_ascii;
    uint8_t  reserved;
    uint32_t output_line_char_nb_max;
    uint64_t af_lo, af_hi;
    uint64_t ubf;
    uint64_t counter_offset;
} sx_mission;

/* `Finding` — src/finding.rs:51-74 (`s` = arena[str_off .. str_off+str_len], UTF-8). */
typedef struct sx_finding {
    uint64_t position;
    uint32_t str_off, str_len;
    uint8_t  precision;
    uint8_t  completes_previous;         /* s_completes_previous_s */
    uint8_t  mission_id;
    uint8_t  reserved;
    int16_t  input_file_id;              /* Option<u8>: -1 = None */
    uint16_t reserved2;
    uint32_t slice_index;                /* 4 KiB slice of this chunk that produced it */
} sx_finding;

/* The same finding in 16 bytes, as string-dense results cross PCIe (round 4): `-e ascii -n 4` on a binary yields a finding per 85
 * bytes, BASELINE config 5 411 M of them per 64 GiB — such scans are bound by moving the records to the host, and half of sx_finding
 * is the same for every record of a segment (input_file_id), follows from the others (slice_index = slice_base + (position -
 * position of the segment's buffer byte 0 for that Mission) / 4096) or is padding.  Segments whose findings were written by the
 * device's dense paths (the wave-cooperative stage B of a single Mission, the device-side merger of several) are stored this way;
 * sx_result_segment_packed() hands them out as they are, sx_result_segment() expands them to sx_finding on first use, and
 * sx_print_findings() reads either. */
typedef struct sx_finding16 {
    uint64_t position;
    uint32_t str_off;
    uint16_t str_len;
    uint8_t  flags;                      /* bits 0-1: precision (SX_PRECISION_*), bit 2: completes_previous */
    uint8_t  mission_id;
} sx_finding16;
typedef struct sx_segment_info {         /* what the records of one packed segment share */
    int32_t  packed;                     /* 1: the segment's records are sx_finding16, 0: sx_finding */
    int32_t  input_file_id;
    uint32_t slice_base;                 /* slice_index of the segment's buffer byte 0 */
    uint32_t reserved;
    uint64_t position0[256];             /* by mission_id: `position` of the segment's buffer byte 0 (counter_offset + bytes consumed before it) */
} sx_segment_info;

/* Device run record: one maximal stretch of bytes belonging to valid,
 * filter-accepted characters (ignoring -g / -r), with its character count.
 * (Inside the library a run that crosses window starts may travel as several pieces, one per window: a piece
 * that begins at a window start has bit 63 of `chars` set and, in the low bits, its distance from the run's start.
 * sx_device_runs never returns pieces; sx_replay_runs accepts them.) */
typedef struct sx_run {
    uint64_t start;                      /* byte offset of the first byte, chunk relative */
    uint64_t end;                        /* one past the last byte */
    uint64_t chars;
} sx_run;

typedef struct sx_stats {
    uint64_t bytes_scanned;              /* input bytes x missions examined on the device */
    uint64_t run_records;                /* long-run records the device reported (all missions) */
    uint64_t replay_bytes;               /* input bytes the host replayed (all missions) */
    uint64_t findings;
    double   kernel_ms[16];              /* per mission: device scan kernel, HIP events on its stream */
    double   device_ms;                  /* all mission streams, first launch -> last completion */
    double   h2d_ms, d2h_ms, replay_ms, total_ms;
    uint64_t heavy_tiles;                /* 1 KiB tiles that needed the general cross-lane path (all missions) */
    uint64_t wave_windows;               /* decoder-input windows replayed by the wave-cooperative stage B (all missions) */
    double   wave_count_ms, wave_write_ms; /* ... its two passes, HIP events around their launches (all missions and slabs) */
    uint64_t rescans;                    /* scan kernels launched a second time (their records overflowed the regions / the pool) */
    double   rescan_ms;                  /* ... host time until their records were there */
    uint64_t wave_desc_overflows;        /* wave stage B: slabs written by the window-parallel writer because a wavefront found more than its descriptors hold */
    uint64_t seq_pieces;                 /* pieces a buffer with gigabytes of output was scanned in, one after the other (0: in one go) */
    uint64_t fast_regions;               /* (ABI 3) stage B, lane per region: regions settled by the fast pre-pass (one run inside one window) ... */
    uint64_t general_regions;            /* ... and regions it left to the general replay kernel */
    uint64_t wave_repairs;               /* (ABI 3) wave stage B: count launches repeated for wavefronts whose warm-up windows gave them a wrong entry state (-g) */
    double   fused_ms;                   /* (ABI 4) fused scan launches (one read of the buffer for several Missions), HIP events around them; kernel_ms[k] of
                                            every Mission such a launch scanned holds the same duration */
    uint64_t fused_launches;             /* (ABI 4) ... how many */
    uint64_t fused_mask;                 /* (ABI 4) ... bit k: Mission k's last buffer was scanned by a fused launch */
} sx_stats;

typedef struct sx_ctx sx_ctx;
typedef struct sx_result sx_result;

/* Tunables (0 = library default). */
typedef struct sx_options {
    uint32_t subchunk_bytes;             /* bytes one wavefront streams sequentially (multiple of 1024) */
    uint32_t record_capacity;            /* device run-record slots per mission */
    uint32_t replay_threads;             /* host threads for the exact replay */
    uint32_t flags;                      /* SX_OPT_* */
} sx_options;
enum {
    SX_OPT_GENERIC_KERNELS = 1u,  /* force the table-driven classifiers (testing) */
    SX_OPT_DEVICE_REPLAY = 2u,    /* run the exact replay (stage B) on the device even for small inputs */
    SX_OPT_HOST_REPLAY = 4u,      /* never run stage B on the device */
    SX_OPT_TILE_TRAVERSAL = 8u,   /* (rounds 1-5: scan kernels over independent overlapping tiles, grid-stride — measured slower in every round
                                     and removed in round 6; the flag is accepted and ignored) */
    SX_OPT_MISSION_STREAMS = 16u, /* a scan stream per mission (default: one scan stream + one for everything else) */
    SX_OPT_NO_FUSED_SCAN = 64u,   /* (round 6) one scan launch per Mission, each reading the whole buffer (rounds 1-5), instead of ONE launch that
                                     reads it once for all Missions whose classifiers the fused kernel holds (csrc/sx_fused.hip) */
    SX_OPT_RESULT_ON_DEVICE = 32u /* A context with ONE Mission (round 5): a buffer's result that the device wrote in one block — a string-dense
                                     buffer (the wave path: text, `-e ascii -n 4` on binaries, where moving the findings to the host is what bounds
                                     the scan: sx_finding16 records) or a sparse one replayed on the device (sx_finding records) — stays in HBM:
                                     sx_result_segment_device() hands out device pointers to its records and strings, for hosts that go on
                                     working there.  Valid until the NEXT buffer is scanned on the context — every chunk of sx_scan_stream / sx_scan_file is one; a
                                     call that accumulates its chunks into one result keeps them in host memory — or the context is destroyed (the memory
                                     is the context's).  The
                                     host accessors (sx_result_segment, ..._packed, sx_print_findings, ...) still work (sx_print_findings_device formats the
                                     findings where they lie, without moving them): the first one copies the
                                     segment to the host (SX_E_STATE if a later scan has overwritten it).  Every other result is in host memory
                                     as without the flag; the sharded entry points ignore it.
                                     A context with SEVERAL Missions, scanned with sx_scan / sx_scan_device (one buffer, one piece): the merged findings
                                     stay in HBM — one segment per part of the merger, in print order, every segment on the device or none.  Records
                                     are sx_finding16, with sx_segment_info as ever, where the merger packs: every Mission's -q <= 16000, SX_PACKED not 0;
                                     else sx_finding.  LAYOUT of these segments: the strings lie back to back in record order — str_off[0] == 0,
                                     str_off[i + 1] == str_off[i] + str_len[i], arena_len == sum(str_len) — so a consumer that walks the records reads
                                     neighbouring bytes with neighbouring lanes; every part starts 256-byte aligned.  The scan call returns when the
                                     kernels that write the result are done: the pointers may be read from any stream at once.  Lifetime and host
                                     access as above; what the host accessors return is what a context without the flag returns (the host result keeps
                                     its own string layout).  The result is in host memory, as without the flag, in these cases and only these: no
                                     findings at all; Missions that do not count from the same origin (different counter_offset); the sharded entry
                                     points; a call that accumulates several buffers into one result; pieces forced by SX_PIECE_MIB / SX_SEQ_PIECE_MIB
                                     / SX_SEQ_PIECE_KIB; SX_HOST_MERGE; a host-only context; more than 16 Missions or 2^32 findings or more in one
                                     part (the radix-sort merger); the device block cannot be allocated (the scan does not fail). */
};

/* ---- Mission front end (src/mission.rs:448-749, src/options.rs:12-33) ------------------------------
 * From the reference's option strings to sx_mission[]: per-encoding overrides
 * (`-e ENC[,MIN[,AF[,UBF[,GREP]]]]`), global flags, defaults, alias prefix matching, WHATWG encoding
 * labels, the reference's error texts.  Pointers may be NULL (= flag not given). */
typedef struct sx_cli_flags {
    const char* counter_offset;          /* -s */
    const char* const* encodings;        /* -e, in command-line order */
    int n_encodings;
    const char* chars_min;               /* -n */
    int same_unicode_block;              /* -r */
    const char* ascii_filter;            /* -a */
    const char* unicode_block_filter;    /* -u */
    const char* grep_char;               /* -g */
    const char* output_line_len;         /* -q */
} sx_cli_flags;
typedef struct sx_enc_opt {              /* Missions::parse_enc_opt's tuple of Options */
    int has_name; char name[64];
    int has_chars_min; uint8_t chars_min;
    int has_af; uint64_t af_lo, af_hi;
    int has_ubf; uint64_t ubf;
    int has_grep_char; uint8_t grep_char;
} sx_enc_opt;
int sx_missions_from_flags(const sx_cli_flags* flags, sx_mission* out, int cap, int* n_out, char* err, size_t err_cap);
int sx_parse_enc_opt(const char* enc_opt, sx_enc_opt* out, char* err, size_t err_cap);
int sx_encoding_for_label(const char* label);      /* SX_ENC_*; -1 not a label; -2 a label of an encoding not built in */
const char* sx_encoding_name(uint32_t encoding);   /* Encoding::name(), e.g. "UTF-16LE" */
/* The decoder table of a legacy encoding as uint16_t words (single byte: 128 code points for 0x80..0xFF;
 * Big5 / EUC-JP: the index blob, layout in csrc/sx_codec_core.hpp); NULL, *n_words = 0 if the encoding has none. */
const uint16_t* sx_decoder_table(uint32_t encoding, uint64_t* n_words);

/* Lower level: does the wave-cooperative stage B (csrc/sx_wave_core.hpp) cover this Mission — no -g, no -r (unless at most one UTF-8
 * lead byte passes the filter: then -r never breaks a string),
 * 1 <= chars_min_nb <= output_line_char_nb_max <= 64, a single-byte encoding or UTF-8 (the reference's rules it
 * relies on: src/helper.rs:315-322, 349-421)?  Returns 0 if not covered, < 0 on error, else the class byte it keeps per
 * input byte in classes[256] and 1 + family: 1 for a single-byte encoding (bit 0 a character, bit 1 its UTF-8 lead byte passes
 * af / ubf — src/mission.rs:333-348 —, bit 2 / 3 its UTF-8 form has 2 / 3 bytes), 2 for UTF-8 (bits 0-2: 0 never valid,
 * 1 ASCII, 2 continuation byte, 3 / 4 / 5 lead byte of 2 / 3 / 4; bit 3 a character that starts with it passes), 3 for
 * UTF-16LE / BE — then classes[] must hold 512 bytes: [hb] per high byte of a unit: bits 0-3 the low byte's quadrants (lo >> 6)
 * whose characters pass, bit 4 hb == 0 (then [256 + lo] bit 0 says whether U+00lo passes), bit 5 / 6 a high / low surrogate
 * (bits 0-3 of a high surrogate: the astral character it begins passes). */
int sx_wave_classes(const sx_mission* mission, uint8_t* classes);
/* ... and for the two-byte family (sx_wave_classes returns 5: Big5 — only if the Mission rejects U+00C0.. and U+0300.. —,
 * Shift_JIS, EUC-KR; classes[]: as a single-byte encoding's for the bytes that are characters on their own, bit 4 = lead byte):
 * 4 bits per byte pair, index lead | trail << 8, eight per word: bit 0 the index maps the pair, bit 1 its character passes the
 * filter, bits 2-3: its UTF-8 form has 2 / 3 / 4 bytes, 3 = it yields two code points.  out8192 or NULL. */
const uint32_t* sx_wave_pair_codes(const sx_mission* mission, uint32_t* out8192);

/* ... and the same classes as SWAR ranges, if the Mission's can be put that way (csrc/sx_device.hpp WvSwar, 26 words): what the wave
 * kernels classify with then.  Returns 1 and fills out26, 0 if the Mission's classes stay a table, < 0 on error.  (Test harness.) */
int sx_wave_swar(const sx_mission* mission, uint32_t* out26);
/* ... two-byte family with sx_wave_swar() == 1: 2 bits per byte pair (bit 0 mapped, bit 1 accepted), index lead | trail << 8, sixteen per word.
 * EUC-JP (family 5): the first 1105 words, 2 bits per cell of index jis0208 (cells 0 .. 8835: (lead - A1) * 94 + trail - A1) and of index jis0212 (from cell 8836). */
const uint32_t* sx_wave_pair_codes2(const sx_mission* mission, uint32_t* out4096);

/* Lower level: which classifier stage A runs for this Mission (csrc/sx_device.hpp ClassifierKind: 0-2 the table kernels, 3 / 4 the
 * two-byte range kernels of the default filters, 5 / 8 single-byte ranges, 6 / 7 the double-byte token classifiers, 9 / 10 the range
 * kernels for filters with three-byte leads / surrogate pairs, csrc/sx_classify_ranges.hpp) and its range parameters: out20 =
 * a_lo, a_hi, u_lo, u_hi, l3_lo, l3_hi, n_ranges, rng_c1[6], rng_c2[6], 0.  generic != 0: as with SX_OPT_GENERIC_KERNELS.
 * Returns the kind (>= 0) or an error (< 0).  (Test harness: a filter that silently fell back to a table kernel would be a
 * performance regression no parity test sees.) */
int sx_scan_classifier(const sx_mission* mission, int generic, uint32_t* out20);

int  sx_abi_version(void);

/* hip_device >= 0: bind to that device.  hip_device == SX_HOST_ONLY: a context
 * without device that supports ONLY sx_replay_runs() (used when run records
 * come from elsewhere: other ranks, tests). */
#define SX_HOST_ONLY (-1)
int  sx_create(sx_ctx** out, const sx_mission* missions, int n_missions, int hip_device,
               const sx_options* opt);
void sx_destroy(sx_ctx* ctx);
const char* sx_last_error(const sx_ctx* ctx); /* ctx may be NULL: last sx_create failure */

/* Replaces the loop src/main.rs:153-168 for `len` bytes of ONE input file.
 * The chunk starts on the reference's slice grid (a multiple of 4096 bytes
 * into the file, src/input.rs:22,121-123); every chunk except the last one of
 * a file is a multiple of 4096 long.  `is_last_input_buffer` reaches the final
 * slice of the chunk exactly as the Slicer's third tuple member would
 * (src/input.rs:118,166) — the reference CLI always passes false.
 * sx_scan: bytes in host memory (copied to HBM first);
 * sx_scan_device: bytes already resident in HBM on this context's device. */
int sx_scan(sx_ctx* ctx, const uint8_t* bytes, uint64_t len, int input_file_id,
            int is_last_input_buffer, sx_result** out);
int sx_scan_device(sx_ctx* ctx, const void* device_bytes, uint64_t len, int input_file_id,
                   int is_last_input_buffer, sx_result** out);

/* Ingest pipeline (the Slicer's job, src/input.rs:57-167, for chunks instead of 4 KiB slices):
 * a reader thread fills pinned buffers from `read` (returns bytes read, 0 at the end of the
 * input, < 0 on error; short reads are fine) and copies them to HBM while the chunk before is
 * scanned.  Every chunk of `chunk_bytes` (rounded to the 4096-byte grid; 0 = 256 MiB) gives
 * one result, handed to `sink` in input order; the sink owns it (sx_result_free) and returns
 * 0 to go on.  sx_scan_file reads a file with read(2) ("-" = stdin). */
typedef int64_t (*sx_read_fn)(void* user, uint8_t* dst, uint64_t max_bytes);
typedef int (*sx_result_fn)(void* user, sx_result* result);
int sx_scan_stream(sx_ctx* ctx, sx_read_fn read, void* read_user, uint64_t chunk_bytes, int input_file_id,
                   sx_result_fn sink, void* sink_user);
int sx_scan_file(sx_ctx* ctx, const char* path, uint64_t chunk_bytes, int input_file_id,
                 sx_result_fn sink, void* sink_user);

/* Reset the carried ScannerState of every mission (scanner.rs:73-88). */
int sx_reset(sx_ctx* ctx);

/* Lower level, stage A: device long-run records of one mission for a
 * device-resident buffer (stream_parity = (stream offset of byte 0) & 1).
 * Returns all maximal runs with >= min_chars characters, sorted by start.
 * *runs is malloc'd; release with sx_free(). */
int sx_device_runs(sx_ctx* ctx, int mission_index, const void* device_bytes, uint64_t len,
                   int stream_parity, uint64_t min_chars, sx_run** runs, uint64_t* n_runs);

/* (ABI 4) The same for n Missions of the context in one call (mission_indices[i], min_chars[i] -> runs[i], n_runs[i]; every runs[i]
 * is malloc'd: sx_free()).  Missions whose classifiers the fused kernel holds (csrc/sx_fused.hip) share ONE launch that reads the
 * buffer once — what sx_scan* does for them; sx_get_stats().fused_mask says which did. */
int sx_device_runs_multi(sx_ctx* ctx, const int* mission_indices, int n, const void* device_bytes, uint64_t len,
                         int stream_parity, const uint64_t* min_chars, sx_run** runs, uint64_t* n_runs);

/* Lower level, stage B: exact replay on the host given run records per
 * mission (runs[m] sorted by start, chunk-relative).  Works on SX_HOST_ONLY
 * contexts; same carry semantics and result as sx_scan. */
int sx_replay_runs(sx_ctx* ctx, const uint8_t* bytes, uint64_t len, int input_file_id,
                   int is_last_input_buffer, const sx_run* const* runs, const uint64_t* n_runs,
                   sx_result** out);

/* Byte-range sharding of ONE input file over several contexts — one process per GPU
 * (multi-GPU row of the scope table).  The buffer holds file bytes
 * [buf_off, buf_off+buf_len), buf_off a multiple of 4096 (the slice grid is the file's);
 * it should reach `halo` bytes beyond [own_lo, own_hi) on both sides where the file does.
 * The call returns the findings of every replay region that BEGINS in
 * [max(own_lo, start_at[m]), own_hi) for mission m, following the last such region to its
 * own end even beyond own_hi, and reports in end_pos[m] (file offset) where mission m's
 * replay stopped: the next rank's start_at[m].  start_at == NULL means own_lo for every
 * mission (first attempt; a rank must repeat the call with reuse_runs=1 if the previous
 * rank's end_pos turns out to lie beyond own_lo).  If end_pos[m] == buf_off+buf_len although
 * the file goes on, the buffer was too short for a run that crosses it: repeat with a
 * larger halo.  A Big5 / EUC-JP mission needs a byte outside the lead range between the buffer start and own_lo
 * (buf_off > 0): without one the call fails with SX_E_HALO — repeat with a larger halo in front.  A mission with
 * chars_min_nb 0 cannot be sharded (SX_E_INVALID).  Positions are counter_offset + file_stream_off + file offset.  The context's
 * carried state is used only by the shard that starts the file (buf_off == own_lo == 0) and
 * updated only by the shard whose own_hi is the buffer end.
 *   sx_scan_shard_device: bytes resident in HBM;  sx_scan_shard: host bytes (uploaded);
 *   sx_replay_shard_runs: stage B only, run records (buffer relative) supplied by the caller. */
int sx_scan_shard_device(sx_ctx* ctx, const void* device_bytes, uint64_t buf_off, uint64_t buf_len,
                         uint64_t own_lo, uint64_t own_hi, const uint64_t* start_at,
                         uint64_t file_stream_off, int input_file_id, int reuse_runs,
                         sx_result** out, uint64_t* end_pos);
int sx_scan_shard(sx_ctx* ctx, const uint8_t* bytes, uint64_t buf_off, uint64_t buf_len,
                  uint64_t own_lo, uint64_t own_hi, const uint64_t* start_at,
                  uint64_t file_stream_off, int input_file_id, int reuse_runs,
                  sx_result** out, uint64_t* end_pos);
int sx_replay_shard_runs(sx_ctx* ctx, const uint8_t* bytes, uint64_t buf_off, uint64_t buf_len,
                         uint64_t own_lo, uint64_t own_hi, const uint64_t* start_at,
                         uint64_t file_stream_off, int input_file_id,
                         const sx_run* const* runs, const uint64_t* n_runs,
                         sx_result** out, uint64_t* end_pos);

/* The whole sharded scan of one file for one rank of a job of `world` ranks (one process per GPU): own range + halo
 * (sx_shard_bounds), the "where did everybody stop" exchange, the repeat when the previous rank ran past this rank's
 * start, wider halos where a run (or, Big5 / EUC-JP, a stretch without token boundary) crosses them.  The transport is
 * the caller's: `allgather` must deliver every rank's `bytes` bytes to all ranks, in rank order (RCCL, MPI, ...), and
 * return 0.  `get_buffer` returns the file bytes [lo, hi) — in HBM of the context's device (*is_device = 1, 16-byte
 * aligned) or in host memory — valid until its next call.  `get_runs` is normally NULL; if given, stage A is skipped
 * and the runs of the buffer come from the caller (host bytes; CPU tests, runs from elsewhere).
 * *out = this rank's findings (segment `rank` of the file's findings, in order); counts[k] / overflow[k] (arrays of
 * `world`, may be NULL) = findings of rank k / how many of its last findings lie behind its range end.  Gathering the
 * Finding buffers is the caller's (e.g. one gather over RCCL); sx_shard_splice() puts gathered buffers in order.
 * Errors: what does not depend on the rank (a Mission with chars_min_nb == 0 or ISO-2022-JP and world > 1, ...) is refused on
 * every rank before anything is exchanged; a rank whose own work fails (memory, HIP, its buffer callback) still joins the
 * exchange with its error code in its row, and EVERY rank returns an error in that round (SX_E_STATE on the healthy ones).
 * A stream of several files: call once per file, in order, on every rank, with file_stream_off = the bytes of the files
 * before.  The state the reference carries from file to file (decoder, leftover, cut flag: src/main.rs:153-168, one
 * ScannerState per Mission for the whole stream) is known to the last rank at the end of a file; it travels to all ranks in
 * one more all-gather of the same callback (<= sizeof decoder + 4q + 40 bytes per Mission) and enters the next file's first
 * shard, so the result is what one process scanning the files in a row gives. */
typedef int (*sx_allgather_fn)(void* user, const void* send, uint64_t bytes, void* recv);
typedef int (*sx_shard_buffer_fn)(void* user, uint64_t lo, uint64_t hi, const void** ptr, int* is_device);
typedef int (*sx_shard_runs_fn)(void* user, const uint8_t* bytes, uint64_t buf_off, uint64_t buf_len,
                                const sx_run* const** runs, const uint64_t** n_runs);
void sx_shard_bounds(uint64_t file_len, int world, int rank, uint64_t* own_lo, uint64_t* own_hi);
int sx_scan_sharded(sx_ctx* ctx, int rank, int world, uint64_t file_len, uint64_t file_stream_off, int input_file_id,
                    uint64_t halo, sx_shard_buffer_fn get_buffer, void* buffer_user, sx_shard_runs_fn get_runs, void* runs_user,
                    sx_allgather_fn allgather, void* allgather_user, sx_result** out, uint64_t* counts, uint64_t* overflow);
/* The ranks' finding buffers -> ONE result in the reference's print order (rank k's findings behind its range end
 * merged into the head of rank k+1's: slice, position, Mission).  str_off of findings[k] is relative to arenas[k]. */
int sx_shard_splice(const sx_finding* const* findings, const uint64_t* n_findings, const uint8_t* const* arenas,
                    const uint64_t* arena_lens, int world, uint64_t file_len, sx_result** out);
/* (ABI 3) The same for ranks whose findings arrive in SEGMENTS (a rank with more than 4 GiB of strings ships its result segment by segment,
 * every segment with its own str_off space): seg s = (findings[s], n_findings[s], arenas[s], arena_lens[s]); rank 0's n_segs_of_rank[0]
 * segments come first, then rank 1's, ...  The result has as many segments as its strings need (< 2 GiB each, cut between findings). */
int sx_shard_splice_segs(const sx_finding* const* findings, const uint64_t* n_findings, const uint8_t* const* arenas,
                         const uint64_t* arena_lens, const uint32_t* n_segs_of_rank, int world, uint64_t file_len, sx_result** out);

/* ---- (round 6) The sharded scan's transport inside the library: RCCL over xGMI, loaded with dlopen ("librccl.so.1"; a host without
 * it still loads this library and scans one GPU).  One process per GPU:
 *     rank 0: sx_transport_rccl_id(id);  ship the 128 bytes to every rank (the launcher's job: a file, an env var, MPI, a socket);
 *     every rank: sx_transport_rccl_create(&t, hip_device, rank, world, id);              -- ncclCommInitRank, a stream of its own
 *     sx_scan_sharded(ctx, rank, world, ..., sx_transport_allgather, t, &mine, counts, overflow);   -- the transport is the callback's `user`
 *     sx_transport_gather(t, mine, 0, file_len, &all);    -- rank 0: ONE result in the reference's order (sx_shard_splice_segs inside); else NULL
 * The gather: an all-gather of the segment sizes, then grouped ncclSend / ncclRecv of exactly those sizes into one device buffer at
 * the root and one copy to the host — no collective on the data path.  Errors: SX_E_STATE without librccl,
 * SX_E_HIP for a failing HIP / RCCL call; text from sx_transport_last_error (NULL: the last failed id / create call). */
#define SX_TRANSPORT_ID_BYTES 128
typedef struct sx_transport sx_transport;
int  sx_transport_rccl_id(uint8_t* id128);
int  sx_transport_rccl_create(sx_transport** out, int hip_device, int rank, int world, const uint8_t* id128);
void sx_transport_destroy(sx_transport* t);
const char* sx_transport_last_error(const sx_transport* t);
int  sx_transport_allgather(void* transport, const void* send, uint64_t bytes, void* recv);   /* an sx_allgather_fn */
int  sx_transport_gather(sx_transport* t, const sx_result* mine, int root, uint64_t file_len, sx_result** out);

/* (round 5, SX_OPT_RESULT_ON_DEVICE) Segment i where it lies in HBM: *d_records = n records (sx_finding16 if *packed, else sx_finding;
 * what they share: *info), *d_arena = arena_len bytes of strings (str_off counts from there).  *d_records == NULL: the segment is in host
 * memory (read it with sx_result_segment / sx_result_segment_packed).  SX_E_STATE: a later scan has reused the memory.  One caller at a
 * time per result: the host accessors' first use of such a segment moves it to host memory (that segment only: the other segments'
 * pointers stay valid).  Several Missions: one segment per merger part, strings back to back in record order (SX_OPT_RESULT_ON_DEVICE). */
int               sx_result_segment_device(const sx_result* r, uint64_t i, const void** d_records, uint64_t* n_findings,
                                           const uint8_t** d_arena, uint64_t* arena_len, int* packed, sx_segment_info* info);
uint64_t          sx_result_count(const sx_result* r);
/* The findings come in one or more segments, in print order: a buffer scanned piece by piece adds a segment per
 * piece; a Mission with millions of runs — alone, or the busy one among Missions with few — is replayed in slabs, one segment
 * each (a slab travels to the host while the next is replayed); several Missions with a large output are interleaved on the device in parts of at most 2 GiB of
 * strings, one segment each (str_off has 32 bits).  The segments' memory is pinned host memory the device wrote
 * directly.  Each segment has its own arena: str_off counts from that arena's start.  A segment stored as sx_finding16 records is
 * expanded to sx_finding on its first sx_result_segment() call (a copy in host memory; sx_result_segment_packed() avoids it). */
uint64_t          sx_result_segments(const sx_result* r);
int               sx_result_segment(const sx_result* r, uint64_t index, const sx_finding** findings,
                                    uint64_t* n_findings, const uint8_t** arena, uint64_t* arena_len);
/* A segment as it is stored: *packed = 1 -> `findings` points at n_findings sx_finding16 and *info says what they share (info may
 * be NULL if the caller only wants to know); *packed = 0 -> at sx_finding, as sx_result_segment() returns them.  No copy either way. */
int               sx_result_segment_packed(const sx_result* r, uint64_t index, const void** findings, uint64_t* n_findings,
                                           const uint8_t** arena, uint64_t* arena_len, int* packed, sx_segment_info* info);
/* Contiguous view of all segments (joined by a copy on first use if there are several;
 * NULL if the strings exceed 4 GiB — use the segments then). */
const sx_finding* sx_result_findings(const sx_result* r);
const uint8_t*    sx_result_arena(const sx_result* r, uint64_t* len);
void              sx_result_free(sx_result* r);

/* `Finding::print` for every finding of a result — src/finding.rs:112-155.
 * n_inputs = ARGS.inputs.len(); radix 0 (no -t) | 'x' | 'd' | 'o'.  The caller
 * frames the whole output with SX_OUTPUT_BOM and a final "\n"
 * (src/main.rs:116,138).  *out is malloc'd; release with sx_free(). */
#define SX_OUTPUT_BOM "\xEF\xBB\xBF"
int sx_print_findings(const sx_ctx* ctx, const sx_result* r, int n_inputs, int radix,
                      int no_metadata, uint8_t** out, uint64_t* out_len);
/* Finding::print for every finding of a result whose segments ALL lie in HBM (SX_OPT_RESULT_ON_DEVICE), written by the device
 * (csrc/sx_print_dev.hip): *d_text = *text_len bytes in HBM, byte for byte what sx_print_findings(ctx, r, n_inputs, radix, no_metadata, ...)
 * returns — same framing contract: no BOM, no final "\n"; the caller adds them.  text_len has 64 bits and so have all offsets behind
 * it: a result's text may exceed 4 GiB.  The text block is the context's memory (grown on demand, reused): valid until the next
 * sx_print_findings_device or sx_scan* call on the context or sx_destroy — the epoch rule of the result block.  The call returns
 * when the kernels that write the text are done: the pointer may be read from any stream at once.  The result is NOT moved: every
 * segment is still on the device afterwards (sx_result_segment_device returns the same pointers) and the host accessors work as
 * before.  SX_E_STATE — and *d_text = NULL, *text_len = 0 — if any segment of the result is in host memory (every case of
 * SX_OPT_RESULT_ON_DEVICE's "the result is in host memory" list, a result without findings among them; a segment a host accessor
 * has already moved; a context without the flag; a host-only context) or a later scan has reused the memory: the caller then
 * uses sx_print_findings.  SX_E_INVALID for a radix other than 0 / 'x' / 'd' / 'o'; SX_E_NOMEM if the text block cannot be
 * allocated (the result stays usable). */
int sx_print_findings_device(sx_ctx* ctx, const sx_result* r, int n_inputs, int radix, int no_metadata,
                             const uint8_t** d_text, uint64_t* text_len);

/* The findings of a result whose segments ALL lie in HBM (SX_OPT_RESULT_ON_DEVICE), selected by substring where they lie
 * (csrc/sx_select_dev.hip) — what `grep -F -f patterns` keeps of the printed lines when only the string part of a line is looked at.
 * Finding i MATCHES if some pattern p equals s[o, o + len_p) for some 0 <= o <= str_len - len_p: bytes compared as bytes (the
 * strings are UTF-8, a pattern is raw bytes), or after the ASCII fold with SX_SELECT_ASCII_NOCASE.  A match never spans two findings; a
 * finding shorter than the pattern does not match.  Finding i is selected iff (matches) XOR (SX_SELECT_INVERT).
 * *out is a new result (sx_result_free) whose segments all lie in HBM: every source segment with at least one selected finding gives
 * one segment, source order and record order kept; the record type (sx_finding16 / sx_finding) and the sx_segment_info are the
 * source segment's and every record is unchanged except str_off.  A segment is [records][strings], 256-byte aligned, its strings back
 * to back in record order — the layout of the merged segments: str_off[0] == 0, str_off[i + 1] == str_off[i] + str_len[i],
 * arena_len == sum(str_len).  Nothing selected: *out is an empty result (sx_result_count 0, no segments: "no findings -> host memory").
 * The source may be any result sx_print_findings_device accepts (both record types, any layout of the strings: they are addressed
 * by str_off), the result of an earlier selection among them: selecting from a selection is AND (grep a | grep b).  The source is
 * read, never moved: its device pointers are the same afterwards and its host accessors work as before.
 * Memory: two selection blocks of the context, grown on demand and used in turn: a selected result is valid until the SECOND
 * sx_result_select_device call after the one that made it (a call that returns SX_E_INVALID or SX_E_STATE writes nothing and does not count), or
 * sx_destroy.  A scan call does not invalidate it — the blocks are not the result block: a host can work on the selection of buffer
 * N while buffer N + 1 is scanned.  Afterwards the accessors answer SX_E_STATE, as for any result on the device.  The call returns
 * when the kernels that write the block are done.  sx_print_findings_device, sx_result_segment_device and the host accessors take a
 * selected result as they take a scan's.
 * SX_E_INVALID: n_patterns outside 1..SX_SELECT_MAX_PATTERNS, a len outside 1..SX_SELECT_MAX_PATTERN_BYTES, a NULL pointer, unknown
 * flag bits.  SX_E_STATE — and *out = NULL — wherever sx_print_findings_device would refuse the source (a segment in host memory, a
 * result without findings, a later scan or selection that reused the memory, a context without the flag, a host-only context): the
 * caller then filters on the host.  SX_E_NOMEM: the block cannot be allocated (the source stays usable). */
#define SX_SELECT_MAX_PATTERNS 16
#define SX_SELECT_MAX_PATTERN_BYTES 64
enum { SX_SELECT_ASCII_NOCASE = 1u,   /* bytes 'A'..'Z' of strings and patterns compare as 'a'..'z'; no other byte is folded */
       SX_SELECT_INVERT = 2u };       /* keep the findings that match NO pattern (grep -v) */
typedef struct sx_pattern { const uint8_t* bytes; uint32_t len; } sx_pattern;   /* raw bytes; the strings are UTF-8 */
int sx_result_select_device(sx_ctx* ctx, const sx_result* r, const sx_pattern* patterns, int n_patterns,
                            uint32_t flags, sx_result** out);

/* The same selection by a keyword LIST — `grep -F -f keywords.txt` with hundreds to tens of thousands of entries —, compiled once
 * and used on buffer after buffer.  sx_select_set_create builds, on the host, the Aho-Corasick automaton of the patterns as a full
 * table (csrc/sx_selset_build.hpp: byte classes, states numbered breadth first, every state that ends a pattern collapsed into one
 * "matched" state) and puts it into HBM on the context's device; the cost of a string byte is then one table look-up, however many
 * patterns there are and whatever bytes they begin with.  flags: 0 or SX_SELECT_ASCII_NOCASE — the fold is compiled into the set.
 * Duplicate patterns are allowed.  The set owns its device memory and does not depend on the context's lifetime: it may be freed
 * before or after sx_destroy, and used with any context on the same HIP device (another device: SX_E_INVALID).
 * SX_E_INVALID: n_patterns outside 1..SX_SELECT_SET_MAX_PATTERNS, a len outside 1..SX_SELECT_SET_MAX_PATTERN_BYTES, lengths that sum
 * to more than SX_SELECT_SET_MAX_TOTAL_BYTES, a NULL pointer, any other flag bit.  SX_E_STATE: a host-only context.  SX_E_NOMEM: the
 * table cannot be allocated.  *out = NULL on every error.
 * sx_select_set_info_get: what was built — table_bytes lie in HBM, the rows of the first lds_states states are what the kernel
 * (csrc/sx_selset_dev.hip) keeps in LDS, the other rows it reads through L2.
 * sx_result_select_set_device: flags 0 or SX_SELECT_INVERT; in everything else the contract of sx_result_select_device, word for
 * word — the match rule, the output layout, the empty result, the source that is read and never moved, the sources accepted (a
 * result of either kind of selection among them: AND), the errors.  It writes the same two selection blocks: calls of both kinds
 * count together for "valid until the SECOND selection after the one that made it". */
#define SX_SELECT_SET_MAX_PATTERNS      65536u
#define SX_SELECT_SET_MAX_PATTERN_BYTES 255u
#define SX_SELECT_SET_MAX_TOTAL_BYTES   (1u << 20)     /* sum of the patterns' lengths */
typedef struct sx_select_set sx_select_set;
typedef struct sx_select_set_info {
    uint32_t n_patterns, states, classes, nocase;
    uint64_t table_bytes;     /* in HBM */
    uint32_t lds_states;      /* states whose rows the kernel keeps in LDS */
    uint32_t reserved;
} sx_select_set_info;
int  sx_select_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_select_set** out);
int  sx_select_set_info_get(const sx_select_set* set, sx_select_set_info* out);
void sx_select_set_free(sx_select_set* set);
int  sx_result_select_set_device(sx_ctx* ctx, const sx_result* r, const sx_select_set* set, uint32_t flags, sx_result** out);

/* The same selection by REGULAR EXPRESSION — `grep -E -f patterns` over the string part of the lines: URLs, e-mail addresses, dotted
 * quads, registry paths, card-number shapes —, compiled once and used on buffer after buffer.  sx_select_regex_create builds, on
 * the host, ONE minimal DFA for "some pattern matches somewhere in the string" (csrc/sx_selre_build.hpp: parser, NFA with the
 * counted repeats unrolled, subset construction, minimisation, byte classes, states numbered breadth first) and puts its table into
 * HBM on the context's device; a string byte costs one table look-up, and a lane stops early where the string has matched for good
 * or can match no more.  A set holds 1..SX_SELECT_REGEX_MAX_PATTERNS patterns of 1..SX_SELECT_REGEX_MAX_PATTERN_BYTES bytes; a
 * finding MATCHES if any pattern is found anywhere in its string (re.search, not fullmatch), and is selected iff (matches) XOR
 * (SX_SELECT_INVERT).  A match never spans two findings.
 * THE PATTERN LANGUAGE is a byte regex: patterns are raw bytes, the strings are UTF-8, a byte >= 0x80 is a literal byte and a
 * quantifier behind it binds that one byte.  The governing rule: every pattern this library accepts means what Python 3's `re`
 * means by it as a bytes pattern, with `$` read as `\Z` — Python's re.search is the tests' oracle —, and whatever would need a
 * different reading is refused:
 *   literals                              accepted
 *   .                                     any byte except 0x0A
 *   \t \n \r \f \v \xHH                   accepted; \x needs two hex digits
 *   backslash + non-alphanumeric byte     that byte as a literal
 *   \d \D \w \W \s \S                     Python's bytes-mode ASCII sets: \s = space \t \n \r \f \v, \w = [A-Za-z0-9_]; allowed
 *                                         inside a class, but not as a range end
 *   [...] [^...]                          ranges a-z need lo <= hi; `-` is a literal when first, last or escaped
 *   ] directly behind [ or [^             refused: escape it
 *   an unescaped [ inside a class         refused
 *   (...) (?:...)                         the same thing: nothing is captured; any other (? is refused
 *   |                                     empty alternatives and () are allowed and match the empty string
 *   * + ? {m} {m,} {m,n} {,n}             m <= n <= SX_SELECT_REGEX_MAX_REPEAT
 *   a trailing ? on a quantifier (lazy)   accepted and ignored: only existence is asked
 *   a second quantifier, *+               refused
 *   a quantifier with nothing in front of it, or on ^ or $        refused
 *   a { that does not begin a well-formed bound                   refused: escape it
 *   ^                                     matches only in front of the string's first byte
 *   $                                     matches only behind its last byte; there is no "in front of a trailing newline" rule:
 *                                         this is the line rule of grep, and a finding is a line
 *   ^ or $ in mid-pattern                 legal: (^a|b)c, a$|b; a^b is legal and matches nothing
 *   every other backslash + alphanumeric (\b \B \A \Z \1 \e ...)  refused
 * Refused means SX_E_INVALID, and sx_last_error names the pattern's index, the byte offset and the reason.  Not in the language:
 * Unicode-aware classes and folding ([а-я] is a byte class; sx_result_fold_device in front of the call folds the strings by simple
 * folding, sx_fold_utf8 a pattern's literals), \b, lookaround, back-references, captures.
 * (Where the matches lie: sx_result_extract_regex_device, below; which patterns match in a finding: sx_result_label_device, below.)
 * flags: 0 or SX_SELECT_ASCII_NOCASE — the fold is compiled into the set, and it is re.IGNORECASE on a bytes pattern: a literal
 * letter matches both cases, a class holds a letter's other case too and negation applies after that ([Z-a] matches z and A,
 * [^Z-a] matches neither); no byte >= 0x80 is folded.
 * The compiled object owns its device memory and does not depend on the context's lifetime: it may be freed before or after
 * sx_destroy, and used with any context on the same HIP device (another device: SX_E_INVALID).
 * sx_select_regex_create: SX_E_INVALID for n_patterns outside 1..SX_SELECT_REGEX_MAX_PATTERNS, a len outside
 * 1..SX_SELECT_REGEX_MAX_PATTERN_BYTES, a NULL pointer, any other flag bit, a refused pattern, or a limit passed — a repeat count
 * above SX_SELECT_REGEX_MAX_REPEAT, more than SX_SELECT_REGEX_MAX_POSITIONS positions (every byte set, anchor and empty branch is
 * one, counted with the repeats unrolled, all patterns together), more than SX_SELECT_REGEX_MAX_STATES states in the subset
 * construction (it runs before the minimisation and stops at the first state above the limit), or that construction's bound on its
 * own memory: its states are kept as lists of positions, and 32 Mi positions in all of them are the most (an unanchored a{51000}
 * meets it, its k-th state holding k positions, though its minimal DFA has 51 001 states; ^a{51000} compiles) —: the text says
 * which.  SX_E_STATE: a host-only context.  SX_E_NOMEM: the table cannot be allocated.  *out = NULL on every error.
 * sx_select_regex_info_get: what was built — table_bytes (states * classes * 2) lie in HBM, the rows of the first lds_states states
 * are what the kernel (csrc/sx_selre_dev.hip) keeps in LDS, the other rows it reads through L2; end_states come from `$`.
 * sx_result_select_regex_device: flags 0 or SX_SELECT_INVERT; in everything else the contract of sx_result_select_set_device, word
 * for word — the output layout, the empty result, the source that is read and never moved, the sources accepted (a result of any
 * of the three kinds of selection among them: AND), the errors.  It writes the same two selection blocks: calls of all three kinds
 * count together for "valid until the SECOND selection after the one that made it". */
#define SX_SELECT_REGEX_MAX_PATTERNS      64u
#define SX_SELECT_REGEX_MAX_PATTERN_BYTES 1024u
#define SX_SELECT_REGEX_MAX_REPEAT        255u
#define SX_SELECT_REGEX_MAX_POSITIONS     65536u  /* NFA positions once counted repeats are unrolled, all patterns together */
#define SX_SELECT_REGEX_MAX_STATES        65536u  /* DFA states: an entry always has 2 bytes */
typedef struct sx_select_regex sx_select_regex;
typedef struct sx_select_regex_info {
    uint32_t n_patterns, states, classes, nocase;
    uint64_t table_bytes;   /* in HBM */
    uint32_t lds_states;    /* states whose rows the kernel keeps in LDS */
    uint32_t end_states;    /* states that select a string only if it ENDS there */
} sx_select_regex_info;
int  sx_select_regex_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_select_regex** out);
int  sx_select_regex_info_get(const sx_select_regex* re, sx_select_regex_info* out);
void sx_select_regex_free(sx_select_regex* re);
int  sx_result_select_regex_device(sx_ctx* ctx, const sx_result* r, const sx_select_regex* re, uint32_t flags, sx_result** out);

/* The regex MATCHES of a result whose segments ALL lie in HBM, cut out where they lie (csrc/sx_extract_dev.hip) — `grep -oE -f patterns`
 * over the string part of the lines: the URLs, e-mail addresses, dotted quads themselves, not the lines that hold them.  The three
 * selections answer WHETHER a finding's string holds something; this answers WHERE, and yields a new device-resident result whose
 * findings are the matches, back to back in HBM, which prints, downloads, selects and tallies like any other.
 * PATTERNS AND FLAGS.  An extract set holds 1..SX_SELECT_REGEX_MAX_PATTERNS patterns.  The language is exactly the regex set's, above:
 * the same refusals, the same limits (SX_SELECT_REGEX_MAX_*, the bound on the construction's memory), the same error texts; flags: 0 or
 * SX_SELECT_ASCII_NOCASE, compiled into the set.  Lazy quantifiers are accepted and ignored: the longest match is taken.
 * sx_extract_regex_create builds, on the host, an ANCHORED minimal DFA (csrc/sx_extract_build.hpp: the regex set's parser and NFA, no
 * re-entry in front of later bytes, one start state for offset 0 and one for every later offset, per state whether a match may end
 * there) and puts its table into HBM on the context's device.  It is an object of its own: a regex set compiles nothing more than
 * before.  It owns its device memory and does not depend on the context's lifetime: it may be freed before or after sx_destroy, and
 * used with any context on the same HIP device (another device: SX_E_INVALID).  Errors as sx_select_regex_create's; *out = NULL on
 * every error.  sx_extract_regex_info_get: what was built — table_bytes (states * classes * 2) lie in HBM, the rows of the first
 * lds_states states are what the kernels keep in LDS, the other rows they read through L2.
 * MATCHING.  For a finding with the string s of n bytes the matches are found as `grep -oE` finds them — leftmost start, longest end
 * over all patterns, non-overlapping, non-empty:
 *   o = 0; while o < n: let e be the largest end in (o, n] such that some pattern matches exactly s[o, e);
 *                       if there is such an e: emit (o, e) and o = e; otherwise o = o + 1.
 * `^` holds only at offset 0 of the string and `$` only at offset n, for every match in the string, not only the first: nothing
 * outside the record's own bytes is looked at.  Patterns that can match the empty string (a*) are legal; empty matches are never
 * emitted.  A match never spans two findings.
 * OUTPUT.  Every match gives one output record, in source order, and in offset order within a finding.  The output record is the
 * source record unchanged except for str_off and str_len: `position`, the precision, completes_previous, mission_id and the rest are
 * the FINDING's, not the match's — the byte offset of a match in the input cannot be derived from an offset into the UTF-8 string of
 * a UTF-16 finding, and is not given.
 * sx_result_extract_regex_device: flags 0; output layout, empty result, memory and lifetime follow the contract of
 * sx_result_select_regex_device, word for word: one output segment per source segment that has at least one match, source order
 * kept; the record type (sx_finding16 / sx_finding) and the sx_segment_info are the source segment's; a segment is [records][strings],
 * 256-byte aligned, its strings back to back in record order (str_off[0] == 0, str_off[i + 1] == str_off[i] + str_len[i], arena_len ==
 * sum(str_len)); no match anywhere: *out is the empty result.  The source is read, never moved.  The call writes the same two
 * selection blocks and counts as a selection for "valid until the SECOND selection after the one that made it".  The sources
 * accepted are exactly those sx_print_findings_device accepts, any selection and any earlier extraction among them.  The output may
 * have MORE records than the source; its strings never have more bytes than the source's.  SX_E_STATE wherever
 * sx_print_findings_device would refuse the source; SX_E_NOMEM if the block cannot be had; SX_E_INVALID for a NULL pointer, a flag, a
 * set on another device, or — with sx_last_error text — a segment whose match count does not fit the 32-bit per-segment counters.
 * COST.  A byte that cannot begin a match costs one table look-up.  A walk that runs far and then fails is repeated from the next
 * start: the worst case is QUADRATIC in a string's length (a*b over a long run of a).  There is no linear-time guarantee.
 * Not built: which pattern a MATCH is of (sx_result_label_device says which patterns match in a finding, and so in an extraction's
 * match taken as a finding of its own), captures, the input-byte positions of the matches. */
typedef struct sx_extract_regex sx_extract_regex;
typedef struct sx_extract_regex_info {
    uint32_t n_patterns, states, classes, nocase;
    uint64_t table_bytes;   /* in HBM */
    uint32_t lds_states;    /* states whose rows the kernels keep in LDS */
    uint32_t reserved;
} sx_extract_regex_info;
int  sx_extract_regex_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_extract_regex** out);
int  sx_extract_regex_info_get(const sx_extract_regex* ex, sx_extract_regex_info* out);
void sx_extract_regex_free(sx_extract_regex* ex);
int  sx_result_extract_regex_device(sx_ctx* ctx, const sx_result* r, const sx_extract_regex* ex, uint32_t flags, sx_result** out);

/* The keyword TALLY of a result whose segments ALL lie in HBM: which entries of an indicator list occur in the findings' strings, how
 * often, and where first — what the three selections throw away —, counted where the findings lie (csrc/sx_seltally_dev.hip), one pass
 * over the strings for up to 65536 keywords.  sx_tally_set_create builds, on the host, the Aho-Corasick automaton of the patterns as
 * a full table with output links (csrc/sx_seltally_build.hpp: byte classes, a state per distinct prefix of the keywords, numbered
 * breadth first, NOT collapsed; per state the keyword that ends there and the next state on the failure chain that ends one) and puts
 * it into HBM on the context's device, with two counters per keyword.  The limits and flags are sx_select_set_create's: 1..
 * SX_SELECT_SET_MAX_PATTERNS patterns of 1..SX_SELECT_SET_MAX_PATTERN_BYTES bytes, SX_SELECT_SET_MAX_TOTAL_BYTES in all; flags 0 or
 * SX_SELECT_ASCII_NOCASE — the fold is compiled into the set.  Duplicate patterns are allowed.  The errors are the same: SX_E_INVALID
 * for a limit passed, a NULL pointer or any other flag bit, SX_E_STATE for a host-only context, SX_E_NOMEM if the tables cannot be
 * allocated; *out = NULL on every error.  The set owns its device memory, tables and counters, and does not depend on the context's
 * lifetime: it may be freed before or after sx_destroy, and used with any context on the same HIP device (another device:
 * SX_E_INVALID).
 * THE HIT RULE.  A HIT of keyword k is a pair (finding i, offset o) with s_i[o, o + len_k) == p_k: bytes compared as bytes, after the
 * ASCII fold of both sides if the set is nocase.  Occurrences of one keyword that overlap themselves all count ("aa" has 3 hits in
 * "aaaa").  A hit never spans two findings.
 * THE COUNTERS, per keyword, read after one or more sx_result_tally_device calls: hits[k] = the number of hits of pattern k;
 * first[k] = the smallest (ordinal_base + index of the finding in the result's print order) among its hits — the print order is
 * segment 0's records, then segment 1's, and so on —, or SX_TALLY_NEVER if there is none.  Patterns that are equal after the fold are
 * one keyword (sx_tally_set_info.unique counts those) and report the same pair.  A new set is reset.
 * sx_result_tally_device ADDS the hits of r's findings to the counters: a stream scanned buffer by buffer gives one tally of the whole
 * stream if the caller passes the number of findings of the buffers before as ordinal_base.  *n_findings (may be NULL) = the number
 * of findings walked.  The call returns when the kernels are done.  The sources are exactly what sx_print_findings_device accepts — both
 * record types, any layout of the strings, the result of any of the three selections (the tally of a regex selection: "which
 * indicators sit on lines that look like URLs") —, and SX_E_STATE comes back wherever that function would refuse the source; that is
 * decided for ALL segments before anything is launched, and a refused call adds nothing.  The source is read, never moved.  The call
 * writes neither the result block nor the selection blocks: it does NOT count towards "valid until the SECOND selection after the one
 * that made it" and invalidates nothing.  SX_E_INVALID: a NULL ctx, r or set, a set on another device.
 * sx_tally_set_reset: every hits = 0, every first = SX_TALLY_NEVER.  sx_tally_set_read: hits and first per INPUT pattern (either array
 * may be NULL); n_patterns must be the set's (else SX_E_INVALID).  sx_tally_set_counters_device: the counters where they lie, in HBM,
 * indexed by UNIQUE id (*unique entries each), and *d_unique_of_pattern = n_patterns words that map an input pattern to its unique id,
 * for hosts that stay on the GPU; any of the four may be NULL; valid until sx_tally_set_free.
 * sx_tally_set_info_get: what was built — states (the distinct prefixes, the empty one included), entries of entry_bytes (2 while
 * states <= 32768, else 4), table_bytes in HBM (everything but the counters), the rows of the first lds_states states are what the
 * kernel keeps in LDS, the other rows it reads through L2.
 * Not thread-safe: one sx_result_tally_device call per set at a time, and no reset or read during it.
 * Not built: the number of FINDINGS per keyword (grep -c; for up to 64 regular expressions sx_result_label_device counts exactly that)
 * and where in a string a hit lies. */
typedef struct sx_tally_set sx_tally_set;
typedef struct sx_tally_set_info {
    uint32_t n_patterns, unique;   /* unique: distinct keywords after the fold */
    uint32_t states, classes, nocase, entry_bytes;   /* entry_bytes 2 or 4 */
    uint64_t table_bytes;          /* everything the set holds in HBM except the counters */
    uint32_t lds_states, reserved;
} sx_tally_set_info;               /* 40 bytes */
#define SX_TALLY_NEVER UINT64_MAX
int  sx_tally_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_tally_set** out);
int  sx_tally_set_info_get(const sx_tally_set* set, sx_tally_set_info* out);
void sx_tally_set_free(sx_tally_set* set);
int  sx_tally_set_reset(sx_tally_set* set);
int  sx_result_tally_device(sx_ctx* ctx, const sx_result* r, sx_tally_set* set, uint64_t ordinal_base, uint64_t* n_findings);
int  sx_tally_set_read(const sx_tally_set* set, uint64_t* hits, uint64_t* first, uint32_t n_patterns);
int  sx_tally_set_counters_device(const sx_tally_set* set, const uint64_t** d_hits, const uint64_t** d_first,
                                  const uint32_t** d_unique_of_pattern, uint32_t* unique);

/* The LABELS of a result whose segments ALL lie in HBM: for every finding, WHICH patterns of a regex list are found in its string,
 * as one 64-bit word — what the regex selection's one bit per finding ("some pattern matched") throws away —, made where the findings
 * lie (csrc/sx_label_dev.hip) in one walk over the strings, with the number of findings per pattern (`grep -c`, exactly) and the first
 * of them counted on the way; and the selection by label, which splits a result into its kinds without reading a string byte.
 * PATTERNS AND FLAGS.  A label set holds 1..SX_SELECT_REGEX_MAX_PATTERNS patterns; pattern p owns bit p.  The language is exactly the
 * regex set's, above: the same refusals, the same limits (SX_SELECT_REGEX_MAX_*, the bound on the construction's memory), the same
 * error texts; flags: 0 or SX_SELECT_ASCII_NOCASE, compiled into the set.  sx_label_set_create builds, on the host, ONE minimal DFA
 * (csrc/sx_label_build.hpp: the regex set's parser and NFA with an accept per pattern, unanchored subset construction, per state the
 * patterns that have matched with the byte that led there and those that match if the string ends there) and puts its tables into HBM
 * on the context's device, with two counters per pattern.  There is no "matched" state that absorbs the walk once ANY pattern has
 * matched, because the others are still asked for: a label set reaches SX_SELECT_REGEX_MAX_STATES sooner than a regex set of the same
 * patterns (SX_E_INVALID, the regex set's text), and a lane stops early only where every pattern has matched or none can any more.
 * It is an object of its own: a regex set compiles nothing more than before.  It owns its device memory, tables and counters, and
 * does not depend on the context's lifetime: it may be freed before or after sx_destroy, and used with any context on the same HIP
 * device (another device: SX_E_INVALID).  Errors as sx_select_regex_create's; *out = NULL on every error.
 * sx_label_set_info_get: what was built — table_bytes in HBM (everything but the counters), the rows of the first lds_states states are
 * what the kernel keeps in LDS, the other rows it reads through L2; here_states: the states that end a match of some pattern.
 * THE RULE.  Bit p of finding i's label is set iff pattern p is found somewhere in its string: Python's re.search on the bytes
 * pattern with `$` read as `\Z`, and re.IGNORECASE for a nocase set.  A match never spans two findings.  The bits of patterns the set
 * does not have are 0.
 * THE COUNTERS, per pattern, read after one or more sx_result_label_device calls: findings[p] = the number of findings with bit p;
 * first[p] = the smallest (ordinal_base + index of the finding in the result's print order) among them — the print order is segment
 * 0's records, then segment 1's, and so on —, or SX_LABEL_NEVER if there is none.  A new set is reset.
 * sx_result_label_device makes *out, the labels of r's findings (sx_labels_free), and ADDS to the set's counters as the tally does: a
 * stream scanned buffer by buffer gives one count of the whole stream if the caller passes the number of findings of the buffers
 * before as ordinal_base.  The labels object owns its device memory: one array of 64-bit words per source segment, in record order
 * (sx_labels_segments, sx_labels_segment_device: *d_labels = *n_findings words in HBM, valid until sx_labels_free, before or after
 * sx_destroy).  The sources are exactly what sx_print_findings_device accepts — both record types, any layout of the strings, the
 * result of any selection or extraction —, and SX_E_STATE comes back wherever that function would refuse the source; that is decided
 * for ALL segments before anything is launched.  The source is read, never moved.  The call writes neither the result block nor the
 * selection blocks: it does NOT count towards "valid until the SECOND selection after the one that made it" and invalidates nothing.
 * It returns when the kernels are done.  SX_E_INVALID: a NULL pointer, a set on another device.  SX_E_NOMEM: the labels cannot be
 * allocated; nothing is counted then (the allocation comes before the launch).
 * sx_label_set_reset: every findings = 0, every first = SX_LABEL_NEVER.  sx_label_set_read: findings and first per pattern (either
 * array may be NULL); n_patterns must be the set's (else SX_E_INVALID).  sx_label_set_counters_device: the counters where they lie,
 * in HBM, 64 words each of which the first n_patterns are used, for hosts that stay on the GPU; either may be NULL; valid until
 * sx_label_set_free.
 * sx_result_select_labels_device: finding i of r is selected iff
 *   (any == 0 || (label_i & any) != 0) && (label_i & all) == all && (label_i & none) == 0
 * — any == all == none == 0 selects everything.  Mask bits at or above n_patterns are legal: such a bit is never set in a label, so
 * in `all` it selects nothing and in `none` it is harmless.  In everything else the contract of sx_result_select_regex_device, word
 * for word — the output layout, the empty result, the source that is read and never moved, the two selection blocks and their
 * epochs —: the call counts as a selection.  It reads 8 bytes per record and the records, no string byte.  `labels` must have been
 * made from r: the labels remember, per segment, where the source's records lie, how many they are and the epoch of their block;
 * another result is SX_E_INVALID (sx_last_error says so), a source whose memory has been reused since is SX_E_STATE, as that source
 * itself would be.  The labels of a selection are not carried to its output: label the output again, or select by label first.
 * Not thread-safe: one sx_result_label_device call per set at a time, and no reset or read during it.
 * Not built: which pattern matched WHERE (labels on an extraction's matches by their own pattern), labels for keyword sets of 65536
 * entries, labels carried through a selection, Unicode folding inside this call (sx_result_fold_device in front of it: simple
 * folding). */
typedef struct sx_label_set sx_label_set;   /* compiled patterns + their counters, in HBM */
typedef struct sx_labels    sx_labels;      /* one result's labels, in HBM */
typedef struct sx_label_set_info {
    uint32_t n_patterns, states, classes, nocase;
    uint64_t table_bytes;     /* everything the set holds in HBM except the counters */
    uint32_t lds_states;      /* states whose rows the kernel keeps in LDS */
    uint32_t here_states;     /* states that end a match of some pattern: a step into one ORs its mask into the label */
} sx_label_set_info;
#define SX_LABEL_NEVER UINT64_MAX
int  sx_label_set_create(sx_ctx* ctx, const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, sx_label_set** out);
int  sx_label_set_info_get(const sx_label_set* set, sx_label_set_info* out);
void sx_label_set_free(sx_label_set* set);
int  sx_label_set_reset(sx_label_set* set);
int  sx_label_set_read(const sx_label_set* set, uint64_t* findings, uint64_t* first, uint32_t n_patterns);
int  sx_label_set_counters_device(const sx_label_set* set, const uint64_t** d_findings, const uint64_t** d_first);
int  sx_result_label_device(sx_ctx* ctx, const sx_result* r, sx_label_set* set, uint64_t ordinal_base, sx_labels** out);
int  sx_labels_segment_device(const sx_labels* labels, uint64_t segment, const uint64_t** d_labels, uint64_t* n_findings);
uint64_t sx_labels_segments(const sx_labels* labels);
void sx_labels_free(sx_labels* labels);
int  sx_result_select_labels_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels,
                                    uint64_t any, uint64_t all, uint64_t none, sx_result** out);

/* The DUPLICATE STRINGS of a result whose segments ALL lie in HBM: `sort -u` / `uniq -c` / `uniq -d` / `uniq -u` over the findings'
 * strings in the result's own order, decided on the device where the findings lie (csrc/sx_distinct_dev.hip) without a sort, as
 * labels that sx_result_select_labels_device takes.
 * THE RULE.  Two findings of r are EQUAL iff their strings — arena[str_off, str_off + str_len), the UTF-8 the result holds — are byte
 * for byte equal; with flags = SX_SELECT_ASCII_NOCASE iff they are equal after 'A'..'Z' became 'a'..'z' (no other byte is folded).
 * Equality is across Missions and across segments; position and metadata play no part; empty strings are equal to each other.  The
 * ORDER is the result's print order — segment 0's records, then segment 1's, and so on.  *out (sx_labels_free) holds one 64-bit word
 * per finding, laid out as sx_result_label_device lays its labels out (sx_labels_segments, sx_labels_segment_device):
 *   bit 0  SX_DISTINCT_FIRST     no earlier finding of r is equal to this one
 *   bit 1  SX_DISTINCT_REPEATED  some other finding of r is equal to this one
 *   bits 32..63                  the number of findings of r equal to this one, itself included (word >> SX_DISTINCT_COUNT_SHIFT); it
 *                                saturates at 2^32 - 1 and is the same in every member of a class
 *   every other bit              0
 * so that sx_result_select_labels_device(r, *out, any, all, none) gives: any = FIRST `sort -u` in the original order; none = FIRST the
 * duplicates that were dropped; all = FIRST | REPEATED `uniq -d`; any = FIRST, none = REPEATED `uniq -u`; and `uniq -c` is the high
 * half of the words that have bit 0.  *info (may be NULL): findings = the words written, distinct = the classes, repeated = the classes
 * of two or more members, rounds and table_log2 = what the method below took.
 * THE METHOD is a tournament by hash that is exact whatever the hash does (csrc/sx_distinct_core.hpp): per round every finding without
 * a class hashes its string with the round's seed into a table of 2^table_log2 slots — the power of two >= 2 x findings —, the smallest
 * key (segment << 32 | record) in a slot wins it, and whoever EQUALS its slot's winner, compared byte for byte, has found its class:
 * equal strings share every slot, so a class is resolved as a whole, to its first member.  Every round resolves at least the winners'
 * classes; the host reads one counter per round and stops at 0.  Words and counters are sums and minima: deterministic.
 * The call reads r and never moves it, writes neither the result block nor a selection block and ages no selection: it is no selection.
 * Its tables — 8 x 2^table_log2 + 16 x findings bytes — are memory of the context's that only this call uses, grown on demand and freed
 * by sx_destroy; the labels are the caller's.  It returns when the kernels are done.  SX_E_INVALID: a NULL pointer (info may be), flags other than 0 or SX_SELECT_ASCII_NOCASE.
 * SX_E_STATE: a host-only context; a result in host memory, or one whose device memory a later call has reused — as
 * sx_result_label_device refuses them.  SX_E_NOMEM: the labels or the tables cannot be allocated.  *out is NULL on every error.
 * Not built: classes per Mission, Unicode folding inside this call (sx_result_fold_device in front of it: simple folding), the
 * counts carried through a selection (they are in the labels of the source:
 * distinct the selection again, or read the words), a sorted output.  (Classes across several results or buffers: the seen set below.) */
enum { SX_DISTINCT_FIRST = 1u, SX_DISTINCT_REPEATED = 2u };
#define SX_DISTINCT_COUNT_SHIFT 32
typedef struct sx_distinct_info {
    uint64_t findings, distinct, repeated;
    uint32_t rounds, table_log2;
} sx_distinct_info;
int  sx_result_distinct_device(sx_ctx* ctx, const sx_result* r, uint32_t flags, sx_labels** out, sx_distinct_info* info);

/* The SEEN SET: strings remembered in HBM from one result to the next — every string once over a stream or a directory of files
 * (`sort -u` of the whole run), and baseline subtraction or intersection (`comm`) against a known-good image —, on the device where
 * the findings lie (csrc/sx_seen_dev.hip).
 * sx_seen_set_create: an exact, open-addressed hash set of byte strings of FIXED capacity — capacity_strings strings whose entries
 * take capacity_bytes at most, a string of len bytes taking SX_SEEN_ENTRY_BYTES(len) —, empty.  flags: 0, or SX_SELECT_ASCII_NOCASE:
 * the fold is a property of the SET, which stores the folded bytes.  The table has the power of two >= 2 x capacity_strings slots (at
 * least 2), so a probe always ends.  SX_E_INVALID: a NULL pointer, other flags, capacity_strings == 0, either capacity above 2^40.
 * SX_E_STATE: a host-only context.  SX_E_NOMEM: no device memory for it.  *out = NULL on every error.  The set owns its device
 * memory as a label set does: it may be freed before or after sx_destroy and used with any context on the same HIP device (another
 * device: SX_E_INVALID).  sx_seen_set_info_get: strings and bytes = what it holds, the capacities, table_log2, nocase, tag_bits.
 * sx_seen_set_reset: the set is empty again, its capacity is kept.
 * sx_result_seen_device gives every finding of r the word sx_result_distinct_device(r, the set's fold) gives it PLUS ONE BIT:
 *   bits 0, 1, 32..63            exactly sx_result_distinct_device's
 *   bit 2  SX_DISTINCT_SEEN      the set held an equal string WHEN THE CALL BEGAN; the same in every member of a class
 *   every other bit              0
 * — equality is the distinct call's, byte for byte or after 'A'..'Z' became 'a'..'z' —, so that of sx_result_select_labels_device
 * any = FIRST, none = SEEN is the stream's `sort -u` (every string new to the stream, once), none = SEEN baseline subtraction, and
 * any = SEEN intersection.  *out is laid out as the distinct call's.  Then, unless flags = SX_SEEN_LOOKUP_ONLY, the call ADDS: after
 * it the set holds (what it held) united with (the strings of r), each once.  *info (may be NULL): findings, distinct, repeated,
 * rounds, table_log2 as sx_distinct_info; seen_findings = the words with SEEN, seen_distinct = the classes with SEEN;
 * added_strings = the classes without SEEN and added_bytes = the sum of SX_SEEN_ENTRY_BYTES(len) over them — what the call put into
 * the set, both 0 for a lookup-only call.
 * CAPACITY is fixed.  If strings + added_strings > capacity_strings or bytes + added_bytes > capacity_bytes the call returns
 * SX_E_NOMEM, sx_last_error names both sums, *out = NULL and THE SET IS UNCHANGED: the host decides it from the lookup's totals before
 * anything is added.  A lookup-only call never fails for capacity.  sx_seen_set_grow (below) gives the set room and keeps what it holds.
 * THE METHOD (csrc/sx_seen_core.hpp): behind the distinct pass a lookup pass — a lane per finding hashes its string, walks from its
 * home slot, and compares with an entry only where the slot's tag equals its hash's — and, behind one read of its totals, an add pass
 * in which only the first finding of a class the set did not hold acts: a wavefront takes its entries' room with one add, a lane
 * writes its entry and takes the first empty slot from its home slot on by compare-and-swap.  No lane waits for another.
 * Words, *info and the set's strings / bytes are deterministic; WHERE an entry lies in the set is not, and is no part of the contract.
 * Sources, refusals and lifetime are exactly sx_result_distinct_device's — SX_E_STATE where that refuses —: r is read and never moved,
 * no result or selection block is written, no selection ages.  SX_E_INVALID also: a NULL set, flags other than 0 or
 * SX_SEEN_LOOKUP_ONLY, a set on another device.  Not thread-safe: one call per set at a time, and no reset or info during it.
 * Not built: removing strings, Unicode folding inside this call (sx_result_fold_device in front of it: simple folding), sharded
 * entry points.  (Growth, saving and loading a set, and a list of strings as
 * the source: below.  A count per stored string over the stream: SX_SEEN_COUNTED, further below.) */
typedef struct sx_seen_set sx_seen_set;         /* the slots, the entries and their cursors, in HBM */
enum { SX_DISTINCT_SEEN = 4u };                 /* bit 2 of a word made by sx_result_seen_device */
#define SX_SEEN_LOOKUP_ONLY 0x100u              /* call flag: mark, add nothing */
#define SX_SEEN_ENTRY_BYTES(len) (8u + (((uint64_t)(len) + 7u) & ~(uint64_t)7u))
typedef struct sx_seen_set_info {
    uint64_t strings, bytes, capacity_strings, capacity_bytes;
    uint32_t table_log2, nocase, tag_bits;
    uint32_t counted;                           /* 1: the set was made with SX_SEEN_COUNTED (below), else 0 */
} sx_seen_set_info;
typedef struct sx_seen_info {
    uint64_t findings, distinct, repeated;      /* as sx_distinct_info */
    uint64_t seen_findings, seen_distinct;      /* findings / classes with SX_DISTINCT_SEEN */
    uint64_t added_strings, added_bytes;        /* what this call put into the set */
    uint32_t rounds, table_log2;                /* as sx_distinct_info: the distinct pass's */
} sx_seen_info;
int  sx_seen_set_create(sx_ctx* ctx, uint64_t capacity_strings, uint64_t capacity_bytes, uint32_t flags, sx_seen_set** out);
int  sx_seen_set_info_get(const sx_seen_set* set, sx_seen_set_info* out);
int  sx_seen_set_reset(sx_seen_set* set);
void sx_seen_set_free(sx_seen_set* set);
int  sx_result_seen_device(sx_ctx* ctx, const sx_result* r, sx_seen_set* set, uint32_t flags, sx_labels** out, sx_seen_info* info);

/* A SEEN SET THAT OUTLIVES A CALL: merged with another, grown, saved and loaded, and fed from a list of strings.  All of it is one
 * mechanism (csrc/sx_seen_merge_core.hpp, csrc/sx_seen_merge_dev.hip): a SOURCE of entries that already are a set — pairwise
 * different, folded under the destination's fold — goes into a destination in two passes, a lane per source entry: a lookup pass
 * that says per entry whether the destination held it and counts what is new, and, behind one read of the cursors and the counts, an
 * add pass that copies the new entries and claims their slots.  Entries are hashed, compared and copied eight bytes at a time.  The
 * source is another set's slot table as it lies (merge, grow) or a list the host built and uploaded (import, add_strings).
 * sx_seen_set_merge: dst = dst united with src.  flags: 0, or SX_SEEN_LOOKUP_ONLY — count, add nothing: already_held is then the size
 * of the intersection.  *info (may be NULL): source_strings = what src holds, already_held = those dst held when the call began,
 * added_strings / added_bytes = what the call put into dst (0 for a lookup-only call).  SX_E_INVALID: a NULL pointer, other flags,
 * sets of different folds, dst == src, a set on another device than the context's.  SX_E_NOMEM: strings + new > capacity_strings or
 * bytes + new bytes > capacity_bytes — sx_last_error names both sums, and DST IS UNCHANGED —, or no device memory for the call's
 * scratch (a bit per slot of src).  src is only read.
 * sx_seen_set_grow: THE SAME HANDLE gets new capacities: new memory is allocated, the set's contents are merged into it — every entry
 * is hashed again for the new table_log2 —, the handle takes the new memory and the old is freed.  The capacities may be smaller than
 * they were as long as they hold what the set holds; otherwise, or with capacity_strings == 0 or either above 2^40, SX_E_INVALID
 * before anything is allocated.  SX_E_NOMEM: no device memory for the new set; the set is as it was.  tag_bits stay the set's.
 * THE BLOB: sx_seen_set_export_size says how many bytes sx_seen_set_export writes: a 64-byte little-endian header — the magic
 * "SXSEEN\0\0", u32 version = 1, u32 nocase, u64 strings, u64 bytes, u64 FNV-1a-64 over the entry area, the rest 0 — and then the
 * set's first `bytes` bytes of entries as they lie: [u32 len][u32 0][the (folded) bytes, zero-padded to 8] each.  cap < that size:
 * SX_E_INVALID, nothing written.  Where entries lie depends on the order of the adds: two exports of equal sets may differ, the
 * contract is the set of strings; two exports of a set that was not written in between are byte-identical.
 * sx_seen_blob_info_get checks a blob completely, on the host and without a device or a context, and says what it holds.  It
 * refuses (SX_E_INVALID) a wrong magic or version, len != 64 + bytes, bytes not a multiple of 8, nocase other than 0 / 1, an entry
 * that overruns the area, a second u32 or padding that is not 0, an entry count other than `strings`, a checksum that does not match,
 * two equal entries, and with nocase a byte 'A'..'Z': what the kernels rely on is checked before they run.
 * sx_seen_set_import: a new set that holds the blob's strings, under the blob's fold and the CONTEXT's tag bits (SX_SEEN_TAG_BITS).
 * A capacity of 0 = what the blob holds (at least one string); one smaller than the blob holds: SX_E_INVALID.  A blob that
 * sx_seen_blob_info_get refuses: SX_E_INVALID, sx_last_error says why, nothing is allocated.  *out = NULL on every error.
 * sx_seen_set_add_strings: n byte strings, string i = bytes[offsets[i], offsets[i + 1]), as a source.  The host folds them under the
 * set's fold and keeps the first of every group of equal ones; source_strings counts those.  held_out (n bytes, may be NULL):
 * held_out[i] = 1 iff the set held string i WHEN THE CALL BEGAN, per input string, duplicates alike.  With SX_SEEN_LOOKUP_ONLY this
 * is `contains` for a list.  A string may be longer than a finding can be.  SX_E_INVALID also: n or offsets[n] above 2^32 - 1,
 * offsets that decrease.  Capacity as sx_seen_set_merge.
 * All of them but the two host-only blob calls refuse a host-only context (SX_E_STATE), age no selection and write no result or
 * selection block; like every call on a set they are not thread-safe per set.
 * Not built: removing strings, canonical (sorted) blobs, Unicode folding inside this call (sx_result_fold_device in front of it:
 * simple folding), sharded entry points. */
typedef struct sx_seen_merge_info { uint64_t source_strings, already_held, added_strings, added_bytes; } sx_seen_merge_info;
typedef struct sx_seen_blob_info  { uint64_t strings, bytes; uint32_t nocase, version; } sx_seen_blob_info;
#define SX_SEEN_BLOB_HEADER_BYTES 64u
#define SX_SEEN_BLOB_VERSION 1u
int  sx_seen_set_merge(sx_ctx* ctx, sx_seen_set* dst, const sx_seen_set* src, uint32_t flags, sx_seen_merge_info* info);
int  sx_seen_set_grow(sx_ctx* ctx, sx_seen_set* set, uint64_t capacity_strings, uint64_t capacity_bytes);
int  sx_seen_set_export_size(const sx_seen_set* set, uint64_t* bytes);
int  sx_seen_set_export(const sx_seen_set* set, void* buf, uint64_t cap, uint64_t* written);
int  sx_seen_blob_info_get(const void* blob, uint64_t len, sx_seen_blob_info* out);
int  sx_seen_set_import(sx_ctx* ctx, const void* blob, uint64_t len, uint64_t capacity_strings, uint64_t capacity_bytes, sx_seen_set** out);
int  sx_seen_set_add_strings(sx_ctx* ctx, sx_seen_set* set, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                             uint32_t flags, uint8_t* held_out, sx_seen_merge_info* info);

/* A SEEN SET THAT COUNTS: how many results held each string, and how often — which strings occur in at least k of the N files
 * scanned so far, which occur in this file and in no more than one other, `sort | uniq -c` over a stream (csrc/sx_seen_count_core.hpp,
 * csrc/sx_seen_count_dev.hip).
 * sx_seen_set_create with SX_SEEN_COUNTED (ORed with SX_SELECT_ASCII_NOCASE or not) makes a set that owns one more array in HBM: a
 * 64-bit COUNT WORD per slot of its table —
 *   bits 0..31   (word >> SX_SEEN_RESULTS_SHIFT)  & 0xFFFFFFFF   results:  the calls that held the string
 *   bits 32..63  (word >> SX_SEEN_FINDINGS_SHIFT) & 0xFFFFFFFF   findings: the findings (or list members) equal to it over those calls
 * — both saturating at 2^32 - 1, each on its own.  sx_seen_set_info.counted says which kind a set is.  A set made without the flag
 * behaves bit for bit as before and runs no kernel it did not run before.  What each call does to a counted set:
 *   sx_result_seen_device, adding   for every class C of r under the set's fold, whether the set held it or not: results += 1,
 *                                   findings += |C| (the class size in the word's high half).  Words and *info are what they are for a
 *                                   plain set.  SX_SEEN_LOOKUP_ONLY and SX_E_NOMEM leave the counts as they were.
 *   sx_seen_set_reset               zeroes the counts.
 *   sx_seen_set_merge(dst, src)     dst counted: for every string of src, dst's counts grow by src's counts, or by (1, 1) if src is
 *                                   plain; lookup-only leaves them.  dst plain: as before, whatever src is.
 *   sx_seen_set_grow                keeps the counts.
 *   sx_seen_set_add_strings         the list is one result: per distinct folded string results += 1, findings += the number of input
 *                                   strings equal to it.
 *   sx_seen_set_export              BLOB VERSION 2: the header with version = 2, the entry area as in version 1, then `strings` 64-bit
 *                                   count words, little-endian, in the order the entries lie in the area; the checksum covers the entry
 *                                   area followed by the count words; the blob has 64 + bytes + 8 x strings bytes.  A plain set's export
 *                                   stays version 1, byte for byte.
 *   sx_seen_blob_info_get           takes both versions (sx_seen_blob_info.version says which); the length rule is the version's, and in
 *                                   version 2 a count word with results == 0 or findings < results is refused.
 *   sx_seen_set_import              a version-2 blob gives a counted set with those counts, a version-1 blob a plain set.
 * The method: behind the add pass one more pass in which the first finding of every class (every entry of a source) looks its string
 * up — every string of the call is held by then —, gets its slot and adds to the slot's word with a plain load and store: no two lanes
 * of a call have the same string.  The pass also runs when nothing is new but some class was seen.
 * sx_result_seen_counts_device: READ THE COUNTS WHERE THE FINDINGS LIE.  *out (sx_labels_free) holds one word per finding of r, laid
 * out as every other labels object: the count word of the finding's string under the set's fold, or 0 if the set does not hold it.
 * Lookup-only, no distinct pass.  A plain set: SX_E_INVALID.  Sources, refusals and lifetime are sx_result_seen_device's; no result or
 * selection block is written and no selection ages.
 * sx_result_select_labels_range_device: SELECTION BY A FIELD OF A LABEL WORD.  Finding i of r is selected iff
 *   lo <= ((label_i >> shift) & mask(bits)) <= hi
 * with 1 <= bits <= 64 and shift + bits <= 64 (else SX_E_INVALID); lo > hi selects nothing.  In everything else the contract of
 * sx_result_select_labels_device, word for word: the labels' binding to r, the epochs, the output layout, the empty result.  It reads
 * 8 bytes per record and the records, no string byte.  It takes any labels: on distinct words shift = 32, bits = 32, lo = 5 gives the
 * strings that occur at least five times in r; on count words shift = SX_SEEN_RESULTS_SHIFT, bits = 32, lo = k the strings at least
 * k results held.
 * Not built: removing strings, counts per Mission, canonical (sorted) blobs, Unicode folding inside this call (sx_result_fold_device
 * in front of it: simple folding), sharded entry points, an accessor to
 * the raw count table for hosts that stay on the GPU. */
#define SX_SEEN_COUNTED 0x200u                  /* sx_seen_set_create flag: the set counts */
#define SX_SEEN_RESULTS_SHIFT 0
#define SX_SEEN_FINDINGS_SHIFT 32
#define SX_SEEN_BLOB_VERSION_COUNTED 2u
int  sx_result_seen_counts_device(sx_ctx* ctx, const sx_result* r, sx_seen_set* set, sx_labels** out);
int  sx_result_select_labels_range_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels, uint32_t shift, uint32_t bits,
                                          uint64_t lo, uint64_t hi, sx_result** out);

/* IN WHICH ORDER: sx_result_order_device.  *out (sx_result_free) is a new result in HBM that holds the findings of r that take part —
 * those the label pick of sx_result_select_labels_device lets through; any = all = none = 0: every finding — in sorted order, the
 * first `limit` of them (0: all).  It is sorted(range(n), key, reverse): findings with equal keys keep print order — segment order,
 * then record order —, and SX_ORDER_DESCENDING reverses the order of the distinct keys and leaves the ties in print order.
 *   SX_ORDER_BY_STRING       the strings as unsigned bytes, memcmp and then the shorter one first: LC_ALL=C sort.  With
 *                            SX_ORDER_NOCASE the bytes are compared after 'A'..'Z' became 'a'..'z', no other byte; the output's
 *                            strings stay as they are.
 *   SX_ORDER_BY_LABEL_FIELD  (label >> shift) & mask(bits) as an unsigned number, 1 <= bits <= 64, shift + bits <= 64: on distinct
 *                            words shift = 32, bits = 32 is the size of the class, on count words a half of the word.
 * `labels` (of r, as sx_result_select_labels_device checks it) serves the filter and the field; it may be NULL where neither needs it.
 * `sort -u` is sx_result_distinct_device, then by = STRING, any = SX_DISTINCT_FIRST; `uniq -c | sort -rn | head -20` is by =
 * LABEL_FIELD, shift = 32, bits = 32, DESCENDING, any = SX_DISTINCT_FIRST, limit = 20.
 * The output is ONE segment of sx_finding records in the order, their strings back to back in record order, every field what
 * sx_result_segment() gives for the source record (a packed source's input_file_id and slice_index come from its sx_segment_info);
 * a call in which nothing takes part gives a result without segments, as a selection that selects nothing does.  It lies in the
 * selection block whose turn it is: the call takes a turn and ages selections exactly as a selection does; a call that returns an
 * error takes none and writes no block.  r is read, never moved.
 * *info (may be NULL): findings = how many took part, kept = how many were written, rounds = the refinement rounds of the string key
 * (a round looks at eight more bytes of the strings still undecided; 0 for the label key and where nothing takes part), tied = the
 * written findings whose key equals another written finding's, max_depth = the deepest 8-byte word a comparison needed (rounds - 1).
 * SX_E_STATE wherever sx_print_findings_device refuses the source, and for a source in the block this call would write.
 * SX_E_INVALID (sx_last_error says which): a NULL pointer, an unknown `by` or flag, SX_ORDER_NOCASE with the label key, `labels` NULL
 * where the key or the filter needs them, a field that sx_result_select_labels_range_device would refuse, labels of another result,
 * more than 2^32 - 2 findings that take part or 2^32 or more bytes of their strings — decided before anything is written.
 * SX_E_NOMEM: a block or the tables cannot be had.  *out = NULL on every error.
 * Not built: locale collation, Unicode folding inside this call (sx_result_fold_device in front of it: simple folding), a second
 * key, numeric-string keys, sharded entry points, top-k without a full sort. */
enum { SX_ORDER_BY_STRING = 0, SX_ORDER_BY_LABEL_FIELD = 1 };
enum { SX_ORDER_DESCENDING = 1u, SX_ORDER_NOCASE = 2u };
typedef struct sx_order_spec {
    uint32_t by;            /* SX_ORDER_BY_STRING | SX_ORDER_BY_LABEL_FIELD */
    uint32_t flags;         /* SX_ORDER_DESCENDING, SX_ORDER_NOCASE (strings only) */
    uint32_t shift, bits;   /* the field of a label word, as sx_result_select_labels_range_device reads it */
    uint64_t any, all, none;/* the label pick of sx_result_select_labels_device; all three 0: every finding */
    uint64_t limit;         /* keep only the first `limit` findings of the order; 0: all */
} sx_order_spec;
typedef struct sx_order_info { uint64_t findings, kept, rounds, tied, max_depth; } sx_order_info;
int  sx_result_order_device(sx_ctx* ctx, const sx_result* r, const sx_labels* labels /* may be NULL */,
                            const sx_order_spec* spec, sx_result** out, sx_order_info* info /* may be NULL */);

/* WHATEVER THE LETTER CASE, IN EVERY SCRIPT: sx_result_fold_device.  *out (sx_result_free) is a new result in HBM with the findings of
 * r in the same order, every string replaced by its Unicode SIMPLE case folding; every operation above then works on the folded
 * strings unchanged, and sx_labels_rebind carries an answer back to the original strings.  Output segment i corresponds to source
 * segment i record for record: the same number of records of the same type (sx_finding or sx_finding16), the same sx_segment_info,
 * every field of a record but str_off and str_len as it was, the folded strings back to back in record order.
 * The rule, SX_FOLD_SIMPLE (flags = 0; no other flag is accepted yet): the string is walked from the left.  At a well-formed UTF-8
 * sequence (Unicode Table 3-7: no overlong form, no surrogate, nothing above U+10FFFF, the whole sequence inside the string) of the
 * code point c, fold(c) is written as UTF-8; any other byte is copied as it is and the walk goes on at the next byte.  fold() is
 * CaseFolding.txt's statuses C and S (csrc/gen_fold_table.py, csrc/sx_fold_table.inc, which names its Unicode version): 'A' -> 'a',
 * 'П' -> 'п', 'Σ' and 'ς' -> 'σ', U+212A KELVIN SIGN -> 'k'; a code point that has only a FULL folding stays: 'ß', 'İ'.  In Python:
 * b.decode('utf-8', 'surrogateescape'), per character x = c.casefold() if that is one character, else c.lower() if that is one, else
 * c; .encode('utf-8', 'surrogateescape').  The fold is idempotent.  A folded string has between a third and one and a half times
 * its source's bytes (U+023A and U+023E grow from 2 to 3 bytes).
 * `grep -i` in every script: fold the result, fold the patterns with sx_fold_utf8, label or select on the fold, sx_labels_rebind the
 * labels to r, sx_result_select_labels_device on r — the ORIGINAL strings whose folding matches.  `sort -u`, the seen sets and the
 * order work on the fold the same way.
 * The fold counts as a selection: it lies in the selection block whose turn it is, takes a turn and ages selections exactly as a
 * selection does; a call that returns an error takes none and writes no block.  r is read, never moved.
 * *info (may be NULL): findings, bytes_in = the source strings' bytes, bytes_out = the folded strings', changed = the findings whose
 * string the fold changes.
 * Sources and SX_E_STATE exactly as sx_result_label_device, and for a source in the block this call would write.  SX_E_INVALID
 * (sx_last_error says which): a NULL pointer, a flag, a segment whose folded strings have 2^32 bytes or more (str_off is 32-bit), a
 * packed segment with a folded string longer than 65535 bytes (its str_len is 16-bit) — decided before anything is written.
 * SX_E_NOMEM: a block or the tables cannot be had.  *out = NULL on every error.
 *
 * sx_fold_utf8: the same rule, the same code, for one byte string on the host; no context.  The folded bytes go to out[0, *written);
 * out = NULL asks for the size: *written = the folded length, nothing is written.  SX_E_INVALID: a NULL pointer, a flag, or cap <
 * the folded length — then *written says what is needed and out is untouched.  A caller folds its patterns with it.
 *
 * sx_labels_rebind: *out (sx_labels_free) is a new labels object with the words of `labels`, copied on the device, bound to the
 * result `to`: sx_result_select_labels_device, sx_result_select_labels_range_device and sx_result_order_device accept it for `to`
 * as they accept the labels made from it.  `to` must lie in HBM as sx_result_label_device asks of its source (else SX_E_STATE) and
 * have as many segments as the labels' source and as many records in each (else SX_E_INVALID).  It is meant for a fold and its
 * source, which correspond record for record; the library checks the shape only — that record i of `to` is the finding that word i
 * speaks of is what the CALLER vouches for.  It is no selection and ages nothing; `labels` stays valid.
 * Not built: full case folding ('ß' -> "ss"), Turkic rules, normalization (NFC / NFKC), locale collation, a packed segment expanded
 * where a folded string outgrows it, sharded entry points. */
enum { SX_FOLD_SIMPLE = 0u };
typedef struct sx_fold_info { uint64_t findings, bytes_in, bytes_out, changed; } sx_fold_info;
int  sx_fold_utf8(const uint8_t* in, uint64_t len, uint32_t flags, uint8_t* out, uint64_t cap, uint64_t* written);
int  sx_result_fold_device(sx_ctx* ctx, const sx_result* r, uint32_t flags, sx_result** out, sx_fold_info* info /* may be NULL */);
int  sx_labels_rebind(sx_ctx* ctx, const sx_labels* labels, const sx_result* to, sx_labels** out);

/* WHAT A STRING LOOKS LIKE: sx_result_measure_device.  *out (sx_labels_free) holds one word per finding of r, laid out and bound to r
 * as every other labels object, so sx_result_select_labels_device, sx_result_select_labels_range_device, sx_result_order_device and
 * sx_labels_rebind take it: `awk 'length >= 32'` is a range on the chars field, "only hex digits" a mask on the class bits, "entropy
 * above 4.5 bits per byte" a range on the entropy field with lo = 4.5 x 4096.
 * The word of a string of n bytes, c[b] = how often byte b occurs in it (n = 0: the word is 0):
 *   bits  0..15  SX_MEASURE_ENTROPY_SHIFT, 16 bits   ENT: the Shannon entropy of the bytes, in bits per byte x 4096: 0 for "aaaa",
 *                                                    4096 for "abab", 16384 for the 16 hex digits once each, 32768 for all 256 bytes
 *                                                    equally often
 *   bits 16..24  SX_MEASURE_DISTINCT_SHIFT, 9 bits   the number of b with c[b] > 0: 0 to 256
 *   bits 25..31  the class bits, each set iff the string holds at least one such byte: SX_MEASURE_LOWER 'a'..'z', SX_MEASURE_UPPER
 *                'A'..'Z', SX_MEASURE_DIGIT '0'..'9', SX_MEASURE_SPACE 0x20 and 0x09, SX_MEASURE_PUNCT the other bytes of 0x21..0x7E,
 *                SX_MEASURE_CONTROL 0x00..0x1F without 0x09, and 0x7F, SX_MEASURE_HIGH 0x80 and above
 *   bits 32..63  SX_MEASURE_CHARS_SHIFT, 32 bits     the bytes outside 0x80..0xBF: the UTF-8 characters of well-formed text, the byte
 *                                                    count of ASCII
 * ENT is defined in integers, so that the device, the host and a restatement agree bit for bit.  LG(x) for 1 <= x < 2^32 is log2(x) in
 * units of 2^-16, at most 1.00001 units below it and never above: e = 31 - clz(x); m = x << (31 - e); f = 0; sixteen times { m = (m * m)
 * >> 31 (a 64-bit product); f <<= 1; if m >= 2^32 { f |= 1; m >>= 1 } }; LG = e << 16 | f.  Then T = n x LG(n) - sum over b of c[b] x
 * LG(c[b]) in 64 bits — LG is monotone, so T >= 0 —, and ENT = min(65535, T / (16 x n)).
 * flags must be 0.  *info (may be NULL): findings, bytes = the strings' bytes, chars = the sum of the chars fields, wide = the strings
 * of more than 255 bytes (which a wavefront measures, where the others take a lane), ascii = the strings without SX_MEASURE_HIGH.
 * The call is no selection: it lies in no selection block, takes no turn, ages nothing, and r is read, never moved; only the words, a
 * list of the wide strings' records and the call's totals are written.  Sources, SX_E_STATE, SX_E_INVALID and SX_E_NOMEM exactly as
 * sx_result_seen_counts_device, and SX_E_INVALID for a flag or a segment of 2^32 findings or more.  *out = NULL on every error.
 *
 * sx_measure_bytes: the same rule, the same code, for one byte string on the host; no context.  SX_E_INVALID: a NULL pointer (s may
 * be NULL where len is 0), a flag, or len >= 2^32.
 * Not built: entropy over characters instead of bytes, n-gram statistics, per-script classes, longest run, sharded entry points. */
#define SX_MEASURE_ENTROPY_SHIFT 0
#define SX_MEASURE_DISTINCT_SHIFT 16
#define SX_MEASURE_CHARS_SHIFT 32
#define SX_MEASURE_LOWER   ((uint64_t)1 << 25)
#define SX_MEASURE_UPPER   ((uint64_t)1 << 26)
#define SX_MEASURE_DIGIT   ((uint64_t)1 << 27)
#define SX_MEASURE_SPACE   ((uint64_t)1 << 28)
#define SX_MEASURE_PUNCT   ((uint64_t)1 << 29)
#define SX_MEASURE_CONTROL ((uint64_t)1 << 30)
#define SX_MEASURE_HIGH    ((uint64_t)1 << 31)
typedef struct sx_measure_info { uint64_t findings, bytes, chars, wide, ascii; } sx_measure_info;
int  sx_result_measure_device(sx_ctx* ctx, const sx_result* r, uint32_t flags, sx_labels** out, sx_measure_info* info /* may be NULL */);
int  sx_measure_bytes(const uint8_t* s, uint64_t len, uint32_t flags, uint64_t* word);

/* WHAT AN ENCODED STRING HOLDS: sx_result_decode_device.  *out (sx_result_free) is a new result in HBM with the findings of r in the
 * same order, every string that decodes under `kind` replaced by the bytes it stands for; a string that does not decode keeps its
 * bytes, copied.  Every operation above then works on the decoded bytes — a label set on what a base64 -EncodedCommand says —, and
 * sx_labels_rebind carries an answer back to the encoded originals, and the call's own words forth to *out.  The output follows
 * sx_result_fold_device's contract: output segment i corresponds to source segment i record for record — the same number of records
 * of the same type, the same sx_segment_info, every field of a record but str_off and str_len as it was, the strings back to back in
 * record order —, and no string is empty.
 * THE RULE.  A string s of n bytes gives raw bytes D, or does not decode:
 *   SX_DECODE_BASE64   pad = the number of trailing '=', two at most; body = the rest, of m bytes.  s decodes iff m >= 2, m % 4 != 1,
 *                      pad == 0 or (m + pad) % 4 == 0, every body byte is of A-Za-z0-9 or one of + / - _, and the body does not hold
 *                      both a byte of "+/" and a byte of "-_".  Unpadded input decodes (a JWT's segments); the bits left over behind
 *                      the last whole byte are dropped whatever they are.  In Python: base64.b64decode(body.translate(
 *                      bytes.maketrans(b"-_", b"+/")) + b"=" * (-m % 4), validate=True).
 *   SX_DECODE_HEX      n is even, n >= 2, every byte is a hex digit of either case: binascii.unhexlify(s).
 *   SX_DECODE_PERCENT  from the left, '%' with two hex digits behind it inside the string is that byte and the walk goes on three
 *                      bytes further; any other byte is copied, '+' stays '+'.  s decodes iff at least one escape was decoded:
 *                      urllib.parse.unquote_to_bytes(s).
 * flags: 0, the output is D; SX_DECODE_UTF16LE, D is read as UTF-16LE and written as UTF-8 — D.decode("utf-16-le").encode("utf-8") —,
 * and an odd length or a lone surrogate makes the whole string "does not decode"; a BOM is an ordinary U+FEFF.
 * THE WORD of a finding, 0 where its string does not decode:
 *   bit 0    SX_DECODE_OK       the string decodes
 *   bit 1    SX_DECODE_TEXT     every OUTPUT byte is 0x20..0x7E, 0x09, 0x0A or 0x0D.  Most identifiers are valid base64:
 *                               sx_result_select_labels_device with all = SX_DECODE_OK | SX_DECODE_TEXT is the filter to use
 *   bit 2    SX_DECODE_WIDE     D, before any transcoding, has an even length >= 2, every odd-index byte 0 and every even-index byte
 *                               of the TEXT class: a second call with SX_DECODE_UTF16LE is worth making
 *   bit 3    SX_DECODE_PADDED   base64 only: pad > 0
 *   bit 4    SX_DECODE_URLSAFE  base64 only: the body held '-' or '_'
 *   bits 32..63  SX_DECODE_LEN_SHIFT, 32 bits   the output's length in bytes
 * *words (may be NULL; sx_labels_free): one word per finding of r, laid out and bound to r exactly as sx_result_measure_device's; it
 * is no selection and ages nothing.  The call itself counts as a selection exactly as sx_result_fold_device does; a call that returns
 * an error takes no turn and writes no block.  r is read, never moved.
 * *info (may be NULL): findings; decoded, text, wide = the findings whose word has SX_DECODE_OK, SX_DECODE_TEXT, SX_DECODE_WIDE;
 * bytes_in = the source strings' bytes, bytes_out = the output strings'.
 * SX_DECODE_UTF16LE can GROW a string: base64 to 9/8 of its source, percent towards 3/2.  Sources and SX_E_STATE exactly as
 * sx_result_fold_device.  SX_E_INVALID (sx_last_error says which): a NULL pointer, an unknown kind or flag, a segment whose output
 * strings have 2^32 bytes or more, a packed segment with an output string longer than 65535 bytes — decided before anything is
 * written.  SX_E_NOMEM: a block, the words or the tables cannot be had.  *out = NULL and *words = NULL on every error.
 *
 * sx_decode_bytes: the same rule, the same code, for one byte string on the host; no context.  The output goes to out[0, *written);
 * out = NULL asks for the size: *written = the output's length, nothing is written.  A string that does not decode is no error:
 * SX_OK, *word = 0, and the output is the source, copied.  *word (may be NULL): the string's word.  SX_E_INVALID: a NULL pointer (in
 * may be NULL where len is 0), an unknown kind or flag, len >= 2^32, or cap < the output's length — then *written says what is
 * needed and out is untouched.
 * Not built: base32, uuencode, quoted-printable; white space or line breaks inside base64; a 0x prefix or \x escapes; UTF-16BE; a
 * well-formed-UTF-8 bit; nested decoding in one call; sharded entry points; a packed segment expanded where an output outgrows it. */
enum { SX_DECODE_BASE64 = 1u, SX_DECODE_HEX = 2u, SX_DECODE_PERCENT = 3u };   /* kind */
enum { SX_DECODE_UTF16LE = 1u };                                               /* flags */
#define SX_DECODE_OK      ((uint64_t)1 << 0)
#define SX_DECODE_TEXT    ((uint64_t)1 << 1)
#define SX_DECODE_WIDE    ((uint64_t)1 << 2)
#define SX_DECODE_PADDED  ((uint64_t)1 << 3)
#define SX_DECODE_URLSAFE ((uint64_t)1 << 4)
#define SX_DECODE_LEN_SHIFT 32
typedef struct sx_decode_info { uint64_t findings, decoded, text, wide, bytes_in, bytes_out; } sx_decode_info;
int  sx_result_decode_device(sx_ctx* ctx, const sx_result* r, uint32_t kind, uint32_t flags, sx_result** out,
                             sx_labels** words /* may be NULL */, sx_decode_info* info /* may be NULL */);
int  sx_decode_bytes(uint32_t kind, uint32_t flags, const uint8_t* in, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* written,
                     uint64_t* word /* may be NULL */);

/* The APPROXIMATE MATCHES of a result whose segments ALL lie in HBM: for every finding, WHICH keywords of a list occur in its string
 * with at most k errors — `agrep` / `tre-agrep` behind `strings`: a flipped byte, a dropped character, `passw0rd` —, as one 64-bit
 * word, made where the findings lie (csrc/sx_fuzzy_dev.hip) with no string byte crossing PCIe.  The word is a label: everything that
 * takes the labels of sx_result_label_device takes these.
 * THE RULE.  A FUZZY SET holds 1..SX_FUZZY_MAX_PATTERNS patterns.  Pattern p owns bit p, has a byte string of
 * 1..SX_FUZZY_MAX_PATTERN_BYTES bytes, and has its own error budget k_p with 0 <= k_p <= SX_FUZZY_MAX_ERRORS and k_p < len_p.
 * Bit p of finding i's word is set iff some substring of the finding's string has Levenshtein distance at most k_p from pattern p.
 * The string is the UTF-8 the result holds, arena[str_off, str_off + str_len).
 *   - A substring is any contiguous byte range, the empty one included.
 *   - Insertion, deletion and substitution of one BYTE each cost 1.
 *   - This is Sellers' table: row 0 all zeros, D[i][j] = min(D[i-1][j-1] + (P[i] != T[j]), D[i-1][j] + 1, D[i][j-1] + 1).  The bit is
 *     set iff min_j D[m][j] <= k.
 *   - k_p < len_p makes the empty substring never a match, so an empty string's word is 0.
 *   - With SX_SELECT_ASCII_NOCASE, 'A'..'Z' and 'a'..'z' compare equal in both pattern and string.  No other byte is folded.
 *   - Distances are in bytes, not characters.  One wrong Cyrillic letter costs up to 2.
 *   - Bits of patterns the set lacks are 0.
 *   - A match never spans two findings.
 *   - k = 0 is exactly the substring selection.
 * sx_fuzzy_set_create builds, on the host (csrc/sx_fuzzy_build.hpp), a byte-class map and one 64-bit mask per class and pattern — bit
 * i: byte i of the pattern is of that class — and puts them into HBM on the context's device, with len_p and k_p per pattern
 * (max_errors[p] = k_p) and two counters per pattern.  flags: 0 or SX_SELECT_ASCII_NOCASE, compiled into the set.  SX_E_INVALID, with
 * a text in sx_last_error that names the pattern's index where one is at fault: an empty pattern, more than 64 bytes, k > 8, k >= len,
 * n_patterns outside 1..64, unknown flags, a NULL pointer.  SX_E_STATE: a host-only context.  *out = NULL on every error.  The set
 * owns its device memory, masks and counters, and does not depend on the context's lifetime: it may be freed before or after
 * sx_destroy, and used with any context on the same HIP device (another device: SX_E_INVALID).
 * sx_fuzzy_set_info_get: what was built — classes: class 0, "no pattern holds this byte", and one per distinct byte value of the
 * patterns (after the case union), ordered by how many pattern positions hold them; the masks of the first lds_classes classes are
 * what the kernel keeps in LDS, the rarest it reads through L2, so no set is refused for its size; table_bytes in HBM (everything
 * but the counters); max_len and max_errors over the patterns.
 * THE WALK is Myers' bit-vector form of Sellers' table (a column of the table as two bit vectors and the score of its last row), a
 * lane per string, the same work per byte whatever k is; a lane takes the set's patterns in groups and walks its string once per
 * group, and leaves a group when all its bits are set.  str_len < len_p - k_p cannot match and is not walked.
 * THE COUNTERS, per pattern, are the label set's: findings[p] = the number of findings with bit p; first[p] = the smallest
 * (ordinal_base + index of the finding in the result's print order) among them, or SX_LABEL_NEVER if there is none.  A new set is
 * reset.  sx_result_fuzzy_device ADDS to them, so a stream scanned buffer by buffer gives one count of the whole stream if the caller
 * passes the number of findings of the buffers before as ordinal_base; sums and minima: they are deterministic.
 * sx_result_fuzzy_device makes *out, the words of r's findings (sx_labels_free), under sx_result_label_device's contract, word for
 * word: the sources are exactly what sx_print_findings_device accepts — both record types, any layout of the strings, the result of
 * any selection, extraction, order or fold —, and SX_E_STATE comes back wherever that function would refuse the source, decided for ALL
 * segments before anything is launched; one array of words per source segment, bound to r, which sx_result_select_labels_device,
 * sx_result_select_labels_range_device, sx_result_order_device and sx_labels_rebind take unchanged; the source is read, never moved;
 * the call is no selection and ages none; it returns when the kernels are done.  SX_E_INVALID: a NULL pointer, a set on another
 * device.  SX_E_NOMEM: the words cannot be allocated; nothing is counted then.  *out is NULL on every error.
 * sx_fuzzy_set_reset, sx_fuzzy_set_read, sx_fuzzy_set_counters_device: as the label set's.
 * sx_fuzzy_bytes: the word of ONE string s[0, len) for the patterns, by the same lane code on the host — no GPU, no context —;
 * SX_E_INVALID (*word = 0) for what sx_fuzzy_set_create refuses, a NULL pointer (s may be NULL if len is 0) or len >= 2^32.
 * Not thread-safe: one sx_result_fuzzy_device call per set at a time, and no reset or read during it.
 * Not built: distance in characters; the best distance per pattern as a field of the word; where the match lies; transpositions as
 * one error; patterns of more than 64 bytes; more than 64 patterns; Unicode folding inside the call (sx_result_fold_device in front
 * of it, sx_labels_rebind behind); the sharded entry points. */
#define SX_FUZZY_MAX_PATTERNS      64u
#define SX_FUZZY_MAX_PATTERN_BYTES 64u
#define SX_FUZZY_MAX_ERRORS        8u
typedef struct sx_fuzzy_set sx_fuzzy_set;   /* compiled patterns + their counters, in HBM */
typedef struct sx_fuzzy_set_info {
    uint32_t n_patterns, classes, lds_classes, nocase;
    uint64_t table_bytes;     /* everything the set holds in HBM except the counters */
    uint32_t max_len, max_errors;
} sx_fuzzy_set_info;
int  sx_fuzzy_set_create(sx_ctx* ctx, const sx_pattern* patterns, const uint8_t* max_errors, uint32_t n_patterns, uint32_t flags, sx_fuzzy_set** out);
int  sx_fuzzy_set_info_get(const sx_fuzzy_set* set, sx_fuzzy_set_info* out);
void sx_fuzzy_set_free(sx_fuzzy_set* set);
int  sx_fuzzy_set_reset(sx_fuzzy_set* set);
int  sx_fuzzy_set_read(const sx_fuzzy_set* set, uint64_t* findings, uint64_t* first, uint32_t n_patterns);
int  sx_fuzzy_set_counters_device(const sx_fuzzy_set* set, const uint64_t** d_findings, const uint64_t** d_first);
int  sx_result_fuzzy_device(sx_ctx* ctx, const sx_result* r, sx_fuzzy_set* set, uint64_t ordinal_base, sx_labels** out);
int  sx_fuzzy_bytes(const sx_pattern* patterns, const uint8_t* max_errors, uint32_t n_patterns, uint32_t flags, const uint8_t* s, uint64_t len, uint64_t* word);

int  sx_get_stats(const sx_ctx* ctx, sx_stats* out); /* of the last scan call */
void sx_free(void* p);

/* Synthetic input: fills device memory with the background
 * byte stream, byte i = little-endian byte (i&7) of splitmix64-mix(seed + ((i>>3)+1)*phi). */
int sx_fill_background_device(sx_ctx* ctx, void* device_bytes, uint64_t first_byte_index,
                              uint64_t len, uint64_t seed);
/* Device memory helpers so that callers without a HIP binding can stage data. */
int sx_device_alloc(sx_ctx* ctx, uint64_t bytes, void** device_ptr);
int sx_device_free(sx_ctx* ctx, void* device_ptr);
int sx_device_upload(sx_ctx* ctx, void* device_dst, const void* host_src, uint64_t bytes);
int sx_device_download(sx_ctx* ctx, void* host_dst, const void* device_src, uint64_t bytes);
/* Read-only streaming pass over a device buffer (measured HBM read ceiling). */
int sx_device_read_bandwidth(sx_ctx* ctx, const void* device_bytes, uint64_t len, int repeats,
                             double* gbytes_per_s);

#ifdef __cplusplus
}
#endif
#endif
