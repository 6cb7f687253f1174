"""stringsext_amd — MI355X-native replacement for stringsext's per-Mission byte-stream scan.

This package is only a ctypes shim over the C-ABI in include/stringsext_amd.h
(libstringsext_amd.so: hand-written HIP kernels for gfx950 + a C++ host that
replays the reference's exact window semantics around the runs the device
reports).  Names follow the reference: Mission (src/mission.rs:382-421),
Finding / Precision (src/finding.rs:34-74).  There is no CPU fallback: creating a
Scanner without a HIP device raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SX_LIB") or os.path.join(_HERE, "libstringsext_amd.so")  # SX_LIB: debugging builds

SX_OK, SX_E_INVALID, SX_E_NO_DEVICE, SX_E_HIP, SX_E_NOMEM, SX_E_STATE, SX_E_HALO = 0, -1, -2, -3, -4, -5, -6
SX_HOST_ONLY = -1
SX_OPT_GENERIC_KERNELS, SX_OPT_DEVICE_REPLAY, SX_OPT_HOST_REPLAY = 1, 2, 4
SX_OPT_NO_FUSED_SCAN = 64      # round 6: one scan launch per Mission instead of the fused one (one read of the buffer for several Missions)
SX_SELECT_MAX_PATTERNS, SX_SELECT_MAX_PATTERN_BYTES = 16, 64   # sx_result_select_device (Result.select_device)
SX_SELECT_ASCII_NOCASE, SX_SELECT_INVERT = 1, 2
SX_SELECT_SET_MAX_PATTERNS, SX_SELECT_SET_MAX_PATTERN_BYTES, SX_SELECT_SET_MAX_TOTAL_BYTES = 65536, 255, 1 << 20   # sx_select_set_create (Scanner.pattern_set)
# sx_select_regex_create (Scanner.regex_set)
SX_SELECT_REGEX_MAX_PATTERNS, SX_SELECT_REGEX_MAX_PATTERN_BYTES, SX_SELECT_REGEX_MAX_REPEAT = 64, 1024, 255
SX_SELECT_REGEX_MAX_POSITIONS, SX_SELECT_REGEX_MAX_STATES = 65536, 65536
SX_TALLY_NEVER = (1 << 64) - 1   # sx_tally_set_read: first[k] of a keyword without a hit
SX_LABEL_NEVER = (1 << 64) - 1   # sx_label_set_read: first[p] of a pattern without a finding
SX_DISTINCT_FIRST, SX_DISTINCT_REPEATED, SX_DISTINCT_COUNT_SHIFT = 1, 2, 32   # sx_result_distinct_device (Result.distinct_device): a word's bits
SX_DISTINCT_SEEN, SX_SEEN_LOOKUP_ONLY = 4, 0x100   # sx_result_seen_device (Result.seen_device): bit 2 of a word, and the call flag "mark, add nothing"
SX_SEEN_BLOB_HEADER_BYTES, SX_SEEN_BLOB_VERSION = 64, 1   # sx_seen_set_export (SeenSet.export): the header of a saved set
# a set that counts (Scanner.seen_set(counted=True)): the create flag, the two halves of a count word, and its blob's version
SX_SEEN_COUNTED, SX_SEEN_RESULTS_SHIFT, SX_SEEN_FINDINGS_SHIFT, SX_SEEN_BLOB_VERSION_COUNTED = 0x200, 0, 32, 2
# sx_result_order_device (Result.order_device): the key, and the flags
SX_ORDER_BY_STRING, SX_ORDER_BY_LABEL_FIELD, SX_ORDER_DESCENDING, SX_ORDER_NOCASE = 0, 1, 1, 2
SX_FOLD_SIMPLE = 0   # sx_result_fold_device (Result.fold_device), sx_fold_utf8 (fold): Unicode simple case folding, the only rule yet
# sx_result_measure_device (Result.measure_device), sx_measure_bytes (measure): the fields and the class bits of a word
SX_MEASURE_ENTROPY_SHIFT, SX_MEASURE_DISTINCT_SHIFT, SX_MEASURE_CHARS_SHIFT = 0, 16, 32
SX_MEASURE_LOWER, SX_MEASURE_UPPER, SX_MEASURE_DIGIT, SX_MEASURE_SPACE = 1 << 25, 1 << 26, 1 << 27, 1 << 28
SX_MEASURE_PUNCT, SX_MEASURE_CONTROL, SX_MEASURE_HIGH = 1 << 29, 1 << 30, 1 << 31
# sx_result_decode_device (Result.decode_device), sx_decode_bytes (decode): the kinds, the flag, a word's bits and its length field
SX_DECODE_BASE64, SX_DECODE_HEX, SX_DECODE_PERCENT, SX_DECODE_UTF16LE = 1, 2, 3, 1
SX_DECODE_OK, SX_DECODE_TEXT, SX_DECODE_WIDE, SX_DECODE_PADDED, SX_DECODE_URLSAFE, SX_DECODE_LEN_SHIFT = 1, 2, 4, 8, 16, 32
DECODE_KINDS = {"base64": SX_DECODE_BASE64, "hex": SX_DECODE_HEX, "percent": SX_DECODE_PERCENT}
SX_FUZZY_MAX_PATTERNS, SX_FUZZY_MAX_PATTERN_BYTES, SX_FUZZY_MAX_ERRORS = 64, 64, 8   # sx_fuzzy_set_create (Scanner.fuzzy_set), sx_fuzzy_bytes (fuzzy)
SX_OPT_RESULT_ON_DEVICE = 32   # a buffer's result stays in HBM (Result.device_segments): one Mission's block, or several Missions' merged parts
ENC = {"x-user-defined": 0, "utf-8": 1, "utf-16le": 2, "utf-16be": 3, "koi8-r": 16, "ibm866": 17,
       "iso-8859-2": 18, "iso-8859-5": 19, "iso-8859-15": 20, "windows-1251": 21, "windows-1252": 22,
       "iso-8859-3": 23, "iso-8859-4": 24, "iso-8859-6": 25, "iso-8859-7": 26, "iso-8859-8": 27,
       "iso-8859-8-i": 28, "iso-8859-10": 29, "iso-8859-13": 30, "iso-8859-14": 31, "iso-8859-16": 32,
       "koi8-u": 33, "macintosh": 34, "windows-874": 35, "windows-1250": 36, "windows-1253": 37,
       "windows-1254": 38, "windows-1255": 39, "windows-1256": 40, "windows-1257": 41, "windows-1258": 42,
       "x-mac-cyrillic": 43, "big5": 64, "euc-jp": 65, "shift_jis": 66, "euc-kr": 67, "gb18030": 68, "gbk": 69, "replacement": 70}
PRECISION = {0: "Before", 1: "Exact", 2: "After"}

# every symbol include/stringsext_amd.h declares
ABI_VERSION = 4   # SX_ABI_VERSION of include/stringsext_amd.h
EXPORTS = ["sx_abi_version", "sx_create", "sx_destroy", "sx_last_error", "sx_scan", "sx_scan_device", "sx_reset",
           "sx_device_runs", "sx_device_runs_multi", "sx_replay_runs", "sx_scan_shard_device", "sx_scan_shard", "sx_replay_shard_runs",
           "sx_scan_stream", "sx_scan_file", "sx_missions_from_flags", "sx_parse_enc_opt", "sx_encoding_for_label", "sx_encoding_name",
           "sx_decoder_table", "sx_wave_classes", "sx_scan_classifier", "sx_result_segment_packed", "sx_wave_swar", "sx_wave_pair_codes2", "sx_wave_pair_codes", "sx_shard_bounds", "sx_scan_sharded", "sx_shard_splice", "sx_shard_splice_segs", "sx_transport_rccl_id", "sx_transport_rccl_create", "sx_transport_destroy", "sx_transport_last_error", "sx_transport_allgather", "sx_transport_gather",
           "sx_result_count", "sx_result_segments", "sx_result_segment", "sx_result_segment_device", "sx_result_findings", "sx_result_arena",
           "sx_result_free", "sx_print_findings", "sx_print_findings_device", "sx_result_select_device",
           "sx_select_set_create", "sx_select_set_info_get", "sx_select_set_free", "sx_result_select_set_device", "sx_select_regex_create", "sx_select_regex_info_get", "sx_select_regex_free",
           "sx_result_select_regex_device", "sx_extract_regex_create", "sx_extract_regex_info_get", "sx_extract_regex_free",
           "sx_result_extract_regex_device", "sx_tally_set_create", "sx_tally_set_info_get", "sx_tally_set_free", "sx_tally_set_reset",
           "sx_result_tally_device", "sx_tally_set_read", "sx_tally_set_counters_device",
           "sx_label_set_create", "sx_label_set_info_get", "sx_label_set_free", "sx_label_set_reset", "sx_label_set_read", "sx_label_set_counters_device",
           "sx_result_label_device", "sx_labels_segment_device", "sx_labels_segments", "sx_labels_free", "sx_result_select_labels_device", "sx_result_distinct_device",
           "sx_seen_set_create", "sx_seen_set_info_get", "sx_seen_set_reset", "sx_seen_set_free", "sx_result_seen_device",
           "sx_seen_set_merge", "sx_seen_set_grow", "sx_seen_set_export_size", "sx_seen_set_export", "sx_seen_blob_info_get", "sx_seen_set_import", "sx_seen_set_add_strings",
           "sx_result_seen_counts_device", "sx_result_select_labels_range_device", "sx_result_order_device",
           "sx_fold_utf8", "sx_result_fold_device", "sx_labels_rebind", "sx_result_measure_device", "sx_measure_bytes",
           "sx_result_decode_device", "sx_decode_bytes",
           "sx_fuzzy_set_create", "sx_fuzzy_set_info_get", "sx_fuzzy_set_free", "sx_fuzzy_set_reset", "sx_fuzzy_set_read", "sx_fuzzy_set_counters_device",
           "sx_result_fuzzy_device", "sx_fuzzy_bytes",
           "sx_get_stats", "sx_free", "sx_fill_background_device",
           "sx_device_alloc", "sx_device_free", "sx_device_upload", "sx_device_download",
           "sx_device_read_bandwidth"]


class Mission(C.Structure):
    """sx_mission — the fields of `Mission` the scan reads."""
    _fields_ = [("mission_id", C.c_uint8), ("encoding", C.c_uint8), ("chars_min_nb", C.c_uint8),
                ("require_same_unicode_block", C.c_uint8), ("grep_char", C.c_int16),
                ("print_encoding_as_ascii", C.c_uint8), ("reserved", C.c_uint8),
                ("output_line_char_nb_max", C.c_uint32), ("af_lo", C.c_uint64), ("af_hi", C.c_uint64),
                ("ubf", C.c_uint64), ("counter_offset", C.c_uint64)]

    @classmethod
    def from_dict(cls, d):
        m = cls()
        m.mission_id = d["mission_id"]
        m.encoding = d["encoding"]
        m.chars_min_nb = d["chars_min_nb"]
        m.require_same_unicode_block = 1 if d["require_same_unicode_block"] else 0
        m.grep_char = -1 if d["grep_char"] is None else d["grep_char"]
        m.print_encoding_as_ascii = 1 if d["print_encoding_as_ascii"] else 0
        m.output_line_char_nb_max = d["output_line_char_nb_max"]
        m.af_lo = d["af"] & 0xFFFFFFFFFFFFFFFF
        m.af_hi = d["af"] >> 64
        m.ubf = d["ubf"]
        m.counter_offset = d["counter_offset"]
        return m

    def to_dict(self):
        return dict(mission_id=self.mission_id, encoding=self.encoding, chars_min_nb=self.chars_min_nb,
                    require_same_unicode_block=bool(self.require_same_unicode_block),
                    grep_char=None if self.grep_char < 0 else self.grep_char,
                    af=(self.af_hi << 64) | self.af_lo, ubf=self.ubf,
                    output_line_char_nb_max=self.output_line_char_nb_max, counter_offset=self.counter_offset,
                    print_encoding_as_ascii=bool(self.print_encoding_as_ascii))


class CliFlags(C.Structure):
    """sx_cli_flags — the option strings of the reference's command line (src/options.rs:46-90)."""
    _fields_ = [("counter_offset", C.c_char_p), ("encodings", C.POINTER(C.c_char_p)), ("n_encodings", C.c_int),
                ("chars_min", C.c_char_p), ("same_unicode_block", C.c_int), ("ascii_filter", C.c_char_p),
                ("unicode_block_filter", C.c_char_p), ("grep_char", C.c_char_p), ("output_line_len", C.c_char_p)]


class EncOpt(C.Structure):
    _fields_ = [("has_name", C.c_int), ("name", C.c_char * 64), ("has_chars_min", C.c_int), ("chars_min", C.c_uint8),
                ("has_af", C.c_int), ("af_lo", C.c_uint64), ("af_hi", C.c_uint64), ("has_ubf", C.c_int), ("ubf", C.c_uint64),
                ("has_grep_char", C.c_int), ("grep_char", C.c_uint8)]


def missions_from_flags(encodings=(), chars_min=None, same_unicode_block=False, ascii_filter=None,
                        unicode_block_filter=None, grep_char=None, output_line_len=None, counter_offset=None):
    """Missions::new (src/mission.rs:514-703) through the C-ABI: option strings -> mission dicts.
    Raises SxError with the reference's message on a bad option."""
    enc = [e.encode() for e in encodings]
    arr = (C.c_char_p * max(1, len(enc)))(*enc)
    b = lambda v: None if v is None else str(v).encode()
    f = CliFlags(b(counter_offset), arr, len(enc), b(chars_min), int(bool(same_unicode_block)), b(ascii_filter),
                 b(unicode_block_filter), b(grep_char), b(output_line_len))
    out = (Mission * 32)()
    n = C.c_int()
    err = C.create_string_buffer(512)
    L = lib()
    L.sx_missions_from_flags.argtypes = [C.POINTER(CliFlags), C.POINTER(Mission), C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    rc = L.sx_missions_from_flags(C.byref(f), out, 32, C.byref(n), err, 512)
    if rc != SX_OK:
        raise SxError(rc, err.value.decode())
    return [out[i].to_dict() for i in range(n.value)]


def encoding_name(enc):
    """Encoding::name() of an SX_ENC_* id (None if unknown)."""
    L = lib()
    L.sx_encoding_name.argtypes, L.sx_encoding_name.restype = [C.c_uint32], C.c_char_p
    s = L.sx_encoding_name(enc)
    return s.decode() if s else None


def decoder_table(enc):
    """The decoder table of a legacy encoding as a ctypes uint16 array view (None if it has none)."""
    L = lib()
    L.sx_decoder_table.argtypes, L.sx_decoder_table.restype = [C.c_uint32, C.POINTER(C.c_uint64)], C.POINTER(C.c_uint16)
    n = C.c_uint64()
    t = L.sx_decoder_table(enc, C.byref(n))
    return (t, n.value) if n.value else None


def encoding_for_label(label):
    """Encoding::for_label: SX_ENC_* id; -1 not a label; -2 a label of an encoding that is not built in."""
    L = lib()
    L.sx_encoding_for_label.argtypes, L.sx_encoding_for_label.restype = [C.c_char_p], C.c_int
    return L.sx_encoding_for_label(label.encode())


def parse_enc_opt(text):
    """Missions::parse_enc_opt (src/mission.rs:713-749): (name, chars_min, af, ubf, grep_char), None where absent."""
    o = EncOpt()
    err = C.create_string_buffer(512)
    L = lib()
    L.sx_parse_enc_opt.argtypes = [C.c_char_p, C.POINTER(EncOpt), C.c_char_p, C.c_size_t]
    rc = L.sx_parse_enc_opt(text.encode(), C.byref(o), err, 512)
    if rc != SX_OK:
        raise SxError(rc, err.value.decode())
    return (o.name.decode() if o.has_name else None, o.chars_min if o.has_chars_min else None,
            ((o.af_hi << 64) | o.af_lo) if o.has_af else None, o.ubf if o.has_ubf else None,
            o.grep_char if o.has_grep_char else None)


class Finding(C.Structure):
    _fields_ = [("position", C.c_uint64), ("str_off", C.c_uint32), ("str_len", C.c_uint32),
                ("precision", C.c_uint8), ("completes_previous", C.c_uint8), ("mission_id", C.c_uint8),
                ("reserved", C.c_uint8), ("input_file_id", C.c_int16), ("reserved2", C.c_uint16),
                ("slice_index", C.c_uint32)]


class Finding16(C.Structure):   # sx_finding16: a finding as string-dense results cross PCIe
    _fields_ = [("position", C.c_uint64), ("str_off", C.c_uint32), ("str_len", C.c_uint16), ("flags", C.c_uint8), ("mission_id", C.c_uint8)]


class SegmentInfo(C.Structure):   # sx_segment_info
    _fields_ = [("packed", C.c_int32), ("input_file_id", C.c_int32), ("slice_base", C.c_uint32), ("reserved", C.c_uint32),
                ("position0", C.c_uint64 * 256)]


class Pattern(C.Structure):   # sx_pattern
    _fields_ = [("bytes", C.c_char_p), ("len", C.c_uint32)]


class SelectSetInfo(C.Structure):   # sx_select_set_info
    _fields_ = [("n_patterns", C.c_uint32), ("states", C.c_uint32), ("classes", C.c_uint32), ("nocase", C.c_uint32),
                ("table_bytes", C.c_uint64), ("lds_states", C.c_uint32), ("reserved", C.c_uint32)]


class SelectRegexInfo(C.Structure):   # sx_select_regex_info
    _fields_ = [("n_patterns", C.c_uint32), ("states", C.c_uint32), ("classes", C.c_uint32), ("nocase", C.c_uint32),
                ("table_bytes", C.c_uint64), ("lds_states", C.c_uint32), ("end_states", C.c_uint32)]


class ExtractRegexInfo(C.Structure):   # sx_extract_regex_info
    _fields_ = [("n_patterns", C.c_uint32), ("states", C.c_uint32), ("classes", C.c_uint32), ("nocase", C.c_uint32),
                ("table_bytes", C.c_uint64), ("lds_states", C.c_uint32), ("reserved", C.c_uint32)]


class TallySetInfo(C.Structure):   # sx_tally_set_info
    _fields_ = [("n_patterns", C.c_uint32), ("unique", C.c_uint32), ("states", C.c_uint32), ("classes", C.c_uint32),
                ("nocase", C.c_uint32), ("entry_bytes", C.c_uint32), ("table_bytes", C.c_uint64), ("lds_states", C.c_uint32),
                ("reserved", C.c_uint32)]


class LabelSetInfo(C.Structure):   # sx_label_set_info
    _fields_ = [("n_patterns", C.c_uint32), ("states", C.c_uint32), ("classes", C.c_uint32), ("nocase", C.c_uint32),
                ("table_bytes", C.c_uint64), ("lds_states", C.c_uint32), ("here_states", C.c_uint32)]


class FuzzySetInfo(C.Structure):   # sx_fuzzy_set_info
    _fields_ = [("n_patterns", C.c_uint32), ("classes", C.c_uint32), ("lds_classes", C.c_uint32), ("nocase", C.c_uint32),
                ("table_bytes", C.c_uint64), ("max_len", C.c_uint32), ("max_errors", C.c_uint32)]


class OrderSpec(C.Structure):   # sx_order_spec
    _fields_ = [("by", C.c_uint32), ("flags", C.c_uint32), ("shift", C.c_uint32), ("bits", C.c_uint32), ("any", C.c_uint64), ("all", C.c_uint64),
                ("none", C.c_uint64), ("limit", C.c_uint64)]


class OrderInfo(C.Structure):   # sx_order_info
    _fields_ = [("findings", C.c_uint64), ("kept", C.c_uint64), ("rounds", C.c_uint64), ("tied", C.c_uint64), ("max_depth", C.c_uint64)]


class FoldInfo(C.Structure):   # sx_fold_info
    _fields_ = [("findings", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("changed", C.c_uint64)]


class MeasureInfo(C.Structure):   # sx_measure_info
    _fields_ = [("findings", C.c_uint64), ("bytes", C.c_uint64), ("chars", C.c_uint64), ("wide", C.c_uint64), ("ascii", C.c_uint64)]


class DecodeInfo(C.Structure):   # sx_decode_info
    _fields_ = [("findings", C.c_uint64), ("decoded", C.c_uint64), ("text", C.c_uint64), ("wide", C.c_uint64), ("bytes_in", C.c_uint64),
                ("bytes_out", C.c_uint64)]


class DistinctInfo(C.Structure):   # sx_distinct_info
    _fields_ = [("findings", C.c_uint64), ("distinct", C.c_uint64), ("repeated", C.c_uint64), ("rounds", C.c_uint32), ("table_log2", C.c_uint32)]


class SeenSetInfo(C.Structure):   # sx_seen_set_info
    _fields_ = [("strings", C.c_uint64), ("bytes", C.c_uint64), ("capacity_strings", C.c_uint64), ("capacity_bytes", C.c_uint64),
                ("table_log2", C.c_uint32), ("nocase", C.c_uint32), ("tag_bits", C.c_uint32), ("counted", C.c_uint32)]


class SeenInfo(C.Structure):   # sx_seen_info
    _fields_ = [("findings", C.c_uint64), ("distinct", C.c_uint64), ("repeated", C.c_uint64), ("seen_findings", C.c_uint64), ("seen_distinct", C.c_uint64),
                ("added_strings", C.c_uint64), ("added_bytes", C.c_uint64), ("rounds", C.c_uint32), ("table_log2", C.c_uint32)]


class SeenMergeInfo(C.Structure):   # sx_seen_merge_info
    _fields_ = [("source_strings", C.c_uint64), ("already_held", C.c_uint64), ("added_strings", C.c_uint64), ("added_bytes", C.c_uint64)]


class SeenBlobInfo(C.Structure):   # sx_seen_blob_info
    _fields_ = [("strings", C.c_uint64), ("bytes", C.c_uint64), ("nocase", C.c_uint32), ("version", C.c_uint32)]


class Run(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("chars", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("bytes_scanned", C.c_uint64), ("run_records", C.c_uint64), ("replay_bytes", C.c_uint64),
                ("findings", C.c_uint64), ("kernel_ms", C.c_double * 16), ("device_ms", C.c_double),
                ("h2d_ms", C.c_double), ("d2h_ms", C.c_double), ("replay_ms", C.c_double),
                ("total_ms", C.c_double), ("heavy_tiles", C.c_uint64), ("wave_windows", C.c_uint64),
                ("wave_count_ms", C.c_double), ("wave_write_ms", C.c_double), ("rescans", C.c_uint64), ("rescan_ms", C.c_double),
                ("wave_desc_overflows", C.c_uint64), ("seq_pieces", C.c_uint64),
                ("fast_regions", C.c_uint64), ("general_regions", C.c_uint64), ("wave_repairs", C.c_uint64),
                ("fused_ms", C.c_double), ("fused_launches", C.c_uint64), ("fused_mask", C.c_uint64)]


class Options(C.Structure):
    _fields_ = [("subchunk_bytes", C.c_uint32), ("record_capacity", C.c_uint32), ("replay_threads", C.c_uint32),
                ("flags", C.c_uint32)]


class SxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"stringsext_amd error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libstringsext_amd.so; fail loudly if the HIP extension was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C stringsext_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u64, cp = C.c_void_p, C.c_uint64, C.c_char_p
    L.sx_abi_version.restype = C.c_int
    if L.sx_abi_version() != ABI_VERSION:   # the ctypes structs below mirror include/stringsext_amd.h of exactly this version
        raise ImportError(f"{LIB_PATH} has ABI version {L.sx_abi_version()}, this binding is written for {ABI_VERSION}: rebuild the library")
    L.sx_create.argtypes = [C.POINTER(vp), C.POINTER(Mission), C.c_int, C.c_int, C.POINTER(Options)]
    L.sx_destroy.argtypes = [vp]
    L.sx_last_error.restype = cp
    L.sx_last_error.argtypes = [vp]
    L.sx_scan.argtypes = [vp, cp, u64, C.c_int, C.c_int, C.POINTER(vp)]
    L.sx_scan_device.argtypes = [vp, vp, u64, C.c_int, C.c_int, C.POINTER(vp)]
    L.sx_reset.argtypes = [vp]
    L.sx_device_runs.argtypes = [vp, C.c_int, vp, u64, C.c_int, u64, C.POINTER(C.POINTER(Run)), C.POINTER(u64)]
    L.sx_device_runs_multi.argtypes = [vp, C.POINTER(C.c_int), C.c_int, vp, u64, C.c_int, C.POINTER(u64), C.POINTER(C.POINTER(Run)), C.POINTER(u64)]
    L.sx_replay_runs.argtypes = [vp, cp, u64, C.c_int, C.c_int, C.POINTER(C.POINTER(Run)), C.POINTER(u64),
                                 C.POINTER(vp)]
    pu64 = C.POINTER(u64)
    L.sx_scan_shard_device.argtypes = [vp, vp, u64, u64, u64, u64, pu64, u64, C.c_int, C.c_int, C.POINTER(vp), pu64]
    L.sx_scan_shard.argtypes = [vp, cp, u64, u64, u64, u64, pu64, u64, C.c_int, C.c_int, C.POINTER(vp), pu64]
    L.sx_replay_shard_runs.argtypes = [vp, cp, u64, u64, u64, u64, pu64, u64, C.c_int, C.POINTER(C.POINTER(Run)), pu64,
                                       C.POINTER(vp), pu64]
    L.sx_result_count.restype = u64
    L.sx_result_count.argtypes = [vp]
    L.sx_result_findings.restype = C.POINTER(Finding)
    L.sx_result_findings.argtypes = [vp]
    L.sx_result_arena.restype = C.POINTER(C.c_uint8)
    L.sx_result_arena.argtypes = [vp, C.POINTER(u64)]
    L.sx_result_free.argtypes = [vp]
    L.sx_result_segments.restype = u64
    L.sx_result_segments.argtypes = [vp]
    L.sx_result_segment.argtypes = [vp, u64, C.POINTER(C.POINTER(Finding)), C.POINTER(u64),
                                    C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(u64)]
    L.sx_print_findings.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(C.c_uint8)),
                                    C.POINTER(u64)]
    L.sx_print_findings_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(u64)]
    L.sx_result_select_device.argtypes = [vp, vp, C.POINTER(Pattern), C.c_int, C.c_uint32, C.POINTER(vp)]
    L.sx_select_set_create.argtypes = [vp, C.POINTER(Pattern), C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sx_select_set_info_get.argtypes = [vp, C.POINTER(SelectSetInfo)]
    L.sx_select_set_free.argtypes, L.sx_select_set_free.restype = [vp], None
    L.sx_result_select_set_device.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(vp)]
    L.sx_select_regex_create.argtypes = [vp, C.POINTER(Pattern), C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sx_select_regex_info_get.argtypes = [vp, C.POINTER(SelectRegexInfo)]
    L.sx_select_regex_free.argtypes, L.sx_select_regex_free.restype = [vp], None
    L.sx_result_select_regex_device.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(vp)]
    L.sx_extract_regex_create.argtypes = [vp, C.POINTER(Pattern), C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sx_extract_regex_info_get.argtypes = [vp, C.POINTER(ExtractRegexInfo)]
    L.sx_extract_regex_free.argtypes, L.sx_extract_regex_free.restype = [vp], None
    L.sx_result_extract_regex_device.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(vp)]
    L.sx_tally_set_create.argtypes = [vp, C.POINTER(Pattern), C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sx_tally_set_info_get.argtypes = [vp, C.POINTER(TallySetInfo)]
    L.sx_tally_set_free.argtypes, L.sx_tally_set_free.restype = [vp], None
    L.sx_tally_set_reset.argtypes = [vp]
    L.sx_result_tally_device.argtypes = [vp, vp, vp, u64, pu64]
    L.sx_tally_set_read.argtypes = [vp, pu64, pu64, C.c_uint32]
    L.sx_tally_set_counters_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint32)]
    L.sx_label_set_create.argtypes = [vp, C.POINTER(Pattern), C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sx_label_set_info_get.argtypes = [vp, C.POINTER(LabelSetInfo)]
    L.sx_label_set_free.argtypes, L.sx_label_set_free.restype = [vp], None
    L.sx_label_set_reset.argtypes = [vp]
    L.sx_label_set_read.argtypes = [vp, pu64, pu64, C.c_uint32]
    L.sx_label_set_counters_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sx_result_label_device.argtypes = [vp, vp, vp, u64, C.POINTER(vp)]
    L.sx_labels_segment_device.argtypes = [vp, u64, C.POINTER(vp), pu64]
    L.sx_labels_segments.argtypes, L.sx_labels_segments.restype = [vp], u64
    L.sx_labels_free.argtypes, L.sx_labels_free.restype = [vp], None
    L.sx_result_select_labels_device.argtypes = [vp, vp, vp, u64, u64, u64, C.POINTER(vp)]
    L.sx_result_distinct_device.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp), C.POINTER(DistinctInfo)]
    L.sx_seen_set_create.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(vp)]
    L.sx_seen_set_info_get.argtypes = [vp, C.POINTER(SeenSetInfo)]
    L.sx_seen_set_reset.argtypes = [vp]
    L.sx_seen_set_free.argtypes, L.sx_seen_set_free.restype = [vp], None
    L.sx_result_seen_device.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(vp), C.POINTER(SeenInfo)]
    L.sx_seen_set_merge.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(SeenMergeInfo)]
    L.sx_seen_set_grow.argtypes = [vp, vp, C.c_uint64, C.c_uint64]
    L.sx_seen_set_export_size.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.sx_seen_set_export.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sx_seen_blob_info_get.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(SeenBlobInfo)]
    L.sx_seen_set_import.argtypes = [vp, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.sx_seen_set_add_strings.argtypes = [vp, vp, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.c_char_p, C.POINTER(SeenMergeInfo)]
    L.sx_result_seen_counts_device.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.sx_result_select_labels_range_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.sx_result_order_device.argtypes = [vp, vp, vp, C.POINTER(OrderSpec), C.POINTER(vp), C.POINTER(OrderInfo)]
    L.sx_fold_utf8.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sx_result_fold_device.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp), C.POINTER(FoldInfo)]
    L.sx_labels_rebind.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.sx_result_measure_device.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp), C.POINTER(MeasureInfo)]
    L.sx_measure_bytes.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.sx_result_decode_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(DecodeInfo)]
    L.sx_decode_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sx_fuzzy_set_create.argtypes = [vp, C.POINTER(Pattern), C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.sx_fuzzy_set_info_get.argtypes = [vp, C.POINTER(FuzzySetInfo)]
    L.sx_fuzzy_set_free.argtypes, L.sx_fuzzy_set_free.restype = [vp], None
    L.sx_fuzzy_set_reset.argtypes = [vp]
    L.sx_fuzzy_set_read.argtypes = [vp, pu64, pu64, C.c_uint32]
    L.sx_fuzzy_set_counters_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sx_result_fuzzy_device.argtypes = [vp, vp, vp, u64, C.POINTER(vp)]
    L.sx_fuzzy_bytes.argtypes = [C.POINTER(Pattern), C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sx_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.sx_free.argtypes = [vp]
    L.sx_fill_background_device.argtypes = [vp, vp, u64, u64, u64]
    L.sx_device_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.sx_device_free.argtypes = [vp, vp]
    L.sx_device_upload.argtypes = [vp, vp, cp, u64]
    L.sx_device_download.argtypes = [vp, vp, vp, u64]
    L.sx_device_read_bandwidth.argtypes = [vp, vp, u64, C.c_int, C.POINTER(C.c_double)]
    _lib = L
    return L


def fold(data):
    """sx_fold_utf8: `data` (bytes) under Unicode SIMPLE case folding, the rule of Result.fold_device() and the same code —
    data.decode('utf-8', 'surrogateescape'), per character c.casefold() if that is one character, else c.lower() if that is one,
    else c, .encode('utf-8', 'surrogateescape'): 'ПАРОЛЬ' -> 'пароль', 'ς' -> 'σ', U+212A -> 'k'; 'ß' and 'İ' stay, and so does every
    byte that is no well-formed UTF-8.  A caller folds its patterns with it before it looks for them in a folded Result."""
    data = bytes(data)
    n = C.c_uint64()
    rc = lib().sx_fold_utf8(data, len(data), SX_FOLD_SIMPLE, None, 0, C.byref(n))
    if rc != SX_OK:
        raise SxError(rc, "sx_fold_utf8")
    out = C.create_string_buffer(max(1, n.value))
    rc = lib().sx_fold_utf8(data, len(data), SX_FOLD_SIMPLE, out, n.value, C.byref(n))
    if rc != SX_OK:
        raise SxError(rc, "sx_fold_utf8")
    return out.raw[:n.value]


def measure(data):
    """sx_measure_bytes: the word of Result.measure_device() for `data` (bytes), by the same code — (word >> SX_MEASURE_ENTROPY_SHIFT)
    & 0xFFFF the entropy of its bytes in bits per byte x 4096, (word >> SX_MEASURE_DISTINCT_SHIFT) & 0x1FF how many different bytes
    it has, the class bits SX_MEASURE_LOWER ... SX_MEASURE_HIGH, word >> SX_MEASURE_CHARS_SHIFT the bytes outside 0x80..0xBF; 0 for
    b"".  SxError SX_E_INVALID for 2^32 bytes or more."""
    data = bytes(data)
    word = C.c_uint64()
    rc = lib().sx_measure_bytes(data, len(data), 0, C.byref(word))
    if rc != SX_OK:
        raise SxError(rc, "sx_measure_bytes")
    return word.value


def _decode_kind(kind):
    if kind not in DECODE_KINDS:
        raise ValueError("a decoding is one of %s" % ", ".join(sorted(DECODE_KINDS)))
    return DECODE_KINDS[kind]


def decode(kind, data, utf16le=False):
    """sx_decode_bytes: (the output, the word) of Result.decode_device(kind, utf16le) for `data` (bytes), by the same code and without
    a GPU.  kind: "base64" — padded or not, either alphabet —, "hex" or "percent"; utf16le: the decoded bytes are read as UTF-16LE and
    returned as UTF-8.  Where `data` does not decode, the output is `data` and the word 0; else the word has SX_DECODE_OK, SX_DECODE_TEXT
    (every output byte is printable ASCII, tab, LF or CR), SX_DECODE_WIDE (the raw bytes look like UTF-16LE text: decode again with
    utf16le=True), SX_DECODE_PADDED, SX_DECODE_URLSAFE, and word >> SX_DECODE_LEN_SHIFT is the output's length."""
    data, k, flags = bytes(data), _decode_kind(kind), SX_DECODE_UTF16LE if utf16le else 0
    n, word = C.c_uint64(), C.c_uint64()
    rc = lib().sx_decode_bytes(k, flags, data, len(data), None, 0, C.byref(n), None)
    if rc != SX_OK:
        raise SxError(rc, "sx_decode_bytes")
    out = C.create_string_buffer(max(1, n.value))
    rc = lib().sx_decode_bytes(k, flags, data, len(data), out, n.value, C.byref(n), C.byref(word))
    if rc != SX_OK:
        raise SxError(rc, "sx_decode_bytes")
    return out.raw[:n.value], word.value


def _error_budgets(max_errors, n):
    """max_errors of fuzzy_set() and fuzzy() — an int for every pattern, or one per pattern — as the n bytes the library takes"""
    ks = [max_errors] * n if isinstance(max_errors, int) else list(max_errors)
    if len(ks) != n:
        raise ValueError("max_errors is an int or has one entry per pattern")
    if any(not 0 <= k <= 255 for k in ks):
        raise ValueError("an error budget is 0..SX_FUZZY_MAX_ERRORS")
    return bytes(ks)


def fuzzy(patterns, max_errors, data, ignore_case=False):
    """sx_fuzzy_bytes: the word of Result.fuzzy_device() for `data` (bytes) and a set of these patterns, by the same code and without
    a GPU — bit p is set iff some substring of `data` is within max_errors (an int, or one per pattern) insertions, deletions and
    substitutions of a byte of patterns[p].  SxError SX_E_INVALID for what Scanner.fuzzy_set refuses, and for 2^32 bytes or more."""
    data = bytes(data)
    arr, n = _pattern_array(patterns)
    word = C.c_uint64()
    rc = lib().sx_fuzzy_bytes(arr, _error_budgets(max_errors, n), n, SX_SELECT_ASCII_NOCASE if ignore_case else 0, data, len(data), C.byref(word))
    if rc != SX_OK:
        raise SxError(rc, "sx_fuzzy_bytes")
    return word.value


class Result:
    """Findings of one sx_scan call, in the reference merger's order (src/main.rs:118-136)."""

    order_info = None      # order_device(): sx_order_info as a dict
    fold_info = None       # fold_device(): sx_fold_info as a dict
    decode_info = None     # decode_device(): sx_decode_info as a dict
    decode_words = None    # decode_device(): the Labels of the call, bound to its SOURCE

    def __init__(self, scanner, handle):
        self._s, self.h = scanner, handle

    def __len__(self):
        return lib().sx_result_count(self.h)

    def raw(self):
        """(findings array bytes, arena bytes) of the whole result as one pair (joined by a copy if it has
        several segments; raises if their strings exceed 4 GiB — read segments() then)."""
        L = lib()
        n = L.sx_result_count(self.h)
        alen = C.c_uint64()
        ap = L.sx_result_arena(self.h, C.byref(alen))
        fp = L.sx_result_findings(self.h)
        if n and not fp:   # flatten failed (sx_result_findings returns NULL): > 4 GiB of strings
            raise SxError(SX_E_INVALID, lib().sx_last_error(self._s.h).decode() or "result too large for one arena: use segments()")
        fb = C.string_at(fp, n * C.sizeof(Finding)) if n else b""
        return fb, (C.string_at(ap, alen.value) if alen.value and ap else b"")

    def segment_pointers(self):
        """[(Finding pointer, n findings, arena pointer, arena bytes)] per segment — no copies."""
        L = lib()
        out = []
        for i in range(L.sx_result_segments(self.h)):
            fp, n, ap, alen = C.POINTER(Finding)(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64()
            self._s._chk(L.sx_result_segment(self.h, i, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen)))
            out.append((fp, n.value, ap, alen.value))
        return out

    def finding_arrays(self):
        """[(Finding pointer, n)] per segment — no copies (the strings stay where they are)."""
        L = lib()
        out = []
        for i in range(L.sx_result_segments(self.h)):
            fp, n, ap, alen = C.POINTER(Finding)(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64()
            self._s._chk(L.sx_result_segment(self.h, i, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen)))
            out.append((fp, n.value))
        return out

    def packed_segments(self):
        """[(packed?, records pointer (Finding16 or Finding), n, arena bytes, SegmentInfo)] — the segments as they are stored"""
        L = lib()
        L.sx_result_segment_packed.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint8)),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(SegmentInfo)]
        out = []
        for i in range(L.sx_result_segments(self.h)):
            fp, n, ap, alen, pk, info = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64(), C.c_int(), SegmentInfo()
            self._s._chk(L.sx_result_segment_packed(self.h, i, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen), C.byref(pk), C.byref(info)))
            recs = C.cast(fp, C.POINTER(Finding16 if pk.value else Finding))
            out.append((bool(pk.value), recs, n.value, C.string_at(ap, alen.value) if alen.value else b"", info))
        return out

    def device_segments(self):
        """[(device pointer to the records or None, n, device pointer to the strings, bytes of strings, packed?, SegmentInfo)] —
        SX_OPT_RESULT_ON_DEVICE: the segments that still lie in HBM (None: that segment is in host memory).  With several Missions
        there is one segment per part of the merger, all of them on the device or none, and a segment's strings lie back to back in
        record order: str_off[0] == 0, str_off[i + 1] == str_off[i] + str_len[i] (include/stringsext_amd.h)."""
        L = lib()
        L.sx_result_segment_device.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(SegmentInfo)]
        out = []
        for i in range(L.sx_result_segments(self.h)):
            fp, n, ap, alen, pk, info = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), C.c_int(), SegmentInfo()
            self._s._chk(L.sx_result_segment_device(self.h, i, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen), C.byref(pk), C.byref(info)))
            out.append((fp.value, n.value, ap.value, alen.value, bool(pk.value), info))
        return out

    def segments(self):
        """[(Finding array, n, arena bytes)]: the result as the library holds it (no copy on the C side)."""
        L = lib()
        out = []
        for i in range(L.sx_result_segments(self.h)):
            fp, n, ap, alen = C.POINTER(Finding)(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64()
            self._s._chk(L.sx_result_segment(self.h, i, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen)))
            out.append((fp, n.value, C.string_at(ap, alen.value) if alen.value else b""))
        return out

    def findings(self):
        out = []
        for v, n, arena in self.segments():
            out += [dict(position=v[i].position, precision=PRECISION[v[i].precision],
                         s=arena[v[i].str_off:v[i].str_off + v[i].str_len].decode("utf-8"),
                         completes=bool(v[i].completes_previous), mission_id=v[i].mission_id,
                         file_id=v[i].input_file_id, slice_index=v[i].slice_index) for i in range(n)]
        return out

    def printed(self, n_inputs=1, radix=None, no_metadata=False):
        """Finding::print of every finding (src/finding.rs:112-155), without BOM / final newline."""
        out = C.POINTER(C.c_uint8)()
        n = C.c_uint64()
        self._s._chk(lib().sx_print_findings(self._s.h, self.h, n_inputs, ord(radix) if radix else 0,
                                             int(no_metadata), C.byref(out), C.byref(n)))
        b = C.string_at(out, n.value)
        lib().sx_free(out)
        return b

    def printed_device(self, n_inputs=1, radix=None, no_metadata=False):
        """(device pointer, length): the same text as printed(), written by the device into the Scanner's text block in HBM
        (sx_print_findings_device) — for a result whose segments all lie there (result_on_device=True); the result is not moved.
        Valid until the next printed_device() or scan on the Scanner.  Raises SxError (SX_E_STATE) if any segment is in host
        memory, a later scan has reused the memory or the Scanner is closed: use printed() then."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        p, n = C.c_void_p(), C.c_uint64()
        self._s._chk(lib().sx_print_findings_device(self._s.h, self.h, n_inputs, ord(radix) if radix else 0, int(no_metadata),
                                                    C.byref(p), C.byref(n)))
        return p.value, n.value

    def select_device(self, patterns, ignore_case=False, invert=False, any=0, all=0, none=0):
        """The findings whose string holds one of `patterns` (bytes, or a list of 1..16 bytes objects of 1..64 bytes each) as a
        substring — `grep -F` over the strings —, selected on the device (sx_result_select_device) out of a result whose segments
        all lie in HBM (result_on_device=True): a new Result on the device, record order kept, strings back to back, which
        device_segments(), printed_device(), select_device() (AND) and the host accessors take like a scan's.  ignore_case: 'A'..'Z'
        compare as 'a'..'z' (no other byte is folded); invert: the findings that hold NO pattern.  This Result is not moved.  The
        selection is valid until the second select_device() on the Scanner after this one (a scan does not invalidate it) or
        close().  Raises SxError: SX_E_INVALID for bad patterns, SX_E_STATE wherever printed_device() would refuse this Result.
        `patterns` may also be a PatternSet (Scanner.pattern_set: a compiled keyword list of up to 65536 patterns, grep -F -f): the
        same selection by sx_result_select_set_device; the fold belongs to the set then, and ignore_case=True raises ValueError.
        Or a RegexSet (Scanner.regex_set: up to 64 byte regular expressions, grep -E -f): sx_result_select_regex_device, with the
        same rule for the fold.  An ExtractSet is no selection (extract_device takes it): TypeError.
        Or the Labels that label_device() made of THIS Result, with the masks any, all, none (sx_result_select_labels_device): the
        findings whose label has a bit of `any` (any == 0: no such condition), every bit of `all` and no bit of `none`; no string
        byte is read.  ignore_case and invert do not apply then (ValueError), and the masks apply to nothing else (ValueError).
        Labels of another Result: SxError SX_E_INVALID."""
        if isinstance(patterns, ExtractSet):
            raise TypeError("select_device takes patterns, a PatternSet, a RegexSet or Labels; an ExtractSet goes to extract_device")
        if isinstance(patterns, (Labels, RegexSet, PatternSet)):
            if isinstance(patterns, Labels):
                if ignore_case or invert:
                    raise ValueError("a selection by Labels takes the masks any, all and none: the fold belongs to the LabelSet, and `none` inverts")
                entry, args = "sx_result_select_labels_device", (any, all, none)
            else:
                if any or all or none:
                    raise ValueError("the masks any, all and none select by Labels (Result.label_device)")
                if ignore_case:
                    raise ValueError("ignore_case belongs to the %s: Scanner.%s(patterns, ignore_case=True)" % (type(patterns).__name__, patterns._maker))
                entry, args = patterns._select, (SX_SELECT_INVERT if invert else 0,)
            if not self._s.h:
                raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
            out = C.c_void_p()
            self._s._chk(getattr(lib(), entry)(self._s.h, self.h, patterns._handle(), *args, C.byref(out)))
            return Result(self._s, out)
        if any or all or none:
            raise ValueError("the masks any, all and none select by Labels (Result.label_device)")
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        arr, n = _pattern_array([patterns] if isinstance(patterns, (bytes, bytearray, memoryview)) else patterns)
        flags = (SX_SELECT_ASCII_NOCASE if ignore_case else 0) | (SX_SELECT_INVERT if invert else 0)
        out = C.c_void_p()
        self._s._chk(lib().sx_result_select_device(self._s.h, self.h, arr, n, flags, C.byref(out)))
        return Result(self._s, out)

    def extract_device(self, extract_set):
        """The regex MATCHES in this Result's strings, cut out on the device (sx_result_extract_regex_device; `extract_set`: an
        ExtractSet, Scanner.extract_set) — `grep -oE` over the strings: per finding the leftmost, longest, non-overlapping, non-empty
        matches, each one a finding of the new Result, which is the source's record with another str_off and str_len (`position` and
        the rest stay the finding's).  The new Result lies on the device like a selection — strings back to back, possibly MORE
        findings than this one has —, counts as one for "valid until the second select_device() after this one", and
        device_segments(), printed_device(), select_device(), tally_device(), extract_device() and the host accessors take it.  This
        Result is not moved.  Raises TypeError for anything but an ExtractSet (a RegexSet selects, it does not extract), SxError
        SX_E_STATE wherever printed_device() would refuse this Result."""
        if not isinstance(extract_set, ExtractSet):
            raise TypeError("extract_device takes an ExtractSet (Scanner.extract_set)")
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        if not extract_set.h:
            raise SxError(SX_E_INVALID, "the ExtractSet has been freed")
        out = C.c_void_p()
        self._s._chk(lib().sx_result_extract_regex_device(self._s.h, self.h, extract_set.h, 0, C.byref(out)))
        return Result(self._s, out)

    def tally_device(self, tally, ordinal_base=0):
        """sx_result_tally_device: the hits of `tally`'s keywords (a TallySet: Scanner.tally_set) in this Result's strings, ADDED to
        the set's counters on the device; a hit's ordinal is ordinal_base + the finding's index in this Result's print order.
        Returns the number of findings walked.  This Result is read, not moved, and no selection ages.  Raises SxError: SX_E_STATE
        wherever printed_device() would refuse this Result (nothing is added then), SX_E_INVALID for a freed set."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        if not isinstance(tally, TallySet) or not tally.h:
            raise SxError(SX_E_INVALID, "the TallySet has been freed" if isinstance(tally, TallySet) else "tally_device takes a TallySet")
        n = C.c_uint64()
        self._s._chk(lib().sx_result_tally_device(self._s.h, self.h, tally.h, ordinal_base, C.byref(n)))
        return n.value

    def label_device(self, label_set, ordinal_base=0):
        """sx_result_label_device: for every finding of this Result WHICH patterns of `label_set` (a LabelSet: Scanner.label_set) are
        found in its string — Labels, one 64-bit word per finding in HBM, bit p for pattern p —, and per pattern the number of such
        findings and the first of them ADDED to the set's counters; a finding's ordinal is ordinal_base + its index in this Result's
        print order.  This Result is read, not moved, and no selection ages.  Raises SxError: SX_E_STATE wherever printed_device()
        would refuse this Result (nothing is counted then), SX_E_INVALID for a freed set."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        if not isinstance(label_set, LabelSet) or not label_set.h:
            raise SxError(SX_E_INVALID, "the LabelSet has been freed" if isinstance(label_set, LabelSet) else "label_device takes a LabelSet")
        out = C.c_void_p()
        self._s._chk(lib().sx_result_label_device(self._s.h, self.h, label_set.h, ordinal_base, C.byref(out)))
        return Labels(self._s, out)

    def fuzzy_device(self, fuzzy_set, ordinal_base=0):
        """sx_result_fuzzy_device: for every finding of this Result WHICH patterns of `fuzzy_set` (a FuzzySet: Scanner.fuzzy_set) occur
        in its string within their error budget — Labels, one 64-bit word per finding in HBM, bit p for pattern p, fuzzy() of its
        string —, and per pattern the number of such findings and the first of them, added to the set's counters (ordinal_base: the
        findings of the buffers before this one).  select_device(labels, any=...), select_range_device(), order_device(labels=...)
        and Labels.rebind() take the Labels as they take label_device()'s.  This Result is read, never moved, and the call is no
        selection.  Raises SxError: SX_E_STATE as printed_device() does, SX_E_INVALID for a set on another device."""
        if not isinstance(fuzzy_set, FuzzySet) or not fuzzy_set.h:
            raise SxError(SX_E_INVALID, "the FuzzySet has been freed" if isinstance(fuzzy_set, FuzzySet) else "fuzzy_device takes a FuzzySet")
        out = C.c_void_p()
        self._s._chk(lib().sx_result_fuzzy_device(self._s.h, self.h, fuzzy_set.h, ordinal_base, C.byref(out)))
        return Labels(self._s, out)

    def distinct_device(self, ignore_case=False):
        """sx_result_distinct_device: WHICH findings of this Result repeat an earlier finding's string — Labels, one 64-bit word per
        finding in HBM: bit 0 (SX_DISTINCT_FIRST) no earlier finding has the same string, bit 1 (SX_DISTINCT_REPEATED) another finding
        has it, word >> SX_DISTINCT_COUNT_SHIFT how many have it.  select_device(labels, any=SX_DISTINCT_FIRST) is `sort -u` in the
        original order, none=SX_DISTINCT_FIRST the duplicates, all=FIRST | REPEATED `uniq -d`, any=FIRST with none=REPEATED `uniq -u`.
        ignore_case: 'A'..'Z' compare as 'a'..'z' (no other byte is folded).  The Labels' .info is sx_distinct_info as a dict:
        findings, distinct, repeated, rounds, table_log2.  This Result is read, not moved, and no selection ages.  Raises SxError:
        SX_E_STATE wherever printed_device() would refuse this Result."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        out, info = C.c_void_p(), DistinctInfo()
        self._s._chk(lib().sx_result_distinct_device(self._s.h, self.h, SX_SELECT_ASCII_NOCASE if ignore_case else 0, C.byref(out), C.byref(info)))
        labels = Labels(self._s, out)
        labels.info = {k: getattr(info, k) for k, _ in DistinctInfo._fields_}
        return labels

    def seen_device(self, seen_set, add=True):
        """sx_result_seen_device: the words of distinct_device() under the fold of `seen_set` (a SeenSet: Scanner.seen_set) plus bit 2
        (SX_DISTINCT_SEEN): the set held an equal string when the call began.  select_device(labels, any=SX_DISTINCT_FIRST,
        none=SX_DISTINCT_SEEN) is every string new to the stream, once; none=SX_DISTINCT_SEEN baseline subtraction; any=SX_DISTINCT_SEEN
        intersection.  add: afterwards the set also holds this Result's strings, each once (False: SX_SEEN_LOOKUP_ONLY, the set is
        only read).  The Labels' .info is sx_seen_info as a dict: findings, distinct, repeated, seen_findings, seen_distinct,
        added_strings, added_bytes, rounds, table_log2.  This Result is read, not moved, and no selection ages.  Raises SxError:
        SX_E_STATE wherever distinct_device() would refuse this Result, SX_E_NOMEM if what is new does not fit the set (which is then
        as it was), SX_E_INVALID for a freed set."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        if not isinstance(seen_set, SeenSet) or not seen_set.h:
            raise SxError(SX_E_INVALID, "the SeenSet has been freed" if isinstance(seen_set, SeenSet) else "seen_device takes a SeenSet")
        out, info = C.c_void_p(), SeenInfo()
        self._s._chk(lib().sx_result_seen_device(self._s.h, self.h, seen_set.h, 0 if add else SX_SEEN_LOOKUP_ONLY, C.byref(out), C.byref(info)))
        labels = Labels(self._s, out)
        labels.info = {k: getattr(info, k) for k, _ in SeenInfo._fields_}
        return labels

    def seen_counts_device(self, seen_set):
        """sx_result_seen_counts_device: for every finding of this Result the count word of its string in `seen_set` (a SeenSet made
        with counted=True) under the set's fold — (word >> SX_SEEN_RESULTS_SHIFT) & 0xFFFFFFFF how many results held it,
        (word >> SX_SEEN_FINDINGS_SHIFT) & 0xFFFFFFFF how many findings they held of it — or 0 if the set does not hold it: Labels,
        which download(), free() and select like any other.  The set is only read and no distinct pass runs.  Raises SxError:
        SX_E_INVALID for a set that does not count or is freed, SX_E_STATE wherever distinct_device() would refuse this Result."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        if not isinstance(seen_set, SeenSet) or not seen_set.h:
            raise SxError(SX_E_INVALID, "the SeenSet has been freed" if isinstance(seen_set, SeenSet) else "seen_counts_device takes a SeenSet")
        out = C.c_void_p()
        self._s._chk(lib().sx_result_seen_counts_device(self._s.h, self.h, seen_set.h, C.byref(out)))
        return Labels(self._s, out)

    def select_range_device(self, labels, shift, bits, lo, hi):
        """sx_result_select_labels_range_device: the findings whose label word has lo <= ((word >> shift) & mask(bits)) <= hi, out of
        the Labels made of THIS Result (1 <= bits <= 64, shift + bits <= 64; lo > hi selects nothing): a new Result on the device, as
        select_device(labels, ...) gives one.  On distinct_device() words shift=32, bits=32, lo=5 are the strings that occur at least
        five times in this Result; on seen_counts_device() words shift=SX_SEEN_RESULTS_SHIFT, bits=32, lo=k the strings at least k
        results held.  No string byte is read.  Labels of another Result, or a bad field: SxError SX_E_INVALID."""
        if not isinstance(labels, Labels):
            raise TypeError("select_range_device takes Labels")
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        if not (0 <= shift < 1 << 32 and 0 <= bits < 1 << 32 and 0 <= lo < 1 << 64 and 0 <= hi < 1 << 64):
            raise SxError(SX_E_INVALID, "select_range_device: shift and bits are 32-bit, lo and hi 64-bit unsigned numbers")
        out = C.c_void_p()
        self._s._chk(lib().sx_result_select_labels_range_device(self._s.h, self.h, labels._handle(), shift, bits, lo, hi, C.byref(out)))
        return Result(self._s, out)

    def order_device(self, by="string", labels=None, shift=0, bits=64, descending=False, ignore_case=False, any=0, all=0, none=0, limit=0):
        """sx_result_order_device: IN WHICH ORDER — a new Result on the device that holds this Result's findings sorted by their
        string (by="string": unsigned bytes, the shorter of two first, `LC_ALL=C sort`; ignore_case: 'A'..'Z' compare as 'a'..'z') or
        by the field (word >> shift) & mask(bits) of their word in `labels` (by="field"; the Labels made of THIS Result).  Findings
        with equal keys keep print order; descending reverses the distinct keys and leaves the ties as they are:
        sorted(range(n), key=..., reverse=descending).  any, all, none: only the findings whose label passes the pick of
        select_device(labels, ...) take part (all 0: every finding); limit: only the first `limit` findings of the order (0: all).
        distinct_device() then order_device(labels=d, any=SX_DISTINCT_FIRST) is `sort -u`; order_device("field", d, shift=32,
        bits=32, descending=True, any=SX_DISTINCT_FIRST, limit=20) is `uniq -c | sort -rn | head -20`.  The new Result is one
        segment of unpacked records, lies on the device like a selection, counts as one for "valid until the second select_device()
        after this one", and .order_info is sx_order_info as a dict: findings (took part), kept (written), rounds, tied, max_depth.
        This Result is not moved.  Raises ValueError for another `by`, SxError: SX_E_INVALID for labels that are missing where the
        key or the masks need them, of another Result or freed, a bad field, ignore_case with by="field"; SX_E_STATE wherever
        printed_device() would refuse this Result."""
        if by not in ("string", "field"):
            raise ValueError('order_device: by is "string" or "field"')
        if labels is not None and not isinstance(labels, Labels):
            raise TypeError("order_device takes Labels")
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        if not (0 <= shift < 1 << 32 and 0 <= bits < 1 << 32 and 0 <= min(any, all, none, limit) and max(any, all, none, limit) < 1 << 64):
            raise SxError(SX_E_INVALID, "order_device: shift and bits are 32-bit, the masks and the limit 64-bit unsigned numbers")
        spec = OrderSpec(SX_ORDER_BY_LABEL_FIELD if by == "field" else SX_ORDER_BY_STRING,
                         (SX_ORDER_DESCENDING if descending else 0) | (SX_ORDER_NOCASE if ignore_case else 0), shift, bits, any, all, none, limit)
        out, info = C.c_void_p(), OrderInfo()
        self._s._chk(lib().sx_result_order_device(self._s.h, self.h, labels._handle() if labels is not None else None, C.byref(spec), C.byref(out), C.byref(info)))
        res = Result(self._s, out)
        res.order_info = {k: getattr(info, k) for k, _ in OrderInfo._fields_}
        return res

    def fold_device(self):
        """sx_result_fold_device: WHATEVER THE LETTER CASE, IN EVERY SCRIPT — a new Result on the device with this Result's findings
        in the same order, segment for segment and record for record, every string replaced by its Unicode simple case folding
        (fold() is the rule); every other field and the segments' SegmentInfo stay.  select_device(), label_device(),
        distinct_device(), seen_device(), order_device() ... of the new Result then compare folded strings — fold() the patterns —,
        and Labels.rebind(this Result) carries their answer back to the original strings: `grep -i` is
        f = r.fold_device(); r.select_device(f.label_device(s.label_set([fold(p)])).rebind(r), any=1).  The new Result lies on the
        device like a selection and counts as one for "valid until the second select_device() after this one"; .fold_info is
        sx_fold_info as a dict: findings, bytes_in, bytes_out, changed.  This Result is not moved.  Raises SxError: SX_E_STATE
        wherever printed_device() would refuse this Result, SX_E_INVALID for a segment whose folded strings outgrow 32-bit offsets
        or a packed record's 16-bit length."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        out, info = C.c_void_p(), FoldInfo()
        self._s._chk(lib().sx_result_fold_device(self._s.h, self.h, SX_FOLD_SIMPLE, C.byref(out), C.byref(info)))
        res = Result(self._s, out)
        res.fold_info = {k: getattr(info, k) for k, _ in FoldInfo._fields_}
        return res

    def decode_device(self, kind, utf16le=False):
        """sx_result_decode_device: WHAT AN ENCODED STRING HOLDS — a new Result on the device with this Result's findings in the same
        order, segment for segment and record for record, every string that decodes as `kind` ("base64", "hex", "percent"; decode() is
        the rule) replaced by the bytes it stands for, every other string copied; utf16le=True reads the decoded bytes as UTF-16LE and
        writes UTF-8 (a PowerShell -EncodedCommand).  Every other field and the segments' SegmentInfo stay.  .decode_words is the
        Labels of the call, one word per finding, bound to THIS Result (rebind() carries them to the new one, and any Labels of the
        new one back); .decode_info is sx_decode_info as a dict: findings, decoded, text, wide, bytes_in, bytes_out.

            runs = r.extract_device(sc.extract_set([rb"[A-Za-z0-9+/]{16,}={0,2}"]))
            d = runs.decode_device("base64", utf16le=True)
            hits = d.label_device(sc.label_set([rb"downloadstring", rb"invoke-"], ignore_case=True))   # on the decoded text
            runs.select_device(hits.rebind(runs), any=3)                                                # the encoded originals
            d.select_device(d.decode_words.rebind(d), all=SX_DECODE_OK | SX_DECODE_TEXT)               # what decodes to text

        The new Result lies on the device like a selection and counts as one; the words are no selection and age nothing.  This
        Result is not moved.  Raises SxError: SX_E_STATE wherever fold_device() would refuse this Result, SX_E_INVALID for a segment
        whose output strings outgrow 32-bit offsets or a packed record's 16-bit length."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        out, words, info = C.c_void_p(), C.c_void_p(), DecodeInfo()
        self._s._chk(lib().sx_result_decode_device(self._s.h, self.h, _decode_kind(kind), SX_DECODE_UTF16LE if utf16le else 0,
                                                   C.byref(out), C.byref(words), C.byref(info)))
        res = Result(self._s, out)
        res.decode_words = Labels(self._s, words)
        res.decode_info = {k: getattr(info, k) for k, _ in DecodeInfo._fields_}
        return res

    def measure_device(self):
        """sx_result_measure_device: WHAT the strings LOOK like — Labels, one 64-bit word per finding in HBM, measure() of its
        string: the entropy of its bytes (bits 0..15, bits per byte x 4096), how many different bytes (bits 16..24), the class bits
        SX_MEASURE_LOWER, UPPER, DIGIT, SPACE, PUNCT, CONTROL, HIGH (set iff the string holds such a byte) and its characters (bits
        32..63: the bytes outside 0x80..0xBF).  select_range_device(m, SX_MEASURE_CHARS_SHIFT, 32, 32, 2**32 - 1) is
        `awk 'length >= 32'`; select_range_device(m, SX_MEASURE_ENTROPY_SHIFT, 16, int(4.5 * 4096), 65535) "entropy above 4.5 bits
        per byte"; select_device(m, none=SX_MEASURE_HIGH | SX_MEASURE_SPACE) one ASCII token; order_device("field", m, shift=0,
        bits=16, descending=True, limit=100) the hundred most random strings.  The Labels' .info is sx_measure_info as a dict:
        findings, bytes, chars, wide (strings of more than 255 bytes), ascii (strings without SX_MEASURE_HIGH).  This Result is read,
        not moved, and no selection ages.  Raises SxError: SX_E_STATE wherever printed_device() would refuse this Result."""
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        out, info = C.c_void_p(), MeasureInfo()
        self._s._chk(lib().sx_result_measure_device(self._s.h, self.h, 0, C.byref(out), C.byref(info)))
        labels = Labels(self._s, out)
        labels.info = {k: getattr(info, k) for k, _ in MeasureInfo._fields_}
        return labels

    def free(self):
        if self.h:
            lib().sx_result_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceHandle:
    """What the compiled sets and the Labels share: `h`, a handle of the library that owns device memory until free().  A class
    names its free function (_free) and, if it has one, its info function and struct (_info_get, _info_type)."""
    _free = _info_get = _info_type = _freed = None

    def __init__(self, handle):
        self.h = handle

    def _handle(self):
        if not self.h:
            raise SxError(SX_E_INVALID, self._freed or "the %s has been freed" % type(self).__name__)
        return self.h

    def _info(self):
        i = self._info_type()
        rc = getattr(lib(), self._info_get)(self._handle(), C.byref(i))
        if rc != SX_OK:
            raise SxError(rc, self._info_get)
        return i

    def _info_dict(self):
        i = self._info()
        return {k: getattr(i, k) for k, _ in self._info_type._fields_ if k != "reserved"}

    def free(self):
        if self.h:
            getattr(lib(), self._free)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _blob_bytes(blob_or_path):
    if isinstance(blob_or_path, (bytes, bytearray, memoryview)):
        return bytes(blob_or_path)
    with open(blob_or_path, "rb") as f:
        return f.read()


def seen_blob_info(blob):
    """sx_seen_blob_info_get: a saved SeenSet (bytes, or the path of a file) checked completely, on the host and without a device;
    sx_seen_blob_info as a dict: strings, bytes, nocase, version.  SxError SX_E_INVALID: it is not a blob a set can be loaded from."""
    blob, info = _blob_bytes(blob), SeenBlobInfo()
    rc = lib().sx_seen_blob_info_get(blob, len(blob), C.byref(info))
    if rc != SX_OK:
        raise SxError(rc, "sx_seen_blob_info_get")
    return {k: getattr(info, k) for k, _ in SeenBlobInfo._fields_}


def _pattern_array(patterns):
    """(an array of sx_pattern, its length) for a list of bytes-like patterns; the array keeps the bytes alive"""
    pats = [bytes(p) for p in patterns]
    return (Pattern * max(1, len(pats)))(*[Pattern(p, len(p)) for p in pats]), len(pats)


class PatternSet(_DeviceHandle):
    """A keyword list compiled for the device (sx_select_set_create; Scanner.pattern_set makes it): Result.select_device() takes it
    in place of a list, on result after result.  It owns its device memory: free() it before or after the Scanner's close()."""

    _free, _info_get, _info_type = "sx_select_set_free", "sx_select_set_info_get", SelectSetInfo
    _select, _maker = "sx_result_select_set_device", "pattern_set"

    def info(self):
        """sx_select_set_info as a dict: n_patterns, states, classes, nocase, table_bytes (in HBM), lds_states"""
        return self._info_dict()


class RegexSet(_DeviceHandle):
    """Byte regular expressions compiled for the device (sx_select_regex_create; Scanner.regex_set makes it): Result.select_device()
    takes it in place of a list, on result after result.  It owns its device memory: free() it before or after the Scanner's
    close()."""

    _free, _info_get, _info_type = "sx_select_regex_free", "sx_select_regex_info_get", SelectRegexInfo
    _select, _maker = "sx_result_select_regex_device", "regex_set"

    def info(self):
        """sx_select_regex_info as a dict: n_patterns, states, classes, nocase, table_bytes (in HBM), lds_states, end_states"""
        return self._info_dict()


class ExtractSet(_DeviceHandle):
    """Byte regular expressions compiled for the extraction on the device (sx_extract_regex_create; Scanner.extract_set makes it):
    Result.extract_device() takes it, on result after result.  It owns its device memory: free() it before or after the Scanner's
    close()."""

    _free, _info_get, _info_type = "sx_extract_regex_free", "sx_extract_regex_info_get", ExtractRegexInfo

    def info(self):
        """sx_extract_regex_info as a dict: n_patterns, states, classes, nocase, table_bytes (in HBM), lds_states"""
        return self._info_dict()


class TallySet(_DeviceHandle):
    """A keyword list compiled for counting on the device (sx_tally_set_create; Scanner.tally_set makes it), with its counters:
    Result.tally_device() adds a result's hits to them, on result after result.  It owns its device memory: free() it before or
    after the Scanner's close()."""

    _free, _info_get, _info_type = "sx_tally_set_free", "sx_tally_set_info_get", TallySetInfo

    def __init__(self, handle, n_patterns):
        self.h, self.n_patterns = handle, n_patterns

    def info(self):
        """sx_tally_set_info as a dict: n_patterns, unique, states, classes, nocase, entry_bytes, table_bytes (in HBM), lds_states"""
        return self._info_dict()

    def read(self):
        """(hits, first): two lists with an entry per input pattern; first[k] is SX_TALLY_NEVER where hits[k] is 0"""
        hits, first = (C.c_uint64 * self.n_patterns)(), (C.c_uint64 * self.n_patterns)()
        rc = lib().sx_tally_set_read(self._handle(), hits, first, self.n_patterns)
        if rc != SX_OK:
            raise SxError(rc, "sx_tally_set_read")
        return list(hits), list(first)

    def reset(self):
        """every hits = 0, every first = SX_TALLY_NEVER"""
        rc = lib().sx_tally_set_reset(self._handle())
        if rc != SX_OK:
            raise SxError(rc, "sx_tally_set_reset")

    def counters_device(self):
        """(d_hits, d_first, d_unique_of_pattern, unique): device addresses — two arrays of `unique` uint64 indexed by unique id, and
        n_patterns uint32 that map an input pattern to its unique id"""
        h, f, m, u = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        rc = lib().sx_tally_set_counters_device(self._handle(), C.byref(h), C.byref(f), C.byref(m), C.byref(u))
        if rc != SX_OK:
            raise SxError(rc, "sx_tally_set_counters_device")
        return h.value, f.value, m.value, u.value


class LabelSet(_DeviceHandle):
    """Byte regular expressions compiled for labelling on the device (sx_label_set_create; Scanner.label_set makes it), with their
    counters: Result.label_device() says which of them every finding holds and adds to the counters, on result after result.  It owns
    its device memory: free() it before or after the Scanner's close()."""

    _free, _info_get, _info_type = "sx_label_set_free", "sx_label_set_info_get", LabelSetInfo

    def __init__(self, handle, n_patterns):
        self.h, self.n_patterns = handle, n_patterns

    @property
    def info(self):
        """a LabelSetInfo (sx_label_set_info): n_patterns, states, classes, nocase, table_bytes (in HBM), lds_states, here_states"""
        return self._info()

    def read(self):
        """(findings, first): two lists with an entry per pattern; first[p] is SX_LABEL_NEVER where findings[p] is 0"""
        findings, first = (C.c_uint64 * self.n_patterns)(), (C.c_uint64 * self.n_patterns)()
        rc = lib().sx_label_set_read(self._handle(), findings, first, self.n_patterns)
        if rc != SX_OK:
            raise SxError(rc, "sx_label_set_read")
        return list(findings), list(first)

    def reset(self):
        """every findings = 0, every first = SX_LABEL_NEVER"""
        rc = lib().sx_label_set_reset(self._handle())
        if rc != SX_OK:
            raise SxError(rc, "sx_label_set_reset")

    def counters_device(self):
        """(d_findings, d_first): device addresses of two arrays of 64 uint64, of which the first n_patterns are used"""
        f, m = C.c_void_p(), C.c_void_p()
        rc = lib().sx_label_set_counters_device(self._handle(), C.byref(f), C.byref(m))
        if rc != SX_OK:
            raise SxError(rc, "sx_label_set_counters_device")
        return f.value, m.value


class FuzzySet(_DeviceHandle):
    """Keywords with error budgets compiled for the approximate match on the device (sx_fuzzy_set_create; Scanner.fuzzy_set makes it),
    with their counters: Result.fuzzy_device() says which of them every finding holds within its budget and adds to the counters, on
    result after result.  It owns its device memory: free() it before or after the Scanner's close()."""

    _free, _info_get, _info_type = "sx_fuzzy_set_free", "sx_fuzzy_set_info_get", FuzzySetInfo

    def __init__(self, handle, n_patterns):
        self.h, self.n_patterns = handle, n_patterns

    @property
    def info(self):
        """a FuzzySetInfo (sx_fuzzy_set_info): n_patterns, classes, lds_classes, nocase, table_bytes (in HBM), max_len, max_errors"""
        return self._info()

    def read(self):
        """(findings, first): two lists with an entry per pattern; first[p] is SX_LABEL_NEVER where findings[p] is 0"""
        findings, first = (C.c_uint64 * self.n_patterns)(), (C.c_uint64 * self.n_patterns)()
        rc = lib().sx_fuzzy_set_read(self._handle(), findings, first, self.n_patterns)
        if rc != SX_OK:
            raise SxError(rc, "sx_fuzzy_set_read")
        return list(findings), list(first)

    def reset(self):
        """every findings = 0, every first = SX_LABEL_NEVER"""
        rc = lib().sx_fuzzy_set_reset(self._handle())
        if rc != SX_OK:
            raise SxError(rc, "sx_fuzzy_set_reset")

    def counters_device(self):
        """(d_findings, d_first): device addresses of two arrays of 64 uint64, of which the first n_patterns are used"""
        f, m = C.c_void_p(), C.c_void_p()
        rc = lib().sx_fuzzy_set_counters_device(self._handle(), C.byref(f), C.byref(m))
        if rc != SX_OK:
            raise SxError(rc, "sx_fuzzy_set_counters_device")
        return f.value, m.value


class SeenSet(_DeviceHandle):
    """Strings remembered in HBM from one Result to the next (sx_seen_set_create; Scanner.seen_set makes it): Result.seen_device() says
    which findings' strings it held and adds the others, on result after result.  Its capacity is fixed.  It owns its device memory:
    free() it before or after the Scanner's close()."""

    _free, _info_get, _info_type = "sx_seen_set_free", "sx_seen_set_info_get", SeenSetInfo

    def __init__(self, handle, scanner=None):
        self.h, self._s = handle, scanner

    def info(self):
        """sx_seen_set_info as a dict: strings, bytes (what it holds), capacity_strings, capacity_bytes, table_log2, nocase, tag_bits
        (whether it counts: the property `counted`)"""
        return {k: v for k, v in self._info_dict().items() if k != "counted"}

    @property
    def counted(self):
        """the set was made with counted=True (SX_SEEN_COUNTED), or loaded from such a set's blob"""
        return bool(self._info().counted)

    def counts(self):
        """{string: (results, findings)} of a set that counts — how many results held the string, and how many findings they held of
        it —, parsed from export(); SxError SX_E_INVALID for a set that does not count"""
        if not self.counted:
            raise SxError(SX_E_INVALID, "the SeenSet was made without counted=True")
        blob = self.export()
        strings = self._strings_of(blob)
        at = len(blob) - 8 * len(strings)
        out = {}
        for k, x in enumerate(strings):
            word = int.from_bytes(blob[at + 8 * k:at + 8 * k + 8], "little")
            out[x] = (word >> SX_SEEN_RESULTS_SHIFT & 0xFFFFFFFF, word >> SX_SEEN_FINDINGS_SHIFT & 0xFFFFFFFF)
        return out

    def reset(self):
        """the set is empty again; its capacity is kept"""
        rc = lib().sx_seen_set_reset(self._handle())
        if rc != SX_OK:
            raise SxError(rc, "sx_seen_set_reset")

    def _scanner(self, scanner):
        """the context of a call that needs one: `scanner`, or the Scanner that made the set (any on the set's device will do)"""
        s = scanner or self._s
        if s is None or not s.h:
            raise SxError(SX_E_STATE, "the Scanner that made the SeenSet is closed: pass scanner=")
        return s

    def merge(self, other, add=True, scanner=None):
        """sx_seen_set_merge: this set united with `other` (a SeenSet of the same fold, which is only read).  add=False
        (SX_SEEN_LOOKUP_ONLY) counts and adds nothing.  sx_seen_merge_info as a dict: source_strings (what `other` holds),
        already_held (of those, what this set held: the intersection), added_strings, added_bytes.  SxError SX_E_NOMEM: what is new
        does not fit, and the set is as it was — grow() it."""
        if not isinstance(other, SeenSet) or not other.h:
            raise SxError(SX_E_INVALID, "the SeenSet has been freed" if isinstance(other, SeenSet) else "merge takes a SeenSet")
        s, info = self._scanner(scanner), SeenMergeInfo()
        s._chk(lib().sx_seen_set_merge(s.h, self._handle(), other.h, 0 if add else SX_SEEN_LOOKUP_ONLY, C.byref(info)))
        return {k: getattr(info, k) for k, _ in SeenMergeInfo._fields_}

    def grow(self, capacity_strings, capacity_bytes, scanner=None):
        """sx_seen_set_grow: this same set with new capacities (smaller ones too, as long as they hold what it holds); every string
        it holds stays"""
        s = self._scanner(scanner)
        s._chk(lib().sx_seen_set_grow(s.h, self._handle(), capacity_strings, capacity_bytes))

    def export(self):
        """sx_seen_set_export: the set as bytes — a 64-byte header and its entries as they lie (include/stringsext_amd.h) —, for
        Scanner.seen_set_from() in this or another process"""
        n, written = C.c_uint64(), C.c_uint64()
        rc = lib().sx_seen_set_export_size(self._handle(), C.byref(n))
        if rc != SX_OK:
            raise SxError(rc, "sx_seen_set_export_size")
        buf = C.create_string_buffer(n.value)
        rc = lib().sx_seen_set_export(self.h, buf, n.value, C.byref(written))
        if rc != SX_OK:
            raise SxError(rc, "sx_seen_set_export")
        return buf.raw[:written.value]

    def save(self, path):
        """export() into a file"""
        with open(path, "wb") as f:
            f.write(self.export())

    def strings(self):
        """the strings the set holds — folded, if it folds — in the order of their entries: parsed from export()"""
        return self._strings_of(self.export())

    @staticmethod
    def _strings_of(blob):
        out, at = [], SX_SEEN_BLOB_HEADER_BYTES
        end = SX_SEEN_BLOB_HEADER_BYTES + int.from_bytes(blob[24:32], "little")      # (behind the entries: a counting set's count words)
        while at < end:
            n = int.from_bytes(blob[at:at + 4], "little")
            out.append(blob[at + 8:at + 8 + n])
            at += 8 + (n + 7) // 8 * 8
        return out

    def add_strings(self, strings, add=True, scanner=None, _held=None):
        """sx_seen_set_add_strings: a list of bytes objects put into the set (add=False: only looked up).  sx_seen_merge_info as a
        dict: source_strings = the distinct ones among them under the set's fold, already_held, added_strings, added_bytes.  SxError
        SX_E_NOMEM: what is new does not fit, and the set is as it was."""
        strings = [bytes(x) for x in strings]
        offsets = (C.c_uint64 * (len(strings) + 1))()
        at = 0
        for i, x in enumerate(strings):
            at += len(x)
            offsets[i + 1] = at
        s, info = self._scanner(scanner), SeenMergeInfo()
        s._chk(lib().sx_seen_set_add_strings(s.h, self._handle(), b"".join(strings), offsets, len(strings), 0 if add else SX_SEEN_LOOKUP_ONLY, _held, C.byref(info)))
        return {k: getattr(info, k) for k, _ in SeenMergeInfo._fields_}

    def contains(self, strings, scanner=None):
        """per string of the list whether the set holds it (under the set's fold): add_strings(add=False) with its held_out"""
        strings = list(strings)
        held = C.create_string_buffer(max(1, len(strings)))
        self.add_strings(strings, add=False, scanner=scanner, _held=held)
        return [b != 0 for b in held.raw[:len(strings)]]


class Labels(_DeviceHandle):
    """One Result's labels in HBM (sx_result_label_device; Result.label_device makes them — or sx_result_distinct_device,
    Result.distinct_device, which also sets .info —): a 64-bit word per finding, an array per segment of the Result.  Result.select_device() of the SAME Result takes them with the masks any, all, none.  They own their
    device memory: free() them before or after the Scanner's close()."""

    _free, _freed = "sx_labels_free", "the Labels have been freed"
    info = None      # distinct_device(): sx_distinct_info as a dict; seen_device(): sx_seen_info; measure_device(): sx_measure_info

    def __init__(self, scanner, handle):
        self._s, self.h = scanner, handle

    def device_segments(self):
        """[(device pointer to the segment's labels, n findings)] per segment of the source"""
        L, h = lib(), self._handle()
        out = []
        for i in range(L.sx_labels_segments(h)):
            p, n = C.c_void_p(), C.c_uint64()
            rc = L.sx_labels_segment_device(h, i, C.byref(p), C.byref(n))
            if rc != SX_OK:
                raise SxError(rc, "sx_labels_segment_device")
            out.append((p.value, n.value))
        return out

    def rebind(self, result):
        """sx_labels_rebind: new Labels with these words, copied on the device, bound to `result` — which select_device(),
        select_range_device() and order_device() of `result` then take as they take the Labels made from it.  `result` lies on the
        device and has this Labels' segments and record counts (else SxError SX_E_INVALID); that record i of `result` is the
        finding word i speaks of — a fold and its source — is what the caller vouches for.  No selection: nothing ages."""
        if not isinstance(result, Result):
            raise TypeError("rebind takes a Result")
        if not self._s.h:
            raise SxError(SX_E_STATE, "the Scanner is closed: its device memory is gone")
        out = C.c_void_p()
        self._s._chk(lib().sx_labels_rebind(self._s.h, self._handle(), result.h, C.byref(out)))
        return Labels(self._s, out)

    def download(self):
        """one list of ints per segment: the labels in record order (sx_device_download)"""
        out = []
        for p, n in self.device_segments():
            raw = self._s.download(p, n * 8) if n else b""
            out.append(list((C.c_uint64 * n).from_buffer_copy(raw)) if n else [])
        return out


class Scanner:
    """One sx_ctx: N missions bound to one HIP device (device=SX_HOST_ONLY: replay stage only).
    result_on_device=True (SX_OPT_RESULT_ON_DEVICE): the result of scan() / scan_device() stays in HBM — Result.device_segments(),
    Scanner.download() —, with one Mission or several; valid until the next buffer is scanned on this Scanner.
    Result.printed_device() formats such a result on the device: the reference's text as one block in HBM;
    Result.select_device() selects its findings by substring there (grep -F): a new Result in HBM."""

    def __init__(self, mission_dicts, device=0, subchunk_bytes=0, record_capacity=0, generic_kernels=False,
                 replay_threads=0, device_replay=None, result_on_device=False, fused_scan=True):
        L = lib()
        self.n = len(mission_dicts)
        self._ms = (Mission * self.n)(*[Mission.from_dict(d) for d in mission_dicts])
        flags = SX_OPT_GENERIC_KERNELS if generic_kernels else 0
        if device_replay is True:
            flags |= SX_OPT_DEVICE_REPLAY   # stage B on the device even for small inputs
        elif device_replay is False:
            flags |= SX_OPT_HOST_REPLAY
        if result_on_device:
            flags |= SX_OPT_RESULT_ON_DEVICE
        if not fused_scan:
            flags |= SX_OPT_NO_FUSED_SCAN
        opt = Options(subchunk_bytes, record_capacity, replay_threads, flags)
        self.h = C.c_void_p()
        rc = L.sx_create(C.byref(self.h), self._ms, self.n, device, C.byref(opt))
        if rc != SX_OK:
            self.h = None
            raise SxError(rc, L.sx_last_error(None).decode())

    def _chk(self, rc):
        if rc != SX_OK:
            raise SxError(rc, lib().sx_last_error(self.h).decode())

    def pattern_set(self, patterns, ignore_case=False):
        """sx_select_set_create: `patterns` (1..65536 bytes objects of 1..255 bytes, 1 MiB in all; duplicates allowed) compiled into
        an automaton in HBM on this Scanner's device, for Result.select_device().  ignore_case: 'A'..'Z' as 'a'..'z', compiled in."""
        arr, n = _pattern_array(patterns)
        out = C.c_void_p()
        self._chk(lib().sx_select_set_create(self.h, arr, n, SX_SELECT_ASCII_NOCASE if ignore_case else 0, C.byref(out)))
        return PatternSet(out)

    def tally_set(self, patterns, ignore_case=False):
        """sx_tally_set_create: `patterns` (the limits of pattern_set) compiled into an automaton with output links and two counters
        per keyword in HBM on this Scanner's device, for Result.tally_device().  ignore_case: 'A'..'Z' as 'a'..'z', compiled in."""
        arr, n = _pattern_array(patterns)
        out = C.c_void_p()
        self._chk(lib().sx_tally_set_create(self.h, arr, n, SX_SELECT_ASCII_NOCASE if ignore_case else 0, C.byref(out)))
        return TallySet(out, n)

    def regex_set(self, patterns, ignore_case=False):
        """sx_select_regex_create: `patterns` (1..64 bytes objects of 1..1024 bytes: the byte regex language of
        include/stringsext_amd.h, which means what Python's `re` means with `$` read as `\\Z`) compiled into one DFA in HBM on this
        Scanner's device, for Result.select_device().  ignore_case: re.IGNORECASE on a bytes pattern, compiled in.  A refused
        pattern raises SxError (SX_E_INVALID) whose text names the pattern's index, the offset and the reason."""
        arr, n = _pattern_array(patterns)
        out = C.c_void_p()
        self._chk(lib().sx_select_regex_create(self.h, arr, n, SX_SELECT_ASCII_NOCASE if ignore_case else 0, C.byref(out)))
        return RegexSet(out)

    def extract_set(self, patterns, ignore_case=False):
        """sx_extract_regex_create: `patterns` (the language and the limits of regex_set) compiled into one anchored DFA in HBM on
        this Scanner's device, for Result.extract_device().  ignore_case: re.IGNORECASE on a bytes pattern, compiled in.  A refused
        pattern raises SxError (SX_E_INVALID) whose text names the pattern's index, the offset and the reason."""
        arr, n = _pattern_array(patterns)
        out = C.c_void_p()
        self._chk(lib().sx_extract_regex_create(self.h, arr, n, SX_SELECT_ASCII_NOCASE if ignore_case else 0, C.byref(out)))
        return ExtractSet(out)

    def label_set(self, patterns, ignore_case=False):
        """sx_label_set_create: `patterns` (the language and the limits of regex_set; pattern p owns bit p of a label) compiled into
        one DFA with a mask per state in HBM on this Scanner's device, with two counters per pattern, for Result.label_device().
        ignore_case: re.IGNORECASE on a bytes pattern, compiled in.  A refused pattern raises SxError (SX_E_INVALID) whose text names
        the pattern's index, the offset and the reason."""
        arr, n = _pattern_array(patterns)
        out = C.c_void_p()
        self._chk(lib().sx_label_set_create(self.h, arr, n, SX_SELECT_ASCII_NOCASE if ignore_case else 0, C.byref(out)))
        return LabelSet(out, n)

    def fuzzy_set(self, patterns, max_errors=1, ignore_case=False):
        """sx_fuzzy_set_create: `patterns` (1..64 byte strings of 1..64 bytes; pattern p owns bit p of a word) with their error budgets
        — max_errors: an int for all of them, or one per pattern; 0..8 and smaller than the pattern's length — compiled into bit masks
        in HBM on this Scanner's device, with two counters per pattern, for Result.fuzzy_device().  ignore_case: 'A'..'Z' and 'a'..'z'
        compare equal in pattern and string.  SxError SX_E_INVALID, with the pattern's index in the text, for what is refused."""
        arr, n = _pattern_array(patterns)
        out = C.c_void_p()
        self._chk(lib().sx_fuzzy_set_create(self.h, arr, _error_budgets(max_errors, n), n, SX_SELECT_ASCII_NOCASE if ignore_case else 0, C.byref(out)))
        return FuzzySet(out, n)

    def seen_set(self, capacity_strings, capacity_bytes, ignore_case=False, counted=False):
        """sx_seen_set_create: an empty SeenSet for capacity_strings strings whose entries take capacity_bytes at most — a string of
        n bytes takes 8 + n rounded up to a multiple of 8 —; ignore_case: the set folds 'A'..'Z' to 'a'..'z', and so does every
        Result.seen_device() call that takes it.  counted (SX_SEEN_COUNTED): the set also counts, per string, the results that held it
        and their findings of it: SeenSet.counts(), Result.seen_counts_device()."""
        out = C.c_void_p()
        flags = (SX_SELECT_ASCII_NOCASE if ignore_case else 0) | (SX_SEEN_COUNTED if counted else 0)
        self._chk(lib().sx_seen_set_create(self.h, capacity_strings, capacity_bytes, flags, C.byref(out)))
        return SeenSet(out, self)

    def seen_set_from(self, blob_or_path, capacity_strings=0, capacity_bytes=0):
        """sx_seen_set_import: a new SeenSet that holds what SeenSet.export() / save() wrote (bytes, or the path of a file), under the
        blob's fold and this Scanner's SX_SEEN_TAG_BITS; a counting set's blob (version 2) gives a set that counts, with those counts.  A capacity of 0: what the blob holds; a smaller one, or a blob that
        seen_blob_info() refuses: SxError SX_E_INVALID."""
        blob = _blob_bytes(blob_or_path)
        out = C.c_void_p()
        self._chk(lib().sx_seen_set_import(self.h, blob, len(blob), capacity_strings, capacity_bytes, C.byref(out)))
        return SeenSet(out, self)

    def scan(self, data, file_id=-1, is_last=False):
        """sx_scan: replaces the loop src/main.rs:153-168 for one chunk held in host memory."""
        data = bytes(data)
        r = C.c_void_p()
        self._chk(lib().sx_scan(self.h, data, len(data), file_id, int(is_last), C.byref(r)))
        return Result(self, r)

    def scan_device(self, dptr, length, file_id=-1, is_last=False):
        r = C.c_void_p()
        self._chk(lib().sx_scan_device(self.h, dptr, length, file_id, int(is_last), C.byref(r)))
        return Result(self, r)

    def replay_runs(self, data, runs_per_mission, file_id=-1, is_last=False):
        """sx_replay_runs: stage B only; runs_per_mission[m] = [(start, end, chars), ...] sorted."""
        data = bytes(data)
        arrs = [(Run * max(1, len(rs)))(*[Run(*t) for t in rs]) for rs in runs_per_mission]
        ptrs = (C.POINTER(Run) * self.n)(*[C.cast(a, C.POINTER(Run)) for a in arrs])
        ns = (C.c_uint64 * self.n)(*[len(rs) for rs in runs_per_mission])
        r = C.c_void_p()
        self._chk(lib().sx_replay_runs(self.h, data, len(data), file_id, int(is_last), ptrs, ns, C.byref(r)))
        return Result(self, r)

    def scan_shard(self, buf, buf_off, own_lo, own_hi, start_at=None, file_stream_off=0, file_id=-1, reuse_runs=False,
                   runs_per_mission=None, buf_len=None):
        """One rank of a byte-range-sharded scan (sx_scan_shard / _device / sx_replay_shard_runs).
        buf: bytes (host) or a ctypes.c_void_p device pointer (then buf_len is required).
        Returns (Result, end_pos per mission)."""
        sa = (C.c_uint64 * self.n)(*start_at) if start_at is not None else None
        ends = (C.c_uint64 * self.n)()
        r = C.c_void_p()
        if isinstance(buf, C.c_void_p):
            self._chk(lib().sx_scan_shard_device(self.h, buf, buf_off, buf_len, own_lo, own_hi, sa, file_stream_off, file_id,
                                                 int(reuse_runs), C.byref(r), ends))
        else:
            buf = bytes(buf)
            if runs_per_mission is not None:
                arrs = [(Run * max(1, len(rs)))(*[Run(*t) for t in rs]) for rs in runs_per_mission]
                ptrs = (C.POINTER(Run) * self.n)(*[C.cast(a, C.POINTER(Run)) for a in arrs])
                ns = (C.c_uint64 * self.n)(*[len(rs) for rs in runs_per_mission])
                self._chk(lib().sx_replay_shard_runs(self.h, buf, buf_off, len(buf), own_lo, own_hi, sa, file_stream_off,
                                                     file_id, ptrs, ns, C.byref(r), ends))
            else:
                self._chk(lib().sx_scan_shard(self.h, buf, buf_off, len(buf), own_lo, own_hi, sa, file_stream_off, file_id,
                                              int(reuse_runs), C.byref(r), ends))
        return Result(self, r), list(ends)

    def device_runs(self, mission_index, dptr, length, stream_parity=0, min_chars=1, count_only=False):
        """Stage A alone: the long runs of one mission over a device buffer (count_only: just their number)."""
        runs = C.POINTER(Run)()
        n = C.c_uint64()
        self._chk(lib().sx_device_runs(self.h, mission_index, dptr, length, stream_parity, min_chars,
                                       C.byref(runs), C.byref(n)))
        out = n.value if count_only else [(runs[i].start, runs[i].end, runs[i].chars) for i in range(n.value)]
        lib().sx_free(runs)
        return out

    def device_runs_multi(self, mission_indices, dptr, length, stream_parity=0, min_chars=None):
        """Stage A for several missions in one call (sx_device_runs_multi): the missions the fused kernel holds share one
        launch that reads the buffer once.  Returns a list of run lists."""
        n = len(mission_indices)
        idx = (C.c_int * n)(*mission_indices)
        mc = (C.c_uint64 * n)(*(min_chars if min_chars is not None else [1] * n))
        runs = (C.POINTER(Run) * n)()
        cnt = (C.c_uint64 * n)()
        self._chk(lib().sx_device_runs_multi(self.h, idx, n, dptr, length, stream_parity, mc, runs, cnt))
        out = []
        for i in range(n):
            out.append([(runs[i][j].start, runs[i][j].end, runs[i][j].chars) for j in range(cnt[i])])
            lib().sx_free(runs[i])
        return out

    def scan_file(self, path, chunk_bytes=0, file_id=1):
        """Ingest pipeline (sx_scan_file): the file is read, copied to HBM and scanned chunk by chunk,
        overlapped; returns the chunks' Results in input order."""
        results = []
        SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)

        def sink(_user, handle):
            results.append(Result(self, C.c_void_p(handle)))
            return 0
        cb = SINK(sink)
        L = lib()
        L.sx_scan_file.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, SINK, C.c_void_p]
        self._chk(L.sx_scan_file(self.h, os.fsencode(path), chunk_bytes, file_id, cb, None))
        return results

    def scan_stream(self, readinto, chunk_bytes=0, file_id=1):
        """sx_scan_stream with a Python reader: readinto(memoryview) -> bytes written (0 at the end)."""
        results = []
        SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
        READ = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64)

        def sink(_user, handle):
            results.append(Result(self, C.c_void_p(handle)))
            return 0

        def read(_user, dst, max_bytes):
            try:
                view = memoryview((C.c_uint8 * max_bytes).from_address(C.addressof(dst.contents))).cast("B")
                return int(readinto(view) or 0)
            except Exception:
                return -1
        cb, rd = SINK(sink), READ(read)
        L = lib()
        L.sx_scan_stream.argtypes = [C.c_void_p, READ, C.c_void_p, C.c_uint64, C.c_int, SINK, C.c_void_p]
        self._chk(L.sx_scan_stream(self.h, rd, None, chunk_bytes, file_id, cb, None))
        return results

    def reset(self):
        self._chk(lib().sx_reset(self.h))

    def stats(self):
        s = Stats()
        self._chk(lib().sx_get_stats(self.h, C.byref(s)))
        return s

    # device memory helpers
    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(lib().sx_device_alloc(self.h, nbytes, C.byref(p)))
        return p

    def free(self, dptr):
        self._chk(lib().sx_device_free(self.h, dptr))

    def upload(self, dptr, data):
        data = bytes(data)
        self._chk(lib().sx_device_upload(self.h, dptr, data, len(data)))

    def download(self, dptr, nbytes):
        b = C.create_string_buffer(nbytes)
        self._chk(lib().sx_device_download(self.h, b, dptr, nbytes))
        return b.raw

    def fill_background(self, dptr, first_index, nbytes, seed=0x5EED5EED5EED5EED):
        self._chk(lib().sx_fill_background_device(self.h, dptr, first_index, nbytes, seed))

    def read_bandwidth(self, dptr, nbytes, repeats=5):
        g = C.c_double()
        self._chk(lib().sx_device_read_bandwidth(self.h, dptr, nbytes, repeats, C.byref(g)))
        return g.value

    def close(self):
        if self.h:
            lib().sx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


OUTPUT_BOM = b"\xEF\xBB\xBF"
