"""A saved seen set checked on the host (sx_seen_blob_info_get, stringsext_amd/csrc/sx_seen_blob.cpp): through the library, without a
device or a context.  The blobs are built by hand here, from the layout include/stringsext_amd.h states: a valid one gives the right
info, and every refusal has a blob of its own that differs from a valid one in that one respect (its checksum is made right again
wherever the checksum is not the point)."""
import struct

import pytest

import stringsext_amd as sx

M64 = (1 << 64) - 1
STRINGS = [b"", b"a", b"seven77", b"eight888", b"nine99999", b"lower case only", bytes(range(1, 65)) + bytes(range(91, 256)), b"x" * 300]


def fnv(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = (h ^ b) * 0x100000001b3 & M64
    return h


def entry(s, second=0, pad=0):
    return struct.pack("<II", len(s), second) + s + bytes([pad]) * (-len(s) % 8)


def blob(area, strings, nocase=0, version=1, magic=b"SXSEEN\0\0", nbytes=None, checksum=None, rest=bytes(24)):
    return (magic + struct.pack("<IIQQQ", version, nocase, strings, len(area) if nbytes is None else nbytes, fnv(area) if checksum is None else checksum)
            + rest + area)


def refused(b):
    with pytest.raises(sx.SxError) as e:
        sx.seen_blob_info(b)
    assert e.value.code == sx.SX_E_INVALID
    return True


def test_a_valid_blob_gives_its_info():
    for nocase in (0, 1):
        area = b"".join(entry(s) for s in STRINGS)
        assert sx.seen_blob_info(blob(area, len(STRINGS), nocase)) == dict(strings=len(STRINGS), bytes=len(area), nocase=nocase, version=1)
    assert sx.seen_blob_info(blob(b"", 0)) == dict(strings=0, bytes=0, nocase=0, version=1)                  # the empty set
    assert len(blob(b"", 0)) == sx.SX_SEEN_BLOB_HEADER_BYTES == 64
    assert sx.seen_blob_info(blob(entry(b"ABC") + entry(b"abc"), 2, nocase=0))["strings"] == 2             # capitals are fine without the fold


def test_every_refusal_has_a_blob_of_its_own():
    area = b"".join(entry(s) for s in STRINGS)
    n = len(STRINGS)
    assert sx.seen_blob_info(blob(area, n))["strings"] == n
    assert refused(blob(area, n, magic=b"SXSEEN\0\1")) and refused(blob(area, n, magic=b"sxseen\0\0"))     # the magic
    assert refused(blob(area, n, version=0)) and refused(blob(area, n, version=2))                          # the version
    assert refused(blob(area, n) + bytes(8)) and refused(blob(area, n, nbytes=len(area) + 8))               # len other than 64 + bytes
    assert refused(blob(area, n, nbytes=len(area) - 8))
    odd = entry(b"abc")[:-4]
    assert refused(blob(odd, 1))                                                                            # bytes no multiple of 8
    over = area + struct.pack("<II", 9, 0) + b"12345678"                                                    # the last entry says 9 bytes and has room for 8
    assert refused(blob(over, n + 1))
    assert refused(blob(area + struct.pack("<II", 0xFFFFFFFF, 0), n + 1))
    assert refused(blob(area + entry(b"abc", second=1), n + 1))                                             # the second u32
    assert refused(blob(area + entry(b"abc", pad=1), n + 1)) and refused(blob(area + b"\x01\0\0\0\0\0\0\0" + b"a" + bytes(6) + b"\x80", n + 1))   # the padding
    assert sx.seen_blob_info(blob(area + entry(b"abc"), n + 1))["strings"] == n + 1                         # (what the three above are one step from)
    assert refused(blob(area, n + 1)) and refused(blob(area, n - 1)) and refused(blob(area, 0))             # the count
    assert refused(blob(area, n, checksum=fnv(area) ^ 1)) and refused(blob(area[:-1] + b"\x01", n, checksum=fnv(area)))      # the checksum
    assert refused(blob(area, n, nocase=2)) and refused(blob(area, n, nocase=0x100))                        # nocase
    assert refused(blob(area + entry(b"seven77"), n + 1)) and refused(blob(entry(b"") + entry(b""), 2))     # two equal entries
    assert refused(blob(area + entry(b"Abc"), n + 1, nocase=1)) and refused(blob(entry(b"az") + entry(b"aZ"), 2, nocase=1))  # not folded
    assert sx.seen_blob_info(blob(entry(b"@[`{"), 1, nocase=1))["nocase"] == 1                              # the neighbours of A..Z are no capitals
    assert refused(blob(area, n, rest=bytes(23) + b"\x01"))                                                 # the rest of the header


def test_truncations():
    area = b"".join(entry(s) for s in STRINGS)
    good = blob(area, len(STRINGS))
    for cut in (0, 1, 8, 12, 16, 24, 32, 40, 63, 64, 64 + 4, 64 + 8, 64 + 12, len(good) - 150, len(good) - 8, len(good) - 1):
        assert refused(good[:cut]), cut
    with pytest.raises(sx.SxError):
        sx.seen_blob_info(b"")


def test_the_new_symbols_are_exported_and_the_abi_version_stays():
    for name in ("sx_seen_set_merge", "sx_seen_set_grow", "sx_seen_set_export_size", "sx_seen_set_export", "sx_seen_blob_info_get", "sx_seen_set_import",
                 "sx_seen_set_add_strings"):
        assert name in sx.EXPORTS and getattr(sx.lib(), name)
    assert sx.lib().sx_abi_version() == 4


def test_the_calls_that_need_a_device_refuse_a_host_only_context():
    import ctypes as C
    import refconfig as rc
    sc = sx.Scanner([rc.mission()], device=sx.SX_HOST_ONLY)
    try:
        out = C.c_void_p(0xDEAD0)
        b = blob(entry(b"abc"), 1)
        assert sx.lib().sx_seen_set_import(sc.h, b, len(b), 0, 0, C.byref(out)) == sx.SX_E_STATE and out.value is None
        assert "host-only" in sx.lib().sx_last_error(sc.h).decode()
    finally:
        sc.close()


# ---- the blob check and the builder of a list's entries under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_checks_blobs_and_builds_entries_the_same(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    native = os.path.join(root, "tests", "native")
    exe, src = os.path.join(native, "seen_blob_main"), os.path.join(native, "seen_blob_main.cpp")
    deps = [src, os.path.join(root, "include", "stringsext_amd.h")] + [os.path.join(root, "stringsext_amd", "csrc", f) for f in ("sx_seen_blob.cpp", "sx_seen_blob.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", tmp, src])
        os.replace(tmp, exe)
    area = b"".join(entry(s) for s in STRINGS)
    n = len(STRINGS)
    good = blob(area, n)
    cases = [(good, 0), (blob(area, n, nocase=1), 0), (blob(b"", 0), 0), (b"", -1), (good[:40], -1), (good[:-1], -1), (good[:64 + 12], -1),
             (blob(area + struct.pack("<II", 0xFFFFFFFF, 0), n + 1), -1), (blob(area + struct.pack("<II", 9, 0) + b"12345678", n + 1), -1),
             (blob(area + entry(b"abc", pad=1), n + 1), -1), (blob(area + entry(b"seven77"), n + 1), -1), (blob(area + entry(b"Abc"), n + 1, nocase=1), -1),
             (blob(area, n, nbytes=len(area) + 8), -1), (blob(area, n, nbytes=(1 << 64) - 8), -1), (blob(area, n + 1), -1)]
    paths = []
    for k, (b, _) in enumerate(cases):
        paths.append(str(tmp_path / ("blob%d" % k)))
        open(paths[-1], "wb").write(b)
    out = subprocess.run([exe, "check"] + paths, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [line.split() for line in out.stdout.splitlines()]
    assert len(got) == len(cases)
    for (b, want), line in zip(cases, got):
        assert int(line[1]) == want == (0 if want == 0 else sx.SX_E_INVALID), (line, want)
        if want == 0:
            strings, nbytes, nocase = struct.unpack("<QQ", b[16:32]) + (struct.unpack("<I", b[12:16])[0],)
            assert [int(x) for x in line[2:]] == [strings, nbytes, nocase, strings]
    # the builder: folded under the set's fold, the first of every group of equal strings kept
    asked = [b"ABC", b"abc", b"", b"Abc", b"seven77", b"eight888", b"", b"nine99999", b"x" * 300, b"abc", b"[BC", b"k\xc0Z"]
    listing = str(tmp_path / "strings")
    open(listing, "w").write("".join(s.hex() + "\n" for s in asked))
    for nocase in (0, 1):
        out = subprocess.run([exe, "build", str(nocase), listing], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        rc_line, arena_line, words_line, kept_line = out.stdout.splitlines()
        keys = [s.lower() if nocase else s for s in asked]
        kept = list(dict.fromkeys(keys))
        assert rc_line == "rc 0" and bytes.fromhex(arena_line.split(" ", 1)[1] if " " in arena_line else "") == b"".join(entry(s) for s in kept)
        want_words, at = [], 0
        for s in kept:
            want_words.append(at // 8)
            at += len(entry(s))
        assert [int(x) for x in words_line.split()[1:]] == want_words and [int(x) for x in kept_line.split()[1:]] == [kept.index(k) for k in keys]
