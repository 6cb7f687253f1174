"""A saved seen set that counts — blob version 2 — checked on the host (sx_seen_blob_info_get, stringsext_amd/csrc/sx_seen_blob.cpp):
through the library, without a device or a context.  The blobs are built by hand here, from the layout include/stringsext_amd.h
states: the version-1 header with version = 2, the entry area, then a 64-bit count word per entry, the checksum over the area followed
by the count words.  Every new refusal has a blob of its own that differs from a valid one in that one respect."""
import struct

import stringsext_amd as sx
from test_seen_blob_host import STRINGS, blob, entry, fnv, refused

M32 = (1 << 32) - 1


def word(results, findings):
    return results << sx.SX_SEEN_RESULTS_SHIFT | findings << sx.SX_SEEN_FINDINGS_SHIFT


def blob2(area, counts, strings=None, nocase=0, version=2, checksum=None, nbytes=None):
    tail = b"".join(struct.pack("<Q", c) for c in counts)
    head = blob(area, len(counts) if strings is None else strings, nocase, version, nbytes=len(area) if nbytes is None else nbytes,
                checksum=fnv(area + tail) if checksum is None else checksum)
    return head + tail


AREA = b"".join(entry(s) for s in STRINGS)
COUNTS = [word(1 + k, 1 + 3 * k) for k in range(len(STRINGS))]


def test_a_version_2_blob_gives_its_info_and_version_1_still_says_1():
    n = len(STRINGS)
    for nocase in (0, 1):
        assert sx.seen_blob_info(blob2(AREA, COUNTS, nocase=nocase)) == dict(strings=n, bytes=len(AREA), nocase=nocase, version=2)
        assert sx.seen_blob_info(blob(AREA, n, nocase)) == dict(strings=n, bytes=len(AREA), nocase=nocase, version=1)
    assert len(blob2(AREA, COUNTS)) == 64 + len(AREA) + 8 * n
    assert sx.seen_blob_info(blob2(b"", [])) == dict(strings=0, bytes=0, nocase=0, version=2)                  # the empty counted set
    assert sx.seen_blob_info(blob2(entry(b"a"), [word(1, 1)]))["version"] == 2                                 # the smallest counts
    assert sx.seen_blob_info(blob2(entry(b"a"), [word(M32, M32)]))["version"] == 2                             # and the saturated ones
    assert sx.SX_SEEN_BLOB_VERSION == 1 and sx.SX_SEEN_BLOB_VERSION_COUNTED == 2


def test_every_new_refusal_has_a_blob_of_its_own():
    n = len(STRINGS)
    good = blob2(AREA, COUNTS)
    assert sx.seen_blob_info(good)["strings"] == n
    # the length: 64 + bytes + 8 x strings, in both directions (the checksum made right for what is there)
    assert refused(blob2(AREA, COUNTS + [word(1, 1)], strings=n))                                              # a count word too many
    assert refused(blob2(AREA, COUNTS[:-1], strings=n))                                                        # one too few
    assert refused(good + bytes(8)) and refused(good[:-8]) and refused(good + bytes(1))
    assert refused(blob(AREA, n, version=2))                                                                   # version 2 with a version-1 length
    assert refused(blob2(AREA, COUNTS, version=1))                                                             # version 1 with a version-2 length
    assert refused(blob2(AREA, COUNTS, nbytes=len(AREA) + 8 * n))                                              # `bytes` says the counts are entries
    assert refused(blob2(AREA, COUNTS, nbytes=(1 << 64) - 8)) and refused(blob2(AREA, COUNTS, strings=(1 << 61) + n))      # sums that would wrap
    # a count word
    for k in (0, n // 2, n - 1):
        assert refused(blob2(AREA, COUNTS[:k] + [word(0, 5)] + COUNTS[k + 1:]))                                # results == 0
        assert refused(blob2(AREA, COUNTS[:k] + [0] + COUNTS[k + 1:]))                                         # an empty slot's word
        assert refused(blob2(AREA, COUNTS[:k] + [word(5, 4)] + COUNTS[k + 1:]))                                # findings < results
        assert sx.seen_blob_info(blob2(AREA, COUNTS[:k] + [word(5, 5)] + COUNTS[k + 1:]))["strings"] == n      # (what it is one step from)
    # the checksum covers the counts
    assert refused(blob2(AREA, COUNTS, checksum=fnv(AREA)))                                                    # over the area alone
    flipped = COUNTS[:-1] + [COUNTS[-1] + word(1, 1)]
    assert refused(blob2(AREA, flipped, checksum=fnv(AREA + b"".join(struct.pack("<Q", c) for c in COUNTS))))  # a count changed behind it
    assert sx.seen_blob_info(blob2(AREA, flipped))["strings"] == n
    # what version 1 refuses, version 2 refuses
    assert refused(blob2(AREA + entry(b"seven77"), COUNTS + [word(1, 1)])) and refused(blob2(AREA + entry(b"Abc"), COUNTS + [word(1, 1)], nocase=1))
    assert refused(blob2(AREA + entry(b"abc", pad=1), COUNTS + [word(1, 1)])) and refused(blob2(AREA, COUNTS, nocase=2))
    assert refused(blob2(AREA, COUNTS, version=3))


def test_truncations_at_every_section_edge():
    good = blob2(AREA, COUNTS)
    edge = 64 + len(AREA)
    for cut in (0, 8, 40, 63, 64, 64 + 8, edge - 8, edge - 1, edge, edge + 1, edge + 7, edge + 8, len(good) - 9, len(good) - 8, len(good) - 1):
        assert refused(good[:cut]), cut
    assert sx.seen_blob_info(good)["version"] == 2
