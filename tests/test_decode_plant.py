"""What tests/decode_plant.py promises of its lines, asserted on the oracle's strings (no GPU): a line is a finding, and the lines hold
every case the decoders treat differently.  These are checks of the plant that tests/test_gpu_decode_device.py stands on; what they
judge the lines by is decode_plant.decode(), the rule in Python, and the library on the host, sx_decode_bytes (stringsext_amd.decode),
has to agree with it on every line."""
import base64

import decode_plant as dp
import fold_plant as fp
import long_plant as lp
import result_plant as rp
import stringsext_amd as sx

N = 3000
ALL = [(kind, flags) for kind in (dp.BASE64, dp.HEX, dp.PERCENT) for flags in (0, dp.UTF16LE)]
NAME = {v: k for k, v in dp.KINDS.items()}


def word(kind, flags, s):
    return dp.decode(kind, flags, s)[1]


def test_the_rule_in_python_says_what_the_issue_says():
    assert dp.decode(dp.BASE64, 0, b"QUJD") == (b"ABC", dp.OK | dp.TEXT | 3 << 32)
    assert dp.decode(dp.BASE64, 0, b"QUI=") == (b"AB", dp.OK | dp.TEXT | dp.PADDED | 2 << 32)
    assert dp.decode(dp.BASE64, 0, b"QUI") == (b"AB", dp.OK | dp.TEXT | 2 << 32)                       # unpadded decodes
    assert dp.decode(dp.BASE64, 0, b"QUJ") == (b"AB", dp.OK | dp.TEXT | 2 << 32)                       # the bits left over are dropped
    assert dp.decode(dp.BASE64, 0, b"-_8") == (b"\xfb\xff", dp.OK | dp.URLSAFE | 2 << 32)
    for s in (b"", b"Q", b"QUJDR", b"QUI==", b"QQ=", b"Q===", b"QU=J", b"+_8A", b"QU J", b"===="):
        assert dp.decode(dp.BASE64, 0, s) == (s, 0), s
    assert dp.decode(dp.BASE64, 0, b"QQBCAA==") == (b"A\0B\0", dp.OK | dp.WIDE | dp.PADDED | 4 << 32)
    assert dp.decode(dp.BASE64, dp.UTF16LE, b"QQBCAA==") == (b"AB", dp.OK | dp.TEXT | dp.WIDE | dp.PADDED | 2 << 32)
    assert dp.decode(dp.HEX, 0, b"4a4B") == (b"JK", dp.OK | dp.TEXT | 2 << 32) and dp.decode(dp.HEX, 0, b"4a4") == (b"4a4", 0)
    assert dp.decode(dp.HEX, dp.UTF16LE, b"fffe4100") == ("\ufeffA".encode(), dp.OK | 4 << 32)          # a BOM is U+FEFF
    assert dp.decode(dp.HEX, dp.UTF16LE, b"3dd8") == (b"3dd8", 0) and dp.decode(dp.HEX, dp.UTF16LE, b"3dd800de")[0] == "\U0001F600".encode()
    assert dp.decode(dp.PERCENT, 0, b"a+%41%zz%4") == (b"a+A%zz%4", dp.OK | dp.TEXT | 8 << 32)
    assert dp.decode(dp.PERCENT, 0, b"a%4") == (b"a%4", 0) and dp.decode(dp.PERCENT, 0, b"%25%34%31") == (b"%41", dp.OK | dp.TEXT | 3 << 32)
    assert dp.decode(dp.PERCENT, 0, b"%00") == (b"\0", dp.OK | 1 << 32)


def test_a_line_is_a_finding_at_the_counts_the_gpu_tests_take():
    for n in (1, 63, 64, 65, 129, N):
        assert rp.expected(fp.ms1(), dp.buffer(n)).strs == dp.lines(n), n
    assert len(dp.lines(N)) == N and 3 * len(dp.SPECIAL) <= 1024          # every special line stands in the merged source's first part
    merged = rp.expected(fp.ms2(), dp.buffer(N))
    assert merged.n == 2 * N and sorted(merged.strs) == sorted(dp.lines(N) * 2)      # ASCII only: each Mission finds every line


def test_the_lines_hold_what_they_are_meant_to():
    lines = dp.lines(3 * len(dp.SPECIAL))
    assert set(dp.SPECIAL) <= set(lines)
    w = {s: word(dp.BASE64, 0, s) for s in lines}
    u = {s: word(dp.BASE64, dp.UTF16LE, s) for s in lines}
    ok = [s for s in lines if w[s]]
    body = {s: s.rstrip(b"=") for s in lines}
    # every m % 4, the refused one among them; padded, unpadded, url-safe
    assert {len(body[s]) % 4 for s in ok} == {0, 2, 3} and all(w[s] == 0 for s in (b"hello", b"admin", b"ABCDEFGHI"))
    assert {(len(body[s]) % 4, bool(w[s] & dp.PADDED)) for s in ok} == {(0, False), (2, False), (2, True), (3, False), (3, True)}
    assert any(w[s] & dp.URLSAFE and w[s] & dp.PADDED for s in ok) and any(w[s] & dp.URLSAFE and not w[s] & dp.PADDED for s in ok)
    assert any(b"+" in s and b"/" in s and w[s] for s in lines)
    # text, UTF-16LE text, and bytes with 0x00, 0x0A and 0xFF
    assert any(w[s] & dp.TEXT and not w[s] & dp.WIDE for s in ok) and any(w[s] & dp.WIDE and not w[s] & dp.TEXT for s in ok)
    assert all({0x00, 0x0A, 0xFF} <= set(dp.decode(dp.BASE64, 0, dp.b64(dp.BYTES, strip, url))[0]) for strip in (False, True) for url in (False, True))
    for t in ("IEX (New-Object Net)", "пароль 1", "a\U0001F600b", "\ufeffbom"):
        s = dp.b64(dp.u16(t))
        assert s in lines and dp.decode(dp.BASE64, dp.UTF16LE, s)[0] == t.encode() and bool(u[s] & dp.TEXT) == t.isascii(), t
        assert bool(w[s] & dp.WIDE) == t.isascii()
    # the lines that just fail
    for s in (b"ab+c_d12", b"QUJD=UVG", b"QUJDR===", b"QUI==", b"QUJDRA=", b"QUJD RUZH", b"QUJD.RUZH"):
        assert s in lines and w[s] == 0 and u[s] == 0, s
    for d in (dp.HIGH_ALONE, dp.LOW_ALONE, dp.ODD, dp.u16("A") + b"\x3d\xd8"):
        s = dp.b64(d)
        assert s in lines and w[s] & dp.OK and u[s] == 0 and dp.decode(dp.BASE64, 0, s)[0] == d, s
    # words that are base64 by accident decode to no text; the others do not decode
    for s in (b"Password", b"getElementById", b"username", b"root"):
        assert s in lines and w[s] & dp.OK and not w[s] & dp.TEXT, s
    assert b"Authorization" in lines and w[b"Authorization"] == 0          # 13 letters
    # hex: both cases, an odd length, a wrong byte at either end
    h = {s: word(dp.HEX, 0, s) for s in lines}
    assert h[b"4a4B6c6D"] == h[b"6a6b6c6d"] == dp.OK | dp.TEXT | 4 << 32 and h[b"4A4B4C4D4E"] == dp.OK | dp.TEXT | 5 << 32
    assert h[b"4a4b6"] == h[b"g14b6c6d"] == h[b"4a4b6c6g"] == 0 and h[b"000aff41"] == dp.OK | 4 << 32
    assert word(dp.HEX, dp.UTF16LE, b"4100420043") == 0 and word(dp.HEX, dp.UTF16LE, b"410000dc") == 0 and h[b"410000dc"] & dp.OK
    # percent
    p = {s: dp.decode(dp.PERCENT, 0, s) for s in lines}
    assert p[b"x%41y"][0] == b"xAy" and p[b"%41start"][0] == b"Astart" and p[b"end%41"][0] == b"endA" and p[b"%25%34%31"][0] == b"%41"
    assert p[b"%%41%"][0] == b"%A%" and p[b"100%4100"][0] == b"100A00" and p[b"a+b%20c"][0] == b"a+b c" and p[b"%00%0a%ff%FF"][0] == b"\x00\x0a\xff\xff"
    for s in (b"x%zzy", b"path%4", b"path%", b"plain/path"):
        assert p[s] == (s, 0), s
    assert dp.decode(dp.PERCENT, dp.UTF16LE, b"%41%00%42%00") == (b"AB", dp.OK | dp.TEXT | dp.WIDE | 2 << 32)
    assert word(dp.PERCENT, dp.UTF16LE, b"%3d%D8 lone") == 0 and p[b"%3d%D8 lone"][1] & dp.OK
    grown = dp.decode(dp.PERCENT, dp.UTF16LE, b"%e2%82%ac%20euro")[0]
    assert grown.decode() == b"\xe2\x82\xac euro".decode("utf-16-le")
    # every kind and flag: some lines decode, some do not, some to text, some to wide; with the flag some outputs are LONGER than their source
    for kind, flags in ALL:
        outs = dp.decoded(kind, flags, dp.lines(N))
        i = dp.info(dp.lines(N), outs)
        assert 0 < i["text"] < i["decoded"] < N and 0 < i["wide"] < i["decoded"], (kind, flags, i)
    assert any(len(o) > len(s) for s, (o, _) in zip(dp.lines(N), dp.decoded(dp.PERCENT, dp.UTF16LE, dp.lines(N))))
    assert base64.b64decode(dp.b64(dp.BYTES)) == dp.BYTES


def test_the_host_decoder_agrees_with_the_rule_on_every_line():
    for kind, flags in ALL:
        for s in set(dp.lines(N)) | set(dp.long_lines()):
            assert sx.decode(NAME[kind], s, bool(flags)) == dp.decode(kind, flags, s), (kind, flags, s)


def test_the_long_lines_are_found_whole():
    lines = dp.long_lines()
    rows = rp.expected(fp.msl(), lp.buffer(lines))
    assert sorted(rows.strs) == sorted(lines * 2)                         # ASCII only: each Mission finds every line
    w = [[dp.decode(kind, 0, s)[1] for s in lines] for kind in (dp.BASE64, dp.HEX, dp.PERCENT)]
    assert [x >> 32 for x in w[0][1:3]] == [768, 768] and w[0][5] == 0 and w[0][2] & dp.WIDE
    assert [x >> 32 for x in w[1][3:5]] == [512, 512] and w[1][6] & dp.WIDE and w[1][6] >> 32 == 512
    assert w[2][7] >> 32 == 1022 and w[2][8] >> 32 == 201 and w[2][8] & dp.TEXT
    assert dp.decode(dp.BASE64, dp.UTF16LE, lines[2])[0] == lp.text(77, 384) and lines[7].endswith(b"%41") and lines[7].count(b"%") == 1


def test_the_limit_line_is_found_whole_and_its_output_outgrows_a_packed_record():
    lines = dp.limit_lines()
    rows = rp.expected(lp.limit_ms(), lp.buffer(lines))
    big = max(lines, key=len)
    assert big in rows.strs and len(big) == 47994 <= 0xFFFF and len(big.decode()) == 16000
    out, w = dp.decode(dp.PERCENT, dp.UTF16LE, big)
    assert w & dp.OK and len(out) == w >> 32 == 71988 > 0xFFFF
    assert max(len(dp.decode(dp.PERCENT, 0, s)[0]) for s in rows.strs) == 47992          # without the flag everything fits
    assert sx.decode("percent", big, True) == (out, w)
