"""A planted buffer of ASCII lines that are, or just fail to be, base64, hex and percent-escaped strings, whose findings are known
line by line, for the decoding of a result lying in HBM (tests/test_decode_plant.py on the CPU, tests/test_gpu_decode_device.py on the
device): what tests/fold_plant.py is for the case fold.  Every line has 4 to 60 characters of printable ASCII, so that a line is a
finding of fold_plant.ms1() and of both Missions of fold_plant.ms2(); everything is a function of the line number: no random state.
Expected findings come from the oracle alone (result_plant.expected()).

decode() is the rule of sx_decode_bytes written in Python as include/stringsext_amd.h states it — the conditions, then base64,
binascii, urllib.parse and codecs for the bytes —: the oracle of every decoding in the tests.

What the lines hold (tests/test_decode_plant.py asserts each)
 base64    encodings of ASCII text, of UTF-16LE text (ASCII, Cyrillic, a surrogate pair) and of bytes that hold 0x00, 0x0A and 0xFF;
           padded, unpadded and url-safe; every m % 4, the refused 1 among them; a line that mixes '+' and '_', one with '=' in its
           middle, one with three '=', one with two '=' where one belongs, one with a space; UTF-16 with a lone high surrogate, with a
           lone low one, and of odd length
 hex       both cases, an odd length, a byte that is no hex digit at the first and at the last place
 percent   %41, %zz, %4 at the end, % as the last byte, %25%34%31, an escape at offset 0 and one as the last three bytes, no escape
 words     Password, getElementById: valid base64 by accident, OK without TEXT; hello, admin: m % 4 == 1

Behind them, for the long strings of the device test: long_lines() for fold_plant.msl() and limit_lines() for long_plant.limit_ms()."""
import base64
import binascii
import re
import urllib.parse

import long_plant as lp
import result_plant as rp

BASE64, HEX, PERCENT, UTF16LE = 1, 2, 3, 1
KINDS = {"base64": BASE64, "hex": HEX, "percent": PERCENT}
OK, TEXT, WIDE, PADDED, URLSAFE, LEN_SHIFT = 1, 2, 4, 8, 16, 32

_B64_BODY = re.compile(rb"[A-Za-z0-9+/_-]*\Z")
_HEX = re.compile(rb"(?:[0-9A-Fa-f]{2})+\Z")
_ESCAPE = re.compile(rb"%[0-9A-Fa-f]{2}")
_TO_STANDARD = bytes.maketrans(b"-_", b"+/")


def is_text(b):
    return 0x20 <= b <= 0x7E or b in (0x09, 0x0A, 0x0D)


def raw(kind, s):
    """(D, the word's PADDED and URLSAFE bits) of the string s under `kind`, or None where it does not decode"""
    if kind == BASE64:
        pad = 2 if s.endswith(b"==") else 1 if s.endswith(b"=") else 0
        body = s[:len(s) - pad]
        m = len(body)
        if m < 2 or m % 4 == 1 or (pad and (m + pad) % 4) or not _B64_BODY.match(body):
            return None
        standard, urlsafe = any(c in body for c in b"+/"), any(c in body for c in b"-_")
        if standard and urlsafe:
            return None
        d = base64.b64decode(body.translate(_TO_STANDARD) + b"=" * (-m % 4), validate=True)
        return d, (PADDED if pad else 0) | (URLSAFE if urlsafe else 0)
    if kind == HEX:
        return (binascii.unhexlify(s), 0) if _HEX.match(s) else None
    assert kind == PERCENT
    return (urllib.parse.unquote_to_bytes(s), 0) if _ESCAPE.search(s) else None


def decode(kind, flags, s):
    """(the output, the word) of sx_decode_bytes(kind, flags, s): (s, 0) where s does not decode"""
    assert flags in (0, UTF16LE)
    got = raw(kind, s)
    if got is None:
        return s, 0
    d, bits = got
    out = d
    if flags & UTF16LE:
        try:
            out = d.decode("utf-16-le").encode("utf-8")
        except UnicodeDecodeError:      # an odd length, a lone surrogate
            return s, 0
    wide = len(d) >= 2 and len(d) % 2 == 0 and not any(d[1::2]) and all(map(is_text, d[0::2]))
    word = OK | bits | (TEXT if all(map(is_text, out)) else 0) | (WIDE if wide else 0) | len(out) << LEN_SHIFT
    return out, word


def b64(d, strip=False, urlsafe=False):
    s = base64.urlsafe_b64encode(d) if urlsafe else base64.b64encode(d)
    return s.rstrip(b"=") if strip else s


def u16(t):
    return t.encode("utf-16-le")


BYTES = bytes([0x00, 0x0A, 0xFF, 0x41, 0xFB, 0xEF, 0xBE, 0x00, 0x7F, 0xFF, 0x0A])      # its base64 holds '+' and '/': url-safe, '-' and '_'
HIGH_ALONE, LOW_ALONE, ODD = u16("A") + b"\x3d\xd8" + u16("B"), u16("A") + b"\x00\xdc" + u16("B"), u16("AB") + b"C"
# what has to be there, whatever the number of lines
SPECIAL = [
    b64(b"Invoke-WebRequest -Uri http://x"), b64(b"ls -la /tmp"), b64(b"ab"), b64(b"abc"), b64(b"abcd"),      # ASCII text; m % 4 = 3 + pad, 0, 2 + pad
    b64(b"abcde", strip=True), b64(b"abcd", strip=True), b64(b"abcdef", strip=True), b64(b"a"),             # unpadded: m % 4 = 3, 2, 0; YQ==
    b64(u16("IEX (New-Object Net)")), b64(u16("whoami"), strip=True), b64(u16("пароль 1")), b64(u16("a\U0001F600b")), b64(b"\xff\xfe" + u16("bom")),
    b64(BYTES), b64(BYTES, strip=True), b64(BYTES, urlsafe=True), b64(BYTES, strip=True, urlsafe=True), b64(b"tab\there\r\nline"),
    b"hello", b"admin", b"ABCDEFGHI",                                            # m % 4 == 1
    b"ab+c_d12", b"QUJD=UVG", b"QUJDR===", b"QUI==", b"QUJDRA=", b"QUJD RUZH", b"QUJD.RUZH",      # mixed alphabets, '=' inside, three '=', wrong padding, a space
    b64(HIGH_ALONE), b64(LOW_ALONE), b64(ODD), b64(u16("A") + b"\x3d\xd8"),     # lone surrogates, an odd length, a high surrogate at the end
    b"4a4B6c6D", b"4A4B4C4D4E", b"6a6b6c6d", b"4a4b6", b"g14b6c6d", b"4a4b6c6g", b"000aff41", binascii.hexlify(u16("wide hex")),
    binascii.hexlify(u16("A") + b"\x00\xdc"), b"4100420043",
    b"x%41y", b"x%zzy", b"path%4", b"path%", b"%25%34%31", b"%41start", b"end%41", b"plain/path", b"a+b%20c", b"%00%0a%ff%FF", b"%41%00%42%00",
    b"%3d%D8 lone", b"%e2%82%ac%20euro", b"%%41%", b"100%4100",
    b"Password", b"getElementById", b"username", b"Authorization", b"root",
]


def generated(k):
    """line k where it is none of SPECIAL: an encoding of some text or bytes, a function of k"""
    m = rp.mix(k + 1)
    words = lp.text(k, 6 + m % 22).strip() or b"x"
    kind = m // 32 % 10
    if kind < 3:
        return b64(words, strip=m % 2 == 1)
    if kind == 3:
        return b64(u16(words[:18].decode()), strip=m % 2 == 1)
    if kind == 4:
        return b64(bytes((m >> j ^ 37 * j) & 0xFF for j in range(3 + m % 30)), strip=m % 4 == 1, urlsafe=m % 4 >= 2)
    if kind == 5:
        return binascii.hexlify(words[:30]).upper() if m % 2 else binascii.hexlify(words[:30])
    if kind == 6:
        return binascii.hexlify(u16(words[:14].decode()))
    if kind == 7:
        return urllib.parse.quote_from_bytes(words[:20], safe="").encode()
    if kind == 8:
        return b"".join(b"%%%02x" % c for c in u16(words[:9].decode()))
    return words                                                                # plain text: mostly nothing decodes


def lines(n):
    """the first n lines: one line of three is of SPECIAL, in turn"""
    out = [SPECIAL[k // 3 % len(SPECIAL)] if k % 3 == 0 else generated(k) for k in range(n)]
    assert all(4 <= len(x) <= 60 and all(0x20 <= c <= 0x7E for c in x) for x in out)
    return out


def buffer(n):
    """n lines"""
    return b"\n".join(lines(n)) + b"\n"


def decoded(kind, flags, strs):
    """per string of strs (the output, the word); one evaluation per different string"""
    memo = {}
    return [memo[s] if s in memo else memo.setdefault(s, decode(kind, flags, s)) for s in strs]


def info(strs, outs):
    """sx_decode_info of the strings strs that gave outs = decoded(...)"""
    return dict(findings=len(strs), decoded=sum(w & OK for _, w in outs), text=sum(w & TEXT != 0 for _, w in outs),
                wide=sum(w & WIDE != 0 for _, w in outs), bytes_in=sum(map(len, strs)), bytes_out=sum(len(o) for o, _ in outs))


# ---- long strings (tests/test_gpu_decode_device.py)

LONG_Q = 1024


def long_lines():
    """for fold_plant.msl(), `-q 1024`: lines of 1024 characters — base64 of 768 bytes that hold every byte value, base64 of UTF-16LE
    text, hex in both cases, a line that an '!' as its last byte keeps from being either —, and percent lines whose only escape is
    their last three bytes"""
    every = bytes(range(256)) * 3
    text16 = u16(lp.text(77, 384).decode())
    out = [b"long first line", b64(every), b64(text16), binascii.hexlify(every[:512]), binascii.hexlify(every[256:768]).upper(),
           b64(every)[:-1] + b"!", binascii.hexlify(text16[:512]), lp.text(5, 1021) + b"%41", lp.text(6, 200) + b"%0a", b"long last line"]
    assert [len(x) for x in out[1:8]] == [LONG_Q] * 7
    return out


LIMIT_CHAR = "中"      # three bytes, E4 B8 AD: read in pairs as UTF-16LE, no unit is a surrogate and every unit takes three bytes of UTF-8


def limit_lines():
    """for long_plant.limit_ms(), `-q 16000`: one line of a percent escape and 15 997 three-byte characters — 16 000 characters, 47 994
    bytes, which a packed record holds; its 47 992 raw bytes are 23 996 UTF-16 units and 71 988 bytes of UTF-8, which it does not"""
    return lp.fitted([b"limit first line", b"%41" + (LIMIT_CHAR * 15997).encode(), b"%41 and a short one", b"limit last line"], 16000)
