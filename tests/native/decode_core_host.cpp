// Test-only program: compiles the lane functions of the decoders (sx_decode_core.hpp) as host code and runs them, under the address
// and undefined-behaviour sanitizers (tests/test_decode_core.py builds it so): every string of 0 to 5 bytes over a small alphabet that
// holds what each kind looks at, every byte value at every place of one valid string per kind, UTF-16 units at the surrogates' edges,
// for the three kinds with and without SX_DECODE_UTF16LE.  Every input lies in an allocation of its own that ENDS where the string
// ends, and every output in one of exactly the measured length: a byte read or written outside is the sanitizer's finding.  The
// output and the word are compared with a plain reference of the rule that first builds D as a whole and then looks at it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>
#define SXD inline
#include "../../stringsext_amd/csrc/sx_decode_core.hpp"

namespace {

bool text_byte(uint8_t b) { return (b >= 0x20 && b <= 0x7E) || b == 9 || b == 10 || b == 13; }
int hex_value(uint8_t b) { return b >= '0' && b <= '9' ? b - '0' : b >= 'a' && b <= 'f' ? b - 'a' + 10 : b >= 'A' && b <= 'F' ? b - 'A' + 10 : -1; }

// D and the base64 bits, or false
bool ref_raw(uint32_t kind, const std::string& in, std::string* d, uint64_t* bits) {
    const size_t n = in.size();
    *bits = 0;
    d->clear();
    if (kind == SX_DECODE_BASE64) {
        static const std::string alphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789";
        size_t pad = 0;
        while (pad < 2 && pad < n && in[n - 1 - pad] == '=') pad++;
        const size_t m = n - pad;
        if (m < 2 || m % 4 == 1 || (pad && (m + pad) % 4)) return false;
        bool standard = false, urlsafe = false;
        std::vector<int> six;
        for (size_t k = 0; k < m; k++) {
            const char c = in[k];
            const size_t at = alphabet.find(c);
            if (c != '\0' && at != std::string::npos) six.push_back((int)at);
            else if (c == '+' || c == '/') { standard = true; six.push_back(c == '+' ? 62 : 63); }
            else if (c == '-' || c == '_') { urlsafe = true; six.push_back(c == '-' ? 62 : 63); }
            else return false;
        }
        if (standard && urlsafe) return false;
        for (size_t k = 0; k + 1 < six.size(); k++) {      // byte j of D: the bits [8 j, 8 j + 8) of the sextets' row
            if (k % 4 == 3) continue;
            const int shift = 2 * (int)(k % 4) + 2;
            *d += (char)(uint8_t)((six[k] << shift | six[k + 1] >> (6 - shift)) & 0xFF);
        }
        *bits = (pad ? SX_DECODE_PADDED : 0) | (urlsafe ? SX_DECODE_URLSAFE : 0);
        return true;
    }
    if (kind == SX_DECODE_HEX) {
        if (n < 2 || n % 2) return false;
        for (size_t k = 0; k < n; k += 2) {
            if (hex_value(in[k]) < 0 || hex_value(in[k + 1]) < 0) return false;
            *d += (char)(hex_value(in[k]) << 4 | hex_value(in[k + 1]));
        }
        return true;
    }
    bool escaped = false;
    for (size_t k = 0; k < n;) {
        if (in[k] == '%' && k + 2 < n && hex_value(in[k + 1]) >= 0 && hex_value(in[k + 2]) >= 0) {
            *d += (char)(hex_value(in[k + 1]) << 4 | hex_value(in[k + 2]));
            escaped = true; k += 3;
        } else *d += in[k++];
    }
    return escaped;
}

// the output and the word; a string that does not decode: itself and 0
uint64_t ref(uint32_t kind, uint32_t flags, const std::string& in, std::string* out) {
    std::string d;
    uint64_t bits;
    *out = in;
    if (!ref_raw(kind, in, &d, &bits)) return 0;
    std::string o = d;
    if (flags & SX_DECODE_UTF16LE) {
        if (d.size() % 2) return 0;
        o.clear();
        for (size_t k = 0; k < d.size(); k += 2) {
            uint32_t c = (uint8_t)d[k] | (uint32_t)(uint8_t)d[k + 1] << 8;
            if (c >= 0xDC00 && c <= 0xDFFF) return 0;
            if (c >= 0xD800 && c <= 0xDBFF) {
                if (k + 4 > d.size()) return 0;
                const uint32_t lo = (uint8_t)d[k + 2] | (uint32_t)(uint8_t)d[k + 3] << 8;
                if (lo < 0xDC00 || lo > 0xDFFF) return 0;
                c = 0x10000 + ((c - 0xD800) << 10) + (lo - 0xDC00);
                k += 2;
            }
            if (c < 0x80) o += (char)c;
            else if (c < 0x800) { o += (char)(0xC0 | c >> 6); o += (char)(0x80 | (c & 63)); }
            else if (c < 0x10000) { o += (char)(0xE0 | c >> 12); o += (char)(0x80 | (c >> 6 & 63)); o += (char)(0x80 | (c & 63)); }
            else { o += (char)(0xF0 | c >> 18); o += (char)(0x80 | (c >> 12 & 63)); o += (char)(0x80 | (c >> 6 & 63)); o += (char)(0x80 | (c & 63)); }
        }
    }
    bool text = true, wide = d.size() >= 2 && d.size() % 2 == 0;
    for (unsigned char c : o) text = text && text_byte(c);
    for (size_t k = 0; k < d.size(); k++) wide = wide && (k % 2 ? d[k] == 0 : text_byte((uint8_t)d[k]));
    *out = o;
    return SX_DECODE_OK | bits | (text ? SX_DECODE_TEXT : 0) | (wide ? SX_DECODE_WIDE : 0) | (uint64_t)o.size() << SX_DECODE_LEN_SHIFT;
}

uint64_t cases = 0;

// the two walks over `in`; false: they differ from the reference
bool check(uint32_t kind, uint32_t flags, const std::string& in) {
    cases++;
    std::string want;
    const uint64_t want_word = ref(kind, flags, in, &want);
    uint8_t* s = (uint8_t*)malloc(in.size() ? in.size() : 1);      // (ends where the string ends)
    if (!s) return false;
    memcpy(s, in.data(), in.size());
    uint64_t need = 0;
    const uint64_t word = sx::decode_measure_string(kind, flags, s, (uint32_t)in.size(), &need);
    bool ok = word == want_word && need == want.size() && sx::decode_out_len(word, (uint32_t)in.size()) == need;
    if (ok) {
        uint8_t* dst = (uint8_t*)malloc(need ? need : 1);
        ok = dst != nullptr;
        if (ok) {
            sx::decode_place_string(kind, flags, word, s, (uint32_t)in.size(), dst);
            ok = !memcmp(dst, want.data(), need);
        }
        free(dst);
    }
    if (!ok) {
        fprintf(stderr, "decode core: kind %u, flags %u, input", kind, flags);
        for (unsigned char ch : in) fprintf(stderr, " %02x", ch);
        fprintf(stderr, ": word %llx, %llu bytes; the reference has %llx, %zu bytes\n", (unsigned long long)word, (unsigned long long)need,
                (unsigned long long)want_word, want.size());
    }
    free(s);
    return ok;
}

bool check_all(const std::string& in) {
    bool ok = true;
    for (uint32_t kind = SX_DECODE_BASE64; kind <= SX_DECODE_PERCENT; kind++)
        for (uint32_t flags = 0; flags < 2; flags++) ok = check(kind, flags, in) && ok;
    return ok;
}

std::string hex_of(const std::vector<uint32_t>& units) {
    static const char digit[] = "0123456789abcdef";
    std::string s;
    for (uint32_t u : units)
        for (uint32_t b : { u & 0xFFu, u >> 8 }) { s += digit[b >> 4]; s += digit[b & 15]; }
    return s;
}

}  // namespace

int main() {
    bool ok = true;
    // every string of 0 to 5 bytes over the alphabet
    const std::string alphabet = "ABab09+/-_=%fF ";
    for (size_t len = 0; ok && len <= 5; len++) {
        std::vector<size_t> at(len, 0);
        for (;;) {
            std::string s;
            for (size_t i : at) s += alphabet[i];
            ok = check_all(s) && ok;
            size_t k = 0;
            while (k < len && ++at[k] == alphabet.size()) at[k++] = 0;
            if (k == len) break;
        }
    }
    // every byte value at every place of a valid string of each kind
    for (const char* valid : { "QUJDREVG", "4a4B6c6D", "ab%41%4a" })
        for (size_t at = 0; ok && at < 8; at++)
            for (uint32_t b = 0; b < 256; b++) {
                std::string s = valid;
                s[at] = (char)b;
                ok = check_all(s) && ok;
            }
    // UTF-16 through hex: every unit singly is for the Python test; here the surrogates' edges, singly, in pairs and in threes
    const uint32_t edges[] = { 0x0000, 0x0041, 0x007F, 0x0080, 0x07FF, 0x0800, 0xD7FF, 0xD800, 0xDBFF, 0xDC00, 0xDFFF, 0xE000, 0xFEFF, 0xFFFF };
    for (uint32_t a : edges) {
        ok = check_all(hex_of({ a })) && ok;
        for (uint32_t b : edges) {
            ok = check_all(hex_of({ a, b })) && ok;
            for (uint32_t c : edges) ok = check_all(hex_of({ a, b, c })) && ok;
        }
    }
    // what the driver asks between the passes, and the records that place writes
    {
        ok = ok && sx::decode_segment_fits(1u, 65536, 65536) == sx::kDecodePackedTooLong && sx::decode_segment_fits(0u, 65536, 65536) == sx::kDecodeFits;
        ok = ok && sx::decode_segment_fits(1u, 65535, 65535) == sx::kDecodeFits && sx::decode_segment_fits(0u, 0xFFFFFFFFull, 100) == sx::kDecodeFits;
        ok = ok && sx::decode_segment_fits(0u, 0x100000000ull, 100) == sx::kDecodeTooManyBytes && sx::decode_segment_fits(1u, 0x100000000ull, 0x10000) == sx::kDecodeTooManyBytes;
        const std::string a = "QUJDRA==", b = "hello";      // record 0 decodes to "ABCD", record 1 is copied
        std::vector<uint8_t> arena(7 + a.size() + b.size()), out(3 + 4 + 5);
        memcpy(arena.data() + 7, a.data(), a.size());
        memcpy(arena.data() + 7 + a.size(), b.data(), b.size());
        sx_finding16 p16[2] = { { 0x1122334455667788ull, 7u, (uint16_t)a.size(), 0x05, 0xA7 }, { 0x99ull, (uint32_t)(7 + a.size()), (uint16_t)b.size(), 0x02, 0x01 } }, o16[2];
        sx_finding p32[2], o32[2];
        memset(p32, 0x5A, sizeof p32);       // (their padding too)
        p32[0].str_off = 7; p32[0].str_len = (uint32_t)a.size(); p32[1].str_off = (uint32_t)(7 + a.size()); p32[1].str_len = (uint32_t)b.size();
        memset(o16, 0, sizeof o16); memset(o32, 0, sizeof o32);
        uint64_t words[2] = { 0, 0 };
        for (uint32_t packed = 0; packed < 2; packed++) {
            sx::DecodeParams P;
            memset(&P, 0, sizeof P);
            P.arena = arena.data(); P.n = 2; P.out_arena = out.data(); P.kind = SX_DECODE_BASE64; P.words = words;
            P.recs = packed ? (const void*)p16 : (const void*)p32; P.packed = packed; P.out_recs = packed ? (void*)o16 : (void*)o32;
            uint32_t len[2];
            uint64_t word[2];
            memset(out.data(), 0xEE, out.size());
            ok = ok && sx::decode_measure_lane(P, 0, 0, &len[0], &word[0]) == 4 && sx::decode_measure_lane(P, 0, 1, &len[1], &word[1]) == 5;
            ok = ok && sx::decode_measure_lane(P, 0, 2, &len[0], &word[0]) == 0 && words[0] == (SX_DECODE_OK | SX_DECODE_TEXT | SX_DECODE_PADDED | 4ull << 32) && words[1] == 0;
            sx::decode_place_lane(P, 0, 0, 3);
            sx::decode_place_lane(P, 0, 1, 7);
            sx::decode_place_lane(P, 0, 2, 12);      // behind the last record: nothing
            ok = ok && !memcmp(out.data(), "\xEE\xEE\xEE" "ABCDhello", 12);
        }
        ok = ok && o16[0].position == p16[0].position && o16[0].str_off == 3 && o16[0].str_len == 4 && o16[0].flags == 0x05 && o16[0].mission_id == 0xA7;
        ok = ok && o16[1].position == 0x99ull && o16[1].str_off == 7 && o16[1].str_len == 5 && o16[1].flags == 0x02 && o16[1].mission_id == 0x01;
        sx_finding want32[2] = { p32[0], p32[1] };
        want32[0].str_off = 3; want32[0].str_len = 4; want32[1].str_off = 7; want32[1].str_len = 5;
        ok = ok && !memcmp(o32, want32, sizeof o32);
        cases += 10;
    }
    if (!ok) return 1;
    printf("decode core: ok, %llu cases\n", (unsigned long long)cases);
    return 0;
}
