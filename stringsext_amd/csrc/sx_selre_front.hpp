// sx_selre_front.hpp — what the three regex builders share (sx_selre_build.cpp: "does a pattern match somewhere in the string";
// sx_extract_build.cpp: "where do the matches lie"; sx_label_build.cpp: "which patterns match"), host only and internal to them: the parser (a syntax tree per pattern; whatever
// Python's `re` would read differently is refused with the offset), the count of the positions with the repeats unrolled (on the
// tree: nothing is allocated for a pattern that is refused for it), the Thompson NFA, the closure over its edges without a byte, the
// byte classes of the construction, the subset construction (a builder's Rule says whether the patterns are re-entered and what
// tells two subsets apart), Hopcroft's minimisation with the merge of the byte classes whose columns have become equal, the
// breadth-first order, the numbering by rank, the rows, and the shell that says what memory ran out for.  All builders accept the
// same language, refuse the same forms and meet the same limits with the same texts because they are these functions; what is left
// in a builder's own file is its Rule, its ranks and the fields that only its table has.  No HIP header: the test-only harnesses
// compile it with g++.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/stringsext_amd.h"
#include "sx_selset_build.hpp"

namespace sx {
namespace refront {

struct ByteSet {
    uint64_t w[4] = { 0, 0, 0, 0 };
    void add(uint32_t x) { w[x >> 6] |= (uint64_t)1 << (x & 63u); }
    void add_range(uint32_t lo, uint32_t hi) { for (uint32_t x = lo; x <= hi; x++) add(x); }
    bool has(uint32_t x) const { return (w[x >> 6] >> (x & 63u)) & 1u; }
    void join(const ByteSet& o) { for (int i = 0; i < 4; i++) w[i] |= o.w[i]; }
    void negate() { for (int i = 0; i < 4; i++) w[i] = ~w[i]; }
    bool operator==(const ByteSet& o) const { return !memcmp(w, o.w, sizeof w); }
};

struct Refused { uint32_t off; const char* why; };

enum NodeKind : uint8_t { kSet, kBol, kEol, kEmpty, kCat, kAlt, kRep };
constexpr uint32_t kInf = 0xFFFFFFFFu;
struct Node {
    NodeKind kind;
    uint32_t set = 0;              // kSet: index into the sets
    uint32_t lo = 0, hi = 0;       // kRep: the bounds, hi == kInf: none
    std::vector<uint32_t> kids;    // kCat, kAlt: all; kRep: one
};

inline bool is_alnum(uint32_t x) { return x - '0' < 10u || (x | 0x20u) - 'a' < 26u; }
inline int hex_of(uint32_t x) { return x - '0' < 10u ? (int)(x - '0') : (x | 0x20u) - 'a' < 6u ? (int)((x | 0x20u) - 'a' + 10) : -1; }

// \d \w \s and their complements; false: `x` is no shorthand
inline bool shorthand(uint32_t x, ByteSet* out) {
    ByteSet s;
    switch (x) {
    case 'd': case 'D': s.add_range('0', '9'); break;
    case 'w': case 'W': s.add_range('0', '9'); s.add_range('A', 'Z'); s.add_range('a', 'z'); s.add('_'); break;
    case 's': case 'S': s.add(' '); s.add_range('\t', '\r'); break;
    default: return false;
    }
    if (!(x & 0x20u)) s.negate();
    *out = s;
    return true;
}

struct Parser {
    const uint8_t* p;
    uint32_t len, at = 0;
    bool nocase;
    std::vector<Node>& nodes;
    std::vector<ByteSet>& sets;

    uint32_t node(Node&& n) { nodes.push_back(std::move(n)); return (uint32_t)nodes.size() - 1; }
    uint32_t leaf(NodeKind k) { Node n; n.kind = k; return node(std::move(n)); }
    uint32_t set_leaf(ByteSet s, bool negated) {
        if (nocase)
            for (uint32_t x = 'a'; x <= 'z'; x++)
                if (s.has(x) || s.has(x - 32)) { s.add(x); s.add(x - 32); }
        if (negated) s.negate();
        uint32_t i = 0;
        while (i < sets.size() && !(sets[i] == s)) i++;
        if (i == sets.size()) sets.push_back(s);
        Node n; n.kind = kSet; n.set = i;
        return node(std::move(n));
    }

    // behind a backslash (at: the byte behind it): one byte, or a shorthand's set (*is_set)
    uint32_t escape(ByteSet* set, bool* is_set) {
        *is_set = false;
        if (at >= len) throw Refused{ at - 1, "a backslash at the end of the pattern" };
        const uint32_t x = p[at++];
        if (!is_alnum(x)) return x;
        switch (x) {
        case 't': return '\t';
        case 'n': return '\n';
        case 'r': return '\r';
        case 'f': return '\f';
        case 'v': return '\v';
        case 'x': {
            if (at + 2 > len || hex_of(p[at]) < 0 || hex_of(p[at + 1]) < 0) throw Refused{ at - 2, "\\x needs two hex digits" };
            const uint32_t v = (uint32_t)(hex_of(p[at]) * 16 + hex_of(p[at + 1]));
            at += 2;
            return v;
        }
        default: break;
        }
        if (shorthand(x, set)) { *is_set = true; return 0; }
        throw Refused{ at - 2, "an escape that is not supported (of backslash + letter or digit only \\t \\n \\r \\f \\v \\xHH \\d \\D \\w \\W \\s \\S are)" };
    }

    // behind '['
    uint32_t klass() {
        const uint32_t open = at - 1;
        ByteSet s;
        bool negated = false;
        if (at < len && p[at] == '^') { negated = true; at++; }
        if (at < len && p[at] == ']') throw Refused{ at, "']' directly behind '[' or '[^': escape it" };
        for (;;) {
            if (at >= len) throw Refused{ open, "a class without its ']'" };
            uint32_t x = p[at++];
            if (x == ']') break;
            if (x == '[') throw Refused{ at - 1, "an unescaped '[' inside a class" };
            ByteSet sh; bool is_set = false;
            const uint32_t item = at - 1;
            if (x == '\\') x = escape(&sh, &is_set);
            if (at + 1 < len && p[at] == '-' && p[at + 1] != ']') {     // a range (a '-' in front of ']' is a literal)
                if (is_set) throw Refused{ item, "a shorthand class as a range end" };
                at++;
                uint32_t y = p[at++];
                const uint32_t hi_at = at - 1;
                if (y == '[') throw Refused{ hi_at, "an unescaped '[' inside a class" };
                bool y_set = false;
                if (y == '\\') y = escape(&sh, &y_set);
                if (y_set) throw Refused{ hi_at, "a shorthand class as a range end" };
                if (x > y) throw Refused{ item, "a range whose ends are in the wrong order" };
                s.add_range(x, y);
            } else if (is_set) s.join(sh);
            else s.add(x);
        }
        return set_leaf(s, negated);
    }

    // behind '{' (at: the byte behind it): the bounds
    void bounds(uint32_t* lo, uint32_t* hi) {
        const uint32_t open = at - 1;
        auto number = [&](uint32_t* v) {
            uint32_t digits = 0; *v = 0;
            while (at < len && (uint32_t)p[at] - '0' < 10u) { if (*v < 100000u) *v = *v * 10 + ((uint32_t)p[at] - '0'); at++; digits++; }
            return digits != 0;
        };
        const bool has_lo = number(lo);
        bool comma = false, has_hi = false;
        if (at < len && p[at] == ',') { comma = true; at++; has_hi = number(hi); }
        if (at >= len || p[at] != '}' || (!has_lo && !has_hi)) throw Refused{ open, "a '{' that does not begin a bound {m}, {m,}, {m,n} or {,n}: escape it" };
        at++;
        if (!has_lo) *lo = 0;
        if (!comma) *hi = *lo;
        else if (!has_hi) *hi = kInf;
        if (*lo > SX_SELECT_REGEX_MAX_REPEAT || (*hi != kInf && *hi > SX_SELECT_REGEX_MAX_REPEAT)) throw Refused{ open, "a repeat count above SX_SELECT_REGEX_MAX_REPEAT (255)" };
        if (*hi != kInf && *lo > *hi) throw Refused{ open, "a bound {m,n} with m > n" };
    }

    uint32_t alternation() {
        Node alt; alt.kind = kAlt;
        for (;;) {
            Node cat; cat.kind = kCat;
            while (at < len && p[at] != '|' && p[at] != ')') cat.kids.push_back(piece());
            alt.kids.push_back(cat.kids.empty() ? leaf(kEmpty) : cat.kids.size() == 1 ? cat.kids[0] : node(std::move(cat)));
            if (at < len && p[at] == '|') { at++; continue; }
            break;
        }
        return alt.kids.size() == 1 ? alt.kids[0] : node(std::move(alt));
    }

    uint32_t piece() {
        const uint32_t start = at;
        const uint32_t x = p[at++];
        uint32_t atom;
        bool anchor = false;
        switch (x) {
        case '(': {
            if (at < len && p[at] == '?') {
                if (at + 1 < len && p[at + 1] == ':') at += 2;
                else throw Refused{ start, "a group that begins with (? and is not (?:" };
            }
            atom = alternation();
            if (at >= len || p[at] != ')') throw Refused{ start, "a '(' without its ')'" };
            at++;
            break;
        }
        case '[': atom = klass(); break;
        case '.': { ByteSet s; s.add('\n'); atom = set_leaf(s, true); break; }
        case '^': atom = leaf(kBol); anchor = true; break;
        case '$': atom = leaf(kEol); anchor = true; break;
        case '*': case '+': case '?': throw Refused{ start, "a quantifier with nothing in front of it" };
        case '{': throw Refused{ start, "a '{' with nothing to repeat in front of it: escape it" };
        case '\\': {
            ByteSet s; bool is_set = false;
            const uint32_t v = escape(&s, &is_set);
            if (!is_set) s.add(v);
            atom = set_leaf(s, false);
            break;
        }
        default: { ByteSet s; s.add(x); atom = set_leaf(s, false); break; }
        }
        if (at >= len) return atom;
        uint32_t lo, hi;
        const uint32_t q = at;
        switch (p[at]) {
        case '*': lo = 0; hi = kInf; at++; break;
        case '+': lo = 1; hi = kInf; at++; break;
        case '?': lo = 0; hi = 1; at++; break;
        case '{': at++; bounds(&lo, &hi); break;
        default: return atom;
        }
        if (anchor) throw Refused{ q, "a quantifier on '^' or '$'" };
        if (at < len && p[at] == '?') at++;      // lazy: only existence is asked
        if (at < len && (p[at] == '*' || p[at] == '+' || p[at] == '?' || p[at] == '{')) throw Refused{ at, "a second quantifier" };
        Node rep; rep.kind = kRep; rep.lo = lo; rep.hi = hi; rep.kids.push_back(atom);
        return node(std::move(rep));
    }

    uint32_t pattern() {
        const uint32_t root = alternation();
        if (at < len) throw Refused{ at, "a ')' without its '('" };     // (alternation stops nowhere else)
        return root;
    }
};

// an upper bound on the NFA nodes that Nfa::build makes of `n`, its repeats unrolled (every leaf and every branch point is one),
// saturating: x{m,n} is n copies of x and n - m branches, x{m,} max(m, 1) copies — the last one loops — and one branch
inline uint64_t unrolled(const std::vector<Node>& nodes, uint32_t n) {
    const Node& N = nodes[n];
    constexpr uint64_t kMuch = (uint64_t)1 << 40;
    uint64_t v = 0;
    switch (N.kind) {
    case kSet: case kBol: case kEol: case kEmpty: return 1;
    case kCat: case kAlt:
        for (uint32_t k : N.kids) v = std::min(v + unrolled(nodes, k), kMuch);
        return N.kind == kAlt ? v + N.kids.size() - 1 : v;
    case kRep: {
        const uint64_t copies = N.hi == kInf ? std::max<uint32_t>(N.lo, 1) : N.hi, branches = N.hi == kInf ? 1 : N.hi - N.lo;
        return std::min(std::max<uint64_t>(unrolled(nodes, N.kids[0]) * copies + branches, 1), kMuch);
    }
    }
    return kMuch;
}

enum NfaKind : uint8_t { nChar, nSplit, nBol, nEol, nAccept };
struct NfaNode { NfaKind kind; uint32_t set, a, b; };     // nAccept: `set` is the pattern's index where every pattern has its own (Front)

struct Nfa {
    std::vector<NfaNode> n;
    size_t most = 0;     // what the count on the trees allows: more is a fault of the count, not a reason to go on allocating
    uint32_t add(NfaKind k, uint32_t set, uint32_t a, uint32_t b) {
        if (n.size() >= most) throw Refused{ 0, "the NFA has more nodes than were counted" };
        n.push_back(NfaNode{ k, set, a, b });
        return (uint32_t)n.size() - 1;
    }
    // the entry of the nodes that match what tree node `t` matches and go on at `next`
    uint32_t build(const std::vector<Node>& nodes, uint32_t t, uint32_t next) {
        const Node& N = nodes[t];
        switch (N.kind) {
        case kSet: return add(nChar, N.set, next, 0);
        case kBol: return add(nBol, 0, next, 0);
        case kEol: return add(nEol, 0, next, 0);
        case kEmpty: return next;
        case kCat:
            for (size_t k = N.kids.size(); k-- > 0;) next = build(nodes, N.kids[k], next);
            return next;
        case kAlt: {
            uint32_t cur = build(nodes, N.kids.back(), next);
            for (size_t k = N.kids.size() - 1; k-- > 0;) { const uint32_t one = build(nodes, N.kids[k], next); cur = add(nSplit, 0, one, cur); }
            return cur;
        }
        case kRep: {
            uint32_t cur = next;
            if (N.hi == kInf) {      // x* = a branch: x and back, or on; x{m,}, m >= 1 = m times x, the last one entered at x: no copy for the loop
                const uint32_t loop = add(nSplit, 0, 0, next);
                const uint32_t body = build(nodes, N.kids[0], loop);
                n[loop].a = body;
                cur = N.lo ? body : loop;
                for (uint32_t k = 1; k < N.lo; k++) cur = build(nodes, N.kids[0], cur);
                return cur;
            } else {                 // x{m,n} = m times x, then (x(x(...)?)?)?
                for (uint32_t k = N.lo; k < N.hi; k++) { const uint32_t body = build(nodes, N.kids[0], cur); cur = add(nSplit, 0, body, next); }
            }
            for (uint32_t k = 0; k < N.lo; k++) cur = build(nodes, N.kids[0], cur);
            return cur;
        }
        }
        return next;
    }
};

// what is reached from NFA nodes without a byte: the byte nodes, and the accept nodes through which the string is accepted here
// whatever follows (`here`) or if it ends here (`end`: through a `$`): bit p for pattern p's (bit 0 alone where the NFA has one
// accept for all)
struct Closure { std::vector<uint32_t> chars; uint64_t here = 0, end = 0; };

struct Closer {
    const Nfa& nfa;
    std::vector<uint32_t> seen[2];     // by mode: 0 in front of any `$`, 1 behind one
    uint32_t stamp = 0;
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    explicit Closer(const Nfa& f) : nfa(f) { seen[0].assign(f.n.size(), 0); seen[1].assign(f.n.size(), 0); }
    void run(uint32_t from, bool at_start, Closure* out) {
        stamp++;
        stack.clear();
        stack.push_back({ from, 0 });
        while (!stack.empty()) {
            const uint32_t v = stack.back().first, mode = stack.back().second;
            stack.pop_back();
            if (seen[mode][v] == stamp) continue;
            seen[mode][v] = stamp;
            const NfaNode& N = nfa.n[v];
            switch (N.kind) {
            case nChar: if (!mode) out->chars.push_back(v); break;
            case nSplit: stack.push_back({ N.b, mode }); stack.push_back({ N.a, mode }); break;
            case nBol: if (at_start) stack.push_back({ N.a, mode }); break;
            case nEol: stack.push_back({ N.a, 1 }); break;
            case nAccept: (mode ? out->end : out->here) |= (uint64_t)1 << N.set; break;
            }
        }
        std::sort(out->chars.begin(), out->chars.end());
    }
};

struct KeyHash {
    size_t operator()(const std::vector<uint32_t>& k) const {
        uint64_t h = 1469598103934665603ull;
        for (uint32_t v : k) { h ^= v; h *= 1099511628211ull; }
        return (size_t)h;
    }
};

inline int fail(std::string* err, const std::string& what) { if (err) *err = what; return SX_E_INVALID; }

constexpr uint32_t kEndMark = 0xFFFFFFFFu;               // in a subset's key: it accepts at the end
constexpr uint64_t kSubsetEntries = (uint64_t)32 << 20;  // the subsets' entries all together: a bound on the construction's memory

// Steps 1 to 3 — the trees, the positions, the NFA with one accept and every pattern an alternative — and the byte classes of the
// construction: the bytes that no set tells apart.  accept_per_pattern (set before front_build; the regex set and the extraction
// leave it alone): every pattern ends in an accept node of its own that carries the pattern's index.
struct Front {
    std::vector<ByteSet> sets;
    Nfa nfa;
    uint32_t start = 0;
    uint32_t K = 1;          // construction classes
    uint8_t cls[256] = {};   // byte -> construction class
    uint8_t rep[256] = {};   // construction class -> its lowest byte
    bool accept_per_pattern = false;
};

// SX_OK, or SX_E_INVALID with *err said: a bad count, flag, length or pointer, a refused pattern, a limit on repeats or positions.
// (`patterns` is not NULL.  std::bad_alloc passes through: the caller says what it was building.)
inline int front_build(const sx_pattern* patterns, uint32_t n_patterns, uint32_t flags, Front* F, std::string* err) {
    if (n_patterns < 1 || n_patterns > SX_SELECT_REGEX_MAX_PATTERNS) return fail(err, "n_patterns must be 1..64");
    if (flags & ~(uint32_t)SX_SELECT_ASCII_NOCASE) return fail(err, "a regex set takes SX_SELECT_ASCII_NOCASE and no other flag");
    for (uint32_t p = 0; p < n_patterns; p++)
        if (!patterns[p].bytes || patterns[p].len < 1 || patterns[p].len > SX_SELECT_REGEX_MAX_PATTERN_BYTES)
            return fail(err, "pattern " + std::to_string(p) + ": a pattern must have 1..1024 bytes and a pointer");
    const bool nocase = (flags & SX_SELECT_ASCII_NOCASE) != 0;
    // 1. the trees
    std::vector<Node> nodes;
    std::vector<ByteSet>& sets = F->sets;
    std::vector<uint32_t> roots;
    uint64_t positions = 0;
    for (uint32_t p = 0; p < n_patterns; p++) {
        Parser ps{ patterns[p].bytes, patterns[p].len, 0, nocase, nodes, sets };
        try {
            roots.push_back(ps.pattern());
        } catch (const Refused& r) {
            return fail(err, "pattern " + std::to_string(p) + ", offset " + std::to_string(r.off) + ": " + r.why);
        }
        // 2. the positions, before anything is unrolled
        positions += unrolled(nodes, roots.back());
        if (positions > SX_SELECT_REGEX_MAX_POSITIONS)
            return fail(err, "pattern " + std::to_string(p) + ": more than SX_SELECT_REGEX_MAX_POSITIONS (65536) positions once the counted repeats are unrolled");
    }
    // 3. the NFA: one accept, every pattern an alternative
    Nfa& nfa = F->nfa;
    // the accept (or one per pattern), the patterns' nodes, a branch per pattern but one
    nfa.most = (size_t)positions + n_patterns + (F->accept_per_pattern ? n_patterns - 1 : 0);
    nfa.n.reserve(nfa.most);
    try {
        const bool per = F->accept_per_pattern;
        uint32_t accept = nfa.add(nAccept, per ? n_patterns - 1 : 0, 0, 0);
        uint32_t start = nfa.build(nodes, roots.back(), accept);
        for (size_t p = roots.size() - 1; p-- > 0;) {
            if (per) accept = nfa.add(nAccept, (uint32_t)p, 0, 0);
            const uint32_t one = nfa.build(nodes, roots[p], accept);
            start = nfa.add(nSplit, 0, one, start);
        }
        F->start = start;
    } catch (const Refused& r) {
        return fail(err, std::string("internal: ") + r.why);
    }
    // the byte classes of the construction
    uint8_t* cls = F->cls;
    uint32_t K = 1;
    for (const ByteSet& s : sets) {
        uint16_t split[256];
        for (uint32_t c = 0; c < K; c++) split[c] = 0xFFFF;
        bool in0[256] = {};   // the side of the set that keeps the class's number: its first byte's
        for (uint32_t x = 0; x < 256; x++) {
            const uint32_t c = cls[x];
            if (split[c] == 0xFFFF) { split[c] = (uint16_t)c; in0[c] = s.has(x); continue; }
            if (s.has(x) == in0[c]) continue;
            if (split[c] == c) split[c] = (uint16_t)K++;
            cls[x] = (uint8_t)split[c];
        }
    }
    F->K = K;
    for (uint32_t x = 256; x-- > 0;) F->rep[cls[x]] = (uint8_t)x;
    return SX_OK;
}

// Step 4.  The subset construction: a complete DFA D[s * K + c] over n subsets of the NFA's byte nodes, each of a kind below
// n_kinds, and its starts (one, twice, where the patterns are re-entered).
struct SubsetDfa {
    uint32_t n = 0, n_kinds = 0, starts[2] = { 0, 0 };
    std::vector<uint32_t> D, kinds;
};

// A Rule says what a builder's automaton is.  `reenter`: the unanchored search — every pattern is entered again in front of every
// byte, without the `^` edges; one start, with them.  A subset then always holds the re-entry's byte nodes, so its key is what it
// holds BESIDES them (a keyword list's re-entry has a node per keyword), and what the re-entry's own nodes give with a byte is worked
// out once per class.  Not `reenter`: the anchored walk, two starts — with the `^` edges, then without them —, and what may be
// accepted in front of the first byte does not count.  mark(here, end, key), of the subset that holds the byte nodes in `key` and
// whose closures' accepts are `here` and `end`: it brings the masks to what counts of them and appends to the key whatever else
// tells two subsets of these nodes apart (the key's words count against kSubsetEntries); true: the subset is, whatever its nodes,
// the ONE absorbing state — made when first needed, its row points at itself.  kind(here, end), of a new subset, with the masks
// as mark left them: what Hopcroft tells states apart by to begin with.
// SX_OK, or SX_E_INVALID with *err said: more than SX_SELECT_REGEX_MAX_STATES subsets, or more than kSubsetEntries words in their keys.
template <class Rule>
inline int subsets(const Front& F, Rule& rule, SubsetDfa* out, std::string* err) {
    const Nfa& nfa = F.nfa;
    const uint32_t K = F.K, none = 0xFFFFFFFFu;
    Closer closer(nfa);
    std::vector<Closure> after(nfa.n.size());      // behind a byte node: closure(its successor), made when first needed
    std::vector<uint8_t> after_made(nfa.n.size(), 0), in_again(nfa.n.size(), 0);
    std::unordered_map<std::vector<uint32_t>, uint32_t, KeyHash> ids;
    std::vector<std::vector<uint32_t>> keys;
    std::vector<uint32_t> held;                    // subset -> how many words of its key are byte nodes: the first ones
    std::vector<uint32_t>& D = out->D, &kinds = out->kinds;
    uint32_t absorber = none;
    uint64_t entries = 0;
    auto state_of = [&](std::vector<uint32_t>&& key, uint64_t here, uint64_t end) -> uint32_t {
        const uint32_t nodes = (uint32_t)key.size(), id = (uint32_t)keys.size();
        if (rule.mark(here, end, key)) {
            if (absorber != none) return absorber;
            absorber = id;
            key.clear();
        } else {
            auto it = ids.find(key);
            if (it != ids.end()) return it->second;
            entries += key.size();
            ids.emplace(key, id);
        }
        held.push_back(absorber == id ? 0 : nodes);
        kinds.push_back(rule.kind(here, end));
        out->n_kinds = std::max(out->n_kinds, kinds.back() + 1);
        keys.push_back(std::move(key));
        return id;
    };
    std::vector<uint32_t> mark(nfa.n.size(), 0);
    uint32_t mark_stamp = 0;
    // `to` joined with what is behind the first `count` nodes of `from` that take a byte of class c
    auto step = [&](const std::vector<uint32_t>& from, size_t count, uint32_t c, Closure* to) {
        for (size_t k = 0; k < count; k++) {
            const uint32_t v = from[k];
            if (!F.sets[nfa.n[v].set].has(F.rep[c])) continue;
            if (!after_made[v]) { closer.run(nfa.n[v].a, false, &after[v]); after_made[v] = 1; }
            const Closure& C = after[v];
            to->here |= C.here; to->end |= C.end;
            for (uint32_t u : C.chars) if (!in_again[u] && mark[u] != mark_stamp) { mark[u] = mark_stamp; to->chars.push_back(u); }
        }
    };
    Closure again;                                 // the re-entry in front of every later byte: no `^` edge
    if (Rule::reenter) closer.run(F.start, false, &again);
    for (uint32_t v : again.chars) in_again[v] = 1;
    std::vector<Closure> again_to(K);
    for (uint32_t c = 0; c < K; c++) {
        again_to[c].here = again.here; again_to[c].end = again.end;
        mark_stamp++;
        step(again.chars, again.chars.size(), c, &again_to[c]);
    }
    for (int k = 0; k < (Rule::reenter ? 1 : 2); k++) {      // with the `^` edges, then, for the anchored walk, without them
        Closure c;
        closer.run(F.start, k == 0, &c);
        c.chars.erase(std::remove_if(c.chars.begin(), c.chars.end(), [&](uint32_t v) { return in_again[v] != 0; }), c.chars.end());
        if (!Rule::reenter) c.here = c.end = 0;              // (a match is never empty)
        out->starts[k] = out->starts[1] = state_of(std::move(c.chars), c.here, c.end);
    }
    bool too_many = false;
    for (uint32_t s = 0; s < keys.size() && !too_many; s++) {
        D.resize((size_t)(s + 1) * K);
        if (s == absorber) { for (uint32_t c = 0; c < K; c++) D[(size_t)s * K + c] = s; continue; }
        const std::vector<uint32_t> key = keys[s];     // (a copy: keys grows)
        for (uint32_t c = 0; c < K; c++) {
            Closure to = again_to[c];
            mark_stamp++;
            for (uint32_t v : to.chars) mark[v] = mark_stamp;
            step(key, held[s], c, &to);
            std::sort(to.chars.begin(), to.chars.end());
            D[(size_t)s * K + c] = state_of(std::move(to.chars), to.here, to.end);
            if (keys.size() > SX_SELECT_REGEX_MAX_STATES || entries > kSubsetEntries) { too_many = true; break; }
        }
    }
    if (too_many)
        return fail(err, keys.size() > SX_SELECT_REGEX_MAX_STATES ? std::string("the patterns need more than SX_SELECT_REGEX_MAX_STATES (65536) states")
                                                                  : "the subset construction was stopped at the bound on its memory: its " + std::to_string(keys.size()) + " states so far hold more than 33554432 NFA positions in all");
    out->n = (uint32_t)keys.size();
    return SX_OK;
}

// Step 5.  The minimal automaton of a subset construction's DFA, whose states are told apart by their kinds to begin with:
// Hopcroft's blocks of states that no string tells apart, the quotient, then the byte classes whose columns are equal in every
// block, numbered by their lowest byte.
struct Quotient {
    uint32_t M = 0, K = 0;            // blocks, construction classes
    std::vector<uint32_t> blk;        // state -> block
    std::vector<uint32_t> kind;       // block -> its states' kind
    std::vector<uint32_t> Q;          // Q[B * K + c]: block, construction class -> block
    std::vector<uint32_t> first_of;   // final class -> a construction class of it
    uint8_t map[256] = {};            // byte -> final class
};

inline void minimise(const SubsetDfa& S, const Front& F, Quotient* out) {
    const uint32_t n = S.n, K = F.K, n_kinds = S.n_kinds;
    const std::vector<uint32_t>&D = S.D, &kinds = S.kinds;
    const uint8_t* cls = F.cls;
    std::vector<uint32_t> elems(n), loc(n), blk(n), bbeg, bend, marked;
    {
        std::vector<uint32_t> at(n_kinds + 1, 0);
        for (uint32_t s = 0; s < n; s++) at[kinds[s] + 1]++;
        for (uint32_t k = 0; k < n_kinds; k++) {
            if (at[k + 1]) { bbeg.push_back(at[k]); bend.push_back(at[k] + at[k + 1]); }
            at[k + 1] += at[k];
        }
        for (uint32_t s = 0; s < n; s++) { const uint32_t to = at[kinds[s]]++; elems[to] = s; loc[s] = to; }
        for (uint32_t B = 0; B < bbeg.size(); B++) for (uint32_t i = bbeg[B]; i < bend[B]; i++) blk[elems[i]] = B;
    }
    if (bbeg.size() > 1) {
        // the sources of every (class, target): inv[inv_at[c * n + q] .. inv_at[c * n + q + 1])
        std::vector<uint32_t> inv_at((size_t)K * n + 1, 0), inv((size_t)K * n);
        for (uint32_t s = 0; s < n; s++) for (uint32_t c = 0; c < K; c++) inv_at[(size_t)c * n + D[(size_t)s * K + c] + 1]++;
        for (size_t i = 0; i < (size_t)K * n; i++) inv_at[i + 1] += inv_at[i];
        {
            std::vector<uint32_t> fill(inv_at.begin(), inv_at.end() - 1);
            for (uint32_t s = 0; s < n; s++) for (uint32_t c = 0; c < K; c++) inv[fill[(size_t)c * n + D[(size_t)s * K + c]]++] = s;
        }
        std::vector<uint32_t> work, members, touched;
        for (uint32_t B = 0; B < bbeg.size(); B++) work.push_back(B);
        marked.assign(bbeg.size(), 0);
        while (!work.empty()) {
            const uint32_t A = work.back();
            work.pop_back();
            members.assign(elems.begin() + bbeg[A], elems.begin() + bend[A]);
            for (uint32_t c = 0; c < K; c++) {
                touched.clear();
                for (uint32_t q : members)
                    for (uint32_t i = inv_at[(size_t)c * n + q]; i < inv_at[(size_t)c * n + q + 1]; i++) {
                        const uint32_t p = inv[i], B = blk[p], to = bbeg[B] + marked[B];
                        if (!marked[B]++) touched.push_back(B);
                        const uint32_t other = elems[to];
                        elems[to] = p; elems[loc[p]] = other; loc[other] = loc[p]; loc[p] = to;
                    }
                for (uint32_t B : touched) {
                    const uint32_t m = marked[B], size = bend[B] - bbeg[B];
                    marked[B] = 0;
                    if (m == size) continue;
                    const uint32_t N = (uint32_t)bbeg.size();     // the smaller part becomes the new block
                    if (m <= size - m) { bbeg.push_back(bbeg[B]); bend.push_back(bbeg[B] + m); bbeg[B] += m; }
                    else { bbeg.push_back(bbeg[B] + m); bend.push_back(bend[B]); bend[B] = bbeg[B] + m; }
                    marked.push_back(0);
                    for (uint32_t i = bbeg[N]; i < bend[N]; i++) blk[elems[i]] = N;
                    work.push_back(N);
                }
            }
        }
    }
    const uint32_t M = (uint32_t)bbeg.size();
    // the quotient, then the byte classes whose columns are equal in every state
    std::vector<uint32_t> Q((size_t)M * K);
    out->kind.assign(M, 0);
    for (uint32_t B = 0; B < M; B++) {
        const uint32_t s = elems[bbeg[B]];
        out->kind[B] = kinds[s];
        for (uint32_t c = 0; c < K; c++) Q[(size_t)B * K + c] = blk[D[(size_t)s * K + c]];
    }
    std::vector<uint32_t> final_of(K), first_of;     // construction class -> final class; final class -> a construction class
    std::vector<uint64_t> column(K, 1469598103934665603ull);   // (a hash: most pairs of columns differ)
    for (uint32_t B = 0; B < M; B++) for (uint32_t c = 0; c < K; c++) column[c] = (column[c] ^ Q[(size_t)B * K + c]) * 1099511628211ull;
    for (uint32_t c = 0; c < K; c++) {
        uint32_t f = 0;
        for (; f < first_of.size(); f++) {
            if (column[c] != column[first_of[f]]) continue;
            uint32_t B = 0;
            while (B < M && Q[(size_t)B * K + c] == Q[(size_t)B * K + first_of[f]]) B++;
            if (B == M) break;
        }
        if (f == first_of.size()) first_of.push_back(c);
        final_of[c] = f;
    }
    {   // final classes numbered by their lowest byte
        std::vector<uint32_t> number(first_of.size(), 0xFFFFFFFFu);
        uint32_t next_number = 0;
        for (uint32_t x = 0; x < 256; x++) {
            const uint32_t f = final_of[cls[x]];
            if (number[f] == 0xFFFFFFFFu) number[f] = next_number++;
            out->map[x] = (uint8_t)number[f];
        }
        std::vector<uint32_t> by_number(first_of.size());
        for (uint32_t f = 0; f < first_of.size(); f++) by_number[number[f]] = first_of[f];
        first_of = by_number;
    }
    out->M = M; out->K = K;
    out->blk = std::move(blk);
    out->Q = std::move(Q);
    out->first_of = std::move(first_of);
}

// Step 6.  The numbering and the rows.  The minimal automaton is unique, its final classes are numbered by their lowest byte and
// the order is breadth first over them, so a table is a function of the language and the ranks alone.

inline bool absorbing(const Quotient& Qt, uint32_t B) {      // every byte leads back to it
    for (uint32_t c = 0; c < Qt.K; c++) if (Qt.Q[(size_t)B * Qt.K + c] != B) return false;
    return true;
}

// the blocks that the starts reach, the starts first, then breadth first with the final classes in ascending order
inline std::vector<uint32_t> bfs_order(const Quotient& Qt, const uint32_t* starts) {
    std::vector<uint32_t> order;
    std::vector<uint8_t> seen(Qt.M, 0);
    auto reach = [&](uint32_t B) { if (!seen[B]) { seen[B] = 1; order.push_back(B); } };
    reach(Qt.blk[starts[0]]); reach(Qt.blk[starts[1]]);
    for (size_t i = 0; i < order.size(); i++)
        for (uint32_t c : Qt.first_of) reach(Qt.Q[(size_t)order[i] * Qt.K + c]);
    return order;
}

// place[B]: the number of block B — the blocks of rank 0 in their order, then those of rank 1, ... —, first[r]: the first number
// of rank r (first[n_ranks]: the count).  root_is_zero: order[0] is number 0 whatever its rank, and counts for none.
struct Numbering { std::vector<uint32_t> place, first; };
template <class Rank>
inline Numbering number_by_rank(const Quotient& Qt, const std::vector<uint32_t>& order, uint32_t n_ranks, bool root_is_zero, Rank rank) {
    Numbering N;
    N.place.assign(Qt.M, 0);
    std::vector<uint32_t> ranks(order.size());
    for (size_t i = 0; i < order.size(); i++) ranks[i] = rank(order[i]);
    uint32_t number = root_is_zero ? 1 : 0;
    for (uint32_t r = 0; r < n_ranks; r++) {
        N.first.push_back(number);
        for (size_t i = root_is_zero ? 1 : 0; i < order.size(); i++) if (ranks[i] == r) N.place[order[i]] = number++;
    }
    N.first.push_back(number);
    return N;
}

// what every builder's table has: the counts, the class map, and the rows next[state * classes + class]
template <class Table>
inline void write_table(const Quotient& Qt, const std::vector<uint32_t>& order, const std::vector<uint32_t>& place, uint32_t n_patterns, uint32_t flags, Table* T) {
    const uint32_t classes = (uint32_t)Qt.first_of.size();
    T->n_patterns = n_patterns; T->nocase = (flags & SX_SELECT_ASCII_NOCASE) ? 1u : 0u;
    T->states = (uint32_t)order.size(); T->classes = classes;
    T->lds_states = std::min(T->states, kSelsetLdsBytes / (classes * 2u));
    memcpy(T->map, Qt.map, sizeof T->map);
    T->next.assign((size_t)T->states * classes, 0);
    for (uint32_t B : order)
        for (uint32_t f = 0; f < classes; f++) T->next[(size_t)place[B] * classes + f] = (uint16_t)place[Qt.Q[(size_t)B * Qt.K + Qt.first_of[f]]];
}

// A builder's shell: `body` makes the table and answers SX_OK or what refused the patterns; `what`: "regex set", ...
template <class Body>
inline int build_table(bool pointers, const char* what, std::string* err, Body body) {
    if (!pointers) return fail(err, "a NULL pointer");
    try {
        return body();
    } catch (const std::bad_alloc&) {
        if (err) *err = std::string("no host memory for the ") + what + "'s table";
        return SX_E_NOMEM;
    }
}

}  // namespace refront
}  // namespace sx
