// utf16_asan.cpp — stand-alone host program for a sanitizer run of the UTF-16 positions in oplog.cpp
// (OpLog::units_of, apply_patches_utf16, patches_since_utf16): CPU only, no device code, no Python.
// tools/asan_utf16.sh builds it with AddressSanitizer + UBSan and runs it.
//
// Per round (40 seeded rounds, RGA, then Fugue) a log goes through steps of local edits, wire
// updates, a join and a delta, with a std::u32string model kept beside it; after each step a mark is
// taken and the model recorded.  After every step, for the version now and for every mark so far,
// every gap asked in codepoints, in UTF-8 bytes and in UTF-16 code units must give the three sums
// over the recording, with the info; the patches since every mark, in UTF-16 code units, spliced
// into the recording's UTF-16 must give the UTF-16 of the text now; and a seeded patch set in UTF-16
// code units applied to a copy must leave the log apply_patches leaves on another copy for the
// set translated through the model.  Input and output blocks are heap blocks of exactly n entries,
// so an access past one is seen.  The malformed calls run after every step and must be refused with
// their outputs, or the log, untouched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crdt_hip.h"
#include "oplog.hpp"
#include "util.hpp"

using crdt::kTextEnd;
using crdt::kUnitBytes;
using crdt::kUnitCodepoints;
using crdt::kUnitUtf16;
using crdt::LogMark;
using crdt::OpLog;
using crdt::PatchRec;
using crdt::TextInfo;
using crdt::UnitInfo;
using crdt::UnitPos;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % (n ? n : 1));
}

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

size_t g_queries = 0, g_refused = 0, g_sets = 0, g_spliced = 0;

const std::u32string kWords[] = {U"a",  U"b\nc", U"é",   U"€",          U"\U0001F600",
                                 U"xyz ", U"\U0001D11E\U0001F600", U"q\U0001D11E"};

// The same positional edits to the log and to the model; three words in eight hold an astral.
void edits(OpLog& log, std::u32string& model, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i) {
        const uint64_t n = log.visible();
        REQUIRE(n == model.size());
        if (n < 4 || rnd(100) < 60) {
            const std::u32string& w = kWords[rnd(8)];
            const uint32_t at = rnd((uint32_t)n + 1);
            REQUIRE(log.insert(at, reinterpret_cast<const uint32_t*>(w.data()), w.size()).empty());
            model.insert(at, w);
        } else {
            const uint64_t a = rnd((uint32_t)n - 1), b = std::min<uint64_t>(n, a + 1 + rnd(3));
            REQUIRE(log.remove(a, b).empty());
            model.erase(a, b - a);
        }
    }
}

std::u32string decode(const std::string& s) {
    std::u32string out;
    for (size_t i = 0; i < s.size();) {
        const uint8_t b = (uint8_t)s[i];
        const size_t k = b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
        REQUIRE(i + k <= s.size());
        char32_t c = k == 1 ? b : b & (0xFFu >> (k + 1));
        for (size_t j = 1; j < k; ++j) c = (c << 6) | ((uint8_t)s[i + j] & 0x3Fu);
        out.push_back(c);
        i += k;
    }
    return out;
}
std::string encode(const std::u32string& t) {
    std::string out;
    for (char32_t c : t) {
        char b[4];
        out.append(b, crdt::utf8_put((uint32_t)c, b));
    }
    return out;
}
std::u16string utf16(const std::u32string& t) {
    std::u16string out;
    for (char32_t c : t) {
        if (c < 0x10000) {
            out.push_back((char16_t)c);
        } else {
            out.push_back((char16_t)(0xD800 + ((c - 0x10000) >> 10)));
            out.push_back((char16_t)(0xDC00 + ((c - 0x10000) & 0x3FF)));
        }
    }
    return out;
}

// The log's whole text now, through text_at (the model after a sync).
std::u32string text_now(const OpLog& log) {
    std::string err;
    size_t need = 0;
    TextInfo i{};
    const int rc = log.text_at(nullptr, 0, kTextEnd, 0, nullptr, 0, &need, &i, err);
    REQUIRE(rc == (need ? CRDT_HIP_ESPACE : CRDT_HIP_OK));
    std::string out(need, '\0');
    if (need)
        REQUIRE(log.text_at(nullptr, 0, kTextEnd, 0, reinterpret_cast<uint8_t*>(&out[0]), need, &need, &i,
                            err) == CRDT_HIP_OK);
    return decode(out);
}

// The model of a version: per gap its bytes and its UTF-16 code units.
struct Gaps {
    std::vector<uint64_t> b, u;
    explicit Gaps(const std::u32string& t) : b(1, 0), u(1, 0) {
        for (char32_t c : t) {
            char tmp[4];
            b.push_back(b.back() + crdt::utf8_put((uint32_t)c, tmp));
            u.push_back(u.back() + (c >= 0x10000 ? 2 : 1));
        }
    }
    uint64_t len() const { return b.size() - 1; }
    uint64_t at(uint32_t unit, uint64_t g) const { return unit == kUnitUtf16 ? u[g] : unit == kUnitBytes ? b[g] : g; }
    uint64_t total(uint32_t unit) const { return at(unit, len()); }
};

// One call into a heap block of exactly n records; the positions in a heap block of exactly n too.
std::vector<UnitPos> ask(const OpLog& log, const LogMark* m, const std::vector<uint64_t>& q, uint32_t unit,
                         const Gaps& want) {
    const size_t n = q.size();
    uint64_t* in = (uint64_t*)std::malloc(n ? n * sizeof(uint64_t) : 1);
    UnitPos* out = (UnitPos*)std::malloc(n ? n * sizeof(UnitPos) : 1);
    REQUIRE(in && out);
    if (n) std::memcpy(in, q.data(), n * sizeof(uint64_t));
    UnitInfo info{7, 7, 7};
    std::string err;
    REQUIRE(log.units_of(m, n ? in : nullptr, n, unit, n ? out : nullptr, &info, err) == CRDT_HIP_OK);
    REQUIRE(info.len == want.len() && info.len_bytes == want.b.back() && info.len_utf16 == want.u.back());
    std::vector<UnitPos> got(out, out + n);
    std::free(in);
    std::free(out);
    g_queries += n;
    return got;
}

void check_version(const OpLog& log, const LogMark* m, const std::u32string& text) {
    const Gaps w(text);
    const uint64_t len = w.len();
    for (uint32_t unit : {kUnitCodepoints, kUnitBytes, kUnitUtf16}) {
        std::vector<uint64_t> q, gap;
        for (uint64_t g = len + 1; g-- > 0;) gap.push_back(g);  // every gap, descending
        gap.push_back(len / 2);                                 // and one again
        for (uint64_t g : gap) q.push_back(w.at(unit, g));
        const std::vector<UnitPos> got = ask(log, m, q, unit, w);
        for (size_t i = 0; i < gap.size(); ++i)
            REQUIRE(got[i].cp == gap[i] && got[i].bytes == w.b[gap[i]] && got[i].utf16 == w.u[gap[i]]);
        ask(log, m, {}, unit, w);  // n == 0 writes only the info
    }
    std::string err;
    UnitPos one{9, 9, 9};
    const uint64_t zero = 0;
    REQUIRE(log.units_of(m, &zero, 1, kUnitUtf16, &one, nullptr, err) == CRDT_HIP_OK);  // info may be null
    REQUIRE(one.cp == 0 && one.bytes == 0 && one.utf16 == 0);
}

// A refused call leaves out and *info as they were.
void refused(const OpLog& log, const LogMark* m, std::vector<uint64_t> q, uint32_t unit, int code,
             bool null_in = false, bool null_out = false) {
    const size_t n = q.size();
    UnitPos* out = (UnitPos*)std::malloc(n * sizeof(UnitPos));
    REQUIRE(out);
    std::memset(out, 0xA5, n * sizeof(UnitPos));
    UnitInfo info{7, 7, 7};
    std::string err;
    const int rc = log.units_of(m, null_in ? nullptr : q.data(), n, unit, null_out ? nullptr : out, &info, err);
    REQUIRE(rc == code && !err.empty() && info.len == 7 && info.len_bytes == 7 && info.len_utf16 == 7);
    for (size_t k = 0; k < n * sizeof(UnitPos); ++k) REQUIRE(reinterpret_cast<uint8_t*>(out)[k] == 0xA5);
    std::free(out);
    ++g_refused;
}

void malformed(const OpLog& log, const LogMark* m, const std::u32string& text) {
    const Gaps w(text);
    for (uint32_t unit : {kUnitCodepoints, kUnitBytes, kUnitUtf16}) {
        refused(log, m, {0, w.total(unit) + 1}, unit, CRDT_HIP_ERANGE);
        refused(log, m, {~0ull}, unit, CRDT_HIP_ERANGE);
        refused(log, m, {0}, unit, CRDT_HIP_EINVAL, true);
        refused(log, m, {0}, unit, CRDT_HIP_EINVAL, false, true);
        refused(log, m, {w.total(unit) + 9}, unit, CRDT_HIP_EINVAL, false, true);  // the earlier check's code
    }
    refused(log, m, {0}, 3, CRDT_HIP_EINVAL);
    refused(log, m, {~0ull}, 3, CRDT_HIP_EINVAL);
    for (uint64_t k = 0; k < w.len(); ++k)
        if (w.u[k + 1] - w.u[k] == 2) {  // an astral: the unit inside the pair, every byte inside it
            refused(log, m, {w.u[k] + 1}, kUnitUtf16, CRDT_HIP_EINVAL);
            refused(log, m, {0, w.u[k] + 1, w.u.back()}, kUnitUtf16, CRDT_HIP_EINVAL);
            refused(log, m, {w.u[k] + 1, w.u.back() + 1}, kUnitUtf16, CRDT_HIP_ERANGE);  // the range error wins
            for (uint64_t x = w.b[k] + 1; x < w.b[k + 1]; ++x) {
                refused(log, m, {0, x, w.b.back()}, kUnitBytes, CRDT_HIP_EINVAL);
                refused(log, m, {x, w.b.back() + 1}, kUnitBytes, CRDT_HIP_ERANGE);
            }
            break;
        }
}

// The patches since a mark in UTF-16 code units, spliced into the recording's UTF-16, give the
// UTF-16 now; the patch count and the ins bytes are the codepoint call's.
void check_since(const OpLog& log, const LogMark& m, const std::u32string& was, const std::u32string& now) {
    std::vector<PatchRec> p, pc;
    std::vector<uint8_t> ins, insc;
    std::string err;
    REQUIRE(log.patches_since_utf16(m, p, ins, err) == CRDT_HIP_OK);
    REQUIRE(log.patches_since(m, pc, insc, err) == CRDT_HIP_OK);
    REQUIRE(p.size() == pc.size() && ins == insc);
    std::u16string t = utf16(was);
    for (size_t k = 0; k < p.size(); ++k) {
        REQUIRE(p[k].ins_off == pc[k].ins_off && p[k].ins_len == pc[k].ins_len);
        REQUIRE(p[k].pos + p[k].del <= t.size());
        const std::string piece(reinterpret_cast<const char*>(ins.data()) + p[k].ins_off, p[k].ins_len);
        t.replace((size_t)p[k].pos, p[k].del, utf16(decode(piece)));
    }
    REQUIRE(t == utf16(now));
    g_spliced += p.size();
}

bool same_log(const OpLog& a, const OpLog& b) {
    if (a.size() != b.size() || a.max_lamport != b.max_lamport || a.visible() != b.visible()) return false;
    for (uint32_t k = 0; k < a.size(); ++k)
        if (a.parent[k] != b.parent[k] || a.lamport[k] != b.lamport[k] || a.agent[k] != b.agent[k] ||
            a.deleted[k] != b.deleted[k] || a.cp[k] != b.cp[k] || (a.fugue && a.side[k] != b.side[k]))
            return false;
    return true;
}

// A seeded ascending patch set in gaps of the model, stated in UTF-16 code units and in codepoints;
// both applied to copies of the log must leave the same log.  Then the malformed sets, the log
// unchanged.
void check_apply(const OpLog& log, const std::u32string& text) {
    const Gaps w(text);
    std::vector<PatchRec> p16, pcp;
    std::string ins;
    int64_t s16 = 0, scp = 0;
    for (uint64_t g = rnd(3); g <= w.len(); g += 1 + rnd(6)) {
        const uint64_t e = std::min<uint64_t>(w.len(), g + rnd(3));
        const std::u32string& word = kWords[rnd(8)];
        const bool typed = e == g || rnd(2);
        const std::string piece = typed ? encode(word) : std::string();
        const uint64_t n16 = typed ? utf16(word).size() : 0, ncp = typed ? word.size() : 0;
        p16.push_back(PatchRec{(uint64_t)((int64_t)w.u[g] + s16), ins.size(), (uint32_t)(w.u[e] - w.u[g]),
                               (uint32_t)piece.size()});
        pcp.push_back(PatchRec{(uint64_t)((int64_t)g + scp), ins.size(), (uint32_t)(e - g), (uint32_t)piece.size()});
        ins += piece;
        s16 += (int64_t)n16 - (int64_t)(w.u[e] - w.u[g]);
        scp += (int64_t)ncp - (int64_t)(e - g);
        g = e + 1;  // (never touching)
    }
    const size_t n = p16.size();
    PatchRec* heap = (PatchRec*)std::malloc(n ? n * sizeof(PatchRec) : 1);
    uint8_t* text8 = (uint8_t*)std::malloc(ins.size() ? ins.size() : 1);
    REQUIRE(heap && text8);
    if (n) std::memcpy(heap, p16.data(), n * sizeof(PatchRec));
    if (!ins.empty()) std::memcpy(text8, ins.data(), ins.size());
    OpLog a = log, b = log;
    std::string err;
    uint32_t add_a = 9, tomb_a = 9, add_b = 9, tomb_b = 9;
    REQUIRE(a.apply_patches_utf16(n ? heap : nullptr, n, ins.empty() ? nullptr : text8, ins.size(), &add_a,
                                  &tomb_a, err) == CRDT_HIP_OK);
    REQUIRE(b.apply_patches(pcp.data(), n, reinterpret_cast<const uint8_t*>(ins.data()), ins.size(), &add_b,
                            &tomb_b, err) == CRDT_HIP_OK);
    REQUIRE(add_a == add_b && tomb_a == tomb_b && same_log(a, b));
    std::free(heap);
    std::free(text8);
    g_sets += n;

    auto bad = [&](std::vector<PatchRec> q, const std::string& t, int code) {
        OpLog c = log;
        std::string e;
        REQUIRE(c.apply_patches_utf16(q.data(), q.size(), reinterpret_cast<const uint8_t*>(t.data()), t.size(),
                                      nullptr, nullptr, e) == code);
        REQUIRE(!e.empty() && same_log(c, log));
        ++g_refused;
    };
    const uint64_t n16 = w.u.back();
    bad({{0, 0, 0, 0}}, "", CRDT_HIP_EINVAL);                          // empty
    bad({{0, 0, 0, 2}}, "\xff\xfe", CRDT_HIP_EINVAL);                  // not UTF-8
    bad({{0, 1, 0, 2}}, "x", CRDT_HIP_EINVAL);                         // a piece outside ins
    bad({{n16, 0, 1, 0}}, "", CRDT_HIP_ERANGE);                        // beyond
    bad({{n16 + 1, 0, 0, 1}}, "x", CRDT_HIP_ERANGE);
    bad({{n16 + 1, 0, 0, 1}, {0, 0, 0, 0}}, "x", CRDT_HIP_ERANGE);     // array order: the range first
    bad({{0, 0, 0, 0}, {n16 + 9, 0, 0, 1}}, "x", CRDT_HIP_EINVAL);
    if (n16 >= 2) bad({{1, 0, 0, 1}, {1, 0, 0, 1}}, "x", CRDT_HIP_EINVAL);  // touching
    if (n16 >= 2) bad({{0, 0, 0, 4}, {2, 0, 0, 1}}, "\xF0\x9F\x98\x80", CRDT_HIP_EINVAL);  // ... in UTF-16
    for (uint64_t k = 0; k < w.len(); ++k)
        if (w.u[k + 1] - w.u[k] == 2) {
            bad({{w.u[k] + 1, 0, 0, 1}}, "x", CRDT_HIP_EINVAL);        // pos inside a pair
            bad({{w.u[k], 0, 1, 0}}, "", CRDT_HIP_EINVAL);             // the end of a delete inside one
            bad({{w.u[k] + 1, 0, 0, 1}, {n16 + 3, 0, 0, 1}}, "x", CRDT_HIP_ERANGE);  // the range error wins
            break;
        }
}

void take(OpLog& dst, const OpLog& src, bool delta) {
    std::string err;
    if (delta) {
        const std::vector<crdt::SvEntry> sv = dst.state_vector();
        std::vector<uint8_t> d;
        REQUIRE(src.encode_diff(sv.data(), sv.size(), d, err) == CRDT_HIP_OK);
        REQUIRE(dst.apply_diff(d.data(), d.size(), nullptr, nullptr, err) == CRDT_HIP_OK);
    } else {
        REQUIRE(dst.join(src.size(), src.parent.data(), src.oright.data(), src.lamport.data(),
                         src.agent.data(), src.deleted.data(), src.cp.data(),
                         src.fugue ? src.side.data() : nullptr, nullptr, nullptr, err) == CRDT_HIP_OK);
    }
}

void run(bool fugue, uint32_t rounds) {
    for (uint32_t round = 0; round < rounds; ++round) {
        OpLog log;
        log.fugue = fugue;
        std::u32string model;
        check_version(log, nullptr, model);  // the empty log
        check_apply(log, model);
        edits(log, model, 10 + rnd(40));
        // two forks that the log takes in later: their edits are concurrent to the log's own
        OpLog fa = log, fb = log;
        std::u32string ma = model, mb = model;
        fa.local_agent = 1;
        fb.local_agent = 2;
        edits(fa, ma, 5 + rnd(20));
        edits(fb, mb, 5 + rnd(20));
        std::vector<LogMark> marks;
        std::vector<std::u32string> recs;
        const uint32_t steps = 6 + rnd(6), at_join = rnd(steps), at_delta = rnd(steps);
        for (uint32_t step = 0; step < steps; ++step) {
            if (step == at_join || step == at_delta) {
                take(log, step == at_join ? fa : fb, step != at_join);
                model = text_now(log);  // the model after a sync is the log's own text
                REQUIRE(model.size() == log.visible());
            } else if (rnd(3) == 0) {  // an update: edits made on a copy, shipped as one wire update
                OpLog src = log;
                const uint64_t v = src.version();
                edits(src, model, 1 + rnd(5));
                const std::vector<uint8_t> u = src.encode_from(v);
                REQUIRE(log.apply_update(u.data(), u.size()).empty());
            } else {
                edits(log, model, 1 + rnd(5));
            }
            marks.push_back(log.mark());
            recs.push_back(model);
            check_version(log, nullptr, model);
            malformed(log, nullptr, model);
            check_apply(log, model);
            for (size_t k = 0; k < marks.size(); ++k) {
                check_version(log, &marks[k], recs[k]);
                check_since(log, marks[k], recs[k], model);
            }
            const uint32_t any = rnd((uint32_t)marks.size());
            malformed(log, &marks[any], recs[any]);
        }
        // a mark of a longer log is refused
        OpLog longer = log;
        edits(longer, model, 3);
        if (longer.size() > log.size()) {
            const LogMark m = longer.mark();
            for (uint32_t unit : {kUnitCodepoints, kUnitBytes, kUnitUtf16}) refused(log, &m, {0}, unit, CRDT_HIP_EINVAL);
            std::vector<PatchRec> p;
            std::vector<uint8_t> ins;
            std::string err;
            REQUIRE(log.patches_since_utf16(m, p, ins, err) == CRDT_HIP_EINVAL);
        }
    }
    std::printf("%s: %u rounds, %zu positions answered, %zu calls refused, %zu patches applied, %zu spliced so far\n",
                fugue ? "fugue" : "rga", rounds, g_queries, g_refused, g_sets, g_spliced);
}

}  // namespace

int main() {
    run(false, 40);
    run(true, 40);
    REQUIRE(g_queries > 100000 && g_refused > 5000 && g_sets > 1000 && g_spliced > 1000);
    std::puts("utf16_asan ok");
    return 0;
}
