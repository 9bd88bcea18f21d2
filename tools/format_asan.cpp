// format_asan.cpp — stand-alone host program for a sanitizer run of formats in oplog.cpp
// (OpLog::spans, format_check): CPU only, no device code, no Python.
// tools/asan_format.sh builds it with AddressSanitizer + UBSan and runs it.
//
// Two forks of a typed base (RGA, then Fugue) edit under their own agents, each beside a model of
// its text that keeps, per character, the winner per key among the formats made while the
// character was there (ops only grow, so such a winner beats every earlier format) and the keys of
// the formats made before it was typed (whether one of those covers it depends on where among the
// tombstones it landed, which the model does not know: those keys are not compared for it).  A
// format made over [s, e) of a fork's text covers exactly the characters there, whatever its biases.
// Spans are checked against the model (positions and byte lengths exactly, attributes where the
// model is sure, touching spans must differ) after edits and after a join one way and a delta the
// other, the model brought over by the patches since a mark; both forks must then paint the union of
// the formats, passed in opposite array orders, byte for byte alike.  Formats and results live in
// heap blocks of exactly the size passed, and every malformed call must be refused with its code
// and leave the outputs and the pending count untouched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "crdt_hip.h"
#include "oplog.hpp"
#include "util.hpp"

using crdt::AnchorRec;
using crdt::FormatRec;
using crdt::OpLog;
using crdt::SpanAttrRec;
using crdt::SpanRec;

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

const std::u32string kWords[] = {U"a", U"bc", U"é", U"€", U"\U0001F600", U"xyz ", U"hello wörld"};
size_t g_calls = 0, g_spans = 0, g_attrs = 0, g_refused = 0, g_pending = 0;

template <class T>
T* heap(const std::vector<T>& v) {  // a block of exactly v.size() elements (one byte when empty)
    T* p = (T*)std::malloc(v.empty() ? 1 : v.size() * sizeof(T));
    REQUIRE(p);
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// OpLog::spans through heap blocks of exactly the sizes passed, with the copy-out the C ABI does; a
// refused call writes nothing to sp, at and pending.
int spans(const OpLog& log, const std::vector<FormatRec>& f, std::vector<SpanRec>& sp,
          std::vector<SpanAttrRec>& at, uint64_t& pending) {
    FormatRec* hf = heap(f);
    std::vector<SpanRec> rs;
    std::vector<SpanAttrRec> ra;
    uint64_t pend = 0;
    std::string err;
    const int rc = log.spans(hf, f.size(), rs, ra, pend, err);
    std::free(hf);
    REQUIRE((rc == CRDT_HIP_OK) == err.empty());
    ++g_calls;
    if (rc) {
        ++g_refused;
        REQUIRE(rs.empty() && ra.empty() && pend == 0);
        return rc;
    }
    SpanRec* ho = heap(rs);  // the copy-out of the ABI, into blocks of exactly the need
    SpanAttrRec* ha = heap(ra);
    sp.assign(ho, ho + rs.size());
    at.assign(ha, ha + ra.size());
    std::free(ho);
    std::free(ha);
    pending = pend;
    g_spans += sp.size();
    g_attrs += at.size();
    g_pending += pend;
    return rc;
}

struct Attr {
    uint64_t op, value;
    bool removed;
};
using AttrSet = std::map<uint32_t, Attr>;  // key -> the winner among the formats the model knows
constexpr uint32_t kKeys = 3;
struct Ch {
    char32_t c;
    AttrSet attrs;    // from the formats made while the character was there
    uint32_t unsure;  // keys (bits) of formats made before it was typed: whether such a format
                      // covers it depends on where among the tombstones it landed
};
struct Model {
    std::vector<Ch> text;
    uint32_t keys_made = 0;
};

uint32_t u8len(char32_t c) {
    char b[4];
    return (uint32_t)crdt::utf8_put((uint32_t)c, b);
}

void edit(OpLog& log, Model& m, uint32_t edits) {
    for (uint32_t k = 0; k < edits; ++k) {
        const uint64_t n = m.text.size();
        if (n == 0 || rnd(10) < 6) {
            const std::u32string& w = kWords[rnd(7)];
            const uint64_t p = rnd((uint32_t)n + 1);
            REQUIRE(log.insert(p, reinterpret_cast<const uint32_t*>(w.data()), w.size()).empty());
            for (size_t j = 0; j < w.size(); ++j)
                m.text.insert(m.text.begin() + (long)(p + j), Ch{w[j], AttrSet{}, m.keys_made});
        } else {
            const uint64_t p = rnd((uint32_t)n), e = std::min<uint64_t>(n, p + 1 + rnd(4));
            REQUIRE(log.remove(p, e).empty());
            m.text.erase(m.text.begin() + (long)p, m.text.begin() + (long)e);
        }
    }
    REQUIRE(log.visible() == m.text.size());
}

// A format over [s, e) of the fork's text, with random biases, applied to the model: it covers
// exactly those of the characters there now, whatever the biases, and ops only grow.
FormatRec make_format(const OpLog& log, Model& m, uint64_t op) {
    const uint64_t n = m.text.size();
    uint64_t s = rnd((uint32_t)n + 1), e = rnd((uint32_t)n + 1);
    if (s > e) std::swap(s, e);
    const uint64_t pos[2] = {s, e};
    const uint8_t bias[2] = {(uint8_t)rnd(2), (uint8_t)rnd(2)};
    AnchorRec a[2];
    std::string err;
    REQUIRE(log.anchors_at(pos, bias, 2, false, a, err) == CRDT_HIP_OK);
    FormatRec f{a[0], a[1], op, 1 + rnd(3), rnd(kKeys), rnd(4) == 0 ? crdt::kFormatRemove : 0u};
    for (uint64_t k = s; k < e; ++k) m.text[k].attrs[f.key] = Attr{op, f.value, f.flags != 0};
    m.keys_made |= 1u << f.key;
    return f;
}

// The spans of `log` under `f` against the model.  Positions and byte lengths are exact; a
// character's attribute of key K is compared where the model is sure of it: a format made while it
// was there covers it (a later op than any made before), or none of key K was made before it.
// Neighbouring spans that touch must differ (the runs are maximal).
void check(const OpLog& log, const Model& m, const std::vector<FormatRec>& f) {
    std::vector<SpanRec> sp;
    std::vector<SpanAttrRec> at;
    uint64_t pending = 99;
    REQUIRE(spans(log, f, sp, at, pending) == CRDT_HIP_OK && pending == 0);
    const uint64_t n = m.text.size();
    std::vector<uint64_t> ends{0};
    for (const Ch& ch : m.text) ends.push_back(ends.back() + u8len(ch.c));
    std::vector<std::map<uint32_t, uint64_t>> got(n);
    uint64_t end = 0, off = 0;
    for (size_t k = 0; k < sp.size(); ++k) {
        const SpanRec& s = sp[k];
        REQUIRE(s.len >= 1 && s.attr_n >= 1 && s.pos >= end && s.pos + s.len <= n && s.attr_off == off);
        REQUIRE(s.pos_bytes == ends[s.pos] && s.len_bytes == ends[s.pos + s.len] - ends[s.pos]);
        REQUIRE(off + s.attr_n <= at.size());
        for (uint32_t q = 0; q < s.attr_n; ++q) {
            REQUIRE(!at[off + q].pad && (q == 0 || at[off + q - 1].key < at[off + q].key));
            for (uint64_t i = s.pos; i < s.pos + s.len; ++i) got[i][at[off + q].key] = at[off + q].value;
        }
        if (k && s.pos == end) {  // touching spans differ
            const SpanRec& p = sp[k - 1];
            REQUIRE(p.attr_n != s.attr_n ||
                    std::memcmp(&at[p.attr_off], &at[s.attr_off], s.attr_n * sizeof(SpanAttrRec)));
        }
        end = s.pos + s.len;
        off += s.attr_n;
    }
    REQUIRE(off == at.size());
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t key = 0; key < kKeys; ++key) {
            const auto it = m.text[i].attrs.find(key);
            if (it == m.text[i].attrs.end() && (m.text[i].unsure >> key & 1u)) continue;
            const bool has = it != m.text[i].attrs.end() && !it->second.removed;
            REQUIRE(has == (got[i].count(key) != 0));
            if (has) REQUIRE(got[i][key] == it->second.value);
        }
}

void malformed(const OpLog& log, const FormatRec good) {
    std::vector<SpanRec> sp{SpanRec{7, 7, 7, 7, 7, 7}};
    std::vector<SpanAttrRec> at{SpanAttrRec{9, 9, 9}};
    uint64_t pending = 99;
    auto refused = [&](std::vector<FormatRec> f, int code) {
        REQUIRE(spans(log, f, sp, at, pending) == code);
        REQUIRE(sp.size() == 1 && sp[0].pos == 7 && at.size() == 1 && at[0].key == 9 && pending == 99);
    };
    FormatRec b = good;
    b.op = good.op + 1;
    b.start.id = 1ull << 48;
    refused({good, b}, CRDT_HIP_EINVAL);
    b = good, b.op = good.op + 1, b.end.bias = 2;
    refused({good, b}, CRDT_HIP_EINVAL);
    b = good, b.op = good.op + 1, b.end.pad = 1;
    refused({b, good}, CRDT_HIP_EINVAL);
    b = good, b.op = 1ull << 48;
    refused({good, b}, CRDT_HIP_EINVAL);
    b = good, b.op = good.op + 1, b.flags = 2;
    refused({good, b}, CRDT_HIP_EINVAL);
    b = good, b.key = good.key + 1;  // the same op
    refused({good, b}, CRDT_HIP_EINVAL);
    std::vector<FormatRec> many(crdt::kFormatMax + 1, good);
    for (size_t k = 0; k < many.size(); ++k) many[k].op = k;
    refused(many, CRDT_HIP_ERANGE);
    // an identity nobody holds is pending, not an error; no format at all is fine
    b = good, b.op = good.op + 1, b.start.id = (1ull << 48) - 1;
    REQUIRE(spans(log, {good, b}, sp, at, pending) == CRDT_HIP_OK && pending == 1);
    REQUIRE(spans(log, {}, sp, at, pending) == CRDT_HIP_OK && sp.empty() && at.empty() && pending == 0);
}

// The model after a sync: the patches since the mark applied to it; a character that came from the
// peer is unsure of every key.
void synced(const OpLog& log, const crdt::LogMark& mk, Model& m) {
    std::vector<crdt::PatchRec> back;
    std::vector<uint8_t> text;
    std::string err;
    REQUIRE(log.patches_since(mk, back, text, err) == CRDT_HIP_OK);
    for (const crdt::PatchRec& r : back) {
        std::vector<uint32_t> cps;
        REQUIRE(crdt::utf8_decode(reinterpret_cast<const char*>(text.data()) + r.ins_off, r.ins_len, cps));
        m.text.erase(m.text.begin() + (long)r.pos, m.text.begin() + (long)(r.pos + r.del));
        for (size_t j = 0; j < cps.size(); ++j)
            m.text.insert(m.text.begin() + (long)(r.pos + j), Ch{(char32_t)cps[j], AttrSet{}, (1u << kKeys) - 1});
    }
    REQUIRE(log.visible() == m.text.size());
}

void run(bool fugue, uint32_t rounds) {
    for (uint32_t round = 0; round < rounds; ++round) {
        OpLog base;
        base.fugue = fugue;
        {  // the empty log: no span, and an item identity is pending
            std::vector<SpanRec> sp;
            std::vector<SpanAttrRec> at;
            uint64_t pending = 0;
            const FormatRec whole{AnchorRec{crdt::kAnchorEdge, 0, 0}, AnchorRec{crdt::kAnchorEdge, 1, 0}, 1, 1, 1, 0};
            FormatRec on = whole;
            on.op = 2;
            on.end.id = 5 << 16;
            REQUIRE(spans(base, {whole, on}, sp, at, pending) == CRDT_HIP_OK && sp.empty() && pending == 1);
        }
        Model mbase;
        const std::u32string& w = kWords[6];
        REQUIRE(base.insert(0, reinterpret_cast<const uint32_t*>(w.data()), w.size()).empty());
        for (char32_t c : w) mbase.text.push_back(Ch{c, AttrSet{}, 0u});
        edit(base, mbase, 4 + rnd(8));
        OpLog a = base, b = base;
        a.local_agent = 1;
        b.local_agent = 2;
        Model ma = mbase, mb = mbase;
        std::vector<FormatRec> fa, fb;
        uint64_t clock = 1;
        for (uint32_t step = 0; step < 4 + rnd(6); ++step) {  // formats and edits, interleaved
            fa.push_back(make_format(a, ma, (clock << 16) | 1u));
            fb.push_back(make_format(b, mb, (clock++ << 16) | 2u));
            edit(a, ma, 1 + rnd(8));
            edit(b, mb, 1 + rnd(8));
            check(a, ma, fa);
            check(b, mb, fb);
        }
        malformed(a, fa[0]);
        // a takes b by a join, b takes a by a delta; both then paint the union alike
        std::string err;
        const OpLog b0 = b;
        const crdt::LogMark mka = a.mark(), mkb = b.mark();
        REQUIRE(a.join(b0.size(), b0.parent.data(), b0.oright.data(), b0.lamport.data(), b0.agent.data(),
                       b0.deleted.data(), b0.cp.data(), fugue ? b0.side.data() : nullptr, nullptr,
                       nullptr, err) == CRDT_HIP_OK);
        std::vector<uint8_t> delta;
        const std::vector<crdt::SvEntry> sv = b.state_vector();
        REQUIRE(a.encode_diff(sv.data(), sv.size(), delta, err) == CRDT_HIP_OK);
        REQUIRE(b.apply_diff(delta.data(), delta.size(), nullptr, nullptr, err) == CRDT_HIP_OK);
        std::vector<FormatRec> all = fa, rev;
        all.insert(all.end(), fb.begin(), fb.end());
        rev.assign(all.rbegin(), all.rend());
        std::vector<SpanRec> sa, sb;
        std::vector<SpanAttrRec> aa, ab;
        uint64_t pa = 9, pb = 9;
        REQUIRE(spans(a, all, sa, aa, pa) == CRDT_HIP_OK && spans(b, rev, sb, ab, pb) == CRDT_HIP_OK);
        REQUIRE(pa == 0 && pb == 0 && sa.size() == sb.size() && aa.size() == ab.size());
        REQUIRE(sa.empty() || !std::memcmp(sa.data(), sb.data(), sa.size() * sizeof(SpanRec)));
        REQUIRE(aa.empty() || !std::memcmp(aa.data(), ab.data(), aa.size() * sizeof(SpanAttrRec)));
        uint64_t end = 0;
        for (const SpanRec& s : sa) {  // ascending, never overlapping, inside the text
            REQUIRE(s.pos >= end && s.len >= 1 && s.attr_n >= 1);
            end = s.pos + s.len;
        }
        REQUIRE(end <= a.visible() && a.visible() == b.visible());
        // each fork's own formats against its model, brought over the sync by the patches since
        synced(a, mka, ma);
        synced(b, mkb, mb);
        check(a, ma, fa);
        check(b, mb, fb);
    }
    std::printf("%s: %u rounds, %zu calls, %zu spans, %zu attrs, %zu pending, %zu calls refused\n",
                fugue ? "fugue" : "rga", rounds, g_calls, g_spans, g_attrs, g_pending, g_refused);
}

}  // namespace

int main() {
    run(false, 60);
    run(true, 60);
    REQUIRE(g_calls > 1000 && g_spans > 1000 && g_refused > 100);
    std::puts("format_asan ok");
    return 0;
}
