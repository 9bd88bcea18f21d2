// anchor_asan.cpp — stand-alone host program for a sanitizer run of anchors in oplog.cpp
// (OpLog::anchors_at / anchors_resolve): CPU only, no device code, no Python.
// tools/asan_anchor.sh builds it with AddressSanitizer + UBSan and runs it.
//
// Two forks of a typed base (RGA, then Fugue) edit under their own agents, each beside a plain
// std::u32string model of its text.  Every round checks the round trip (every gap, both biases, in
// codepoints and at every UTF-8 boundary; every byte offset inside a codepoint refused), the
// stickiness (an insert at the anchored gap, a delete of the anchored item), and the convergence:
// anchors made on both forks resolve alike once one fork took the other by a join and the other the
// first by a delta, and an anchor on the peer's own item is UNKNOWN before that.  Positions, biases,
// anchors and results live in heap blocks of exactly the size passed, and every malformed argument
// must be refused with its code and leave `out` untouched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crdt_hip.h"
#include "oplog.hpp"
#include "util.hpp"

using crdt::AnchorPosRec;
using crdt::AnchorRec;
using crdt::OpLog;

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
size_t g_made = 0, g_resolved = 0, g_refused = 0;

template <class T>
T* heap(const std::vector<T>& v) {  // a block of exactly v.size() elements (one byte when empty)
    T* p = (T*)std::malloc(v.empty() ? 1 : v.size() * sizeof(T));
    REQUIRE(p);
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// anchors_at through heap blocks; `out` starts as `fill` and is returned whatever the code.
int at(const OpLog& log, const std::vector<uint64_t>& pos, const std::vector<uint8_t>& bias, bool bytes,
       std::vector<AnchorRec>& out, const AnchorRec fill = AnchorRec{7, 1, 9}) {
    out.assign(pos.size(), fill);
    uint64_t* hp = heap(pos);
    uint8_t* hb = bias.empty() ? nullptr : heap(bias);
    AnchorRec* ho = heap(out);
    std::string err;
    const int rc = log.anchors_at(hp, hb, pos.size(), bytes, ho, err);
    REQUIRE((rc == CRDT_HIP_OK) == err.empty());
    if (!out.empty()) std::memcpy(out.data(), ho, out.size() * sizeof(AnchorRec));
    std::free(hp);
    std::free(hb);
    std::free(ho);
    if (rc) {
        ++g_refused;
        for (const AnchorRec& a : out) REQUIRE(!std::memcmp(&a, &fill, sizeof a));
    } else {
        g_made += pos.size();
    }
    return rc;
}

int resolve(const OpLog& log, const std::vector<AnchorRec>& a, std::vector<AnchorPosRec>& out) {
    const AnchorPosRec fill{11, 12, 13, 14};
    out.assign(a.size(), fill);
    AnchorRec* ha = heap(a);
    AnchorPosRec* ho = heap(out);
    std::string err;
    const int rc = log.anchors_resolve(ha, a.size(), ho, err);
    REQUIRE((rc == CRDT_HIP_OK) == err.empty());
    if (!out.empty()) std::memcpy(out.data(), ho, out.size() * sizeof(AnchorPosRec));
    std::free(ha);
    std::free(ho);
    if (rc) {
        ++g_refused;
        for (const AnchorPosRec& p : out) REQUIRE(!std::memcmp(&p, &fill, sizeof p));
    } else {
        g_resolved += a.size();
    }
    return rc;
}

std::vector<uint64_t> byte_ends(const std::u32string& text) {  // ends[v]: bytes of the first v
    std::vector<uint64_t> ends{0};
    for (char32_t c : text) {
        char b[4];
        ends.push_back(ends.back() + crdt::utf8_put((uint32_t)c, b));
    }
    return ends;
}

void edit(OpLog& log, std::u32string& model, uint32_t edits) {
    for (uint32_t k = 0; k < edits; ++k) {
        const uint64_t n = model.size();
        if (n == 0 || rnd(10) < 6) {
            const std::u32string& w = kWords[rnd(7)];
            const uint64_t p = rnd((uint32_t)n + 1);
            REQUIRE(log.insert(p, reinterpret_cast<const uint32_t*>(w.data()), w.size()).empty());
            model.insert(p, w);
        } else {
            const uint64_t p = rnd((uint32_t)n), e = std::min<uint64_t>(n, p + 1 + rnd(4));
            REQUIRE(log.remove(p, e).empty());
            model.erase(p, e - p);
        }
    }
    REQUIRE(log.visible() == model.size());
}

// Every gap under both biases, in codepoints and in bytes; every offset inside a codepoint.
void round_trip(const OpLog& log, const std::u32string& model) {
    const uint64_t len = model.size();
    const std::vector<uint64_t> ends = byte_ends(model);
    std::vector<uint64_t> pos, bpos;
    std::vector<uint8_t> bias;
    for (uint32_t b = 0; b < 2; ++b)
        for (uint64_t p = 0; p <= len; ++p) {
            pos.push_back(p);
            bpos.push_back(ends[p]);
            bias.push_back((uint8_t)b);
        }
    std::vector<AnchorRec> a, ab;
    std::vector<AnchorPosRec> r;
    REQUIRE(at(log, pos, bias, false, a) == CRDT_HIP_OK);
    REQUIRE(at(log, bpos, bias, true, ab) == CRDT_HIP_OK);
    REQUIRE(!std::memcmp(a.data(), ab.data(), a.size() * sizeof(AnchorRec)));
    REQUIRE(resolve(log, a, r) == CRDT_HIP_OK);
    for (size_t k = 0; k < pos.size(); ++k) {
        REQUIRE(r[k].pos == pos[k] && r[k].pos_bytes == bpos[k] && r[k].state == crdt::kAnchorLive && !r[k].pad);
        REQUIRE(a[k].bias == bias[k] && !a[k].pad);
        REQUIRE((a[k].id == crdt::kAnchorEdge) == (bias[k] ? pos[k] == len : pos[k] == 0));
    }
    for (uint64_t v = 0; v < len; ++v)
        for (uint64_t off = ends[v] + 1; off < ends[v + 1]; ++off)
            REQUIRE(at(log, {0, off}, {(uint8_t)rnd(2), (uint8_t)rnd(2)}, true, a) == CRDT_HIP_EINVAL);
    // all AFTER through a null bias
    REQUIRE(at(log, {0, len, len / 2}, {}, false, a) == CRDT_HIP_OK);
    REQUIRE(a[0].id == crdt::kAnchorEdge && a[0].bias == crdt::kAnchorAfter && a[2].bias == crdt::kAnchorAfter);
}

void stickiness(OpLog log, std::u32string model) {  // (on copies)
    const uint64_t len = model.size();
    REQUIRE(len >= 4);
    const uint64_t p = rnd((uint32_t)len + 1);
    std::vector<AnchorRec> a;
    std::vector<AnchorPosRec> r;
    REQUIRE(at(log, {p, p}, {0, 1}, false, a) == CRDT_HIP_OK);
    const std::u32string& w = kWords[rnd(7)];
    REQUIRE(log.insert(p, reinterpret_cast<const uint32_t*>(w.data()), w.size()).empty());
    REQUIRE(resolve(log, a, r) == CRDT_HIP_OK);
    REQUIRE(r[0].pos == p && r[1].pos == p + w.size() && r[0].state == 0 && r[1].state == 0);
    // delete the q-th visible item: both anchors on it are DEAD where it was
    const uint64_t q = 1 + rnd((uint32_t)log.visible());
    REQUIRE(at(log, {q, q - 1}, {0, 1}, false, a) == CRDT_HIP_OK);
    REQUIRE(a[0].id == a[1].id && a[0].id != crdt::kAnchorEdge);
    REQUIRE(log.remove(q - 1, q).empty());
    REQUIRE(resolve(log, a, r) == CRDT_HIP_OK);
    REQUIRE(r[0].pos == q - 1 && r[1].pos == q - 1 && r[0].pos_bytes == r[1].pos_bytes);
    REQUIRE(r[0].state == crdt::kAnchorDead && r[1].state == crdt::kAnchorDead);
}

void malformed(const OpLog& log) {
    const uint64_t len = log.visible(), nb = log.visible_bytes();
    std::vector<AnchorRec> a;
    std::vector<AnchorPosRec> r;
    REQUIRE(at(log, {0, len + 1}, {0, 0}, false, a) == CRDT_HIP_ERANGE);
    REQUIRE(at(log, {0, nb + 1}, {1, 1}, true, a) == CRDT_HIP_ERANGE);
    REQUIRE(at(log, {0, len}, {0, 2}, false, a) == CRDT_HIP_EINVAL);
    REQUIRE(at(log, {len + 1, len}, {0, 2}, false, a) == CRDT_HIP_ERANGE);  // array order
    REQUIRE(at(log, {~0ull}, {}, false, a) == CRDT_HIP_ERANGE);
    REQUIRE(at(log, {}, {}, false, a) == CRDT_HIP_OK && at(log, {}, {}, true, a) == CRDT_HIP_OK);
    REQUIRE(at(log, {len}, {1}, false, a) == CRDT_HIP_OK);
    const AnchorRec good = a[0];
    REQUIRE(resolve(log, {good, AnchorRec{1ull << 48, 0, 0}}, r) == CRDT_HIP_EINVAL);
    REQUIRE(resolve(log, {good, AnchorRec{crdt::kAnchorEdge - 1, 0, 0}}, r) == CRDT_HIP_EINVAL);
    REQUIRE(resolve(log, {AnchorRec{5, 2, 0}, good}, r) == CRDT_HIP_EINVAL);
    REQUIRE(resolve(log, {good, AnchorRec{5, 1, 1}}, r) == CRDT_HIP_EINVAL);
    REQUIRE(resolve(log, {}, r) == CRDT_HIP_OK);
    REQUIRE(resolve(log, {good, AnchorRec{(1ull << 48) - 1, 0, 0}}, r) == CRDT_HIP_OK);
    REQUIRE(r[0].pos == len && r[0].pos_bytes == nb && r[1].state == crdt::kAnchorUnknown && !r[1].pos);
}

std::u32string text_of(const OpLog& log, const crdt::LogMark& m, std::u32string model) {
    std::vector<crdt::PatchRec> back;
    std::vector<uint8_t> text;
    std::string err;
    REQUIRE(log.patches_since(m, back, text, err) == CRDT_HIP_OK);
    for (const crdt::PatchRec& r : back) {
        std::vector<uint32_t> cps;
        REQUIRE(crdt::utf8_decode(reinterpret_cast<const char*>(text.data()) + r.ins_off, r.ins_len, cps));
        model.replace(r.pos, r.del, std::u32string(cps.begin(), cps.end()));
    }
    return model;
}

void run(bool fugue, uint32_t rounds) {
    for (uint32_t round = 0; round < rounds; ++round) {
        OpLog base;
        base.fugue = fugue;
        std::u32string mbase;
        {  // the empty log: both edges, nothing else
            std::vector<AnchorRec> a;
            std::vector<AnchorPosRec> r;
            REQUIRE(at(base, {0, 0}, {0, 1}, round & 1, a) == CRDT_HIP_OK);
            REQUIRE(a[0].id == crdt::kAnchorEdge && a[1].id == crdt::kAnchorEdge);
            REQUIRE(resolve(base, a, r) == CRDT_HIP_OK && !r[0].pos && !r[1].pos && !r[1].pos_bytes);
            REQUIRE(at(base, {1}, {}, false, a) == CRDT_HIP_ERANGE);
        }
        edit(base, mbase, 6 + rnd(10));
        OpLog a = base, b = base;
        a.local_agent = 1;
        b.local_agent = 2;
        std::u32string ma = mbase, mb = mbase;
        edit(a, ma, 1 + rnd(25));
        edit(b, mb, 1 + rnd(25));
        {  // both type at the same gap of the common text
            const uint64_t p = rnd((uint32_t)std::min(ma.size(), mb.size()) + 1);
            REQUIRE(a.insert(p, reinterpret_cast<const uint32_t*>(kWords[2].data()), 1).empty());
            REQUIRE(b.insert(p, reinterpret_cast<const uint32_t*>(kWords[3].data()), 1).empty());
            ma.insert(p, kWords[2]);
            mb.insert(p, kWords[3]);
        }
        round_trip(a, ma);
        round_trip(b, mb);
        if (ma.size() >= 4) stickiness(a, ma);
        malformed(a);
        // anchors of both forks, and one on each fork's last own item
        std::vector<AnchorRec> made, part;
        std::vector<uint64_t> pos;
        std::vector<uint8_t> bias;
        for (uint32_t k = 0; k < 12; ++k) {
            pos.push_back(rnd((uint32_t)ma.size() + 1));
            bias.push_back((uint8_t)rnd(2));
        }
        REQUIRE(at(a, pos, bias, false, made) == CRDT_HIP_OK);
        for (uint64_t& p : pos) p = rnd((uint32_t)mb.size() + 1);
        REQUIRE(at(b, pos, bias, false, part) == CRDT_HIP_OK);
        made.insert(made.end(), part.begin(), part.end());
        const AnchorRec own_b{((uint64_t)b.lamport.back() << 16) | 2u, 0, 0};
        REQUIRE(b.agent.back() == 2);
        std::vector<AnchorPosRec> ra, rb;
        REQUIRE(resolve(a, {own_b}, ra) == CRDT_HIP_OK && ra[0].state == crdt::kAnchorUnknown);
        made.push_back(own_b);
        // a takes b by a join, b takes a by a delta
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
        ma = text_of(a, mka, ma);
        mb = text_of(b, mkb, mb);
        REQUIRE(ma == mb && a.size() == b.size());
        REQUIRE(resolve(a, made, ra) == CRDT_HIP_OK && resolve(b, made, rb) == CRDT_HIP_OK);
        REQUIRE(!std::memcmp(ra.data(), rb.data(), ra.size() * sizeof(AnchorPosRec)));
        for (const AnchorPosRec& p : ra) REQUIRE(p.state != crdt::kAnchorUnknown && p.pos <= ma.size());
        round_trip(a, ma);  // (the order now comes from a joined log)
        round_trip(b, mb);
    }
    std::printf("%s: %u rounds, %zu anchors made, %zu resolved, %zu calls refused\n",
                fugue ? "fugue" : "rga", rounds, g_made, g_resolved, g_refused);
}

}  // namespace

int main() {
    run(false, 60);
    run(true, 60);
    REQUIRE(g_made > 1000 && g_resolved > 1000 && g_refused > 100);
    std::puts("anchor_asan ok");
    return 0;
}
