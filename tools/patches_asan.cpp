// patches_asan.cpp — stand-alone host program for a sanitizer run of patches since a mark in
// oplog.cpp (OpLog::mark / patches_since / document_order): CPU only, no device code, no Python.
// tools/asan_patches.sh builds it with AddressSanitizer + UBSan and runs it.
//
// Two forks of a typed base (RGA, then Fugue) each keep a plain std::u32string model of their own
// document, applying the same positional edits to model and log.  Each fork takes a mark and
// takes the other in (a join on even pairs, the other's delta on odd ones), then applies its own
// patches_since to its own model.  The two models must then be equal (convergence) and as long as
// the logs' visible length (what crdt_hip_oplog_visible_len returns).  A few hundred seeded pairs;
// the patches and their text are read from heap blocks of exactly the reported size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crdt_hip.h"
#include "oplog.hpp"

using crdt::LogMark;
using crdt::OpLog;
using crdt::PatchRec;

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

// The same positional edits to the log and to the model.
void edits(OpLog& log, std::u32string& model, uint32_t k) {
    static const std::u32string words[] = {U"a", U"bc", U"é", U"€", U"\U0001F600", U"xyz "};
    for (uint32_t i = 0; i < k; ++i) {
        const uint64_t n = log.visible();
        REQUIRE(n == model.size());
        if (n < 4 || rnd(100) < 60) {
            const std::u32string& w = words[rnd(6)];
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

std::u32string decode(const uint8_t* s, size_t len) {
    std::u32string out;
    for (size_t i = 0; i < len;) {
        const uint8_t b = s[i];
        const size_t k = b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
        REQUIRE(i + k <= len);
        char32_t c = k == 1 ? b : b & (0xFFu >> (k + 1));
        for (size_t j = 1; j < k; ++j) c = (c << 6) | (s[i + j] & 0x3Fu);
        out.push_back(c);
        i += k;
    }
    return out;
}

// log.patches_since(m) applied to the model as replace(pos..pos + del, ins), patch after patch.
size_t apply_patches(const OpLog& log, const LogMark& m, std::u32string& model) {
    std::vector<PatchRec> p;
    std::vector<uint8_t> text;
    std::string err;
    REQUIRE(log.patches_since(m, p, text, err) == CRDT_HIP_OK);
    // blocks of exactly the reported size, so that a read past either is seen
    PatchRec* hp = (PatchRec*)std::malloc(p.size() ? p.size() * sizeof(PatchRec) : 1);
    uint8_t* ht = (uint8_t*)std::malloc(text.size() ? text.size() : 1);
    REQUIRE(hp && ht);
    if (!p.empty()) std::memcpy(hp, p.data(), p.size() * sizeof(PatchRec));
    if (!text.empty()) std::memcpy(ht, text.data(), text.size());
    uint64_t off = 0, last_end = 0;
    for (size_t k = 0; k < p.size(); ++k) {
        const PatchRec& r = hp[k];
        REQUIRE(r.ins_off == off && r.ins_off + r.ins_len <= text.size());
        REQUIRE(r.del || r.ins_len);
        REQUIRE(k == 0 || r.pos > last_end);  // two patches never touch
        REQUIRE(r.pos + r.del <= model.size());
        const std::u32string ins = decode(ht + r.ins_off, r.ins_len);
        model.replace(r.pos, r.del, ins);
        off += r.ins_len;
        last_end = r.pos + ins.size();
    }
    REQUIRE(off == text.size());
    std::free(hp);
    std::free(ht);
    return p.size();
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

void run(bool fugue, uint32_t pairs) {
    size_t total = 0;
    for (uint32_t pair = 0; pair < pairs; ++pair) {
        OpLog base;
        base.fugue = fugue;
        std::u32string mbase;
        edits(base, mbase, 10 + rnd(60));
        OpLog a = base, b = base;
        std::u32string ma = mbase, mb = mbase;
        a.local_agent = 1;
        b.local_agent = 2;
        edits(a, ma, rnd(40));
        edits(b, mb, rnd(40));
        const LogMark xa = a.mark(), xb = b.mark();
        const bool delta = pair & 1;
        const OpLog b0 = b;
        take(a, b0, delta);
        take(b, a, delta);
        std::u32string mid = ma;
        total += apply_patches(a, xa, ma);
        total += apply_patches(b, xb, mb);
        REQUIRE(ma == mb);
        REQUIRE(ma.size() == a.visible() && mb.size() == b.visible());
        // nothing changed since a fresh mark; local edits after the sync keep the model in step,
        // and the old mark still takes the old text to the new one
        const LogMark now = a.mark();
        std::u32string same = ma;
        REQUIRE(apply_patches(a, now, same) == 0 && same == ma);
        edits(a, ma, rnd(10));
        apply_patches(a, xa, mid);
        REQUIRE(mid == ma);
        // a mark of a longer log is refused
        std::vector<PatchRec> p;
        std::vector<uint8_t> text;
        std::string err;
        if (a.size() > base.size())
            REQUIRE(base.patches_since(a.mark(), p, text, err) == CRDT_HIP_EINVAL && !err.empty());
    }
    std::printf("%s: %u pairs, %zu patches applied\n", fugue ? "fugue" : "rga", pairs, total);
    REQUIRE(total > pairs);
}

}  // namespace

int main() {
    run(false, 300);
    run(true, 300);
    std::puts("patches_asan ok");
    return 0;
}
