// edit_asan.cpp — stand-alone host program for a sanitizer run of local edits as positional patches
// in oplog.cpp (edit_plan / OpLog::apply_patches): CPU only, no device code, no Python.
// tools/asan_edit.sh builds it with AddressSanitizer + UBSan and runs it.
//
// A log (RGA, then Fugue) and a clone of it take the same seeded sets of non-touching patches, the
// log through apply_patches in one call, the clone through remove + insert per patch (what
// crdt_hip_oplog_replace does); a plain std::u32string model takes them too.  After every set the
// two logs must hold the same columns and delete ops and the model must be as long as the logs'
// visible length; between sets another agent's fork is joined in, so the next set rebuilds the
// positional index first.  The patches and their text are read from heap blocks of exactly the
// size passed, and every malformed set must be refused with its code and change nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crdt_hip.h"
#include "oplog.hpp"
#include "util.hpp"

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

const std::u32string kWords[] = {U"a", U"bc", U"é", U"€", U"\U0001F600", U"xyz ", U"hello wörld"};

struct Set {
    std::vector<PatchRec> p;
    std::vector<std::u32string> text;  // per patch, as codepoints
    std::string ins;                   // the pieces, contiguous
};

// Ascending, non-touching patches over a document of `len` codepoints.
Set random_set(uint64_t len, uint32_t count) {
    Set s;
    uint64_t old = 0;
    int64_t shift = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const uint64_t start = old + (k ? 1 : 0) + (len ? rnd(12) : 0);
        if (start > len) break;
        const uint32_t kind = rnd(10);
        uint32_t del = kind < 4 ? 0u : (uint32_t)std::min<uint64_t>(len - start, 1 + rnd(5));
        std::u32string w = (kind >= 4 && kind < 7 && del) ? std::u32string() : kWords[rnd(7)];
        if (!del && w.empty()) w = U"z";
        PatchRec r;
        r.pos = (uint64_t)((int64_t)start + shift);
        r.ins_off = s.ins.size();
        r.del = del;
        for (char32_t c : w) {
            char b[4];
            s.ins.append(b, crdt::utf8_put((uint32_t)c, b));
        }
        r.ins_len = (uint32_t)(s.ins.size() - r.ins_off);
        s.p.push_back(r);
        s.text.push_back(w);
        shift += (int64_t)w.size() - (int64_t)del;
        old = start + del;
    }
    return s;
}

bool same(const OpLog& a, const OpLog& b) {
    auto eq = [](const auto& x, const auto& y) {
        return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])));
    };
    return eq(a.parent, b.parent) && eq(a.oright, b.oright) && eq(a.lamport, b.lamport) &&
           eq(a.cp, b.cp) && eq(a.agent, b.agent) && eq(a.deleted, b.deleted) &&
           eq(a.del_ops, b.del_ops) && a.side == b.side && a.visible() == b.visible() &&
           a.max_lamport == b.max_lamport;
}

// apply_patches with the arrays in heap blocks of exactly the size passed.
int apply(OpLog& log, const std::vector<PatchRec>& p, const std::string& ins, uint32_t* added,
          uint32_t* tomb, std::string& err) {
    PatchRec* hp = (PatchRec*)std::malloc(p.size() ? p.size() * sizeof(PatchRec) : 1);
    uint8_t* ht = (uint8_t*)std::malloc(ins.size() ? ins.size() : 1);
    REQUIRE(hp && ht);
    if (!p.empty()) std::memcpy(hp, p.data(), p.size() * sizeof(PatchRec));
    if (!ins.empty()) std::memcpy(ht, ins.data(), ins.size());
    const int rc = log.apply_patches(hp, p.size(), ht, ins.size(), added, tomb, err);
    std::free(hp);
    std::free(ht);
    return rc;
}

void refuse(OpLog& log, std::vector<PatchRec> p, const std::string& ins, int code) {
    const OpLog before = log;
    std::string err;
    REQUIRE(apply(log, p, ins, nullptr, nullptr, err) == code && !err.empty());
    REQUIRE(same(log, before));
}

void rejections(OpLog& log) {
    const uint64_t n = log.visible();
    REQUIRE(n >= 20);
    refuse(log, {{3, 0, 0, 2}, {5, 2, 1, 0}}, "xy", CRDT_HIP_EINVAL);           // touching
    refuse(log, {{9, 0, 1, 0}, {4, 0, 1, 0}}, "", CRDT_HIP_EINVAL);             // descending
    refuse(log, {{2, 0, 1, 0}, {6, 0, 0, 0}}, "", CRDT_HIP_EINVAL);             // an empty patch
    refuse(log, {{n + 1, 0, 0, 1}}, "x", CRDT_HIP_ERANGE);                      // pos past the end
    refuse(log, {{n - 2, 0, 3, 0}}, "", CRDT_HIP_ERANGE);                       // del past the end
    refuse(log, {{0, 0, (uint32_t)n, 0}, {2, 0, 0, 1}}, "x", CRDT_HIP_ERANGE);  // ... as left
    refuse(log, {{1, 2, 0, 1}}, "xy", CRDT_HIP_EINVAL);                         // a bad ins_off
    refuse(log, {{1, ~0ull - 1, 0, 4}}, "xy", CRDT_HIP_EINVAL);                 // ... that wraps
    refuse(log, {{1, 0, 0, 2}}, "\xE2\x82", CRDT_HIP_EINVAL);                   // truncated UTF-8
    refuse(log, {{1, 0, 0, 1}}, "\x80", CRDT_HIP_EINVAL);                       // stray continuation
    refuse(log, {{1, 0, 0, 5}}, "\xF8\x88\x80\x80\x80", CRDT_HIP_EINVAL);       // 5-byte form
}

void run(bool fugue, uint32_t rounds) {
    size_t total = 0;
    for (uint32_t round = 0; round < rounds; ++round) {
        OpLog log;
        log.fugue = fugue;
        log.local_agent = 1;
        std::u32string model;
        std::string err;
        uint32_t added = 0, tomb = 0;
        {  // from the empty log: one insert at the document start
            Set s = random_set(0, 1);
            REQUIRE(s.p.size() == 1);
            REQUIRE(apply(log, s.p, s.ins, &added, &tomb, err) == CRDT_HIP_OK);
            model = s.text[0];
            const std::u32string seed = U"the quick brown fox jumps over the lazy dog ";
            REQUIRE(log.insert(model.size(), reinterpret_cast<const uint32_t*>(seed.data()), seed.size()).empty());
            model += seed;
        }
        OpLog other = log;
        other.local_agent = 2;
        for (uint32_t step = 0; step < 6; ++step) {
            REQUIRE(log.visible() == model.size());
            const Set s = random_set(model.size(), step == 0 ? 1 : 1 + rnd(30));
            OpLog ref = log;
            for (size_t k = 0; k < s.p.size(); ++k) {
                if (s.p[k].del) REQUIRE(ref.remove(s.p[k].pos, s.p[k].pos + s.p[k].del).empty());
                if (!s.text[k].empty())
                    REQUIRE(ref.insert(s.p[k].pos, reinterpret_cast<const uint32_t*>(s.text[k].data()),
                                       s.text[k].size()).empty());
                model.replace(s.p[k].pos, s.p[k].del, s.text[k]);
            }
            REQUIRE(apply(log, s.p, s.ins, &added, &tomb, err) == CRDT_HIP_OK);
            REQUIRE(same(log, ref));
            uint64_t na = 0, nt = 0;
            for (size_t k = 0; k < s.p.size(); ++k) {
                na += s.text[k].size();
                nt += s.p[k].del;
            }
            REQUIRE(added == na && tomb == nt && log.visible() == model.size());
            total += s.p.size();
            if (log.visible() >= 20) rejections(log);
            // another agent's edits come in by a join: the next set rebuilds the index first.
            // The model follows through patches_since.
            const Set o = random_set(other.visible(), 1 + rnd(4));
            REQUIRE(apply(other, o.p, o.ins, nullptr, nullptr, err) == CRDT_HIP_OK);
            const crdt::LogMark m = log.mark();
            REQUIRE(log.join(other.size(), other.parent.data(), other.oright.data(), other.lamport.data(),
                             other.agent.data(), other.deleted.data(), other.cp.data(),
                             fugue ? other.side.data() : nullptr, nullptr, nullptr, err) == CRDT_HIP_OK);
            std::vector<PatchRec> back;
            std::vector<uint8_t> text;
            REQUIRE(log.patches_since(m, back, text, err) == CRDT_HIP_OK);
            for (const PatchRec& r : back) {
                std::vector<uint32_t> cps;
                REQUIRE(crdt::utf8_decode(reinterpret_cast<const char*>(text.data()) + r.ins_off, r.ins_len, cps));
                model.replace(r.pos, r.del, std::u32string(cps.begin(), cps.end()));
            }
        }
        // an empty set changes nothing
        const OpLog before = log;
        REQUIRE(apply(log, {}, "", &added, &tomb, err) == CRDT_HIP_OK && added == 0 && tomb == 0);
        REQUIRE(same(log, before));
    }
    std::printf("%s: %u rounds, %zu patches applied\n", fugue ? "fugue" : "rga", rounds, total);
    REQUIRE(total > rounds);
}

}  // namespace

int main() {
    run(false, 200);
    run(true, 200);
    std::puts("edit_asan ok");
    return 0;
}
