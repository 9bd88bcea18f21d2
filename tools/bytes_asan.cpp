// bytes_asan.cpp — stand-alone host program for a sanitizer run of the byte-offset reading of
// positional patches in oplog.cpp (edit_plan_bytes / OpLog::apply_patches_bytes /
// OpLog::patches_since_bytes): CPU only, no device code, no Python.  tools/asan_bytes.sh builds it
// with AddressSanitizer + UBSan and runs it.
//
// A log (RGA, then Fugue) and a clone of it take the same seeded sets of non-touching patches, the
// log in UTF-8 byte offsets through apply_patches_bytes in one call, the clone in codepoints
// through remove + insert per patch (what crdt_hip_oplog_replace does); a std::u32string model
// gives the byte offsets.  After every set the two logs must hold the same columns and delete ops;
// between sets another agent's fork is joined in and the model follows through
// patches_since_bytes, spliced into a UTF-8 buffer kept beside it.  The patches and their text are
// read from heap blocks of exactly the size passed, and every malformed set, and every boundary
// inside a codepoint, must be refused with its code and change nothing.
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

uint64_t g_rng = 0x2545F4914F6CDD1Dull;
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

std::string utf8(const std::u32string& s, size_t first = 0, size_t count = std::u32string::npos) {
    std::string out;
    const size_t last = count == std::u32string::npos ? s.size() : first + count;
    for (size_t i = first; i < last; ++i) {
        char b[4];
        out.append(b, crdt::utf8_put((uint32_t)s[i], b));
    }
    return out;
}

struct Set {
    std::vector<PatchRec> cp, by;      // the same patches in codepoints and in bytes
    std::vector<std::u32string> text;  // per patch, as codepoints
    std::string ins;                   // the pieces, contiguous
};

// Ascending, non-touching patches over the document `doc`, pos counted as the earlier ones left it.
Set random_set(const std::u32string& doc, uint32_t count) {
    Set s;
    std::u32string cur = doc;
    const uint64_t len = doc.size();
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
        s.ins += utf8(w);
        r.ins_len = (uint32_t)(s.ins.size() - r.ins_off);
        PatchRec b = r;
        b.pos = utf8(cur, 0, r.pos).size();
        b.del = (uint32_t)utf8(cur, r.pos, del).size();
        cur.replace(r.pos, del, w);
        s.cp.push_back(r);
        s.by.push_back(b);
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

// apply_patches_bytes with the arrays in heap blocks of exactly the size passed.
int apply(OpLog& log, const std::vector<PatchRec>& p, const std::string& ins, uint32_t* added,
          uint32_t* tomb, std::string& err) {
    PatchRec* hp = (PatchRec*)std::malloc(p.size() ? p.size() * sizeof(PatchRec) : 1);
    uint8_t* ht = (uint8_t*)std::malloc(ins.size() ? ins.size() : 1);
    REQUIRE(hp && ht);
    if (!p.empty()) std::memcpy(hp, p.data(), p.size() * sizeof(PatchRec));
    if (!ins.empty()) std::memcpy(ht, ins.data(), ins.size());
    const int rc = log.apply_patches_bytes(hp, p.size(), ht, ins.size(), added, tomb, err);
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

void rejections(OpLog& log, const std::u32string& model) {
    const uint64_t n = log.visible_bytes();
    REQUIRE(n >= 20 && n == utf8(model).size());
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
    // every byte offset inside a codepoint, as a pos and as the end of a delete
    uint64_t b = 0, inside = 0;
    for (char32_t c : model) {
        const uint64_t w = crdt::utf8_len_cp((uint32_t)c);
        for (uint64_t k = 1; k < w; ++k) {
            refuse(log, {{b + k, 0, 0, 1}}, "x", CRDT_HIP_EINVAL);
            refuse(log, {{0, 0, (uint32_t)(b + k), 0}}, "", CRDT_HIP_EINVAL);
            // an argument error in a later patch wins over the boundary error
            refuse(log, {{b + k, 0, 0, 1}, {n + 1, 0, 3, 0}}, "x", CRDT_HIP_ERANGE);
            ++inside;
        }
        b += w;
        if (inside > 40) break;
    }
}

void run(bool fugue, uint32_t rounds) {
    size_t total = 0, differed = 0;
    for (uint32_t round = 0; round < rounds; ++round) {
        OpLog log;
        log.fugue = fugue;
        log.local_agent = 1;
        std::u32string model;
        std::string err;
        uint32_t added = 0, tomb = 0;
        {  // from the empty log: one insert at the document start
            Set s = random_set(model, 1);
            REQUIRE(s.by.size() == 1);
            REQUIRE(apply(log, s.by, s.ins, &added, &tomb, err) == CRDT_HIP_OK);
            model = s.text[0];
            const std::u32string seed = U"thé quick brown fox jumps over the lazy dog ";
            REQUIRE(log.insert(model.size(), reinterpret_cast<const uint32_t*>(seed.data()), seed.size()).empty());
            model += seed;
        }
        OpLog other = log;
        other.local_agent = 2;
        std::u32string other_model = model;
        for (uint32_t step = 0; step < 6; ++step) {
            REQUIRE(log.visible() == model.size() && log.visible_bytes() == utf8(model).size());
            const Set s = random_set(model, step == 0 ? 1 : 1 + rnd(30));
            OpLog ref = log;
            uint64_t na = 0, nt = 0;
            for (size_t k = 0; k < s.cp.size(); ++k) {
                if (s.cp[k].del) REQUIRE(ref.remove(s.cp[k].pos, s.cp[k].pos + s.cp[k].del).empty());
                if (!s.text[k].empty())
                    REQUIRE(ref.insert(s.cp[k].pos, reinterpret_cast<const uint32_t*>(s.text[k].data()),
                                       s.text[k].size()).empty());
                model.replace(s.cp[k].pos, s.cp[k].del, s.text[k]);
                na += s.text[k].size();
                nt += s.cp[k].del;
                differed += s.cp[k].pos != s.by[k].pos || s.cp[k].del != s.by[k].del;
            }
            REQUIRE(apply(log, s.by, s.ins, &added, &tomb, err) == CRDT_HIP_OK);
            REQUIRE(same(log, ref));
            REQUIRE(added == na && tomb == nt && log.visible() == model.size());
            total += s.by.size();
            if (log.visible_bytes() >= 20) rejections(log, model);
            // another agent's edits come in by a join; a UTF-8 buffer follows through
            // patches_since_bytes, each patch a splice of bytes
            const Set o = random_set(other_model, 1 + rnd(4));
            REQUIRE(apply(other, o.by, o.ins, nullptr, nullptr, err) == CRDT_HIP_OK);
            for (size_t k = 0; k < o.cp.size(); ++k) other_model.replace(o.cp[k].pos, o.cp[k].del, o.text[k]);
            const crdt::LogMark m = log.mark();
            REQUIRE(log.join(other.size(), other.parent.data(), other.oright.data(), other.lamport.data(),
                             other.agent.data(), other.deleted.data(), other.cp.data(),
                             fugue ? other.side.data() : nullptr, nullptr, nullptr, err) == CRDT_HIP_OK);
            std::vector<PatchRec> back, back_b;
            std::vector<uint8_t> text, text_b;
            REQUIRE(log.patches_since(m, back, text, err) == CRDT_HIP_OK);
            REQUIRE(log.patches_since_bytes(m, back_b, text_b, err) == CRDT_HIP_OK);
            REQUIRE(back.size() == back_b.size() && text == text_b);
            std::string buf = utf8(model);
            for (size_t k = 0; k < back.size(); ++k) {
                const PatchRec &r = back[k], &rb = back_b[k];
                std::vector<uint32_t> cps;
                REQUIRE(crdt::utf8_decode(reinterpret_cast<const char*>(text.data()) + r.ins_off, r.ins_len, cps));
                REQUIRE(rb.pos == utf8(model, 0, r.pos).size() && rb.del == utf8(model, r.pos, r.del).size());
                REQUIRE(rb.ins_off == r.ins_off && rb.ins_len == r.ins_len);
                if (k) REQUIRE(rb.pos > back_b[k - 1].pos + back_b[k - 1].ins_len);
                model.replace(r.pos, r.del, std::u32string(cps.begin(), cps.end()));
                REQUIRE(rb.pos + rb.del <= buf.size());
                buf.replace(rb.pos, rb.del, reinterpret_cast<const char*>(text_b.data()) + rb.ins_off, rb.ins_len);
            }
            REQUIRE(buf == utf8(model));
        }
        // an empty set changes nothing
        const OpLog before = log;
        REQUIRE(apply(log, {}, "", &added, &tomb, err) == CRDT_HIP_OK && added == 0 && tomb == 0);
        REQUIRE(same(log, before));
    }
    std::printf("%s: %u rounds, %zu patches applied, %zu of them differ in bytes\n",
                fugue ? "fugue" : "rga", rounds, total, differed);
    REQUIRE(total > rounds && differed * 2 > total);
}

}  // namespace

int main() {
    run(false, 100);
    run(true, 100);
    std::puts("bytes_asan ok");
    return 0;
}
