// delta_asan.cpp — stand-alone host program for a sanitizer run of the delta sync in oplog.cpp
// (OpLog::state_vector / encode_diff / apply_diff and delta_frame): CPU only, no device code, no
// Python.  tools/asan_delta.sh builds it with AddressSanitizer + UBSan and runs it.
//
// Two forks of a typed base (RGA, then Fugue) are synced both ways and compared with the join;
// then the delta's bytes are damaged (every truncation, every single-byte change of the header
// and of a spread of positions, seeded random multi-byte damage, oversized buffers) and applied to
// a clone: every call must return a status, and a rejected delta must leave the log as it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crdt_hip.h"
#include "oplog.hpp"

using crdt::OpLog;
using crdt::SvEntry;

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

void edits(OpLog& log, uint32_t k) {
    static const char* words[] = {"a", "bc", "\xC3\xA9", "\xE2\x82\xAC", "\xF0\x9F\x98\x80", "xyz "};
    for (uint32_t i = 0; i < k; ++i) {
        const uint64_t n = log.visible();
        if (n < 4 || rnd(100) < 60) {
            const char* w = words[rnd(6)];
            REQUIRE(log.insert_utf8(rnd((uint32_t)n + 1), w, std::strlen(w)).empty());
        } else {
            const uint64_t a = rnd((uint32_t)n - 1);
            REQUIRE(log.remove(a, std::min<uint64_t>(n, a + 1 + rnd(3))).empty());
        }
    }
}

bool same(const OpLog& x, const OpLog& y, bool oright) {
    return x.parent == y.parent && x.lamport == y.lamport && x.agent == y.agent &&
           x.deleted == y.deleted && x.cp == y.cp && x.side == y.side &&
           (!oright || x.oright == y.oright) && x.del_ops.size() == y.del_ops.size();
}

std::vector<uint8_t> diff(const OpLog& src, const std::vector<SvEntry>& sv) {
    std::vector<uint8_t> d;
    std::string err;
    REQUIRE(src.encode_diff(sv.data(), sv.size(), d, err) == CRDT_HIP_OK);
    return d;
}

// Apply `bytes` (copied into a heap block of exactly its size, so that a read past it is seen)
// to a clone of dst; a rejected delta must change nothing.
int apply_damaged(const OpLog& dst, const std::vector<uint8_t>& bytes) {
    OpLog d = dst;
    uint8_t* heap = (uint8_t*)std::malloc(bytes.size() ? bytes.size() : 1);
    REQUIRE(heap);
    if (!bytes.empty()) std::memcpy(heap, bytes.data(), bytes.size());
    uint32_t added = 0, tomb = 0;
    std::string err;
    const int rc = d.apply_diff(heap, bytes.size(), &added, &tomb, err);
    std::free(heap);
    if (rc) {
        REQUIRE(rc == CRDT_HIP_EINVAL || rc == CRDT_HIP_EBADLOG || rc == CRDT_HIP_ERANGE);
        REQUIRE(!err.empty() && same(d, dst, true) && d.del_ops == dst.del_ops);
    } else {
        REQUIRE(d.size() == dst.size() + added);
    }
    return rc;
}

void run(bool fugue) {
    OpLog base;
    base.fugue = fugue;
    edits(base, 120);
    OpLog a = base, b = base;
    a.local_agent = 1;
    b.local_agent = 65535;
    edits(a, 90);
    edits(b, 70);

    // sync b into a, against the join (origin_right absent)
    OpLog j = a, d = a;
    uint32_t ja = 0, jt = 0, da = 0, dt = 0;
    std::string err;
    REQUIRE(j.join(b.size(), b.parent.data(), nullptr, b.lamport.data(), b.agent.data(),
                   b.deleted.data(), b.cp.data(), fugue ? b.side.data() : nullptr, &ja, &jt, err) == 0);
    const std::vector<SvEntry> sva = a.state_vector();
    REQUIRE(sva.size() == 2 && sva[0].agent == 0 && sva[1].agent == 1);
    const std::vector<uint8_t> delta = diff(b, sva);
    REQUIRE(d.apply_diff(delta.data(), delta.size(), &da, &dt, err) == 0);
    REQUIRE(da == ja && dt == jt && ja > 0 && same(d, j, true));
    REQUIRE(d.apply_diff(delta.data(), delta.size(), &da, &dt, err) == 0 && da == 0 && dt == 0);
    REQUIRE(same(d, j, true));
    // the other way, an empty vector, the log's own vector, an empty log
    OpLog e = b;
    const std::vector<uint8_t> back = diff(a, b.state_vector());
    REQUIRE(e.apply_diff(back.data(), back.size(), nullptr, nullptr, err) == 0 && e.size() == d.size());
    const std::vector<uint8_t> whole = diff(d, {});
    OpLog fresh;
    fresh.fugue = fugue;
    REQUIRE(fresh.apply_diff(whole.data(), whole.size(), &da, &dt, err) == 0 && da == d.size());
    REQUIRE(diff(fresh, {}) == whole);
    const std::vector<uint8_t> own = diff(d, d.state_vector());
    // (ranges only; `a` lacks some of the items they name, and says so)
    REQUIRE(own.size() > 16 && apply_damaged(fresh, own) == 0 && apply_damaged(a, own) == CRDT_HIP_EBADLOG);
    REQUIRE(fresh.state_vector().size() == 3 && OpLog().state_vector().empty());
    // positional edits after an apply rebuild the index
    edits(d, 20);
    // bad vectors
    const SvEntry unsorted[2] = {{2, 1}, {1, 1}}, wide[1] = {{65536, 1}};
    std::vector<uint8_t> out;
    REQUIRE(a.encode_diff(unsorted, 2, out, err) == CRDT_HIP_EINVAL);
    REQUIRE(a.encode_diff(wide, 1, out, err) == CRDT_HIP_EINVAL);

    // ---- damaged deltas --------------------------------------------------------------------
    unsigned rejected = 0, taken = 0;
    auto tally = [&](int rc) { (rc ? rejected : taken)++; };
    REQUIRE(apply_damaged(a, delta) == 0);
    for (size_t len = 0; len < delta.size(); len += (len < 64 ? 1 : 37))
        tally(apply_damaged(a, std::vector<uint8_t>(delta.begin(), delta.begin() + len)));
    for (size_t extra : {1u, 4u, 20u, 4096u}) {
        std::vector<uint8_t> big = delta;
        big.resize(delta.size() + extra, 0xAB);
        tally(apply_damaged(a, big));
    }
    for (size_t pos = 0; pos < delta.size(); pos += (pos < 16 ? 1 : 1 + rnd(23)))
        for (uint8_t v : {(uint8_t)0x00, (uint8_t)0xFF, (uint8_t)(delta[pos] ^ 1), (uint8_t)(delta[pos] ^ 0x80)}) {
            std::vector<uint8_t> m = delta;
            m[pos] = v;
            tally(apply_damaged(a, m));
        }
    for (int it = 0; it < 400; ++it) {
        std::vector<uint8_t> m = it & 1 ? delta : own;
        for (uint32_t k = 1 + rnd(6); k; --k) m[rnd((uint32_t)m.size())] = (uint8_t)rnd(256);
        tally(apply_damaged(a, m));
    }
    // headers that promise far more than the buffer holds, and counts that overflow
    for (uint32_t n : {0xFFFFFFFFu, 0x0CCCCCCCu, 0x7FFFFFFFu})
        for (int field = 2; field < 4; ++field) {
            std::vector<uint8_t> m = delta;
            std::memcpy(m.data() + 4 * field, &n, 4);
            REQUIRE(apply_damaged(a, m) == CRDT_HIP_EINVAL);
        }
    // the other kind's delta
    OpLog other;
    other.fugue = !fugue;
    REQUIRE(other.apply_diff(whole.data(), whole.size(), nullptr, nullptr, err) == CRDT_HIP_EINVAL);
    std::printf("%s: delta %zu bytes, %u damaged deltas rejected, %u taken\n", fugue ? "fugue" : "rga",
                delta.size(), rejected, taken);
    REQUIRE(rejected > 100);
}

}  // namespace

int main() {
    run(false);
    run(true);
    std::puts("delta_asan ok");
    return 0;
}
