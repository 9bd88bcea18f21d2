// text_asan.cpp — stand-alone host program for a sanitizer run of text windows in oplog.cpp
// (OpLog::text_at): CPU only, no device code, no Python.  tools/asan_text.sh builds it with
// AddressSanitizer + UBSan and runs it.
//
// Per round (60 seeded rounds, RGA, then Fugue) a log goes through steps of local edits, wire
// updates, a join and a delta, with a std::u32string model kept beside it; after each step a mark is
// taken and the model recorded as UTF-8.  At the end every text_at(mark) must equal its recording
// (the history property), random windows of it in codepoints and in bytes must equal the slice of
// the recording with all six fields of the info (the window-slice property), and patches_since(mark)
// applied to text_at(mark) must give the text now.  Output buffers are heap blocks of exactly the
// size passed, so a write past one is seen.  The malformed calls run in every round and must be
// refused with their outputs untouched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crdt_hip.h"
#include "oplog.hpp"
#include "util.hpp"

using crdt::kTextBytes;
using crdt::kTextEnd;
using crdt::LogMark;
using crdt::OpLog;
using crdt::PatchRec;
using crdt::TextInfo;

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

size_t g_windows = 0, g_refused = 0;

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

std::string encode(const std::u32string& s, std::vector<uint64_t>* ends = nullptr) {
    std::string out;
    if (ends) ends->assign(1, 0);
    for (char32_t c : s) {
        char b[4];
        out.append(b, crdt::utf8_put((uint32_t)c, b));
        if (ends) ends->push_back(out.size());
    }
    return out;
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

// One window: sized with no buffer, then read into a heap block of exactly n_bytes.
std::string window(const OpLog& log, const LogMark* m, uint64_t start, uint64_t end, uint32_t flags,
                   TextInfo& info) {
    std::string err;
    size_t need = ~(size_t)0;
    const int rc = log.text_at(m, start, end, flags, nullptr, 0, &need, &info, err);
    REQUIRE(rc == (need ? CRDT_HIP_ESPACE : CRDT_HIP_OK) && need == info.n_bytes);
    uint8_t* block = (uint8_t*)std::malloc(need ? need : 1);
    REQUIRE(block);
    size_t got = 0;
    TextInfo again{};
    REQUIRE(log.text_at(m, start, end, flags, need ? block : nullptr, need, &got, &again, err) == CRDT_HIP_OK);
    REQUIRE(got == need && std::memcmp(&again, &info, sizeof info) == 0);
    std::string out(reinterpret_cast<char*>(block), need);
    std::free(block);
    ++g_windows;
    return out;
}

// Window [a, b) in codepoints of the version whose text is `rec`, asked in both units.
void check_window(const OpLog& log, const LogMark* m, const std::string& rec,
                  const std::vector<uint64_t>& ends, uint64_t a, uint64_t b) {
    const uint64_t len = ends.size() - 1;
    const std::string want = rec.substr(ends[a], ends[b] - ends[a]);
    for (uint32_t flags : {0u, kTextBytes}) {
        TextInfo i{};
        const uint64_t s = flags ? ends[a] : a;
        const uint64_t e = b == len && rnd(2) ? kTextEnd : flags ? ends[b] : b;
        REQUIRE(window(log, m, s, e, flags, i) == want);
        REQUIRE(i.len == len && i.len_bytes == rec.size() && i.start == a && i.start_bytes == ends[a] &&
                i.n == b - a && i.n_bytes == want.size());
    }
}

// A refused call leaves out, *out_len and *info as they were.
void refused(const OpLog& log, const LogMark* m, uint64_t start, uint64_t end, uint32_t flags,
             int code, bool null_len = false) {
    uint8_t* block = (uint8_t*)std::malloc(8);
    REQUIRE(block);
    std::memset(block, 0xA5, 8);
    size_t n = 0xDEAD;
    TextInfo i{7, 7, 7, 7, 7, 7};
    std::string err;
    REQUIRE(log.text_at(m, start, end, flags, block, 8, null_len ? nullptr : &n, &i, err) == code);
    REQUIRE(!err.empty() && n == 0xDEAD && i.len == 7 && i.n_bytes == 7);
    for (int k = 0; k < 8; ++k) REQUIRE(block[k] == 0xA5);
    std::free(block);
    ++g_refused;
}

void malformed(const OpLog& log, const LogMark& m, const std::string& rec,
               const std::vector<uint64_t>& ends) {
    const uint64_t len = ends.size() - 1, nb = rec.size();
    refused(log, &m, 0, 1, 2, CRDT_HIP_EINVAL);
    refused(log, &m, 0, 1, 0, CRDT_HIP_EINVAL, true);
    refused(log, &m, 3, 2, 0, CRDT_HIP_EINVAL);
    refused(log, &m, len + 1, kTextEnd, 0, CRDT_HIP_ERANGE);
    refused(log, &m, 0, len + 1, 0, CRDT_HIP_ERANGE);
    refused(log, &m, 0, nb + 1, kTextBytes, CRDT_HIP_ERANGE);
    refused(log, &m, len + 1, kTextEnd, 2, CRDT_HIP_EINVAL);  // two faults: the earlier check's code
    refused(log, &m, len + 5, len + 2, 0, CRDT_HIP_EINVAL);
    for (uint64_t k = 0; k + 1 < ends.size(); ++k)
        if (ends[k + 1] - ends[k] > 1) {  // a multi-byte codepoint: every cut inside it
            for (uint64_t x = ends[k] + 1; x < ends[k + 1]; ++x) {
                refused(log, &m, x, kTextEnd, kTextBytes, CRDT_HIP_EINVAL);
                refused(log, &m, 0, x, kTextBytes, CRDT_HIP_EINVAL);
                refused(log, &m, x, nb + 1, kTextBytes, CRDT_HIP_ERANGE);
            }
            break;
        }
    if (nb) {  // ESPACE one byte short: *out_len and *info set, the block of nb - 1 bytes untouched
        uint8_t* block = (uint8_t*)std::malloc(nb > 1 ? nb - 1 : 1);
        REQUIRE(block);
        std::memset(block, 0xA5, nb > 1 ? nb - 1 : 1);
        size_t n = 0;
        TextInfo i{};
        std::string err;
        REQUIRE(log.text_at(&m, 0, kTextEnd, 0, block, nb - 1, &n, &i, err) == CRDT_HIP_ESPACE);
        REQUIRE(n == nb && i.n_bytes == nb && i.len == len);
        for (uint64_t k = 0; k + 1 < nb; ++k) REQUIRE(block[k] == 0xA5);
        std::free(block);
        ++g_refused;
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

// log.patches_since(m) applied to `text` (codepoints) as replace(pos..pos + del, ins).
std::u32string patched(const OpLog& log, const LogMark& m, std::u32string text) {
    std::vector<PatchRec> p;
    std::vector<uint8_t> ins;
    std::string err;
    REQUIRE(log.patches_since(m, p, ins, err) == CRDT_HIP_OK);
    for (const PatchRec& r : p) {
        REQUIRE(r.pos + r.del <= text.size() && r.ins_off + r.ins_len <= ins.size());
        text.replace(r.pos, r.del,
                     decode(std::string(reinterpret_cast<const char*>(ins.data()) + r.ins_off, r.ins_len)));
    }
    return text;
}

void run(bool fugue, uint32_t rounds) {
    for (uint32_t round = 0; round < rounds; ++round) {
        OpLog log;
        log.fugue = fugue;
        std::u32string model;
        edits(log, model, 10 + rnd(40));
        // two forks that the log takes in later: their edits are concurrent to the log's own
        OpLog fa = log, fb = log;
        std::u32string ma = model, mb = model;
        fa.local_agent = 1;
        fb.local_agent = 2;
        edits(fa, ma, 5 + rnd(20));
        edits(fb, mb, 5 + rnd(20));
        std::vector<LogMark> marks;
        std::vector<std::string> recs;
        const uint32_t steps = 8 + rnd(8), at_join = rnd(steps), at_delta = rnd(steps);
        for (uint32_t step = 0; step < steps; ++step) {
            if (step == at_join || step == at_delta) {
                // the model after a sync is the log's own text: read it whole, through text_at
                take(log, step == at_join ? fa : fb, step != at_join);
                TextInfo i{};
                model = decode(window(log, nullptr, 0, kTextEnd, 0, i));
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
            recs.push_back(encode(model));
        }
        const std::string now = encode(model);
        TextInfo i{};
        REQUIRE(window(log, nullptr, 0, kTextEnd, 0, i) == now);
        for (size_t k = 0; k < marks.size(); ++k) {
            std::vector<uint64_t> ends;
            const std::u32string at = decode(recs[k]);
            REQUIRE(encode(at, &ends) == recs[k]);
            const uint64_t len = at.size();
            REQUIRE(window(log, &marks[k], 0, kTextEnd, 0, i) == recs[k]);  // history
            for (int w = 0; w < 4; ++w) {                                    // window slices
                const uint64_t a = rnd((uint32_t)len + 1), b = a + rnd((uint32_t)(len - a) + 1);
                check_window(log, &marks[k], recs[k], ends, a, b);
            }
            REQUIRE(patched(log, marks[k], at) == model);
            if (k + 1 == marks.size() || k == 0) malformed(log, marks[k], recs[k], ends);
        }
        // a mark of a longer log is refused
        OpLog longer = log;
        edits(longer, model, 3);
        if (longer.size() > log.size()) {
            const LogMark m = longer.mark();
            refused(log, &m, 0, kTextEnd, 0, CRDT_HIP_EINVAL);
        }
    }
    std::printf("%s: %u rounds, %zu windows read, %zu calls refused so far\n", fugue ? "fugue" : "rga",
                rounds, g_windows, g_refused);
}

}  // namespace

int main() {
    run(false, 60);
    run(true, 60);
    REQUIRE(g_windows > 5000 && g_refused > 1000);
    std::puts("text_asan ok");
    return 0;
}
