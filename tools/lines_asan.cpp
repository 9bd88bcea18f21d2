// lines_asan.cpp — stand-alone host program for a sanitizer run of the line index in oplog.cpp
// (OpLog::line_starts, OpLog::lines_of): CPU only, no device code, no Python.  tools/asan_lines.sh
// builds it with AddressSanitizer + UBSan and runs it.
//
// Per round (40 seeded rounds, RGA, then Fugue) a log goes through steps of local edits, wire
// updates, a join and a delta, with a std::u32string model kept beside it; after each step a mark is
// taken and the model recorded.  After every step, for the version now and for every mark so far,
// every line number 0..L + 1 and every position, in codepoints and in UTF-8 bytes, must give what a
// scan of the recording for U+000A gives, with the info.  Output blocks are heap blocks of exactly n
// records, so a write past one is seen.  The malformed calls run after every step and must be
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
using crdt::LineInfo;
using crdt::LinePos;
using crdt::LogMark;
using crdt::OpLog;
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

size_t g_queries = 0, g_refused = 0;

// The same positional edits to the log and to the model; one word in four holds a line break.
void edits(OpLog& log, std::u32string& model, uint32_t k) {
    static const std::u32string words[] = {U"a",   U"b\nc", U"é",      U"€", U"\U0001F600",
                                           U"\n",  U"xyz ", U"\n\n\r"};
    for (uint32_t i = 0; i < k; ++i) {
        const uint64_t n = log.visible();
        REQUIRE(n == model.size());
        if (n < 4 || rnd(100) < 60) {
            const std::u32string& w = words[rnd(8)];
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

// The model of a version: per gap its bytes, and per line its start in codepoints.
struct Lines {
    std::vector<uint64_t> ends, starts;
    explicit Lines(const std::u32string& t) : ends(1, 0), starts(1, 0) {
        for (size_t k = 0; k < t.size(); ++k) {
            char b[4];
            ends.push_back(ends.back() + crdt::utf8_put((uint32_t)t[k], b));
            if (t[k] == U'\n') starts.push_back(k + 1);
        }
    }
    uint64_t len() const { return ends.size() - 1; }
    uint64_t breaks() const { return starts.size() - 1; }
};

// One call into a heap block of exactly n records; the queries in a heap block of exactly n too.
std::vector<LinePos> ask(const OpLog& log, const LogMark* m, bool positions, const std::vector<uint64_t>& q,
                         uint32_t flags, const Lines& want) {
    const size_t n = q.size();
    uint64_t* in = (uint64_t*)std::malloc(n ? n * sizeof(uint64_t) : 1);
    LinePos* out = (LinePos*)std::malloc(n ? n * sizeof(LinePos) : 1);
    REQUIRE(in && out);
    if (n) std::memcpy(in, q.data(), n * sizeof(uint64_t));
    LineInfo info{7, 7, 7};
    std::string err;
    const int rc = positions ? log.lines_of(m, n ? in : nullptr, n, flags, n ? out : nullptr, &info, err)
                             : log.line_starts(m, n ? in : nullptr, n, n ? out : nullptr, &info, err);
    REQUIRE(rc == CRDT_HIP_OK);
    REQUIRE(info.lines == want.breaks() + 1 && info.len == want.len() && info.len_bytes == want.ends.back());
    std::vector<LinePos> got(out, out + n);
    std::free(in);
    std::free(out);
    g_queries += n;
    return got;
}

void check_version(const OpLog& log, const LogMark* m, const std::u32string& text) {
    const Lines w(text);
    const uint64_t L = w.breaks(), len = w.len();
    std::vector<uint64_t> q;
    for (uint64_t k = L + 2; k-- > 0;) q.push_back(k);  // every line number, descending
    q.push_back(L / 2);                                   // and one again
    std::vector<LinePos> got = ask(log, m, false, q, 0, w);
    for (size_t i = 0; i < q.size(); ++i) {
        const uint64_t s = q[i] <= L ? w.starts[q[i]] : len;
        REQUIRE(got[i].line == q[i] && got[i].start == s && got[i].start_bytes == w.ends[s] &&
                got[i].col == 0 && got[i].col_bytes == 0);
    }
    for (uint32_t flags : {0u, kTextBytes}) {
        q.clear();
        for (uint64_t p = 0; p <= len; ++p) q.push_back(flags ? w.ends[p] : p);
        got = ask(log, m, true, q, flags, w);
        uint64_t line = 0;
        for (uint64_t p = 0; p <= len; ++p) {
            while (line < L && w.starts[line + 1] <= p) ++line;
            const uint64_t s = w.starts[line];
            REQUIRE(got[p].line == line && got[p].start == s && got[p].start_bytes == w.ends[s] &&
                    got[p].col == p - s && got[p].col_bytes == w.ends[p] - w.ends[s]);
        }
    }
    ask(log, m, false, {}, 0, w);  // n == 0 writes only the info
    ask(log, m, true, {}, kTextBytes, w);
}

// A refused call leaves out and *info as they were.
void refused(const OpLog& log, const LogMark* m, bool positions, std::vector<uint64_t> q, uint32_t flags,
             int code, bool null_in = false, bool null_out = false) {
    const size_t n = q.size();
    LinePos* out = (LinePos*)std::malloc(n * sizeof(LinePos));
    REQUIRE(out);
    std::memset(out, 0xA5, n * sizeof(LinePos));
    LineInfo info{7, 7, 7};
    std::string err;
    const uint64_t* in = null_in ? nullptr : q.data();
    LinePos* o = null_out ? nullptr : out;
    const int rc = positions ? log.lines_of(m, in, n, flags, o, &info, err)
                             : log.line_starts(m, in, n, o, &info, err);
    REQUIRE(rc == code && !err.empty() && info.lines == 7 && info.len == 7 && info.len_bytes == 7);
    for (size_t k = 0; k < n * sizeof(LinePos); ++k) REQUIRE(reinterpret_cast<uint8_t*>(out)[k] == 0xA5);
    std::free(out);
    ++g_refused;
}

void malformed(const OpLog& log, const LogMark* m, const std::u32string& text) {
    const Lines w(text);
    const uint64_t L = w.breaks(), len = w.len(), nb = w.ends.back();
    refused(log, m, false, {0, L + 2}, 0, CRDT_HIP_ERANGE);
    refused(log, m, false, {~0ull}, 0, CRDT_HIP_ERANGE);
    refused(log, m, true, {0, len + 1}, 0, CRDT_HIP_ERANGE);
    refused(log, m, true, {nb + 1, 0}, kTextBytes, CRDT_HIP_ERANGE);
    refused(log, m, true, {0}, 2, CRDT_HIP_EINVAL);
    refused(log, m, true, {len + 1}, 2, CRDT_HIP_EINVAL);  // two faults: the earlier check's code
    refused(log, m, true, {0}, 0, CRDT_HIP_EINVAL, true);
    refused(log, m, true, {0}, 0, CRDT_HIP_EINVAL, false, true);
    refused(log, m, false, {0}, 0, CRDT_HIP_EINVAL, true);
    refused(log, m, false, {L + 9}, 0, CRDT_HIP_EINVAL, false, true);
    for (uint64_t k = 0; k < len; ++k)
        if (w.ends[k + 1] - w.ends[k] > 1) {  // a multi-byte codepoint: every byte inside it
            for (uint64_t x = w.ends[k] + 1; x < w.ends[k + 1]; ++x) {
                refused(log, m, true, {0, x, nb}, kTextBytes, CRDT_HIP_EINVAL);
                refused(log, m, true, {x, nb + 1}, kTextBytes, CRDT_HIP_ERANGE);
            }
            if (w.ends[k + 1] - w.ends[k] == 4) break;
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
        check_version(log, nullptr, model);  // the empty log: one line
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
            for (size_t k = 0; k < marks.size(); ++k) check_version(log, &marks[k], recs[k]);
            const uint32_t any = rnd((uint32_t)marks.size());
            malformed(log, &marks[any], recs[any]);
        }
        // a mark of a longer log is refused
        OpLog longer = log;
        edits(longer, model, 3);
        if (longer.size() > log.size()) {
            const LogMark m = longer.mark();
            refused(log, &m, false, {0}, 0, CRDT_HIP_EINVAL);
            refused(log, &m, true, {0}, 0, CRDT_HIP_EINVAL);
        }
    }
    std::printf("%s: %u rounds, %zu queries answered, %zu calls refused so far\n", fugue ? "fugue" : "rga",
                rounds, g_queries, g_refused);
}

}  // namespace

int main() {
    run(false, 40);
    run(true, 40);
    REQUIRE(g_queries > 100000 && g_refused > 5000);
    std::puts("lines_asan ok");
    return 0;
}
