// oplog.cpp — order-statistic resolver over a chunked span sequence (runs of consecutive ids,
// chunks of <= 64 spans + a Fenwick tree of per-chunk visible counts): O(log C + 64) per
// positional lookup, O(1) amortised appends while typing on (the span of the last item grows).
// A chunk hint and a span hint make the lookup of an edit next to the previous one O(1); the
// Fenwick tree is rebuilt only when a lookup misses the hints after chunks were split.
#include "oplog.hpp"

#include <algorithm>
#include <cstring>

#include "crdt_hip.h"
#include "trace.hpp"
#include "util.hpp"

namespace crdt {

namespace {
constexpr size_t kSpanMax = 64;
constexpr uint32_t kMagic = kUpdateMagic;
constexpr uint32_t kWireVersion = kUpdateVersion;

void put32(std::vector<uint8_t>& b, uint32_t v) {
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
uint32_t get32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
}  // namespace

OpLog::OpLog() {
    chunks_.push_back(new_chunk());
    fen_build();
    nxt_.push_back(NIL);
}

void OpLog::reserve(size_t items, size_t dels) {
    del_ops.reserve(dels);
    parent.reserve(items);
    oright.reserve(items);
    lamport.reserve(items);
    cp.reserve(items);
    agent.reserve(items);
    deleted.reserve(items);
    nxt_.reserve(items + 1);
}

OpLog::Chunk OpLog::new_chunk() const {
    Chunk c;
    c.s.reserve(kSpanMax + 4);
    return c;
}

void OpLog::fen_build() const {
    fen_dirty_ = false;
    fen_.assign(chunks_.size() + 1, 0);
    for (size_t i = 0; i < chunks_.size(); ++i) {
        size_t j = i + 1;
        fen_[j] += chunks_[i].vis;
        size_t up = j + (j & (~j + 1));
        if (up <= chunks_.size()) fen_[up] += fen_[j];
    }
}

void OpLog::fen_add(size_t i, int64_t d) {
    if (fen_dirty_) return;  // (the rebuild counts the chunks as they are then)
    for (size_t j = i + 1; j < fen_.size(); j += j & (~j + 1)) fen_[j] += d;
}

size_t OpLog::fen_find(uint64_t& p) const {
    if (fen_dirty_) fen_build();
    size_t pos = 0;
    size_t step = 1;
    while (step * 2 < fen_.size()) step *= 2;
    for (; step; step >>= 1) {
        size_t nx = pos + step;
        if (nx < fen_.size() && (uint64_t)fen_[nx] < p) {
            pos = nx;
            p -= (uint64_t)fen_[nx];
        }
    }
    return pos;  // 0-based chunk; p is now the rank inside it
}

bool OpLog::find_visible(uint64_t p, size_t& c, size_t& si, uint32_t& off) const {
    if (p == 0 || p > nvis_) return false;
    uint64_t r = p;
    if (hint_c_ < chunks_.size() && p > hint_base_ && p - hint_base_ <= chunks_[hint_c_].vis) {
        c = hint_c_;
        r = p - hint_base_;
    } else {
        c = fen_find(r);
        if (c >= chunks_.size()) return false;
        hint_c_ = c;
        hint_base_ = p - r;
        hint_si_ = SIZE_MAX;
    }
    const std::vector<Span>& v = chunks_[c].s;
    si = 0;
    uint64_t vb = 0;  // visible items of the chunk before span si
    if (hint_si_ < v.size() && r > hint_vb_) {
        si = hint_si_;
        vb = hint_vb_;
    }
    for (; si < v.size(); ++si) {
        if (v[si].del()) continue;
        const uint32_t len = v[si].len();
        if (r - vb <= len) {
            off = (uint32_t)(r - vb) - 1;
            hint_si_ = si;
            hint_vb_ = vb;
            return true;
        }
        vb += len;
    }
    return false;
}

uint32_t OpLog::first_id_from(size_t c, size_t si) const {
    for (; c < chunks_.size(); ++c, si = 0)
        if (si < chunks_[c].s.size()) return chunks_[c].s[si].id;
    return NIL;
}

bool OpLog::split_chunk(size_t c) {
    if (chunks_[c].s.size() <= kSpanMax) return false;
    Chunk hi = new_chunk();
    std::vector<Span>& lo = chunks_[c].s;
    size_t half = lo.size() / 2;
    hi.s.assign(lo.begin() + half, lo.end());
    lo.resize(half);
    for (const Span& x : hi.s)
        if (!x.del()) hi.vis += x.len();
    chunks_[c].vis -= hi.vis;
    chunks_.insert(chunks_.begin() + c + 1, std::move(hi));
    fen_dirty_ = true;
    if (hint_c_ == c && hint_si_ >= half) hint_si_ = SIZE_MAX;  // the span moved to chunk c + 1
    if (hint_c_ != SIZE_MAX && hint_c_ > c) hint_c_++;         // (its visible base is unchanged)
    return true;
}

std::string OpLog::insert(uint64_t pos, const uint32_t* cps, size_t k) {
    if (stale_) {
        std::string e = rebuild_index();
        if (!e.empty()) return e;
    }
    if (!fugue) return insert_rga(pos, cps, k);
    if (pos > nvis_) return "insert position out of range";
    if (k == 0) return "";
    if ((uint64_t)size() + k >= 0x7FFFFFF0ull) return "op log too large";
    const uint32_t first = size() + 1;
    size_t c = 0, at = 0;  // new span goes to chunks_[c].s[at]
    uint32_t left = 0, right;
    bool extend = false;
    if (pos == 0) {
        right = first_id_from(0, 0);
        hint_c_ = 0;  // chunk 0 changes: keep the hint on it
        hint_base_ = 0;
        hint_si_ = SIZE_MAX;
    } else {
        size_t si;
        uint32_t off;
        if (!find_visible(pos, c, si, off)) return "resolver index corrupt";
        std::vector<Span>& v = chunks_[c].s;
        const Span S = v[si];
        left = S.id + off;
        if (off + 1 < S.len()) {  // split S after `left`
            right = left + 1;
            v[si].n = off + 1;
            v.insert(v.begin() + si + 1, Span{left + 1, S.len() - off - 1});
        } else {
            right = first_id_from(c, si + 1);
            extend = (S.id + S.len() == first);  // typing on: left is the last item created
        }
        at = si + 1;
    }
    if (fugue) {  // Fugue anchors (see oplog.hpp); every char after the first is a right child
        if (hasright_.size() < (size_t)first + k) hasright_.resize(std::max<size_t>(first + k, 2 * hasright_.size()), 0);
        const bool as_left = hasright_[left] != 0;
        if (as_left && right == NIL) return "resolver index corrupt (Fugue: no right neighbour)";
        side.resize(side.size() + k, 0);
        side[first - 1] = as_left ? 1 : 0;
        if (!as_left) hasright_[left] = 1;
        for (size_t j = 1; j < k; ++j) hasright_[first + j - 1] = 1;
        if (k == 1) {
            parent.push_back(as_left ? right : left);
            oright.push_back(right);
            lamport.push_back(++max_lamport);
            agent.push_back(local_agent);
            deleted.push_back(0);
            cp.push_back(cps[0]);
        } else {
            const size_t n0 = parent.size();
            parent.resize(n0 + k);
            oright.resize(n0 + k, right);
            lamport.resize(n0 + k);
            agent.resize(n0 + k, local_agent);
            deleted.resize(n0 + k, 0);
            cp.resize(n0 + k);
            parent[n0] = as_left ? right : left;
            for (size_t j = 1; j < k; ++j) parent[n0 + j] = first + (uint32_t)j - 1;
            for (size_t j = 0; j < k; ++j) lamport[n0 + j] = max_lamport + 1 + (uint32_t)j;
            max_lamport += (uint32_t)k;
            std::memcpy(cp.data() + n0, cps, k * sizeof(uint32_t));
        }
    } else if (k == 1) {  // typing: one item
        parent.push_back(left);
        oright.push_back(right);
        lamport.push_back(++max_lamport);
        agent.push_back(local_agent);
        deleted.push_back(0);
        cp.push_back(cps[0]);
    } else {  // a paste: every column grown once, then filled
        const size_t n0 = parent.size();
        parent.resize(n0 + k);
        oright.resize(n0 + k);
        lamport.resize(n0 + k);
        agent.resize(n0 + k, local_agent);
        deleted.resize(n0 + k, 0);
        cp.resize(n0 + k);
        uint32_t* P = parent.data() + n0;
        uint32_t* O = oright.data() + n0;
        uint32_t* L = lamport.data() + n0;
        P[0] = left;
        for (size_t j = 1; j < k; ++j) P[j] = first + (uint32_t)j - 1;
        for (size_t j = 0; j < k; ++j) {
            O[j] = right;
            L[j] = max_lamport + 1 + (uint32_t)j;
        }
        max_lamport += (uint32_t)k;
        std::memcpy(cp.data() + n0, cps, k * sizeof(uint32_t));
    }
    std::vector<Span>& v = chunks_[c].s;
    if (extend)
        v[at - 1].n += (uint32_t)k;
    else
        v.insert(v.begin() + at, Span{first, (uint32_t)k});
    chunks_[c].vis += (uint32_t)k;
    nvis_ += k;
    fen_add(c, (int64_t)k);
    split_chunk(c);
    return "";
}

// ---- RGA: gap buffer of visible id spans + full-list successors --------------------------------
void OpLog::gb_move(uint64_t pos) {
    while (gvis_ > pos) {
        GSpan& sp = gb_[g0_ - 1];
        if (gvis_ - sp.len >= pos) {
            gb_[--g1_] = sp;
            --g0_;
            gvis_ -= sp.len;
        } else {  // split: the part after pos goes right of the gap
            const uint32_t o = (uint32_t)(pos - (gvis_ - sp.len));
            gb_[--g1_] = GSpan{sp.id + o, sp.len - o};
            sp.len = o;
            gvis_ = pos;
        }
    }
    while (gvis_ < pos) {
        GSpan& sp = gb_[g1_];
        if (gvis_ + sp.len <= pos) {
            gb_[g0_++] = sp;
            ++g1_;
            gvis_ += sp.len;
        } else {
            const uint32_t o = (uint32_t)(pos - gvis_);
            gb_[g0_++] = GSpan{sp.id, o};
            sp.id += o;
            sp.len -= o;
            gvis_ = pos;
        }
    }
}

void OpLog::gb_reserve(size_t k) {
    if (g1_ - g0_ >= k) return;
    const size_t tail = gb_.size() - g1_;
    const size_t cap = std::max<size_t>({2 * gb_.size(), gb_.size() + k + 64, 1024});
    gb_.resize(cap);
    std::memmove(gb_.data() + cap - tail, gb_.data() + g1_, tail * sizeof(GSpan));
    g1_ = cap - tail;
}

std::string OpLog::insert_rga(uint64_t pos, const uint32_t* cps, size_t k) {
    if (pos > nvis_) return "insert position out of range";
    if (k == 0) return "";
    if ((uint64_t)size() + k >= 0x7FFFFFF0ull) return "op log too large";
    const uint32_t first = size() + 1;
    gb_reserve(2);  // (a split and a new span)
    gb_move(pos);
    // origin_left: the pos-th visible item, the last one before the gap
    const uint32_t left = pos ? gb_[g0_ - 1].id + gb_[g0_ - 1].len - 1u : 0u;
    const uint32_t right = nxt_[left];  // origin_right (tombstones included)
    // the new items follow left in the full list, before whatever followed it
    nxt_[left] = first;
    const size_t n0 = parent.size();
    if (k == 1) {  // typing: one item
        parent.push_back(left);
        oright.push_back(right);
        lamport.push_back(++max_lamport);
        agent.push_back(local_agent);
        deleted.push_back(0);
        cp.push_back(cps[0]);
        nxt_.push_back(right);
    } else {  // a paste: every column grown once, then filled
        parent.resize(n0 + k);
        oright.resize(n0 + k, right);
        lamport.resize(n0 + k);
        agent.resize(n0 + k, local_agent);
        deleted.resize(n0 + k, 0);
        cp.resize(n0 + k);
        nxt_.resize(n0 + 1 + k);
        uint32_t* P = parent.data() + n0;
        uint32_t* L = lamport.data() + n0;
        uint32_t* N = nxt_.data() + n0 + 1;
        P[0] = left;
        for (size_t j = 1; j < k; ++j) P[j] = first + (uint32_t)j - 1;
        for (size_t j = 0; j < k; ++j) {
            L[j] = max_lamport + 1 + (uint32_t)j;
            N[j] = first + (uint32_t)j + 1;
        }
        N[k - 1] = right;
        max_lamport += (uint32_t)k;
        std::memcpy(cp.data() + n0, cps, k * sizeof(uint32_t));
    }
    if (g0_ && gb_[g0_ - 1].id + gb_[g0_ - 1].len == first)
        gb_[g0_ - 1].len += (uint32_t)k;  // typing on: the span before the gap grows
    else
        gb_[g0_++] = GSpan{first, (uint32_t)k};
    gvis_ += k;
    nvis_ += k;
    return "";
}

std::string OpLog::remove_rga(uint64_t start, uint64_t end) {
    if (end < start || end > nvis_) return "remove range out of range";
    uint64_t left = end - start;
    if (!left) return "";
    gb_reserve(1);
    gb_move(start);
    nvis_ -= left;
    while (left) {  // the visible items right of the gap, span by span
        GSpan& sp = gb_[g1_];
        const uint32_t take = (uint32_t)std::min<uint64_t>(left, sp.len);
        const size_t m0 = del_ops.size();
        del_ops.resize(m0 + take);
        uint32_t* D = del_ops.data() + m0;
        for (uint32_t j = 0; j < take; ++j) D[j] = sp.id + j;
        std::memset(deleted.data() + sp.id - 1, 1, take);
        if (take == sp.len) {
            ++g1_;
        } else {
            sp.id += take;
            sp.len -= take;
        }
        left -= take;
    }
    return "";
}

// The resolver's hot loop for RGA logs (the upstream closure, main.rs:28-36).  The same steps as
// remove_rga + insert_rga, fused: every column is sized once to the trace's bound and written by
// index (no per-item push_back), a one-byte insert (typing) and a one-codepoint delete
// (backspace) take straight-line paths, and no std::string is made per patch.
std::string OpLog::replay(const Patch* pt, size_t np, const char* ins, size_t ins_total) {
    if (fugue || stale_) {
        for (size_t i = 0; i < np; ++i) {
            const Patch& q = pt[i];
            std::string e;
            if (q.del) e = remove(q.pos, q.pos + q.del);
            if (e.empty() && q.ins_len) e = insert_utf8(q.pos, ins + q.ins_off, q.ins_len);
            if (!e.empty()) return e;
        }
        return "";
    }
    // bounds without a pass over the patches: items <= the inserted bytes, and every item is
    // deleted at most once (the columns are default-initialised: the slack costs no writes)
    size_t n = parent.size(), m = del_ops.size();
    const size_t ib = ins_total, db = n + ib;
    if ((uint64_t)n + ib >= 0x7FFFFFF0ull) return "op log too large";
    parent.resize(n + ib);
    oright.resize(n + ib);
    lamport.resize(n + ib);
    agent.resize(n + ib);
    deleted.resize(n + ib);
    cp.resize(n + ib);
    nxt_.resize(n + 1 + ib);
    del_ops.resize(m + db);
    uint32_t *P = parent.data(), *O = oright.data(), *L = lamport.data(), *C = cp.data();
    uint16_t* A = agent.data();
    uint8_t* Dl = deleted.data();
    uint32_t *N = nxt_.data(), *Do = del_ops.data();
    // the gap buffer's state and the counters in locals for the whole loop (the byte stores to
    // the deleted column may alias any member, which would reload them after every store)
    // (a patch adds at most three spans: a split at its delete, a split at its insert and the
    // new span; the gap buffer is default-initialised, so the room costs no writes)
    gb_reserve(3 * np + 64);
    GSpan* G = gb_.data();
    size_t g0 = g0_, g1 = g1_;
    uint64_t gvis = gvis_, nvis = nvis_;
    uint32_t maxl = max_lamport;
    const uint16_t agent0 = local_agent;
    // the gap to visible position pos (gb_move on the locals)
    auto move_to = [&](uint64_t pos) {
        while (gvis > pos) {
            GSpan& sp = G[g0 - 1];
            if (gvis - sp.len >= pos) {
                G[--g1] = sp;
                --g0;
                gvis -= sp.len;
            } else {  // split: the part after pos goes right of the gap
                const uint32_t o = (uint32_t)(pos - (gvis - sp.len));
                G[--g1] = GSpan{sp.id + o, sp.len - o};
                sp.len = o;
                gvis = pos;
            }
        }
        while (gvis < pos) {
            GSpan& sp = G[g1];
            if (gvis + sp.len <= pos) {
                G[g0++] = sp;
                ++g1;
                gvis += sp.len;
            } else {
                const uint32_t o = (uint32_t)(pos - gvis);
                G[g0++] = GSpan{sp.id, o};
                sp.id += o;
                sp.len -= o;
                gvis = pos;
            }
        }
    };
    const char* err = nullptr;
    for (size_t i = 0; i < np && !err; ++i) {
        const uint64_t pos = pt[i].pos, del = pt[i].del, ioff = pt[i].ins_off, ilen = pt[i].ins_len;
        if (del) {  // (remove_rga)
            if (pos + del > nvis) {
                err = "remove range out of range";
                break;
            }
            move_to(pos);
            nvis -= del;
            uint64_t left = del;
            while (left) {
                GSpan& sp = G[g1];
                const uint32_t take = (uint32_t)std::min<uint64_t>(left, sp.len);
                for (uint32_t j = 0; j < take; ++j) Do[m + j] = sp.id + j;
                m += take;
                std::memset(Dl + sp.id - 1, 1, take);
                if (take == sp.len) {
                    ++g1;
                } else {
                    sp.id += take;
                    sp.len -= take;
                }
                left -= take;
            }
        }
        if (!ilen) continue;
        // (insert_rga) the codepoints: one ASCII byte while typing, else decoded
        const unsigned char* s8 = reinterpret_cast<const unsigned char*>(ins + ioff);
        uint32_t c1;
        const uint32_t* cps;
        size_t k;
        if (ilen == 1 && s8[0] < 0x80u) {
            c1 = s8[0];
            cps = &c1;
            k = 1;
        } else {
            cps_.clear();
            if (!utf8_decode(reinterpret_cast<const char*>(s8), ilen, cps_)) {
                err = "invalid UTF-8";
                break;
            }
            cps = cps_.data();
            k = cps_.size();
        }
        if (pos > nvis) {
            err = "insert position out of range";
            break;
        }
        const uint32_t first = (uint32_t)n + 1;
        move_to(pos);
        const uint32_t lft = pos ? G[g0 - 1].id + G[g0 - 1].len - 1u : 0u;
        const uint32_t rgt = N[lft];
        N[lft] = first;
        if (k == 1) {  // (typing)
            P[n] = lft;
            O[n] = rgt;
            L[n] = maxl + 1u;
            A[n] = agent0;
            Dl[n] = 0;
            C[n] = cps[0];
        } else {  // (a paste: column by column, each loop vectorises)
            P[n] = lft;
            for (size_t j = 1; j < k; ++j) P[n + j] = first + (uint32_t)j - 1u;
            std::fill(O + n, O + n + k, rgt);
            for (size_t j = 0; j < k; ++j) L[n + j] = maxl + 1u + (uint32_t)j;
            std::fill(A + n, A + n + k, agent0);
            std::memset(Dl + n, 0, k);
            std::memcpy(C + n, cps, k * sizeof(uint32_t));
            for (size_t j = 0; j + 1 < k; ++j) N[n + 1 + j] = first + (uint32_t)j + 1u;
        }
        N[n + k] = rgt;
        maxl += (uint32_t)k;
        n += k;
        if (g0 && G[g0 - 1].id + G[g0 - 1].len == first)
            G[g0 - 1].len += (uint32_t)k;  // typing on: the span before the gap grows
        else
            G[g0++] = GSpan{first, (uint32_t)k};
        gvis += k;
        nvis += k;
    }
    g0_ = g0;
    g1_ = g1;
    gvis_ = gvis;
    nvis_ = nvis;
    max_lamport = maxl;
    parent.resize(n);
    oright.resize(n);
    lamport.resize(n);
    agent.resize(n);
    deleted.resize(n);
    cp.resize(n);
    nxt_.resize(n + 1);
    del_ops.resize(m);
    return err ? std::string(err) : std::string();
}

// The gap buffer and the successors from the full document order (ids, tombstones included).
std::string OpLog::rebuild_index_rga(const std::vector<uint32_t>& order) {
    nxt_.assign((size_t)size() + 1, NIL);
    gb_.assign(1024, GSpan{0, 0});
    g0_ = 0;
    g1_ = gb_.size();
    uint32_t prev = 0;
    uint64_t v = 0;
    for (uint32_t id : order) {
        nxt_[prev] = id;
        prev = id;
        if (deleted[id - 1]) continue;
        ++v;
        if (g0_ && gb_[g0_ - 1].id + gb_[g0_ - 1].len == id) {
            gb_[g0_ - 1].len++;
        } else {
            gb_reserve(1);
            gb_[g0_++] = GSpan{id, 1};
        }
    }
    gvis_ = v;
    nvis_ = v;
    stale_ = false;
    return "";
}

std::string OpLog::insert_utf8(uint64_t pos, const char* s, size_t nbytes) {
    if (nbytes == 1 && (unsigned char)s[0] < 0x80u) {  // typing one ASCII character
        const uint32_t c = (unsigned char)s[0];
        return insert(pos, &c, 1);
    }
    cps_.clear();
    if (!utf8_decode(s, nbytes, cps_)) return "invalid UTF-8";
    return insert(pos, cps_.data(), cps_.size());
}

// Tombstone items [off, off+take) of visible span si; merges the tombstone span with deleted
// neighbours whose ids continue it.  Returns the index of the span after the tombstones.
size_t OpLog::delete_in_span(Chunk& ch, size_t si, uint32_t off, uint32_t take) {
    std::vector<Span>& v = ch.s;
    const Span S = v[si];
    const uint32_t len = S.len(), did = S.id + off, dend = did + take;
    if (take == 1) {  // backspace
        deleted[did - 1] = 1;
        del_ops.push_back(did);
    } else {
        std::memset(deleted.data() + did - 1, 1, take);
        const size_t m0 = del_ops.size();
        del_ops.resize(m0 + take);
        for (uint32_t j = 0; j < take; ++j) del_ops[m0 + j] = did + j;
    }
    Span rep[3];
    int nr = 0;
    if (off) rep[nr++] = Span{S.id, off};
    size_t mid = si + nr;
    rep[nr++] = Span{did, take | 0x80000000u};
    const bool tail = off + take < len;
    if (tail) rep[nr++] = Span{dend, len - off - take};
    v[si] = rep[0];
    if (nr > 1) v.insert(v.begin() + si + 1, rep + 1, rep + nr);
    if (!tail && mid + 1 < v.size() && v[mid + 1].del() && v[mid + 1].id == dend) {
        v[mid].n += v[mid + 1].len();
        v.erase(v.begin() + mid + 1);
    }
    if (mid > 0 && v[mid - 1].del() && v[mid - 1].id + v[mid - 1].len() == did) {
        v[mid - 1].n += v[mid].len();
        v.erase(v.begin() + mid);
        --mid;
    }
    return mid + 1;
}

std::string OpLog::remove(uint64_t start, uint64_t end) {
    if (stale_) {
        std::string e = rebuild_index();
        if (!e.empty()) return e;
    }
    if (!fugue) return remove_rga(start, end);
    if (end < start || end > nvis_) return "remove range out of range";
    uint64_t left = end - start;
    if (!left) return "";
    size_t c, si;
    uint32_t off;
    if (!find_visible(start + 1, c, si, off)) return "resolver index corrupt";
    const size_t c0 = c;
    while (left) {
        Chunk& ch = chunks_[c];
        if (si >= ch.s.size()) {
            if (++c >= chunks_.size()) return "resolver index corrupt";
            si = 0;
            off = 0;
            continue;
        }
        if (ch.s[si].del()) {
            ++si;
            off = 0;
            continue;
        }
        uint32_t take = ch.s[si].len() - off;
        if (take > left) take = (uint32_t)left;
        si = delete_in_span(ch, si, off, take);
        off = 0;
        ch.vis -= take;
        fen_add(c, -(int64_t)take);
        left -= take;
    }
    nvis_ -= end - start;
    for (size_t cc = c + 1; cc-- > c0;) split_chunk(cc);
    return "";
}

void OpLog::push_item(uint32_t par, uint32_t orr, uint32_t lam, uint16_t ag, uint8_t del,
                      uint32_t c, uint8_t sd) {
    if (fugue) side.push_back(sd);
    parent.push_back(par);
    oright.push_back(orr);
    lamport.push_back(lam);
    agent.push_back(ag);
    deleted.push_back(del);
    cp.push_back(c);
    if (lam > max_lamport) max_lamport = lam;
    nvis_ += !del;
    stale_ = true;
}

void OpLog::mark_deleted(uint32_t id) {
    if (id == 0 || id > size() || deleted[id - 1]) return;
    deleted[id - 1] = 1;
    nvis_--;
    stale_ = true;
}

// Rebuild the positional index from the op log itself (RGA document order) after remote
// items arrived.  Host resolver bookkeeping only: merged documents always come from the device.
std::string OpLog::rebuild_index() {
    if (fugue) return rebuild_index_fugue();
    std::vector<uint32_t> order;
    std::string e = order_rga(order);
    if (!e.empty()) return e;
    return rebuild_index_rga(order);
}

// The RGA pre-order of every item (tombstones included), from the log alone.
std::string OpLog::order_rga(std::vector<uint32_t>& order) const {
    uint32_t n = size();
    std::vector<uint32_t> start(n + 2, 0), kids(n);
    for (uint32_t i = 1; i <= n; ++i) {
        uint32_t p = parent[i - 1];
        if (p > n || p == i) return "malformed op log (parent out of range)";
        start[p + 1]++;
    }
    for (uint32_t v = 0; v <= n; ++v) start[v + 1] += start[v];
    {
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (uint32_t i = 1; i <= n; ++i) kids[fill[parent[i - 1]]++] = i;
    }
    auto newer = [&](uint32_t a, uint32_t b) {  // a sorts before b (greater timestamp first)
        if (lamport[a - 1] != lamport[b - 1]) return lamport[a - 1] > lamport[b - 1];
        return agent[a - 1] > agent[b - 1];
    };
    order.clear();
    order.reserve(n);
    std::vector<uint32_t> stack;
    stack.reserve(n + 1);
    stack.push_back(0);
    while (!stack.empty()) {
        uint32_t v = stack.back();
        stack.pop_back();
        if (v) order.push_back(v);
        uint32_t a = start[v], b = start[v + 1];
        std::sort(kids.begin() + a, kids.begin() + b, [&](uint32_t x, uint32_t y) { return newer(y, x); });
        for (uint32_t j = a; j < b; ++j) stack.push_back(kids[j]);  // oldest pushed first
    }
    if (order.size() != n) return "malformed op log (cycle)";
    return "";
}

// Appends item v to the end of the rebuilt sequence.
void OpLog::index_append(uint32_t v) {
    const bool del = deleted[v - 1] != 0;
    Chunk* ch = &chunks_.back();
    Span* last = ch->s.empty() ? nullptr : &ch->s.back();
    if (last && last->del() == del && last->id + last->len() == v) {
        last->n++;
    } else {
        if (ch->s.size() >= kSpanMax / 2) {
            chunks_.push_back(new_chunk());
            ch = &chunks_.back();
        }
        ch->s.push_back(Span{v, 1u | (del ? 0x80000000u : 0u)});
    }
    if (!del) { ch->vis++; nvis_++; }
}

// The Fugue in-order (left children by timestamp descending, the item, then its right children
// by timestamp descending), as orc_merge_fugue (oracle/oracle.c) walks it; also recomputes
// hasright_ with the remote right children.
std::string OpLog::rebuild_index_fugue() {
    const uint32_t n = size();
    std::vector<uint32_t> order;
    std::string e = order_fugue(order);
    if (!e.empty()) return e;
    hasright_.assign(std::max<size_t>(hasright_.size(), (size_t)n + 1), 0);
    for (uint32_t i = 1; i <= n; ++i)
        if (!side[i - 1]) hasright_[parent[i - 1]] = 1;
    chunks_.clear();
    chunks_.push_back(new_chunk());
    nvis_ = 0;
    hint_c_ = SIZE_MAX;
    hint_si_ = SIZE_MAX;
    for (uint32_t id : order) index_append(id);
    fen_build();
    stale_ = false;
    return "";
}

// The Fugue in-order of every item (tombstones included), from the log alone.
std::string OpLog::order_fugue(std::vector<uint32_t>& order) const {
    const uint32_t n = size();
    if (side.size() != n) return "malformed op log (side column)";
    std::vector<uint32_t> start(2ull * n + 3, 0), kids(n);  // groups 2v (left), 2v + 1 (right)
    for (uint32_t i = 1; i <= n; ++i) {
        const uint32_t p = parent[i - 1];
        if (p > n || p == i || (p == 0 && side[i - 1])) return "malformed op log (parent out of range)";
        start[2ull * p + (side[i - 1] ? 0 : 1) + 1]++;
    }
    for (uint64_t g = 0; g < 2ull * n + 2; ++g) start[g + 1] += start[g];
    {
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (uint32_t i = 1; i <= n; ++i) kids[fill[2ull * parent[i - 1] + (side[i - 1] ? 0 : 1)]++] = i;
    }
    auto older = [&](uint32_t a, uint32_t b) {  // a has the smaller timestamp
        if (lamport[a - 1] != lamport[b - 1]) return lamport[a - 1] < lamport[b - 1];
        return agent[a - 1] < agent[b - 1];
    };
    order.clear();
    order.reserve(n);
    constexpr uint32_t EMIT = 0x80000000u;
    std::vector<uint32_t> stack;
    stack.reserve(2ull * n + 2);
    stack.push_back(0);
    while (!stack.empty()) {
        const uint32_t e = stack.back();
        stack.pop_back();
        if (e & EMIT) {
            order.push_back(e & ~EMIT);
            continue;
        }
        // pushed in reverse of the walk: right children, e, left children (each oldest first)
        const uint32_t l0 = start[2ull * e], l1 = start[2ull * e + 1], r1 = start[2ull * e + 2];
        std::sort(kids.begin() + l0, kids.begin() + l1, older);
        std::sort(kids.begin() + l1, kids.begin() + r1, older);
        for (uint32_t j = l1; j < r1; ++j) stack.push_back(kids[j]);
        if (e) stack.push_back(e | EMIT);
        for (uint32_t j = l0; j < l1; ++j) stack.push_back(kids[j]);
    }
    if (order.size() != n) return "malformed op log (cycle)";
    return "";
}

std::string OpLog::document_order(std::vector<uint32_t>& order) const {
    return fugue ? order_fugue(order) : order_rga(order);
}

LogMark OpLog::mark() const {
    LogMark m;
    m.n = size();
    m.deleted.assign(deleted.begin(), deleted.end());
    return m;
}

// ---- what the views below share, each rule once (`order`: the log's document_order) -------------
namespace {
// A version of the log: now (m null) or at a mark.  The host counterparts of mark_fits
// (replica.hpp) and of SelNow / SelMark (order.hpp).
int mark_check(const OpLog& log, const LogMark* m, std::string& err) {
    if (m && (log.size() < m->n || m->deleted.size() != m->n)) {
        err = "the log holds fewer items than the mark";
        return CRDT_HIP_EINVAL;
    }
    return CRDT_HIP_OK;
}
bool in_version(const OpLog& log, const LogMark* m, uint32_t id) {
    return m ? id <= m->n && !m->deleted[id - 1] : !log.deleted[id - 1];
}

// ends[v]: UTF-8 bytes of the first v visible items of `ids` (the order, or its visible items), the
// only byte offsets that lie inside no codepoint; byte_rank: the v with ends[v] == b, or false.
std::vector<uint64_t> byte_ends(const OpLog& log, const std::vector<uint32_t>& ids) {
    std::vector<uint64_t> ends;
    ends.reserve((size_t)log.visible() + 1);
    ends.push_back(0);
    for (uint32_t id : ids)
        if (!log.deleted[id - 1]) ends.push_back(ends.back() + utf8_len_cp(log.cp[id - 1]));
    return ends;
}
bool byte_rank(const std::vector<uint64_t>& ends, uint64_t b, uint64_t& v) {
    const auto it = std::lower_bound(ends.begin(), ends.end(), b);
    if (it == ends.end() || *it != b) return false;
    v = (uint64_t)(it - ends.begin());
    return true;
}

constexpr uint32_t kNoGap = ~0u;
// The identities a call's anchors name and where the log holds them (locate.hpp on the device).
struct Located {
    std::vector<uint64_t> want;  // the identities asked for; find() leaves them sorted and distinct
    std::vector<uint32_t> rank;  // per identity the rank, 1-based, of the slot that holds it (0: none)
    void ask(const AnchorRec& a) {
        if (a.id != kAnchorEdge) want.push_back(a.id);
    }
    size_t index(uint64_t ident) const {  // of an identity in `want`, or where it would be
        return (size_t)(std::lower_bound(want.begin(), want.end(), ident) - want.begin());
    }
    // One scan of the log; of two slots of a malformed log that share an identity, the lower wins.
    void find(const OpLog& log, const std::vector<uint32_t>& order) {
        std::sort(want.begin(), want.end());
        want.erase(std::unique(want.begin(), want.end()), want.end());
        rank.assign(want.size(), 0u);
        if (want.empty()) return;
        const uint32_t n = log.size();
        Column<uint32_t> rk(n + 1ull);  // slot -> rank (the order names every slot)
        for (uint32_t k = 0; k < n; ++k) rk[order[k]] = k + 1;
        for (uint32_t id = 1; id <= n; ++id) {  // (in slot order: the identities mostly ascend)
            const uint64_t ident = log.ident(id);
            const size_t j = index(ident);
            if (j < want.size() && want[j] == ident && !rank[j]) rank[j] = rk[id];
        }
    }
    // The gap an anchor names among the n items in document order (gap g lies right after rank g,
    // gap 0 at the document start), or kNoGap: no item holds its identity.
    uint32_t gap(const AnchorRec& a, uint32_t n) const {
        if (a.id == kAnchorEdge) return a.bias == kAnchorAfter ? 0u : n;
        const uint32_t r = rank[index(a.id)];
        return !r ? kNoGap : a.bias == kAnchorAfter ? r : r - 1;
    }
};

// The visible codepoints and their UTF-8 bytes before each of `gaps`, which leave sorted and
// distinct (view_walk, view.hpp, on the device).
void visible_before(const OpLog& log, const std::vector<uint32_t>& order, std::vector<uint32_t>& gaps,
                    std::vector<uint64_t>& vis, std::vector<uint64_t>& visb) {
    std::sort(gaps.begin(), gaps.end());
    gaps.erase(std::unique(gaps.begin(), gaps.end()), gaps.end());
    vis.resize(gaps.size());
    visb.resize(gaps.size());
    uint64_t v = 0, vb = 0;
    size_t j = 0;
    for (uint32_t k = 0; k <= order.size() && j < gaps.size(); ++k) {
        if (k && !log.deleted[order[k - 1] - 1]) {
            ++v;
            vb += utf8_len_cp(log.cp[order[k - 1] - 1]);
        }
        if (gaps[j] == k) {
            vis[j] = v;
            visb[j] = vb;
            ++j;
        }
    }
}
}  // namespace

int OpLog::patches_since(const LogMark& m, std::vector<PatchRec>& out, std::vector<uint8_t>& ins,
                         std::string& err) const {
    return patches_walk(m, false, out, ins, err);
}
int OpLog::patches_since_bytes(const LogMark& m, std::vector<PatchRec>& out,
                               std::vector<uint8_t>& ins, std::string& err) const {
    return patches_walk(m, true, out, ins, err);
}

// The one walk behind both: an item weighs 1 (codepoints) or its UTF-8 length (bytes) in pos and
// del; ins, ins_off and ins_len are bytes either way.
int OpLog::patches_walk(const LogMark& m, bool bytes, std::vector<PatchRec>& out,
                        std::vector<uint8_t>& ins, std::string& err) const {
    out.clear();
    ins.clear();
    if (int rc = mark_check(*this, &m, err)) return rc;
    std::vector<uint32_t> order;
    err = document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    uint64_t pos = 0;   // `now` items (or their bytes) so far
    uint64_t del = 0;   // what the open run deletes
    bool open = false;  // the previous K, D or I item was a D or an I: its run goes on
    for (uint32_t id : order) {
        const bool was = in_version(*this, &m, id), now = in_version(*this, nullptr, id);
        if (!was && !now) continue;
        const uint64_t w = bytes ? utf8_len_cp(cp[id - 1]) : 1;
        if (was && now) {
            pos += w;
            open = false;
            continue;
        }
        if (!open) {
            out.push_back(PatchRec{pos, (uint64_t)ins.size(), 0u, 0u});
            open = true;
            del = 0;
        }
        if (was) {
            del += w;
            if (del >= (1ull << 32)) {  // (bytes only: a log holds fewer than 2^31 items)
                err = "a patch deletes 4 GiB or more";
                return CRDT_HIP_ERANGE;
            }
            out.back().del = (uint32_t)del;
        } else {
            char b[4];
            const size_t k = utf8_put(cp[id - 1], b);
            ins.insert(ins.end(), b, b + k);
            out.back().ins_len += (uint32_t)k;
            pos += bytes ? k : 1;
            if (ins.size() >= (1ull << 32)) {
                err = "4 GiB or more of inserted bytes";
                return CRDT_HIP_ERANGE;
            }
        }
    }
    return CRDT_HIP_OK;
}

// ---- text windows ------------------------------------------------------------------------------
int text_check(uint64_t start, uint64_t end, uint32_t flags, const size_t* out_len, std::string& err) {
    if (flags & ~kTextBytes) {
        err = "text flags are neither 0 nor BYTES";
        return CRDT_HIP_EINVAL;
    }
    if (!out_len) {
        err = "null out_len";
        return CRDT_HIP_EINVAL;
    }
    if (end != kTextEnd && start > end) {
        err = "text window starts after its end";
        return CRDT_HIP_EINVAL;
    }
    return CRDT_HIP_OK;
}

int text_check_window(uint64_t start, uint64_t end, uint64_t total, bool inside, const TextInfo& w,
                      const uint8_t* out, size_t cap, size_t* out_len, TextInfo* info, std::string& err) {
    if (start > total || end > total) {
        err = "text window beyond the version";
        return CRDT_HIP_ERANGE;
    }
    if (inside) {
        err = "text window boundary inside a codepoint";
        return CRDT_HIP_EINVAL;
    }
    if (w.n_bytes >= (1ull << 32)) {
        err = "a text window of 4 GiB or more";
        return CRDT_HIP_ERANGE;
    }
    *out_len = (size_t)w.n_bytes;
    if (info) *info = w;
    if (w.n_bytes && (!out || cap < w.n_bytes)) {
        err = "buffer too small";
        return CRDT_HIP_ESPACE;
    }
    return CRDT_HIP_OK;
}

int OpLog::text_at(const LogMark* m, uint64_t start, uint64_t end, uint32_t flags, uint8_t* out,
                   size_t cap, size_t* out_len, TextInfo* info, std::string& err) const {
    if (int rc = mark_check(*this, m, err)) return rc;
    int rc = text_check(start, end, flags, out_len, err);
    if (rc) return rc;
    const bool bytes = (flags & kTextBytes) != 0;
    std::vector<uint32_t> order;
    err = document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    // one walk: the totals, and each boundary where the unit's running count meets it (a gap
    // between two selected items, the start or the end of the version)
    TextInfo w{};
    uint64_t c = 0, b = 0, end_c = 0, end_b = 0;
    bool got_start = false, got_end = false;
    auto gap = [&]() {
        const uint64_t p = bytes ? b : c;
        if (!got_start && p == start) {
            got_start = true;
            w.start = c;
            w.start_bytes = b;
        }
        if (!got_end && p == end) {
            got_end = true;
            end_c = c;
            end_b = b;
        }
    };
    for (uint32_t id : order) {
        if (!in_version(*this, m, id)) continue;
        gap();
        ++c;
        b += utf8_len_cp(cp[id - 1]);
    }
    if (end == kTextEnd) end = bytes ? b : c;
    gap();
    w.len = c;
    w.len_bytes = b;
    w.n = end_c - w.start;
    w.n_bytes = end_b - w.start_bytes;
    rc = text_check_window(start, end, bytes ? b : c, !got_start || !got_end, w, out, cap, out_len,
                           info, err);
    if (rc || w.n_bytes == 0) return rc;
    uint64_t k = 0;  // selected items so far
    uint8_t* o = out;
    for (uint32_t id : order) {
        if (!in_version(*this, m, id)) continue;
        if (k >= w.start + w.n) break;
        if (k++ < w.start) continue;
        o += utf8_put(cp[id - 1], reinterpret_cast<char*>(o));
    }
    return CRDT_HIP_OK;
}

// ---- the line index ----------------------------------------------------------------------------
int line_check(const uint64_t* in, size_t n, uint32_t flags, const LinePos* out, std::string& err) {
    if (flags & ~kTextBytes) {
        err = "line flags are neither 0 nor BYTES";
        return CRDT_HIP_EINVAL;
    }
    if (n && (!in || !out)) {
        err = "null argument";
        return CRDT_HIP_EINVAL;
    }
    if (n >= (1ull << 31)) {
        err = "2^31 or more line queries";
        return CRDT_HIP_ERANGE;
    }
    return CRDT_HIP_OK;
}

int line_check_version(bool lines, bool beyond, bool inside, std::string& err) {
    if (beyond) {
        err = lines ? "line number beyond the version" : "line position beyond the version";
        return CRDT_HIP_ERANGE;
    }
    if (inside) {
        err = "line position inside a codepoint";
        return CRDT_HIP_EINVAL;
    }
    return CRDT_HIP_OK;
}

namespace {
// A version's line index: ends[v] the UTF-8 bytes of its first v items (byte_ends, under the
// version's selector), and per line k = 0..L its start in items; the entry L + 1 is the end.
struct LineIndex {
    std::vector<uint64_t> ends, starts;
    LineInfo info{};
};
int line_index(const OpLog& log, const LogMark* m, LineIndex& x, std::string& err) {
    std::vector<uint32_t> order;
    err = log.document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    x.ends.assign(1, 0);
    x.starts.assign(1, 0);
    for (uint32_t id : order) {
        if (!in_version(log, m, id)) continue;
        x.ends.push_back(x.ends.back() + utf8_len_cp(log.cp[id - 1]));
        if (log.cp[id - 1] == kLineBreak) x.starts.push_back(x.ends.size() - 1);
    }
    x.info = LineInfo{(uint64_t)x.starts.size(), (uint64_t)x.ends.size() - 1, x.ends.back()};
    x.starts.push_back(x.info.len);
    return CRDT_HIP_OK;
}
}  // namespace

int OpLog::line_starts(const LogMark* m, const uint64_t* lines, size_t n, LinePos* out, LineInfo* info,
                       std::string& err) const {
    if (int rc = mark_check(*this, m, err)) return rc;
    if (int rc = line_check(lines, n, 0, out, err)) return rc;
    LineIndex x;
    if (int rc = line_index(*this, m, x, err)) return rc;
    bool beyond = false;
    for (size_t k = 0; k < n; ++k) beyond |= lines[k] > x.info.lines;
    if (int rc = line_check_version(true, beyond, false, err)) return rc;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t s = x.starts[(size_t)lines[k]];
        out[k] = LinePos{lines[k], s, x.ends[(size_t)s], 0, 0};
    }
    if (info) *info = x.info;
    return CRDT_HIP_OK;
}

int OpLog::lines_of(const LogMark* m, const uint64_t* pos, size_t n, uint32_t flags, LinePos* out,
                    LineInfo* info, std::string& err) const {
    if (int rc = mark_check(*this, m, err)) return rc;
    if (int rc = line_check(pos, n, flags, out, err)) return rc;
    const bool bytes = (flags & kTextBytes) != 0;
    LineIndex x;
    if (int rc = line_index(*this, m, x, err)) return rc;
    const uint64_t total = bytes ? x.info.len_bytes : x.info.len;
    bool beyond = false, inside = false;
    for (size_t k = 0; k < n; ++k) beyond |= pos[k] > total;
    std::vector<uint64_t> gap(n);  // items before each position
    for (size_t k = 0; k < n && !beyond; ++k) {
        gap[k] = pos[k];
        if (bytes && !byte_rank(x.ends, pos[k], gap[k])) inside = true;
    }
    if (int rc = line_check_version(false, beyond, inside, err)) return rc;
    for (size_t k = 0; k < n; ++k) {
        // the line: the last of lines 0..L that starts at or before the gap
        const size_t line =
            (size_t)(std::upper_bound(x.starts.begin(), x.starts.end() - 1, gap[k]) - x.starts.begin()) - 1;
        const uint64_t s = x.starts[line], sb = x.ends[(size_t)s];
        out[k] = LinePos{(uint64_t)line, s, sb, gap[k] - s, x.ends[(size_t)gap[k]] - sb};
    }
    if (info) *info = x.info;
    return CRDT_HIP_OK;
}

// ---- UTF-16 positions ----------------------------------------------------------------------------
int unit_check(const uint64_t* pos, size_t n, uint32_t unit, const UnitPos* out, std::string& err,
               uint64_t bound) {
    if (unit > kUnitUtf16) {
        err = "unit is neither CODEPOINTS, BYTES nor UTF16";
        return CRDT_HIP_EINVAL;
    }
    if (n && (!pos || !out)) {
        err = "null argument";
        return CRDT_HIP_EINVAL;
    }
    if (n >= bound) {
        err = "2^31 or more positions";
        return CRDT_HIP_ERANGE;
    }
    return CRDT_HIP_OK;
}

int unit_check_version(uint32_t unit, bool beyond, bool inside, std::string& err) {
    if (beyond) {
        err = "position beyond the version";
        return CRDT_HIP_ERANGE;
    }
    if (inside) {
        err = unit == kUnitUtf16 ? "position inside a surrogate pair" : "position inside a codepoint";
        return CRDT_HIP_EINVAL;
    }
    return CRDT_HIP_OK;
}

int OpLog::units_of(const LogMark* m, const uint64_t* pos, size_t n, uint32_t unit, UnitPos* out,
                    UnitInfo* info, std::string& err, uint64_t bound) const {
    if (int rc = mark_check(*this, m, err)) return rc;
    if (int rc = unit_check(pos, n, unit, out, err, bound)) return rc;
    std::vector<uint32_t> order;
    err = document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    // the one walk: per gap v (the first v selected items) its bytes and its UTF-16 code units
    std::vector<uint64_t> eb(1, 0), e16(1, 0);
    for (uint32_t id : order) {
        if (!in_version(*this, m, id)) continue;
        const uint32_t len = (uint32_t)utf8_len_cp(cp[id - 1]);
        eb.push_back(eb.back() + len);
        e16.push_back(e16.back() + utf16_units(len));
    }
    const UnitInfo total{(uint64_t)eb.size() - 1, eb.back(), e16.back()};
    const std::vector<uint64_t>* ends = unit == kUnitBytes ? &eb : unit == kUnitUtf16 ? &e16 : nullptr;
    const uint64_t len = ends ? ends->back() : total.len;
    bool beyond = false, inside = false;
    for (size_t k = 0; k < n; ++k) beyond |= pos[k] > len;
    std::vector<uint64_t> gap(n);  // items before each position
    for (size_t k = 0; k < n && !beyond; ++k) {
        gap[k] = pos[k];
        if (ends && !byte_rank(*ends, pos[k], gap[k])) inside = true;
    }
    if (int rc = unit_check_version(unit, beyond, inside, err)) return rc;
    for (size_t k = 0; k < n; ++k) out[k] = UnitPos{gap[k], eb[(size_t)gap[k]], e16[(size_t)gap[k]]};
    if (info) *info = total;
    return CRDT_HIP_OK;
}

// ---- anchors -----------------------------------------------------------------------------------
int anchor_check_at(const uint64_t* pos, const uint8_t* bias, size_t n, uint64_t visible,
                    std::string& err) {
    if (n >= (1ull << 31)) {
        err = "2^31 or more anchors";
        return CRDT_HIP_ERANGE;
    }
    for (size_t k = 0; k < n; ++k) {
        if (bias && bias[k] > kAnchorBefore) {
            err = "anchor bias is neither AFTER nor BEFORE";
            return CRDT_HIP_EINVAL;
        }
        if (pos[k] > visible) {
            err = "anchor position beyond the document";
            return CRDT_HIP_ERANGE;
        }
    }
    return CRDT_HIP_OK;
}

int anchor_check_resolve(const AnchorRec* a, size_t n, std::string& err) {
    if (n >= (1ull << 31)) {
        err = "2^31 or more anchors";
        return CRDT_HIP_ERANGE;
    }
    for (size_t k = 0; k < n; ++k) {
        if ((a[k].id >= kDeltaKeyEnd && a[k].id != kAnchorEdge) || a[k].bias > kAnchorBefore || a[k].pad) {
            err = "malformed anchor";
            return CRDT_HIP_EINVAL;
        }
    }
    return CRDT_HIP_OK;
}

int OpLog::anchors_at(const uint64_t* pos, const uint8_t* bias, size_t n, bool bytes, AnchorRec* out,
                      std::string& err) const {
    const int rc = anchor_check_at(pos, bias, n, bytes ? visible_bytes() : nvis_, err);
    if (rc || n == 0) return rc;
    std::vector<uint32_t> order;
    err = document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    std::vector<uint32_t> vis;  // vis[v - 1]: the v-th visible item
    vis.reserve((size_t)nvis_);
    for (uint32_t id : order)
        if (!deleted[id - 1]) vis.push_back(id);
    const std::vector<uint64_t> ends = bytes ? byte_ends(*this, vis) : std::vector<uint64_t>();
    std::vector<AnchorRec> res(n);
    for (size_t k = 0; k < n; ++k) {
        uint64_t v = pos[k];  // visible items before the gap
        if (bytes && !byte_rank(ends, pos[k], v)) {
            err = "anchor position inside a codepoint";
            return CRDT_HIP_EINVAL;
        }
        const uint32_t b = bias ? bias[k] : kAnchorAfter;
        const uint64_t item = b == kAnchorAfter ? v : v + 1;  // 1-based visible rank (0, len + 1: edge)
        if (item > vis.size() && b == kAnchorAfter) {  // (the log does not bear out its counter)
            err = "the visible items disagree with the log's counter";
            return CRDT_HIP_EBADLOG;
        }
        res[k] = AnchorRec{item == 0 || item > vis.size() ? kAnchorEdge : ident(vis[item - 1]), b, 0u};
    }
    std::memcpy(out, res.data(), n * sizeof(AnchorRec));
    return CRDT_HIP_OK;
}

int OpLog::anchors_resolve(const AnchorRec* a, size_t n, AnchorPosRec* out, std::string& err) const {
    const int rc = anchor_check_resolve(a, n, err);
    if (rc || n == 0) return rc;
    std::vector<uint32_t> order;
    err = document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    Located l;
    l.want.reserve(n);
    for (size_t k = 0; k < n; ++k) l.ask(a[k]);
    l.find(*this, order);
    std::vector<uint32_t> at(n), gaps;  // the gap each anchor names, and the gaps named
    for (size_t k = 0; k < n; ++k) {
        at[k] = l.gap(a[k], size());
        if (at[k] != kNoGap) gaps.push_back(at[k]);
    }
    std::vector<uint64_t> vis, visb;
    visible_before(*this, order, gaps, vis, visb);
    std::vector<AnchorPosRec> res(n);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t g = at[k];
        if (g == kNoGap) {
            res[k] = AnchorPosRec{0, 0, kAnchorUnknown, 0u};
            continue;
        }
        // (a dead item counts nothing: the gaps on either side of it lie at one position)
        const bool dead = a[k].id != kAnchorEdge && deleted[order[a[k].bias == kAnchorAfter ? g - 1 : g] - 1];
        const size_t j = (size_t)(std::lower_bound(gaps.begin(), gaps.end(), g) - gaps.begin());
        res[k] = AnchorPosRec{vis[j], visb[j], dead ? kAnchorDead : kAnchorLive, 0u};
    }
    std::memcpy(out, res.data(), n * sizeof(AnchorPosRec));
    return CRDT_HIP_OK;
}

// ---- formats -----------------------------------------------------------------------------------
int format_check(const FormatRec* f, size_t n, std::vector<uint32_t>& sorted, std::string& err) {
    sorted.clear();
    if (n > kFormatMax) {
        err = "more than 65,536 formats";
        return CRDT_HIP_ERANGE;
    }
    for (size_t k = 0; k < n; ++k) {
        const AnchorRec ends[2] = {f[k].start, f[k].end};
        const int rc = anchor_check_resolve(ends, 2, err);
        if (rc) return rc;
        if (f[k].op >= kDeltaKeyEnd) {
            err = "format op of 2^48 or more";
            return CRDT_HIP_EINVAL;
        }
        if (f[k].flags > kFormatRemove) {
            err = "format flags are neither 0 nor REMOVE";
            return CRDT_HIP_EINVAL;
        }
    }
    sorted.resize(n);
    for (size_t k = 0; k < n; ++k) sorted[k] = (uint32_t)k;
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return f[x].op < f[y].op; });
    for (size_t k = 1; k < n; ++k)
        if (f[sorted[k]].op == f[sorted[k - 1]].op) {
            sorted.clear();
            err = "two formats with the same op";
            return CRDT_HIP_EINVAL;
        }
    std::stable_sort(sorted.begin(), sorted.end(),
                     [&](uint32_t x, uint32_t y) { return f[x].key < f[y].key; });
    return CRDT_HIP_OK;
}

int OpLog::spans(const FormatRec* f, size_t n, std::vector<SpanRec>& out, std::vector<SpanAttrRec>& attrs,
                 uint64_t& pending, std::string& err) const {
    out.clear();
    attrs.clear();
    pending = 0;
    std::vector<uint32_t> by;  // the formats by (key, op)
    const int rc = format_check(f, n, by, err);
    if (rc || n == 0) return rc;
    std::vector<uint32_t> order;
    err = document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    const uint32_t N = size();
    Located l;
    l.want.reserve(2 * n);
    for (size_t k = 0; k < n; ++k) {
        l.ask(f[k].start);
        l.ask(f[k].end);
    }
    l.find(*this, order);
    // per format its two gaps (a format that covers nothing: 1, 0), and the gaps that bound a range
    std::vector<uint32_t> gs(n, 1u), ge(n, 0u), bound;
    for (size_t k = 0; k < n; ++k) {
        const uint32_t s = l.gap(f[k].start, N), e = l.gap(f[k].end, N);
        if (s == kNoGap || e == kNoGap) {
            ++pending;
        } else if (s < e) {
            gs[k] = s;
            ge[k] = e;
            bound.push_back(s);
            bound.push_back(e);
        }
    }
    std::vector<uint64_t> vis, visb;  // the visible codepoints and bytes before each boundary
    visible_before(*this, order, bound, vis, visb);
    // per segment between two boundaries that holds a visible item: its attribute set, compared
    // with the set of the segment with a visible item before it
    std::vector<SpanRec> sp;
    std::vector<SpanAttrRec> at, cur;
    bool open = false;  // the previous segment with a visible item had a set, which ends sp.back()
    for (size_t j = 0; j + 1 < bound.size(); ++j) {
        if (vis[j + 1] == vis[j]) continue;
        const uint32_t lo = bound[j], hi = bound[j + 1];
        cur.clear();
        for (size_t i = 0; i < n;) {
            const uint32_t key = f[by[i]].key;
            const FormatRec* win = nullptr;
            for (; i < n && f[by[i]].key == key; ++i)
                if (gs[by[i]] <= lo && hi <= ge[by[i]]) win = &f[by[i]];
            if (win && !(win->flags & kFormatRemove)) cur.push_back(SpanAttrRec{win->value, key, 0u});
        }
        if (cur.empty()) {
            open = false;
            continue;
        }
        bool same = open && sp.back().attr_n == cur.size();
        for (size_t q = 0; same && q < cur.size(); ++q) {
            const SpanAttrRec& p = at[sp.back().attr_off + q];
            same = p.key == cur[q].key && p.value == cur[q].value;
        }
        if (same) {
            sp.back().len = vis[j + 1] - sp.back().pos;
            sp.back().len_bytes = visb[j + 1] - sp.back().pos_bytes;
            continue;
        }
        if (at.size() + cur.size() >= (1ull << 32)) {
            err = "2^32 or more span attributes";
            return CRDT_HIP_ERANGE;
        }
        sp.push_back(SpanRec{vis[j], visb[j], vis[j + 1] - vis[j], visb[j + 1] - visb[j],
                             (uint32_t)at.size(), (uint32_t)cur.size()});
        at.insert(at.end(), cur.begin(), cur.end());
        open = true;
    }
    out.swap(sp);
    attrs.swap(at);
    return CRDT_HIP_OK;
}

// ---- local edits as positional patches ---------------------------------------------------------
// The argument-only checks of a patch array, in the UNIT of pos and del (kUnit*): `visible` and the
// non-touching rule are in that unit.  emit(old position, del, first codepoint, codepoints) per
// patch, the position in the document before the call.  In UTF-16 code units no length is known
// before the document is read: the range is left to the translation of the old positions, and the
// item bound to the codepoint call that follows it (crdt_hip_utf16.h).
namespace {
constexpr const char* kPatchBeyond = "patch range beyond the document";
template <uint32_t UNIT, class Emit>
int plan_walk(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len, uint64_t visible,
              uint64_t items, std::vector<uint32_t>& cps, std::string& err, Emit&& emit) {
    cps.clear();
    if (n >= (1ull << 31)) {
        err = "2^31 or more patches";
        return CRDT_HIP_ERANGE;
    }
    uint64_t len = visible;   // the document as the earlier patches left it
    uint64_t next_min = 0;    // pos[k] must exceed pos[k - 1] + what patch k - 1 inserted
    int64_t shift = 0;        // sum of (inserted - deleted) of the earlier patches
    for (size_t k = 0; k < n; ++k) {
        const PatchRec& r = p[k];
        if (r.del == 0 && r.ins_len == 0) {
            err = "empty patch";
            return CRDT_HIP_EINVAL;
        }
        if (r.ins_off > ins_len || r.ins_len > ins_len - r.ins_off || (r.ins_len && !ins)) {
            err = "patch text outside the ins buffer";
            return CRDT_HIP_EINVAL;
        }
        const size_t c0 = cps.size();
        if (r.ins_len && !utf8_decode(reinterpret_cast<const char*>(ins) + r.ins_off, r.ins_len, cps)) {
            err = "invalid UTF-8";
            return CRDT_HIP_EINVAL;
        }
        const uint64_t ncp = cps.size() - c0;
        uint64_t added = UNIT == kUnitBytes ? (uint64_t)r.ins_len : ncp;
        if (UNIT == kUnitUtf16)
            for (size_t c = c0; c < cps.size(); ++c) added += utf16_units(utf8_len_cp(cps[c])) - 1u;
        if (k && r.pos < next_min) {
            err = "patches are not ascending and non-touching";
            return CRDT_HIP_EINVAL;
        }
        if (UNIT != kUnitUtf16) {
            if (r.pos > len || r.del > len - r.pos) {
                err = kPatchBeyond;
                return CRDT_HIP_ERANGE;
            }
            if (items + cps.size() >= 0x7FFFFFF0ull) {
                err = "op log too large";
                return CRDT_HIP_ERANGE;
            }
        }
        emit((uint64_t)((int64_t)r.pos - shift), r.del, (uint32_t)c0, (uint32_t)ncp);
        len = len - r.del + added;
        shift += (int64_t)added - (int64_t)r.del;
        next_min = r.pos + added + 1;
    }
    return CRDT_HIP_OK;
}
}  // namespace

int edit_plan(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len, uint64_t visible,
              uint64_t items, EditPlan& plan, std::string& err) {
    plan.patch.clear();
    plan.ndel = 0;
    if (n < (1ull << 31)) plan.patch.reserve(n);
    return plan_walk<kUnitCodepoints>(p, n, ins, ins_len, visible, items, plan.cps, err,
                            [&](uint64_t old_pos, uint32_t del, uint32_t c0, uint32_t ncp) {
                                plan.patch.push_back(EditPatch{(uint32_t)old_pos, del, c0, ncp,
                                                               (uint32_t)plan.ndel, 0u});
                                plan.ndel += del;
                            });
}

int edit_plan_bytes(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                    uint64_t visible_bytes, uint64_t items, EditPlanBytes& plan, std::string& err) {
    plan.patch.clear();
    if (n < (1ull << 31)) plan.patch.reserve(n);
    return plan_walk<kUnitBytes>(p, n, ins, ins_len, visible_bytes, items, plan.cps, err,
                           [&](uint64_t old_pos_b, uint32_t del_b, uint32_t c0, uint32_t ncp) {
                               plan.patch.push_back(BytePatch{old_pos_b, del_b, c0, ncp});
                           });
}

uint64_t OpLog::visible_bytes() const {
    uint64_t b = 0;
    for (uint32_t k = 0; k < size(); ++k)
        if (!deleted[k]) b += utf8_len_cp(cp[k]);
    return b;
}

int OpLog::apply_patches_bytes(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                               uint32_t* added, uint32_t* tombstoned, std::string& err) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    if (n == 0) return CRDT_HIP_OK;
    EditPlanBytes plan;
    const int rc = edit_plan_bytes(p, n, ins, ins_len, visible_bytes(), size(), plan, err);
    if (rc) return rc;
    std::vector<uint32_t> order;
    err = document_order(order);
    if (!err.empty()) return CRDT_HIP_EBADLOG;
    const std::vector<uint64_t> ends = byte_ends(*this, order);  // the only offsets a patch may name
    std::vector<PatchRec> q(n);
    int64_t shift = 0;  // codepoints inserted - deleted by the earlier patches
    for (size_t k = 0; k < n; ++k) {
        const BytePatch& e = plan.patch[k];
        uint64_t v0, v1;
        if (!byte_rank(ends, e.old_pos_b, v0) || !byte_rank(ends, e.old_pos_b + e.del_b, v1)) {
            err = "patch boundary inside a codepoint";
            return CRDT_HIP_EINVAL;
        }
        q[k] = PatchRec{(uint64_t)((int64_t)v0 + shift), p[k].ins_off, (uint32_t)(v1 - v0), p[k].ins_len};
        shift += (int64_t)e.ncp - (int64_t)(v1 - v0);
    }
    return apply_patches(q.data(), n, ins, ins_len, added, tombstoned, err);
}

// ---- edits and patches in UTF-16 code units (crdt_hip_utf16.h) ---------------------------------
int edit_plan_utf16(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                    EditPlanUtf16& plan, std::string& err) {
    plan.bounds.clear();
    plan.ncp.clear();
    std::vector<uint32_t> cps;
    return plan_walk<kUnitUtf16>(p, n, ins, ins_len, 0, 0, cps, err,
                                 [&](uint64_t old_pos, uint32_t del, uint32_t, uint32_t ncp) {
                                     plan.bounds.push_back(old_pos);
                                     plan.bounds.push_back(old_pos + del);
                                     plan.ncp.push_back(ncp);
                                 });
}

int edit_patches_utf16(const EditPlanUtf16& plan, int rc_plan, const std::string& err_plan, int rc_units,
                       const PatchRec* p, size_t n, const UnitPos* tr, std::vector<PatchRec>& q,
                       std::string& err) {
    if (rc_units == CRDT_HIP_ERANGE) {
        err = kPatchBeyond;
        return rc_units;
    }
    if (rc_units && rc_units != CRDT_HIP_EINVAL) return rc_units;  // (the document could not be read)
    if (rc_plan) {
        err = err_plan;
        return rc_plan;
    }
    if (rc_units) {
        err = "patch boundary inside a surrogate pair";
        return rc_units;
    }
    q.resize(n);
    int64_t shift = 0;  // codepoints inserted - deleted by the earlier patches
    for (size_t k = 0; k < n; ++k) {
        const uint64_t v0 = tr[2 * k].cp, v1 = tr[2 * k + 1].cp;
        q[k] = PatchRec{(uint64_t)((int64_t)v0 + shift), p[k].ins_off, (uint32_t)(v1 - v0), p[k].ins_len};
        shift += (int64_t)plan.ncp[k] - (int64_t)(v1 - v0);
    }
    return CRDT_HIP_OK;
}

int OpLog::apply_patches_utf16(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                               uint32_t* added, uint32_t* tombstoned, std::string& err) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    if (n == 0) return CRDT_HIP_OK;
    EditPlanUtf16 plan;
    std::string err_plan;
    const int rc_plan = edit_plan_utf16(p, n, ins, ins_len, plan, err_plan);
    std::vector<UnitPos> tr(plan.bounds.size());
    const int rc_units = units_of(nullptr, plan.bounds.data(), plan.bounds.size(), kUnitUtf16, tr.data(),
                                  nullptr, err, 1ull << 32);
    std::vector<PatchRec> q;
    if (int rc = edit_patches_utf16(plan, rc_plan, err_plan, rc_units, p, n, tr.data(), q, err)) return rc;
    return apply_patches(q.data(), n, ins, ins_len, added, tombstoned, err);
}

namespace {
// The codepoints and the UTF-16 code units of a piece of valid UTF-8.
void utf8_units(const uint8_t* s, uint32_t len, uint64_t& ncp, uint64_t& n16) {
    ncp = n16 = 0;
    for (uint32_t i = 0; i < len; ++i) {
        ncp += (s[i] & 0xC0u) != 0x80u;
        n16 += (s[i] & 0xC0u) != 0x80u ? 1u + (s[i] >= 0xF0u) : 0u;
    }
}
}  // namespace

void since_bounds(const PatchRec* p, size_t n, const uint8_t* ins, std::vector<uint64_t>& bounds) {
    bounds.resize(2 * n);
    int64_t shift = 0;  // codepoints inserted - deleted by the earlier patches
    for (size_t k = 0; k < n; ++k) {
        uint64_t ncp = 0, n16 = 0;
        if (p[k].ins_len) utf8_units(ins + p[k].ins_off, p[k].ins_len, ncp, n16);
        bounds[2 * k] = (uint64_t)((int64_t)p[k].pos - shift);
        bounds[2 * k + 1] = bounds[2 * k] + p[k].del;
        shift += (int64_t)ncp - (int64_t)p[k].del;
    }
}

int since_utf16(PatchRec* p, size_t n, const uint8_t* ins, const UnitPos* tr, std::string& err) {
    for (size_t k = 0; k < n; ++k) {
        if (tr[2 * k + 1].utf16 - tr[2 * k].utf16 >= (1ull << 32)) {
            err = "a patch deletes 2^32 or more UTF-16 code units";
            return CRDT_HIP_ERANGE;
        }
    }
    int64_t shift = 0;  // UTF-16 code units inserted - deleted by the earlier patches
    for (size_t k = 0; k < n; ++k) {
        uint64_t ncp = 0, n16 = 0;
        if (p[k].ins_len) utf8_units(ins + p[k].ins_off, p[k].ins_len, ncp, n16);
        const uint64_t a = tr[2 * k].utf16, del = tr[2 * k + 1].utf16 - a;
        p[k].pos = (uint64_t)((int64_t)a + shift);
        p[k].del = (uint32_t)del;
        shift += (int64_t)n16 - (int64_t)del;
    }
    return CRDT_HIP_OK;
}

int OpLog::patches_since_utf16(const LogMark& m, std::vector<PatchRec>& out, std::vector<uint8_t>& ins,
                               std::string& err) const {
    if (int rc = patches_since(m, out, ins, err)) return rc;
    std::vector<uint64_t> bounds;
    since_bounds(out.data(), out.size(), ins.data(), bounds);
    std::vector<UnitPos> tr(bounds.size());
    if (int rc = units_of(&m, bounds.data(), bounds.size(), kUnitCodepoints, tr.data(), nullptr, err,
                          1ull << 32))
        return rc == CRDT_HIP_ERANGE || rc == CRDT_HIP_EINVAL ? CRDT_HIP_EBADLOG : rc;
    return since_utf16(out.data(), out.size(), ins.data(), tr.data(), err);
}

int OpLog::apply_patches(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                         uint32_t* added, uint32_t* tombstoned, std::string& err) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    if (n == 0) return CRDT_HIP_OK;
    EditPlan plan;
    const int rc = edit_plan(p, n, ins, ins_len, nvis_, size(), plan, err);
    if (rc) return rc;
    if ((uint64_t)max_lamport + plan.cps.size() >= 0xFFFFFFFFull) {
        err = "lamports would reach 0xFFFFFFFF";
        return CRDT_HIP_ERANGE;
    }
    if (stale_) {  // (a malformed log is found here, before anything changes)
        err = rebuild_index();
        if (!err.empty()) return CRDT_HIP_EBADLOG;
    }
    for (size_t k = 0; k < n; ++k) {
        const EditPatch& e = plan.patch[k];
        if (p[k].del) err = remove(p[k].pos, p[k].pos + p[k].del);
        if (err.empty() && e.ncp) err = insert(p[k].pos, plan.cps.data() + e.cp0, e.ncp);
        if (!err.empty()) return CRDT_HIP_EBADLOG;  // (the index disagrees with the log)
    }
    if (added) *added = (uint32_t)plan.cps.size();
    if (tombstoned) *tombstoned = (uint32_t)plan.ndel;
    return CRDT_HIP_OK;
}

// Wire format (little-endian): magic, version, first_id, n_items, first_del, n_dels,
// parent[n], origin_right[n], lamport[n], cp[n] (u32), agent[n] (u16, padded to 4), dels[m].
// Fugue logs write version 2, with bit 31 of cp[k] = side (1: left child of parent[k]).
std::vector<uint8_t> OpLog::encode_from(uint64_t ver) const {
    uint32_t from_items = (uint32_t)(ver >> 32), from_dels = (uint32_t)ver;
    if (from_items > size()) from_items = size();
    if (from_dels > del_ops.size()) from_dels = (uint32_t)del_ops.size();
    uint32_t n = size() - from_items, m = (uint32_t)del_ops.size() - from_dels;
    std::vector<uint8_t> b;
    b.reserve(24 + (size_t)n * 18 + 4 + (size_t)m * 4);
    put32(b, kMagic);
    put32(b, fugue ? kUpdateVersionFugue : kWireVersion);
    put32(b, from_items + 1);
    put32(b, n);
    put32(b, from_dels);
    put32(b, m);
    for (uint32_t k = 0; k < n; ++k) put32(b, parent[from_items + k]);
    for (uint32_t k = 0; k < n; ++k) put32(b, oright[from_items + k]);
    for (uint32_t k = 0; k < n; ++k) put32(b, lamport[from_items + k]);
    if (fugue)
        for (uint32_t k = 0; k < n; ++k)
            put32(b, cp[from_items + k] | (side[from_items + k] ? kUpdateSideBit : 0u));
    else
        for (uint32_t k = 0; k < n; ++k) put32(b, cp[from_items + k]);
    for (uint32_t k = 0; k < n; ++k) {
        b.push_back((uint8_t)agent[from_items + k]);
        b.push_back((uint8_t)(agent[from_items + k] >> 8));
    }
    while (b.size() % 4) b.push_back(0);
    for (uint32_t k = 0; k < m; ++k) put32(b, del_ops[from_dels + k]);
    return b;
}

std::string OpLog::apply_update(const uint8_t* buf, size_t len) {
    if (len < 24 || get32(buf) != kMagic) return "not an update";
    const uint32_t ver = get32(buf + 4);
    if (ver == kUpdateVersionFugue && !fugue) return "Fugue update into an RGA log";
    if (ver != kWireVersion && ver != kUpdateVersionFugue) return "unsupported update version";
    uint32_t first = get32(buf + 8), n = get32(buf + 12);
    uint32_t first_del = get32(buf + 16), m = get32(buf + 20);
    size_t agent_bytes = ((size_t)n * 2 + 3) / 4 * 4;
    size_t need = 24 + (size_t)n * 16 + agent_bytes + (size_t)m * 4;
    if (len < need) return "truncated update";
    if (first == 0 || first > size() + 1) return "update is not causally ready (missing items)";
    if (first_del > del_ops.size()) return "update is not causally ready (missing deletes)";
    if ((uint64_t)first + n > 0xFFFFFFFFull) return "update item ids out of range";
    const uint8_t* P = buf + 24;
    const uint8_t* O = P + (size_t)n * 4;
    const uint8_t* L = O + (size_t)n * 4;
    const uint8_t* C = L + (size_t)n * 4;
    const uint8_t* A = C + (size_t)n * 4;
    const uint8_t* D = A + agent_bytes;
    // validate everything before changing anything: a rejected update leaves the log as it was
    // (as the device decoder does with a rejected batch)
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t id = first + k, par = get32(P + 4 * k);
        if (id > size() && par >= id && par != 0) return "update item references an unknown parent";
        if (fugue && id > size()) {
            if (par == 0 && (get32(C + 4 * k) & kUpdateSideBit))
                return "update item is a left child of the document start";
            if (get32(L + 4 * k) == 0xFFFFFFFFu) return "Fugue update item with lamport 0xFFFFFFFF";
        }
    }
    const uint64_t known = std::max<uint64_t>(size(), n ? (uint64_t)first + n - 1 : 0);
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t id = get32(D + 4 * k);
        if (id == 0 || id > known) return "update deletes an unknown item";
    }
    for (uint32_t k = 0; k < n; ++k) {
        uint32_t id = first + k;
        if (id <= size()) continue;  // already known (decode_and_add is idempotent)
        const uint32_t c = get32(C + 4 * k);
        push_item(get32(P + 4 * k), get32(O + 4 * k), get32(L + 4 * k),
                  (uint16_t)(A[2 * k] | (A[2 * k + 1] << 8)), 0, c & ~kUpdateSideBit,
                  fugue && (c & kUpdateSideBit) ? 1 : 0);
    }
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t id = get32(D + 4 * k);
        if (first_del + k >= del_ops.size()) del_ops.push_back(id);
        mark_deleted(id);
    }
    return "";
}

// ---- state-based merge -------------------------------------------------------------------------
namespace {
// Identity (lamport << 16 | agent; a Fugue item's side is no part of it) -> item id, open addressing over a power of two of at least
// twice the items (the device join's table, join.hip, on the host).
struct IdTable {
    std::vector<uint32_t> slot;
    uint32_t mask = 0;
    explicit IdTable(uint64_t items) {
        uint64_t c = 64;
        while (c < 2 * items) c <<= 1;
        slot.assign(c, 0u);  // 0: free (ids start at 1)
        mask = (uint32_t)(c - 1);
    }
    static uint32_t hash(uint64_t k) {
        k ^= k >> 29;
        k *= 0x9E3779B97F4A7C15ull;
        return (uint32_t)(k >> 32);
    }
    // The id holding key k, or 0; `key_of(id)` gives the key of a stored id.
    template <class K>
    uint32_t find(uint64_t k, K&& key_of) const {
        for (uint32_t h = hash(k) & mask;; h = (h + 1u) & mask) {
            const uint32_t e = slot[h];
            if (!e || key_of(e) == k) return e;
        }
    }
    // Stores id under k; returns the id that already held k (then nothing is stored), or 0.
    template <class K>
    uint32_t insert(uint64_t k, uint32_t id, K&& key_of) {
        for (uint32_t h = hash(k) & mask;; h = (h + 1u) & mask) {
            const uint32_t e = slot[h];
            if (!e) {
                slot[h] = id;
                return 0;
            }
            if (key_of(e) == k) return e;
        }
    }
};

// What join and apply_diff share of "this <- this U foreign items, named by identity": the table of
// the items held, the numbering and the bound of the new ones, the side-column check, and the two
// ways the log changes.  The checks on an item both hold and the Fugue rules for a new one stay
// with each caller: they differ in where a parent's identity comes from.
struct Merge {
    OpLog& log;
    const uint32_t nd;  // items held before the call
    IdTable dt;         // their identities
    uint32_t nnew = 0, ntomb = 0;
    explicit Merge(OpLog& l) : log(l), nd(l.size()), dt(nd) {}

    int side_column(std::string& err) const {
        if (log.fugue && log.side.size() != nd) {
            err = "malformed op log (side column)";
            return CRDT_HIP_EBADLOG;
        }
        return CRDT_HIP_OK;
    }
    // Fills dt, refusing two items of one identity with the caller's message; before_msg: also
    // refuses, item by item, a parent that does not precede its item.
    int build(const char* before_msg, const char* dup_msg, std::string& err) {
        auto key = [&](uint32_t id) { return log.ident(id); };
        for (uint32_t id = 1; id <= nd; ++id) {
            if (before_msg && log.parent[id - 1] >= id) {
                err = before_msg;
                return CRDT_HIP_EBADLOG;
            }
            if (dt.insert(key(id), id, key)) {
                err = dup_msg;
                return CRDT_HIP_EBADLOG;
            }
        }
        return CRDT_HIP_OK;
    }
    uint32_t held(uint64_t k) const {  // the id that holds identity k, or 0
        return dt.find(k, [&](uint32_t id) { return log.ident(id); });
    }
    uint32_t fresh() { return nd + 1u + nnew++; }  // a new item's id: nd + 1 + its rank among them
    int bound(std::string& err) const {
        if ((uint64_t)nd + nnew >= 0x7FFFFFF0ull) {
            err = "op log too large";
            return CRDT_HIP_ERANGE;
        }
        return CRDT_HIP_OK;
    }
    void reserve(size_t dels) {  // dels: at least the entries the call adds to del_ops
        if (!nnew) return;
        log.reserve((size_t)nd + nnew, log.del_ops.size() + dels);
        if (log.fugue) log.side.reserve((size_t)nd + nnew);
    }
    void tombstone(uint32_t d) {  // (an item this call appended counts as added, not tombstoned)
        if (log.deleted[d - 1]) return;
        log.del_ops.push_back(d);
        log.mark_deleted(d);
        ntomb += d <= nd;
    }
    void append(uint32_t par, uint32_t orr, uint64_t ident, bool del, uint32_t c, bool left) {
        log.push_item(par, orr, (uint32_t)(ident >> 16), (uint16_t)ident, del, c, left);
        if (del) log.del_ops.push_back(log.size());
    }
};
}  // namespace

int OpLog::join(uint32_t ns, const uint32_t* s_parent, const uint32_t* s_oright,
                const uint32_t* s_lamport, const uint16_t* s_agent, const uint8_t* s_deleted,
                const uint32_t* s_cp, const uint8_t* s_side, uint32_t* added,
                uint32_t* tombstoned, std::string& err) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    // (the kind is the presence of the side column, never its contents; checked before anything
    // else, an empty source included)
    if (fugue != (s_side != nullptr)) {
        err = "join of a Fugue log with an RGA log: both sides must be of one kind";
        return CRDT_HIP_EINVAL;
    }
    Merge mg(*this);
    if (int rc = mg.side_column(err)) return rc;
    if (fugue)  // the rules every path that takes a caller's Fugue view applies
        for (uint32_t id = 1; id <= ns; ++id) {
            if (s_lamport[id - 1] == 0xFFFFFFFFu) {
                err = "join: Fugue item with lamport 0xFFFFFFFF";
                return CRDT_HIP_EBADLOG;
            }
            if (s_side[id - 1] && s_parent[id - 1] == 0) {
                err = "join: an item is a left child of the document start";
                return CRDT_HIP_EBADLOG;
            }
        }
    auto skey = [&](uint32_t id) { return ((uint64_t)s_lamport[id - 1] << 16) | s_agent[id - 1]; };
    // ---- validate: nothing changes before every check has passed -------------------------------
    if (int rc = mg.build("join: an item's parent does not precede it",
                          "join: two items of the destination share an identity (lamport, agent)", err))
        return rc;
    // src id -> id in this log (new items in src's slot order)
    IdTable st(ns);
    std::vector<uint32_t> mp((size_t)ns + 1);
    mp[0] = 0;
    for (uint32_t id = 1; id <= ns; ++id) {
        if (s_parent[id - 1] >= id) {
            err = "join: an item's parent does not precede it";
            return CRDT_HIP_EBADLOG;
        }
        const uint64_t k = skey(id);
        if (st.insert(k, id, skey)) {
            err = "join: two items of the source share an identity (lamport, agent)";
            return CRDT_HIP_EBADLOG;
        }
        const uint32_t d = mg.held(k);
        mp[id] = d ? d : mg.fresh();
    }
    if (int rc = mg.bound(err)) return rc;
    size_t ndels = 0;  // entries the join adds to del_ops: new tombstones of held and of new items
    for (uint32_t id = 1; id <= ns; ++id) {
        const uint32_t d = mp[id];
        if (d > mg.nd) {
            ndels += s_deleted[id - 1] != 0;
            continue;
        }
        if ((cp[d - 1] ^ s_cp[id - 1]) & 0x1FFFFFu) {  // (codepoints: the device keeps 21 bits)
            err = "join: an item both logs hold has another codepoint in each";
            return CRDT_HIP_EBADLOG;
        }
        if (parent[d - 1] != mp[s_parent[id - 1]]) {
            err = "join: an item both logs hold has another parent in each";
            return CRDT_HIP_EBADLOG;
        }
        if (fugue && (side[d - 1] != 0) != (s_side[id - 1] != 0)) {
            err = "join: an item both logs hold has another side in each";
            return CRDT_HIP_EBADLOG;
        }
        ndels += s_deleted[id - 1] && !deleted[d - 1];
    }
    // ---- apply (src may be a view of this very log: then nothing is new and no column grows) ---
    mg.reserve(ndels);
    for (uint32_t id = 1; id <= ns; ++id) {
        const uint32_t d = mp[id];
        if (d <= mg.nd) {
            if (s_deleted[id - 1]) mg.tombstone(d);
            continue;
        }
        // origin_right: an item id is translated like a parent; 0 and NIL (or anything beyond
        // src's ids) stay as they are
        const uint32_t o = s_oright ? s_oright[id - 1] : NIL;
        mg.append(mp[s_parent[id - 1]], o && o <= ns ? mp[o] : o, skey(id), s_deleted[id - 1] != 0,
                  s_cp[id - 1], fugue && s_side[id - 1]);
    }
    if (added) *added = mg.nnew;
    if (tombstoned) *tombstoned = mg.ntomb;
    return CRDT_HIP_OK;
}

// ---- state-vector delta sync -------------------------------------------------------------------
namespace {
uint64_t get64(const uint8_t* p) { return (uint64_t)get32(p) | ((uint64_t)get32(p + 4) << 32); }
void put64(std::vector<uint8_t>& b, uint64_t v) {
    put32(b, (uint32_t)v);
    put32(b, (uint32_t)(v >> 32));
}
}  // namespace

int delta_frame(const uint8_t* buf, size_t len, bool fugue, uint64_t held, DeltaFrame& f,
                std::string& err) {
    f = DeltaFrame{};
    if (!buf || len < 16 || get32(buf) != kDeltaMagic) {
        err = "not a delta";
        return CRDT_HIP_EINVAL;
    }
    f.version = get32(buf + 4);
    if (f.version != kDeltaVersion && f.version != kDeltaVersionFugue) {
        err = "unsupported delta version";
        return CRDT_HIP_EINVAL;
    }
    if ((f.version == kDeltaVersionFugue) != fugue) {
        err = fugue ? "RGA delta into a Fugue log: both sides must be of one kind"
                    : "Fugue delta into an RGA log: both sides must be of one kind";
        return CRDT_HIP_EINVAL;
    }
    f.n = get32(buf + 8);
    f.r = get32(buf + 12);
    f.key = 16;
    f.pkey = f.key + 8ull * f.n;
    f.rkey = f.pkey + 8ull * f.n;
    f.cp = f.rkey + 8ull * f.r;
    f.rcount = f.cp + 4ull * f.n;
    f.bytes = f.rcount + 4ull * f.r;
    if (f.bytes >= (1ull << 32) || (uint64_t)len != f.bytes) {
        err = (uint64_t)len < f.bytes ? "truncated delta" : "delta size does not match its header";
        return CRDT_HIP_EINVAL;
    }
    for (uint32_t k = 0; k < f.r; ++k) {
        const uint32_t c = get32(buf + f.rcount + 4ull * k);
        if (!c) {
            err = "delta has an empty tombstone range";
            return CRDT_HIP_EINVAL;
        }
        f.range_items += c;
    }
    if (f.range_items > held + f.n) {
        err = "delta: a tombstone range names an unknown item";
        return CRDT_HIP_EBADLOG;
    }
    return CRDT_HIP_OK;
}

std::vector<SvEntry> OpLog::state_vector() const {
    std::vector<uint64_t> top(65536, 0);  // lamport + 1 (0: the agent has no item)
    const uint32_t n = size();
    for (uint32_t k = 0; k < n; ++k) top[agent[k]] = std::max<uint64_t>(top[agent[k]], (uint64_t)lamport[k] + 1);
    std::vector<SvEntry> sv;
    for (uint32_t a = 0; a < 65536; ++a)
        if (top[a]) sv.push_back(SvEntry{a, (uint32_t)(top[a] - 1)});
    return sv;
}

int OpLog::encode_diff(const SvEntry* sv, size_t nsv, std::vector<uint8_t>& out,
                       std::string& err) const {
    out.clear();
    std::vector<uint64_t> bound(65536, 0);  // lamport + 1 (0: covers nothing of the agent)
    for (size_t i = 0; i < nsv; ++i) {
        if (sv[i].agent > 65535u || (i && sv[i].agent <= sv[i - 1].agent)) {
            err = "state vector is not sorted strictly by agent, or names an agent above 65535";
            return CRDT_HIP_EINVAL;
        }
        bound[sv[i].agent] = (uint64_t)sv[i].lamport + 1;
    }
    const uint32_t n = size();
    auto key = [&](uint32_t k) { return ident(k + 1); };  // of slot k, 0-based as the loops below
    auto covered = [&](uint32_t k) { return (uint64_t)lamport[k] < bound[agent[k]]; };
    std::vector<uint32_t> items, heads, counts;
    for (uint32_t k = 0; k < n; ++k) {
        if (!covered(k)) {
            items.push_back(k);
            continue;
        }
        if (!deleted[k]) continue;
        // (a covered tombstone extends the range of the slot before it, or begins one)
        if (k && covered(k - 1) && deleted[k - 1] && key(k) == key(k - 1) + (1ull << 16)) counts.back()++;
        else {
            heads.push_back(k);
            counts.push_back(1);
        }
    }
    const uint64_t bytes = 16 + 20ull * items.size() + 12ull * heads.size();
    if (bytes >= (1ull << 32)) {
        err = "delta too large";
        return CRDT_HIP_ERANGE;
    }
    out.reserve(bytes);
    put32(out, kDeltaMagic);
    put32(out, fugue ? kDeltaVersionFugue : kDeltaVersion);
    put32(out, (uint32_t)items.size());
    put32(out, (uint32_t)heads.size());
    for (uint32_t k : items) put64(out, key(k));
    for (uint32_t k : items) put64(out, parent[k] ? key(parent[k] - 1) : kDeltaStart);
    for (uint32_t k : heads) put64(out, key(k));
    for (uint32_t k : items)
        put32(out, (cp[k] & kDeltaCpMask) | (deleted[k] ? kDeltaTombBit : 0u) |
                       (fugue && side[k] ? kDeltaSideBit : 0u));
    for (uint32_t c : counts) put32(out, c);
    return CRDT_HIP_OK;
}

int OpLog::apply_diff(const uint8_t* buf, size_t len, uint32_t* added, uint32_t* tombstoned,
                      std::string& err) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    DeltaFrame f;
    if (int rc = delta_frame(buf, len, fugue, size(), f, err)) return rc;
    Merge mg(*this);
    if (int rc = mg.side_column(err)) return rc;
    const uint32_t n = f.n;
    auto K = [&](uint32_t i) { return get64(buf + f.key + 8ull * i); };      // delta item i (0-based)
    auto PK = [&](uint32_t i) { return get64(buf + f.pkey + 8ull * i); };
    auto CP = [&](uint32_t i) { return get32(buf + f.cp + 4ull * i); };
    auto ikey = [&](uint32_t e) { return K(e - 1); };  // (table entries are 1-based)
    const uint32_t reserved = ~(kDeltaCpMask | kDeltaTombBit | (fugue ? kDeltaSideBit : 0u));
    // ---- validate: nothing changes before every check has passed -------------------------------
    if (int rc = mg.build(nullptr, "delta: two items of the log share an identity (lamport, agent)", err))
        return rc;
    // delta item -> id in this log (new items in the delta's order), and the translated parent of
    // a new item
    IdTable it(n);
    std::vector<uint32_t> mp(n), tpar(n);
    // The id in this log of identity k: of an item the log holds, else of one of the delta's first
    // `upto` items (0: neither).
    auto where = [&](uint64_t k, uint32_t upto) -> uint32_t {
        if (k >= kDeltaKeyEnd) return 0u;
        if (const uint32_t d = mg.held(k)) return d;
        const uint32_t e = it.find(k, ikey);
        return e && e - 1 < upto ? mp[e - 1] : 0u;
    };
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t k = K(i);
        const uint32_t c = CP(i);
        if (k >= kDeltaKeyEnd || (c & reserved)) {
            err = "delta: malformed item";
            return CRDT_HIP_EBADLOG;
        }
        if (it.insert(k, i + 1, ikey)) {
            err = "delta: two items share an identity (lamport, agent)";
            return CRDT_HIP_EBADLOG;
        }
        const uint64_t pk = PK(i);
        const uint32_t d = mg.held(k);
        if (d) {  // the log holds the item
            mp[i] = d;
            const uint32_t p = parent[d - 1];
            if ((cp[d - 1] ^ c) & kDeltaCpMask) {
                err = "delta: an item both hold has another codepoint in each";
                return CRDT_HIP_EBADLOG;
            }
            if ((p ? ident(p) : kDeltaStart) != pk) {
                err = "delta: an item both hold has another parent in each";
                return CRDT_HIP_EBADLOG;
            }
            if (fugue && (side[d - 1] != 0) != ((c & kDeltaSideBit) != 0)) {
                err = "delta: an item both hold has another side in each";
                return CRDT_HIP_EBADLOG;
            }
            continue;
        }
        mp[i] = mg.fresh();
        if (fugue) {
            if ((k >> 16) == 0xFFFFFFFFull) {
                err = "delta: Fugue item with lamport 0xFFFFFFFF";
                return CRDT_HIP_EBADLOG;
            }
            if ((c & kDeltaSideBit) && pk == kDeltaStart) {
                err = "delta: an item is a left child of the document start";
                return CRDT_HIP_EBADLOG;
            }
        }
        if (pk == kDeltaStart) {
            tpar[i] = 0;
            continue;
        }
        const uint32_t p = where(pk, i);  // (in the delta: an earlier item, new like this one)
        if (!p) {
            err = "delta: an item's parent is unknown or does not precede it";
            return CRDT_HIP_EBADLOG;
        }
        tpar[i] = p;
    }
    if (int rc = mg.bound(err)) return rc;
    // every identity of every range, after the items
    std::vector<uint32_t> rid;
    rid.reserve(f.range_items);
    for (uint32_t q = 0; q < f.r; ++q) {
        const uint64_t k0 = get64(buf + f.rkey + 8ull * q);
        const uint32_t cnt = get32(buf + f.rcount + 4ull * q);
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t k = k0 + ((uint64_t)j << 16);
            const uint32_t d = k0 < kDeltaKeyEnd ? where(k, n) : 0u;
            if (!d) {
                err = "delta: a tombstone range names an unknown item";
                return CRDT_HIP_EBADLOG;
            }
            rid.push_back(d);
        }
    }
    // ---- apply ---------------------------------------------------------------------------------
    mg.reserve((size_t)n + rid.size());
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = CP(i);
        if (mp[i] <= mg.nd) {
            if (c & kDeltaTombBit) mg.tombstone(mp[i]);
            continue;
        }
        mg.append(tpar[i], NIL, K(i), (c & kDeltaTombBit) != 0, c & kDeltaCpMask,
                  fugue && (c & kDeltaSideBit));
    }
    for (uint32_t d : rid) mg.tombstone(d);
    if (added) *added = mg.nnew;
    if (tombstoned) *tombstoned = mg.ntomb;
    return CRDT_HIP_OK;
}

}  // namespace crdt
