// lines.hip — the line index of a device-resident replica (replica.hpp,
// crdt_hip_replica_line_starts / _lines_of): line numbers -> where each line starts, and gap
// positions -> line, line start and column, now or at a mark.  The semantics are stated in
// crdt_hip_lines.h; the host twins are OpLog::line_starts and OpLog::lines_of (oplog.cpp), and both
// sides return the same arrays byte for byte.
//
// As text.hip, over the document order the replica keeps after a merge_inc (IncState::seq[cur],
// rank -> slot, tombstones included) under the version's selector (SelNow or SelMark, order.hpp),
// the one template parameter of every kernel here.  A third weight rides beside the codepoints and
// their UTF-8 bytes: the line break, a selected item whose codepoint is U+000A.
//
//   k_line_count  a workgroup per tile of kOrderTile = 4,096 consecutive ranks, four ranks per
//                 thread as a uint4 (order_lens4); per tile the selected codepoints, their UTF-8
//                 bytes and the selected line breaks.  SelMark never reads the plane for a slot above
//                 n_mark or a word at or past its words.
//   k_line_top    one workgroup scans the three tile aggregates into exclusive prefixes, in rounds of
//                 kOrdTop tiles with a carry (order_tile_scan: 32-bit for the codepoints, 64-bit for
//                 the bytes; block_scan_counts: 32-bit for the line breaks, at most n < 2^31), and
//                 writes the version's totals.
//   k_line_seek   a wave per query.  A line number k: 0 and L + 1 come from the totals; otherwise a
//                 binary search of the line break prefixes for the last tile whose exclusive prefix
//                 is below k (strict, as seek_tile: a tile may hold no line break, and then shares
//                 its prefix with the next) and a walk of that tile, 64 ranks a step, to the lane
//                 whose item is a selected line break with inclusive line break count k; its
//                 inclusive codepoint and byte prefixes are the line start.  A position p: 0 and the
//                 version's length come from the totals; otherwise the same search and walk in the
//                 unit asked to the selected item that ends at p (in bytes an item that steps over p
//                 raises EL_INSIDE), whose inclusive line break count is the line; then the first
//                 seek for that line.  The walk's loads are issued in chunks of kWalkChunk steps, as
//                 view_seek's (view.hpp): a walk that loads as it goes pays one dependent round trip
//                 per 64 ranks.
// No atomic decides a value (an OR raises an error bit); every slot, tile and mark word is checked
// against n, n_mark, the mark's words and ntiles before use; every loop is bounded (a search by the
// tiles, a walk by the tile).  A query that fails writes no record; the host waits once, runs the
// checks of crdt_hip_lines.h from the totals and the error bits and copies the n records out in one
// transfer.
//
// Known cost: a call streams every rank of the replica once (the count), however few the queries,
// and after a join or a delta it also pays inc_rebuild's ORDER-mode merge.
#include <cstring>
#include <type_traits>
#include <vector>

#include "idtab.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "view.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// device counters (u64): what the host reads after its one wait
enum LCtl { L_ERR = 0, L_LEN, L_LENB, L_BREAKS, L_N };
// L_ERR bits, after E_ORD_SLOT (order.hpp)
constexpr uint64_t EL_BEYOND = 2;  // a line number above L + 1, a position beyond the version
constexpr uint64_t EL_INSIDE = 4;  // (bytes) a position inside a codepoint
constexpr uint64_t EL_WALK = 8;    // a query's item is not in the tile the prefixes name

// what a walk seeks: the k-th line break, or the item that ends at a position in codepoints / bytes
enum : uint32_t { W_LINE = 0, W_CP = 1, W_BYTES = 2 };
constexpr uint32_t kLineW = kJB / 64;  // queries (waves) per workgroup
constexpr uint32_t kBreakBit = 8;      // beside an item's UTF-8 length (1..4): it is a line break

template <class Sel>
struct LineArgs {
    OrderView v;         // the kept order and the version's codepoint and byte prefixes
    Sel sel;             // the version
    uint32_t* tcount;    // v.tcount and v.tbpre as the count and the scan write them
    uint32_t* tbytes;    // per tile: the selected UTF-8 bytes (at most 16 KiB)
    uint64_t* tbpre;
    uint32_t* tbreaks;   // per tile: the selected line breaks, then those before the tile
    const uint64_t* q;   // the queries: line numbers (unit W_LINE) or positions
    uint32_t m;          // their number
    uint32_t unit;       // W_LINE, W_CP or W_BYTES
    LinePos* out;        // m records
    uint64_t* ctl;
};

__global__ void k_line_init(uint64_t* ctl) {
    if (threadIdx.x < (uint32_t)L_N) ctl[threadIdx.x] = 0;
}

// ---- count -------------------------------------------------------------------------------------
template <class Sel>
__global__ __launch_bounds__(kOrdT) void k_line_count(LineArgs<Sel> a) {
    __shared__ uint32_t red[kOrdW];
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t len[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    order_lens4(a.v.seq, a.v.cp, a.v.n, a.sel, k0, len, cpw, err);
    ctl_or(&a.ctl[L_ERR], err);
    uint32_t c = 0, b = 0, l = 0;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        c += len[j] ? 1u : 0u;
        b += len[j];
        l += len[j] && cpw[j] == kLineBreak ? 1u : 0u;
    }
    const uint32_t tc = block_sum_t0<kOrdW>(c, red), tb = block_sum_t0<kOrdW>(b, red),
                   tl = block_sum_t0<kOrdW>(l, red);
    if (threadIdx.x == 0 && blockIdx.x < a.v.ntiles) {
        a.tcount[blockIdx.x] = tc;
        a.tbytes[blockIdx.x] = tb;
        a.tbreaks[blockIdx.x] = tl;
    }
}

// ---- top ---------------------------------------------------------------------------------------
template <class Sel>
__global__ __launch_bounds__(kOrdTop) void k_line_top(LineArgs<Sel> a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    uint64_t c_cnt, c_by;
    order_tile_scan(a.v.ntiles, a.tcount, a.tbytes, a.tbpre, lds, c_cnt, c_by);
    const uint64_t c_br = block_scan_counts<kOrdTop>(a.tbreaks, a.v.ntiles, lds);
    if (threadIdx.x == 0) {
        a.ctl[L_LEN] = c_cnt;
        a.ctl[L_LENB] = c_by;
        a.ctl[L_BREAKS] = c_br;
    }
}

// ---- seek --------------------------------------------------------------------------------------
// The weight of the single rank k (a walk's lane): 0 when it is not selected (rank 0, a rank past n,
// a slot that is no item, which also raises E_ORD_SLOT), else its UTF-8 length, with kBreakBit when
// it is a line break.  As order_len_at: no load sits behind a branch (a rank or a slot that is
// refused reads entry 0 of its array), so that a chunk's loads can all be in flight at once.
template <class Sel>
__device__ __forceinline__ uint32_t line_weight_at(const OrderView& v, const Sel& sel, uint64_t k,
                                                   uint64_t& err) {
    const bool inr = k != 0 && k <= v.n;
    const uint32_t s = v.seq[inr ? k : 0];
    const bool item = inr && s != 0 && s <= v.n;
    err |= inr && !item ? E_ORD_SLOT : 0;
    const uint32_t sl = item ? s : 0u;
    const uint32_t c = cp3_get(v.cp, sl), cpv = c & kDeltaCpMask;
    return sel(sl, c, item, utf8_len(cpv) | (cpv == kLineBreak ? kBreakBit : 0u));
}

// The seek of one item by a whole wave, with a wave-uniform `what` and thr (0 < thr <= the version's
// total of that weight): the selected line break whose inclusive line break count is thr (W_LINE),
// or the first selected item whose inclusive prefix in codepoints (W_CP) or bytes (W_BYTES) is at
// least thr.  On true, in every lane: the selected codepoints up to and including that item, their
// UTF-8 bytes and the line breaks among them.  false: no lane of the tile the prefixes name held it
// (the caller's EL_WALK).
template <class Sel>
__device__ __forceinline__ bool line_walk(const LineArgs<Sel>& a, uint32_t what, uint64_t thr,
                                          uint32_t lane, uint64_t& err, uint64_t& inc_c, uint64_t& inc_b,
                                          uint64_t& inc_l) {
    auto pre = [&](uint32_t t) {
        return what == W_LINE ? (uint64_t)a.tbreaks[t] : what == W_BYTES ? a.tbpre[t] : (uint64_t)a.tcount[t];
    };
    uint32_t tile = 0;  // the last tile whose exclusive prefix is below thr (tile 0's is 0)
    for (uint32_t hi = a.v.ntiles; hi - tile > 1u;) {
        const uint32_t mid = (tile + hi) >> 1;
        if (pre(mid) < thr) tile = mid;
        else hi = mid;
    }
    uint64_t run_c = a.tcount[tile], run_b = a.tbpre[tile], run_l = a.tbreaks[tile];
    const uint64_t le = ~0ull >> (63u - lane);  // this lane and the ones below
    bool found = false;
    constexpr uint32_t kSteps = kOrderTile / 64u;
    static_assert(kSteps % kWalkChunk == 0, "a tile is a whole number of chunks");
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < kSteps && !found; c0 += kWalkChunk) {
        uint32_t wts[kWalkChunk];
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st)
            wts[st] = line_weight_at(a.v, a.sel, (uint64_t)tile * kOrderTile + (c0 + st) * 64u + lane, err);
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st) {
            if (found) continue;  // (wave-uniform)
            const uint32_t len = wts[st] & (kBreakBit - 1u);
            const bool br = (wts[st] & kBreakBit) != 0;
            const uint64_t on = __ballot(len != 0), brm = __ballot(br);
            const uint32_t lc = (uint32_t)__popcll(on & le), ll = (uint32_t)__popcll(brm & le);
            const uint32_t lb = wave_incl_scan(len);
            bool hit;
            if (what == W_LINE) {
                hit = br && run_l + ll == thr;
            } else {
                const uint64_t inc = what == W_BYTES ? run_b + lb : run_c + lc;
                hit = len != 0 && inc >= thr && inc - (what == W_BYTES ? len : 1u) < thr;
            }
            const uint64_t hm = __ballot(hit);  // (at most one lane: the prefixes ascend over items)
            if (hm) {
                const int src = (int)__builtin_ctzll(hm);
                inc_c = run_c + (uint32_t)__shfl((int)lc, src);
                inc_b = run_b + (uint32_t)__shfl((int)lb, src);
                inc_l = run_l + (uint32_t)__shfl((int)ll, src);
                found = true;
            } else {
                run_c += (uint32_t)__popcll(on);
                run_b += (uint32_t)__builtin_amdgcn_readlane((int)lb, 63);
                run_l += (uint32_t)__popcll(brm);
            }
        }
    }
    return found;
}

// A wave per query.  Everything that branches depends on the query alone, so a wave stays whole
// through the ballots and the wave scans.  Two passes at most through the one walk: a position is
// sought first (its codepoints, bytes and line), then the start of its line; a line number takes
// the second pass alone.
template <class Sel>
__global__ __launch_bounds__(kJB) void k_line_seek(LineArgs<Sel> a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kLineW + (threadIdx.x >> 6);
    if (i >= a.m) return;
    const uint64_t len = a.ctl[L_LEN], lenb = a.ctl[L_LENB], breaks = a.ctl[L_BREAKS];
    uint64_t err = 0;
    uint32_t what = a.unit;
    uint64_t thr = a.q[i];
    uint64_t pc = 0, pb = 0;  // the position
    LinePos o{0, 0, 0, 0, 0};
    bool done = false;
#pragma unroll 1
    for (uint32_t pass = 0; pass < 2u && !done; ++pass) {
        const bool line = what == W_LINE;
        const uint64_t total = line ? breaks + 1 : what == W_BYTES ? lenb : len;
        uint64_t rc = 0, rb = 0, rl = 0;
        if (thr > total) {
            err |= EL_BEYOND;
            break;
        }
        if (thr == total) {  // the end of the version
            rc = len;
            rb = lenb;
            rl = breaks;
        } else if (thr != 0) {
            if (!line_walk(a, what, thr, lane, err, rc, rb, rl)) {
                err |= EL_WALK;
                break;
            }
            if (!line && (what == W_BYTES ? rb : rc) != thr) {
                err |= EL_INSIDE;
                break;
            }
        }
        if (line) {
            o.line = thr;
            o.start = rc;
            o.start_bytes = rb;
            done = true;
        } else {
            pc = rc;
            pb = rb;
            what = W_LINE;
            thr = rl;
        }
    }
    if (done && a.unit != W_LINE) {
        if (pc < o.start || pb < o.start_bytes) {  // a line starts at or before every gap of it
            err |= EL_WALK;
            done = false;
        }
        o.col = pc - o.start;
        o.col_bytes = pb - o.start_bytes;
    }
    if (done && lane == 0) a.out[i] = o;
    ctl_or(&a.ctl[L_ERR], err);  // (E_ORD_SLOT is a lane's own)
}

template <class Sel>
int lines_impl(Engine& E, Replica& r, const OrderView& v, const Sel& sel, uint32_t unit, const uint64_t* q,
               size_t n, LinePos* out, LineInfo* info, LineStats* stats) {
    hipStream_t s = E.stream;
    CallScratch sc(s);
    const uint32_t ntiles = v.ntiles;
    LineArgs<Sel> a{};
    a.v = v;
    a.sel = sel;
    a.unit = unit;
    a.m = (uint32_t)n;
    uint64_t* dq = nullptr;
    HIPTRY(E, sc.counters(L_N), "hipMalloc line counters");
    HIPTRY(E, sc.alloc(&a.tcount, (uint64_t)ntiles), "hipMalloc line tiles");
    HIPTRY(E, sc.alloc(&a.tbytes, (uint64_t)ntiles), "hipMalloc line tiles");
    HIPTRY(E, sc.alloc(&a.tbpre, (uint64_t)ntiles), "hipMalloc line tiles");
    HIPTRY(E, sc.alloc(&a.tbreaks, (uint64_t)ntiles), "hipMalloc line tiles");
    HIPTRY(E, sc.alloc(&dq, n), "hipMalloc line queries");
    HIPTRY(E, sc.alloc(&a.out, n), "hipMalloc line records");
    a.v.tcount = a.tcount;
    a.v.tbpre = a.tbpre;
    a.q = dq;
    a.ctl = sc.ctl;
    // (the caller's array outlives the wait below, so the upload may read it until then)
    if (n) HIPTRY(E, hipMemcpyAsync(dq, q, n * 8, hipMemcpyHostToDevice, s), "upload line queries");
    HIPTRY(E, sc.time_begin(), "line event");
    k_line_init<<<1, 64, 0, s>>>(sc.ctl);
    k_line_count<<<ntiles, kOrdT, 0, s>>>(a);
    k_line_top<<<1, kOrdTop, 0, s>>>(a);
    if (n) k_line_seek<<<grid_for(n, kLineW), kJB, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "line kernels");
    HIPTRY(E, sc.time_end(), "line event");
    std::vector<LinePos> res(n);
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, L_N * 8, hipMemcpyDeviceToHost, s), "copy line counters");
    if (n)
        HIPTRY(E, hipMemcpyAsync(res.data(), a.out, n * sizeof(LinePos), hipMemcpyDeviceToHost, s),
               "copy line records");
    HIPTRY(E, hipStreamSynchronize(s), "line sync");  // the one wait
    sc.time_add();
    if (stats) {
        stats->queries = n;
        stats->ranks = r.n;
        stats->device_ns = sc.dev_ns;
    }
    const uint64_t* h = sc.hctl;
    const uint64_t e = h[L_ERR];
    if (e & E_ORD_SLOT) {
        E.err = "lines: the kept document order names a slot that is no item";
        return CRDT_HIP_EBADLOG;
    }
    bool off;
    if constexpr (std::is_same<Sel, SelMark>::value) off = h[L_LEN] > sel.m.n_mark;
    else off = h[L_LEN] != r.vis_cp || h[L_LENB] != r.vis_bytes;
    if (off || h[L_BREAKS] > h[L_LEN] || h[L_LENB] < h[L_LEN] || h[L_LENB] > 4 * h[L_LEN]) {
        E.err = "lines: the selected items of the kept order disagree with the replica's counters";
        return CRDT_HIP_EBADLOG;
    }
    const bool lines = unit == W_LINE;
    if (int rc = line_check_version(lines, (e & EL_BEYOND) != 0, (e & EL_INSIDE) != 0, E.err)) return rc;
    // what the kernels found is what was asked for
    bool ok = !(e & EL_WALK);
    for (size_t k = 0; k < n && ok; ++k) {
        const LinePos& p = res[k];
        ok = lines ? p.line == q[k] && p.col == 0 && p.col_bytes == 0
                   : (unit == W_BYTES ? p.start_bytes + p.col_bytes : p.start + p.col) == q[k];
        ok = ok && p.line <= h[L_BREAKS] + 1 && p.start + p.col <= h[L_LEN] &&
             p.start_bytes + p.col_bytes <= h[L_LENB];
    }
    if (!ok) {
        E.err = "lines: a query's item is not where the tile prefixes say";
        return CRDT_HIP_EBADLOG;
    }
    if (n) std::memcpy(out, res.data(), n * sizeof(LinePos));
    if (info) *info = LineInfo{h[L_BREAKS] + 1, h[L_LEN], h[L_LENB]};
    return CRDT_HIP_OK;
}

}  // namespace

int replica_lines(Engine& E, Replica& r, const DeviceMark* m, bool positions, const uint64_t* q, size_t n,
                  uint32_t flags, LinePos* out, LineInfo* info, LineStats* stats) {
    if (stats) *stats = LineStats{};
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    if (m && (rc = mark_fits(E, r, *m))) return rc;
    if ((rc = line_check(q, n, positions ? flags : 0u, out, E.err))) return rc;
    const uint32_t unit = !positions ? W_LINE : (flags & kTextBytes) ? W_BYTES : W_CP;
    if (r.n == 0) {  // nothing held: every version is empty, one line that starts and ends at 0
        bool beyond = false;
        for (size_t k = 0; k < n; ++k) beyond |= q[k] > (positions ? 0u : 1u);
        if ((rc = line_check_version(!positions, beyond, false, E.err))) return rc;
        for (size_t k = 0; k < n; ++k) out[k] = LinePos{q[k], 0, 0, 0, 0};
        if (info) *info = LineInfo{1, 0, 0};
        if (stats) stats->queries = n;
        return CRDT_HIP_OK;
    }
    OrderView v{};
    if ((rc = replica_kept_order(E, r, "lines", &v.seq, &v.ntiles))) return rc;
    v.cp = r.logs.cp;
    v.n = r.n;
    if (!m) return lines_impl(E, r, v, SelNow{}, unit, q, n, out, info, stats);
    return lines_impl(E, r, v, SelMark{{m->bits, m->n, m->words}}, unit, q, n, out, info, stats);
}

}  // namespace crdt
