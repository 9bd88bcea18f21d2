// text.hip — text windows of a device-resident replica (replica.hpp, crdt_hip_replica_text_at): a
// range of the document, now or at a mark, as UTF-8 and nothing else.  The semantics are stated in
// crdt_hip.h, "text windows"; the host twin is OpLog::text_at (oplog.cpp), and both give the same
// bytes and the same crdt_hip_text_info.
//
// A version selects items: NOW the ones that are not tombstoned, AT_MARK the ones the mark saw alive
// (slot <= n_mark and its bit in the mark's plane clear).  After a merge_inc the replica keeps the
// document order of every item it holds (IncState::seq[cur], rank -> slot, tombstones included, RGA
// and Fugue alike), and later items never reorder earlier ones, so either version's text is a count,
// a scan and a compaction over that order under the version's predicate, the one template parameter
// of every kernel here:
//
//   k_text_count  a workgroup per tile of kOrderTile = 4,096 consecutive ranks, four ranks per
//                 thread (order_load4); per tile the selected codepoints and their UTF-8 bytes.
//                 AT_MARK gathers the mark bit exactly as k_patch_classify does and never reads the
//                 plane for a slot above n_mark or a word at or past mark_words.
//   k_text_top    one workgroup scans the tile aggregates into exclusive prefixes (64-bit for both)
//                 and the version's totals.  Then a wave per boundary (`start`, `end`) searches the
//                 prefixes, in the unit asked, for the last tile that begins before the boundary and
//                 walks it 64 ranks a step with a wave scan (in chunks of 16 steps, a chunk's
//                 loads issued first), to the selected item that ends at the boundary: its inclusive prefixes
//                 are the boundary in codepoints and bytes.  In
//                 bytes an item that steps over the boundary raises ET_INSIDE.  A thread each then finds
//                 the window's first and last tile in the byte prefixes and writes the totals, the
//                 window in both units, the two tiles and the error bits: the host waits here, once,
//                 runs the checks of crdt_hip.h and returns ESPACE without a write pass.
//   k_text_write  a workgroup per tile in [first tile, last tile] only (a 4 KiB viewport of a
//                 200 k-item replica: one or two workgroups, not 50): selects again (no per-rank
//                 class is stored, as in patch.hip), scans the thread sums and every selected item
//                 stores its UTF-8 at (tile byte prefix + bytes before it in the tile - start_bytes)
//                 when that lies inside the window.  The bytes go straight from registers to the
//                 output, as k_patch_write places its I bytes: a typing run's stores are consecutive
//                 across the lanes, and a viewport's one or two tiles leave nothing for an LDS
//                 staging pass to win.
// No atomic decides an order (an OR raises an error bit); every slot, tile and mark word is checked
// against n, n_mark, mark_words and ntiles before use, every store against the window's bytes, which
// is what the output buffer holds; every loop is bounded (a search by the tiles, a walk by the
// tile).  The result is copied out in one transfer.
//
// Known cost: a call streams every rank of the replica once (the count), however small the window,
// and after a join or a delta it also pays inc_rebuild's ORDER-mode merge.
#include <cstring>

#include "idtab.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// device counters (u64): what the host reads after its one wait
enum TCtl { T_ERR = 0, T_LEN, T_LENB, T_START, T_STARTB, T_END, T_ENDB, T_FIRST, T_LAST, T_N };
constexpr uint64_t ET_SLOT = 1;    // the order names a slot that is no item of the replica
constexpr uint64_t ET_RANGE = 2;   // start or end beyond the version (the host says which)
constexpr uint64_t ET_INSIDE = 4;  // (bytes) a boundary inside a codepoint
constexpr uint64_t ET_WALK = 8;    // a boundary's item is not in the tile the prefixes name

struct TextArgs {
    const uint32_t* seq;   // rank -> slot, ranks 0..n (replica_kept_order)
    const uint8_t* cp;     // 3-byte codepoint words of slots 0..n
    const uint64_t* mark;  // AT_MARK: bit s = slot s was tombstoned at the mark, or is not an item
    uint32_t n, n_mark;
    uint64_t mark_words;
    uint32_t ntiles;
    uint32_t* tcnt;        // per tile: selected codepoints
    uint32_t* tbytes;      //   and their UTF-8 bytes (at most 16 KiB)
    uint64_t* pcnt;        // their exclusive prefixes over the tiles
    uint64_t* pbytes;
    uint64_t start, end;   // the window as asked (end: kTextEnd for the version's end)
    uint32_t bytes;        // the unit of start and end: UTF-8 bytes (else codepoints)
    // write pass (as the host read them)
    uint32_t first_tile;
    uint64_t start_bytes, n_bytes;
    uint8_t* out;          // n_bytes
    uint64_t* ctl;
};

__global__ void k_text_init(uint64_t* ctl) {
    if (threadIdx.x < (uint32_t)T_N) ctl[threadIdx.x] = 0;
}

// Whether the version selects slot s (1..n) with codepoint word c.
template <bool AT_MARK>
__device__ __forceinline__ bool text_sel(const TextArgs& a, uint32_t s, uint32_t c) {
    if constexpr (AT_MARK)
        return s <= a.n_mark && (uint64_t)(s >> 6) < a.mark_words &&
               !((a.mark[s >> 6] >> (s & 63u)) & 1ull);
    else
        return !(c & kDelBit);
}

// The UTF-8 lengths (0: not selected, rank 0, a rank past n, a slot that is no item) and the
// codepoints of the thread's four ranks k0..k0 + 3.
template <bool AT_MARK>
__device__ __forceinline__ void text_load(const TextArgs& a, uint64_t k0, uint32_t len[kOrdPer],
                                          uint32_t cpw[kOrdPer], uint64_t& err) {
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        len[j] = 0;
        cpw[j] = 0;
    }
    order_load4(a.seq, a.cp, a.n, k0, err, ET_SLOT, [&](uint32_t j, uint32_t s, uint32_t c) {
        if (text_sel<AT_MARK>(a, s, c)) {
            cpw[j] = c & kDeltaCpMask;
            len[j] = utf8_len(cpw[j]);
        }
    });
}

// The same for the single rank k (a walk's lane).  No load sits behind a branch: a rank or a slot
// that is refused reads entry 0 of its array instead (rank 0, slot 0 and mark word 0 always exist),
// so that the loads of a chunk of a walk's steps can all be in flight at once.
template <bool AT_MARK>
__device__ __forceinline__ uint32_t text_len_at(const TextArgs& a, uint64_t k, uint64_t& err) {
    const bool inr = k != 0 && k <= a.n;
    const uint32_t s = a.seq[inr ? k : 0];
    const bool item = inr && s != 0 && s <= a.n;
    err |= inr && !item ? ET_SLOT : 0;
    const uint32_t sc = item ? s : 0u;
    const uint32_t c = cp3_get(a.cp, sc);
    bool sel = item;
    if constexpr (AT_MARK) {
        const bool inm = sc <= a.n_mark && (uint64_t)(sc >> 6) < a.mark_words;
        const uint64_t w = a.mark[inm ? sc >> 6 : 0u];
        sel = sel && inm && !((w >> (sc & 63u)) & 1ull);
    } else {
        sel = sel && !(c & kDelBit);
    }
    return sel ? utf8_len(c & kDeltaCpMask) : 0u;
}

// ---- count -------------------------------------------------------------------------------------
template <bool AT_MARK>
__global__ __launch_bounds__(kOrdT) void k_text_count(TextArgs a) {
    __shared__ uint32_t red[kOrdW];
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t len[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    text_load<AT_MARK>(a, k0, len, cpw, err);
    ctl_or(&a.ctl[T_ERR], err);
    uint32_t cnt = 0, by = 0;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        cnt += len[j] ? 1u : 0u;
        by += len[j];
    }
    const uint32_t s_cnt = block_sum_t0<kOrdW>(cnt, red), s_by = block_sum_t0<kOrdW>(by, red);
    if (threadIdx.x == 0 && blockIdx.x < a.ntiles) {
        a.tcnt[blockIdx.x] = s_cnt;
        a.tbytes[blockIdx.x] = s_by;
    }
}

// ---- top ---------------------------------------------------------------------------------------
// The boundary 0 < p < total of the version, in the unit asked, as (codepoints, bytes): the prefixes
// of the last tile that begins before p and a walk of that tile to the selected item whose inclusive
// prefix is p.  Called by a whole wave with a wave-uniform p; the item's lane stores into res[0..1].
template <bool AT_MARK>
__device__ __forceinline__ void text_boundary(const TextArgs& a, uint64_t p, uint32_t lane,
                                              uint64_t* res, uint64_t& err) {
    auto pre = [&](uint32_t t) { return a.bytes ? a.pbytes[t] : a.pcnt[t]; };
    uint32_t lo = 0, hi = a.ntiles;  // (tile 0 begins at 0 < p)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre(mid) < p) lo = mid;
        else hi = mid;
    }
    uint64_t rc = a.pcnt[lo], rb = a.pbytes[lo];
    // in chunks of kWalkChunk steps, a chunk's loads first: the steps' gathers are independent of
    // one another, and a walk that loads as it goes pays one dependent round trip (order, then
    // codepoint word) per step.  A chunk, not the whole tile, keeps the registers of the loads in
    // flight to kWalkChunk and lets a walk end after the chunk that holds the boundary.
    constexpr uint32_t kSteps = kOrderTile / 64u, kWalkChunk = 16;
    static_assert(kSteps % kWalkChunk == 0, "a tile is a whole number of chunks");
    bool found = false;
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < kSteps && !found; c0 += kWalkChunk) {
        uint32_t lens[kWalkChunk];
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st)
            lens[st] = text_len_at<AT_MARK>(a, (uint64_t)lo * kOrderTile + (c0 + st) * 64u + lane, err);
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st) {
            if (found) continue;  // (wave-uniform)
            const uint32_t len = lens[st];
            const uint64_t sel = __ballot(len != 0);
            const uint32_t inc_c = (uint32_t)__popcll(sel & (~0ull >> (63u - lane)));
            const uint32_t inc_b = wave_incl_scan(len);
            const uint64_t inc = a.bytes ? rb + inc_b : rc + inc_c;
            const uint32_t wt = a.bytes ? len : 1u;
            const bool hit = len != 0 && inc >= p && inc - wt < p;
            found = __ballot(hit) != 0;  // (at most one lane: the prefixes ascend strictly over items)
            if (hit) {
                if (inc == p) {
                    res[0] = rc + inc_c;
                    res[1] = rb + inc_b;
                } else {
                    err |= ET_INSIDE;
                }
            }
            rc += (uint32_t)__popcll(sel);
            rb += (uint32_t)__builtin_amdgcn_readlane((int)inc_b, 63);
        }
    }
    if (!found) err |= ET_WALK;
}

template <bool AT_MARK>
__global__ __launch_bounds__(kOrdTop) void k_text_top(TextArgs a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    __shared__ uint64_t bnd[2][2];  // start, end: codepoints and bytes before the boundary
    if (threadIdx.x < 4u) bnd[threadIdx.x >> 1][threadIdx.x & 1u] = 0;
    uint64_t c_cnt = 0, c_by = 0;
    for (uint32_t base = 0; base < a.ntiles; base += kOrdTop) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x_cnt = i < a.ntiles ? a.tcnt[i] : 0u, x_by = i < a.ntiles ? a.tbytes[i] : 0u;
        uint32_t tot;
        const uint32_t e_cnt = block_excl_scan<kOrdTop / 64>(x_cnt, lds, tot);
        if (i < a.ntiles) a.pcnt[i] = c_cnt + e_cnt;
        c_cnt += tot;
        const uint32_t e_by = block_excl_scan<kOrdTop / 64>(x_by, lds, tot);
        if (i < a.ntiles) a.pbytes[i] = c_by + e_by;
        c_by += tot;
    }
    __syncthreads();  // the prefixes, written by this workgroup, are read below
    const uint64_t total = a.bytes ? c_by : c_cnt;
    const uint64_t endv = a.end == kTextEnd ? total : a.end;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (w < 2u) {  // a wave per boundary
        const uint64_t p = w == 0 ? a.start : endv;
        uint64_t err = 0;
        if (p > total) {
            err = ET_RANGE;
        } else if (p == total) {
            if (lane == 0) {
                bnd[w][0] = c_cnt;
                bnd[w][1] = c_by;
            }
        } else if (p != 0) {
            text_boundary<AT_MARK>(a, p, lane, bnd[w], err);
        }
        ctl_or(&a.ctl[T_ERR], err);
    }
    __syncthreads();
    // the window's first item lies in the last tile that begins at or before start_bytes, its last
    // item in the last tile that begins before end_bytes (tile 0 begins at 0); a thread each
    if (lane == 0 && w < 2u) {
        const uint64_t b = bnd[w][1];
        uint32_t t = 0;
        for (uint32_t lo = 0, hi = a.ntiles; hi - lo > 1u;) {
            const uint32_t mid = (lo + hi) >> 1;
            if (w == 0 ? a.pbytes[mid] <= b : a.pbytes[mid] < b) t = lo = mid;
            else hi = mid;
        }
        if (w == 0) {
            a.ctl[T_LEN] = c_cnt;
            a.ctl[T_LENB] = c_by;
        }
        a.ctl[w == 0 ? T_START : T_END] = bnd[w][0];
        a.ctl[w == 0 ? T_STARTB : T_ENDB] = b;
        a.ctl[w == 0 ? T_FIRST : T_LAST] = t;
    }
}

// ---- write -------------------------------------------------------------------------------------
template <bool AT_MARK>
__global__ __launch_bounds__(kOrdT) void k_text_write(TextArgs a) {
    __shared__ uint32_t lds[kOrdW];
    const uint64_t tile = (uint64_t)a.first_tile + blockIdx.x;
    if (tile >= a.ntiles) return;
    const uint64_t k0 = tile * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t len[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    text_load<AT_MARK>(a, k0, len, cpw, err);  // (k_text_count reported any error)
    uint32_t tot;
    uint64_t g = a.pbytes[tile] + block_excl_scan<kOrdW>(len[0] + len[1] + len[2] + len[3], lds, tot);
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        const uint32_t l = len[j], v = cpw[j];
        // (a boundary lies between two selected items: an item is inside the window or outside it)
        if (l && g >= a.start_bytes && g - a.start_bytes + l <= a.n_bytes) {
            uint8_t* o = a.out + (g - a.start_bytes);
            if (l == 1) {
                o[0] = (uint8_t)v;
            } else if (l == 2) {
                o[0] = (uint8_t)(0xC0u | (v >> 6));
                o[1] = (uint8_t)(0x80u | (v & 63u));
            } else if (l == 3) {
                o[0] = (uint8_t)(0xE0u | (v >> 12));
                o[1] = (uint8_t)(0x80u | ((v >> 6) & 63u));
                o[2] = (uint8_t)(0x80u | (v & 63u));
            } else {
                o[0] = (uint8_t)(0xF0u | (v >> 18));
                o[1] = (uint8_t)(0x80u | ((v >> 12) & 63u));
                o[2] = (uint8_t)(0x80u | ((v >> 6) & 63u));
                o[3] = (uint8_t)(0x80u | (v & 63u));
            }
        }
        g += l;
    }
}

template <bool AT_MARK>
int text_at_impl(Engine& E, Replica& r, TextArgs& a, bool bytes, uint64_t start, uint64_t end,
                 uint8_t* out, size_t cap, size_t* out_len, TextInfo* info, TextStats* stats) {
    hipStream_t s = E.stream;
    CallScratch sc(s);
    HIPTRY(E, sc.counters(T_N), "hipMalloc text counters");
    HIPTRY(E, sc.alloc(&a.tcnt, (uint64_t)a.ntiles), "hipMalloc text tiles");
    HIPTRY(E, sc.alloc(&a.tbytes, (uint64_t)a.ntiles), "hipMalloc text tiles");
    HIPTRY(E, sc.alloc(&a.pcnt, (uint64_t)a.ntiles), "hipMalloc text tiles");
    HIPTRY(E, sc.alloc(&a.pbytes, (uint64_t)a.ntiles), "hipMalloc text tiles");
    a.ctl = sc.ctl;
    HIPTRY(E, sc.time_begin(), "text event");
    k_text_init<<<1, 64, 0, s>>>(sc.ctl);
    k_text_count<AT_MARK><<<a.ntiles, kOrdT, 0, s>>>(a);
    k_text_top<AT_MARK><<<1, kOrdTop, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "text count kernels");
    HIPTRY(E, sc.time_end(), "text event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, T_N * 8, hipMemcpyDeviceToHost, s), "copy text counters");
    HIPTRY(E, hipStreamSynchronize(s), "text sync");  // the one wait: the totals and the window
    sc.time_add();
    if (stats) {
        stats->ranks = r.n;
        stats->device_ns = sc.dev_ns;
    }
    const uint64_t* h = sc.hctl;
    const uint64_t e = h[T_ERR];
    if (e & ET_SLOT) {
        E.err = "text: the kept document order names a slot that is no item";
        return CRDT_HIP_EBADLOG;
    }
    if (AT_MARK ? h[T_LEN] > a.n_mark : (h[T_LEN] != r.vis_cp || h[T_LENB] != r.vis_bytes)) {
        E.err = "text: the selected items of the kept order disagree with the replica's counters";
        return CRDT_HIP_EBADLOG;
    }
    const uint64_t total = bytes ? h[T_LENB] : h[T_LEN];
    const uint64_t endv = end == kTextEnd ? total : end;
    const bool in_range = start <= total && endv <= total, inside = (e & ET_INSIDE) != 0;
    TextInfo w{h[T_LEN], h[T_LENB], h[T_START], h[T_STARTB], h[T_END] - h[T_START],
               h[T_ENDB] - h[T_STARTB]};
    const uint64_t first = h[T_FIRST], last = h[T_LAST];
    if (in_range && !inside) {
        // what the kernels found is the window that was asked for, and its tiles exist
        const bool ok = !(e & ET_WALK) && h[T_END] >= h[T_START] && h[T_ENDB] >= h[T_STARTB] &&
                        (bytes ? h[T_STARTB] == start && h[T_ENDB] == endv
                               : h[T_START] == start && h[T_END] == endv) &&
                        h[T_ENDB] <= h[T_LENB] && w.n <= w.n_bytes && w.n_bytes <= 4 * w.n &&
                        (w.n_bytes == 0 || (first <= last && last < a.ntiles));
        if (!ok) {
            E.err = "text: a boundary's item is not where the tile prefixes say";
            return CRDT_HIP_EBADLOG;
        }
    }
    const int rc = text_check_window(start, endv, total, inside, w, out, cap, out_len, info, E.err);
    if (rc || w.n_bytes == 0) return rc;
    a.first_tile = (uint32_t)first;
    a.start_bytes = w.start_bytes;
    a.n_bytes = w.n_bytes;
    const uint32_t wtiles = (uint32_t)(last - first + 1);
    HIPTRY(E, sc.alloc(&a.out, w.n_bytes), "hipMalloc text");
    HIPTRY(E, sc.time_begin(), "text event");
    k_text_write<AT_MARK><<<wtiles, kOrdT, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "text write kernel");
    HIPTRY(E, sc.time_end(), "text event");
    HIPTRY(E, hipMemcpyAsync(out, a.out, w.n_bytes, hipMemcpyDeviceToHost, s), "copy text");
    HIPTRY(E, hipStreamSynchronize(s), "text sync");
    sc.time_add();
    if (stats) {
        stats->tiles_written = wtiles;
        stats->bytes = w.n_bytes;
        stats->device_ns = sc.dev_ns;
    }
    return CRDT_HIP_OK;
}

}  // namespace

int replica_text_at(Engine& E, Replica& r, const DeviceMark* m, uint64_t start, uint64_t end,
                    uint32_t flags, uint8_t* out, size_t cap, size_t* out_len, TextInfo* info,
                    TextStats* stats) {
    if (stats) *stats = TextStats{};
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    if (m && (r.n < m->n || !m->bits || m->words != ((uint64_t)m->n + 1 + 63) / 64)) {
        E.err = "the replica holds fewer items than the mark";
        return CRDT_HIP_EINVAL;
    }
    if ((rc = text_check(start, end, flags, out_len, E.err))) return rc;
    const bool bytes = (flags & kTextBytes) != 0;
    if (r.n == 0)  // nothing held: every version is empty (an empty replica may have no columns yet)
        return text_check_window(start, end == kTextEnd ? 0 : end, 0, false, TextInfo{}, out, cap,
                                 out_len, info, E.err);
    TextArgs a{};
    if ((rc = replica_kept_order(E, r, "text", &a.seq, &a.ntiles))) return rc;
    a.cp = r.logs.cp;
    a.n = r.n;
    a.start = start;
    a.end = end;
    a.bytes = bytes ? 1u : 0u;
    if (!m) return text_at_impl<false>(E, r, a, bytes, start, end, out, cap, out_len, info, stats);
    a.mark = m->bits;
    a.n_mark = m->n;
    a.mark_words = m->words;
    return text_at_impl<true>(E, r, a, bytes, start, end, out, cap, out_len, info, stats);
}

}  // namespace crdt
