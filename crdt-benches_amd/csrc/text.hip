// text.hip — text windows of a device-resident replica (replica.hpp, crdt_hip_replica_text_at): a
// range of the document, now or at a mark, as UTF-8 and nothing else.  The semantics are stated in
// crdt_hip.h, "text windows"; the host twin is OpLog::text_at (oplog.cpp), and both give the same
// bytes and the same crdt_hip_text_info.
//
// A version selects items: NOW the ones that are not tombstoned, AT_MARK the ones the mark saw alive
// (slot <= n_mark and its bit in the mark's plane clear).  After a merge_inc the replica keeps the
// document order of every item it holds (IncState::seq[cur], rank -> slot, tombstones included, RGA
// and Fugue alike), and later items never reorder earlier ones, so either version's text is a count,
// a scan and a compaction over that order under the version's selector (SelNow or SelMark,
// order.hpp), the one template parameter of every kernel here:
//
//   k_text_count  a workgroup per tile of kOrderTile = 4,096 consecutive ranks, four ranks per
//                 thread (order_tile_count); per tile the selected codepoints and their UTF-8 bytes.
//                 SelMark never reads the plane for a slot above n_mark or a word at or past its
//                 words.
//   k_text_top    one workgroup scans the tile aggregates into exclusive prefixes (order_tile_scan:
//                 32-bit for the codepoints, 64-bit for the bytes) and the version's totals.  Then a
//                 wave per boundary (`start`, `end`) seeks it in the unit asked (view_seek,
//                 view.hpp: the last tile that begins before the boundary, and a walk of it to the
//                 selected item that ends at the boundary): its inclusive prefixes are the boundary
//                 in codepoints and bytes.  In bytes an item that steps over the boundary raises
//                 ET_INSIDE.  A thread each then finds the window's first and last tile in the byte
//                 prefixes and writes the totals, the window in both units, the two tiles and the
//                 error bits: the host waits here, once, runs the checks of crdt_hip.h and returns
//                 ESPACE without a write pass.
//   k_text_write  a workgroup per tile in [first tile, last tile] only (a 4 KiB viewport of a
//                 200 k-item replica: one or two workgroups, not 50): selects again (no per-rank
//                 class is stored, as in patch.hip), scans the thread sums and every selected item
//                 stores its UTF-8 at (tile byte prefix + bytes before it in the tile - start_bytes)
//                 when that lies inside the window.  The bytes go straight from registers to the
//                 output, as k_patch_write places its I bytes: a typing run's stores are consecutive
//                 across the lanes, and a viewport's one or two tiles leave nothing for an LDS
//                 staging pass to win.
// No atomic decides an order (an OR raises an error bit); every slot, tile and mark word is checked
// against n, n_mark, the mark's words and ntiles before use, every store against the window's bytes,
// which is what the output buffer holds; every loop is bounded (a search by the tiles, a walk by the
// tile).  The result is copied out in one transfer.
//
// Known cost: a call streams every rank of the replica once (the count), however small the window,
// and after a join or a delta it also pays inc_rebuild's ORDER-mode merge.
#include <cstring>
#include <type_traits>

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
enum TCtl { T_ERR = 0, T_LEN, T_LENB, T_START, T_STARTB, T_END, T_ENDB, T_FIRST, T_LAST, T_N };
// T_ERR bits, after E_ORD_SLOT (order.hpp)
constexpr uint64_t ET_RANGE = 2;   // start or end beyond the version (the host says which)
constexpr uint64_t ET_INSIDE = 4;  // (bytes) a boundary inside a codepoint
constexpr uint64_t ET_WALK = 8;    // a boundary's item is not in the tile the prefixes name

template <class Sel>
struct TextArgs {
    OrderView v;           // the kept order (rank, key and vis: not used) and the version's prefixes
    Sel sel;               // the version
    uint32_t* tcount;      // v.tcount and v.tbpre as the count and the scan write them
    uint32_t* tbytes;      // per tile: the selected UTF-8 bytes (at most 16 KiB)
    uint64_t* tbpre;
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

// ---- count -------------------------------------------------------------------------------------
template <class Sel>
__global__ __launch_bounds__(kOrdT) void k_text_count(TextArgs<Sel> a) {
    __shared__ uint32_t red[kOrdW];
    order_tile_count(a.v.seq, a.v.cp, a.v.n, a.sel, a.v.ntiles, a.tcount, a.tbytes, &a.ctl[T_ERR], red);
}

// ---- top ---------------------------------------------------------------------------------------
// The boundary 0 < p < total of the version, in the unit asked, as (codepoints, bytes): the
// inclusive prefixes of the selected item that ends at p.  Called by a whole wave with a
// wave-uniform p; the item's lane stores into res[0..1].
template <class Sel>
__device__ __forceinline__ void text_boundary(const TextArgs<Sel>& a, uint64_t p, uint32_t lane,
                                              uint64_t* res, uint64_t& err) {
    const bool found = view_seek(a.v, a.sel, a.bytes != 0, p, lane, err,
                                 [&](uint64_t inc_c, uint64_t inc_b, uint32_t, uint32_t) {
                                     if ((a.bytes ? inc_b : inc_c) == p) {
                                         res[0] = inc_c;
                                         res[1] = inc_b;
                                     } else {
                                         err |= ET_INSIDE;
                                     }
                                 });
    if (!found) err |= ET_WALK;
}

template <class Sel>
__global__ __launch_bounds__(kOrdTop) void k_text_top(TextArgs<Sel> a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    __shared__ uint64_t bnd[2][2];  // start, end: codepoints and bytes before the boundary
    if (threadIdx.x < 4u) bnd[threadIdx.x >> 1][threadIdx.x & 1u] = 0;
    uint64_t c_cnt, c_by;
    order_tile_scan(a.v.ntiles, a.tcount, a.tbytes, a.tbpre, lds, c_cnt, c_by);
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
            text_boundary(a, p, lane, bnd[w], err);
        }
        ctl_or(&a.ctl[T_ERR], err);
    }
    __syncthreads();
    // the window's first item lies in the last tile that begins at or before start_bytes, its last
    // item in the last tile that begins before end_bytes (tile 0 begins at 0); a thread each
    if (lane == 0 && w < 2u) {
        const uint64_t b = bnd[w][1];
        uint32_t t = 0;
        for (uint32_t lo = 0, hi = a.v.ntiles; hi - lo > 1u;) {
            const uint32_t mid = (lo + hi) >> 1;
            if (w == 0 ? a.v.tbpre[mid] <= b : a.v.tbpre[mid] < b) t = lo = mid;
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
template <class Sel>
__global__ __launch_bounds__(kOrdT) void k_text_write(TextArgs<Sel> a) {
    __shared__ uint32_t lds[kOrdW];
    const uint64_t tile = (uint64_t)a.first_tile + blockIdx.x;
    if (tile >= a.v.ntiles) return;
    const uint64_t k0 = tile * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t len[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    order_lens4(a.v.seq, a.v.cp, a.v.n, a.sel, k0, len, cpw, err);  // (k_text_count reported any error)
    uint32_t tot;
    uint64_t g = a.v.tbpre[tile] + block_excl_scan<kOrdW>(len[0] + len[1] + len[2] + len[3], lds, tot);
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        const uint32_t l = len[j];
        // (a boundary lies between two selected items: an item is inside the window or outside it)
        if (l && g >= a.start_bytes && g - a.start_bytes + l <= a.n_bytes)
            utf8_store(a.out + (g - a.start_bytes), cpw[j], l);
        g += l;
    }
}

template <class Sel>
int text_at_impl(Engine& E, Replica& r, const OrderView& v, const Sel& sel, bool bytes,
                 uint64_t start, uint64_t end, uint8_t* out, size_t cap, size_t* out_len, TextInfo* info,
                 TextStats* stats) {
    hipStream_t s = E.stream;
    CallScratch sc(s);
    const uint32_t ntiles = v.ntiles;
    TextArgs<Sel> a{};
    a.v = v;
    a.sel = sel;
    a.start = start;
    a.end = end;
    a.bytes = bytes ? 1u : 0u;
    HIPTRY(E, sc.counters(T_N), "hipMalloc text counters");
    HIPTRY(E, sc.alloc(&a.tcount, (uint64_t)ntiles), "hipMalloc text tiles");
    HIPTRY(E, sc.alloc(&a.tbytes, (uint64_t)ntiles), "hipMalloc text tiles");
    HIPTRY(E, sc.alloc(&a.tbpre, (uint64_t)ntiles), "hipMalloc text tiles");
    a.v.tcount = a.tcount;
    a.v.tbpre = a.tbpre;
    a.ctl = sc.ctl;
    HIPTRY(E, sc.time_begin(), "text event");
    k_text_init<<<1, 64, 0, s>>>(sc.ctl);
    k_text_count<<<ntiles, kOrdT, 0, s>>>(a);
    k_text_top<<<1, kOrdTop, 0, s>>>(a);
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
    if (e & E_ORD_SLOT) {
        E.err = "text: the kept document order names a slot that is no item";
        return CRDT_HIP_EBADLOG;
    }
    bool off;
    if constexpr (std::is_same<Sel, SelMark>::value) off = h[T_LEN] > sel.m.n_mark;
    else off = h[T_LEN] != r.vis_cp || h[T_LENB] != r.vis_bytes;
    if (off) {
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
                        (w.n_bytes == 0 || (first <= last && last < ntiles));
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
    k_text_write<<<wtiles, kOrdT, 0, s>>>(a);
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
    if (m && (rc = mark_fits(E, r, *m))) return rc;
    if ((rc = text_check(start, end, flags, out_len, E.err))) return rc;
    const bool bytes = (flags & kTextBytes) != 0;
    if (r.n == 0)  // nothing held: every version is empty (an empty replica may have no columns yet)
        return text_check_window(start, end == kTextEnd ? 0 : end, 0, false, TextInfo{}, out, cap,
                                 out_len, info, E.err);
    OrderView v{};
    if ((rc = replica_kept_order(E, r, "text", &v.seq, &v.ntiles))) return rc;
    v.cp = r.logs.cp;
    v.n = r.n;
    if (!m) return text_at_impl(E, r, v, SelNow{}, bytes, start, end, out, cap, out_len, info, stats);
    return text_at_impl(E, r, v, SelMark{{m->bits, m->n, m->words}}, bytes, start, end, out, cap, out_len,
                        info, stats);
}

}  // namespace crdt
