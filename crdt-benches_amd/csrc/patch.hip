// patch.hip — patches since a mark of a device-resident replica (replica.hpp,
// crdt_hip_replica_mark / crdt_hip_replica_patches_since): what an update, a join or a delta
// changed in the document, as the reference's positional edits TestPatch(pos, del, ins) applied as
// Upstream::replace (rope.rs:21-32).  The semantics are stated in crdt_hip.h; the host twin is
// OpLog::patches_since (oplog.cpp), and both give the same patch array and the same bytes.
//
// A mark is the replica's item count and one bit per slot (1 = tombstoned or not an item).  After
// a merge_inc the replica keeps the document order of every item it holds (IncState::seq[cur],
// rank -> slot, tombstones included, RGA and Fugue alike), so the patches are a classification,
// a scan and a compaction over that order: a streaming pass, not another merge.
//
//   k_mark_pack      one pass over the 3-byte codepoint column: the wave ballots the tombstone
//                    flags and one lane stores each 64-bit word of the mark's bit plane
//   k_patch_classify a workgroup per tile of kOrderTile = 4,096 consecutive ranks, four ranks per
//                    thread (one 16-byte load of the order); per rank the slot's codepoint word
//                    and its mark bit are gathered (typing runs make both mostly coalesced) and
//                    the item is K (was and now), D (was, not now), I (now, not was) or nothing.
//                    A head is a D or I item whose previous K, D or I item is a K or does not
//                    exist: inside a thread the four items are walked in order; across the lanes
//                    of a wave the previous item comes from the ballot of the lanes that hold one
//                    (mask below the lane, highest set bit, shuffle of that lane's last class);
//                    across waves through LDS.  Per tile one aggregate: `now` items, D items, I
//                    bytes, the heads decided inside the tile, and the class of the tile's first
//                    and last K, D or I item (none: the tile holds nothing).  The tile's first
//                    item, if a D or an I, is left undecided.
//   k_patch_top      one workgroup scans the aggregates.  The carry is the associative "last seen
//                    class" operator (a max-scan of tile index << 2 | class over the tiles that
//                    hold something), so empty tiles pass their predecessor's class through; a
//                    tile's first D or I item is a head iff the carried class is K or the start
//                    of the document.  Exclusive prefixes per tile, and the totals: the host
//                    waits here, once, for the sizes of the outputs.
//   k_patch_write    classifies again (no per-rank class is stored, as k_enc_classify /
//                    k_enc_write of delta.hip do): each head h stores its pos (`now` items before
//                    it), the D items and the I bytes before it; each I item its UTF-8 at the I
//                    bytes before it
//   k_patch_finish   one thread per patch: del and ins_len are the differences to entry h + 1
//                    (the totals as the sentinel): D and I items occur only inside runs, so no
//                    thread walks a run
// No atomic decides an order; every index is checked against n, n_mark and the output sizes
// before use; the patch array and the text are copied out in one transfer each.
//
// The byte-offset reading (crdt_hip_replica_patches_since_bytes; crdt_hip.h, "byte offsets") is the
// BYTES instantiation of the same kernels: an item weighs its UTF-8 length instead of 1 in the
// `now` and D sums, the prefixes over the tiles are 64-bit, and k_patch_finish refuses a patch
// that deletes 4 GiB or more instead of truncating its del.
//
// Known cost: a call streams every rank of the replica however small the change, and after a join
// or a delta it also pays inc_rebuild's ORDER-mode merge with its host round trip for the order.
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "idtab.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// classes of an item (0: neither was nor now; also "no item" as a carried class)
constexpr uint32_t C_NONE = 0, C_K = 1, C_D = 2, C_I = 3;

// device counters (u64)
enum PCtl { P_ERR = 0, P_PATCHES, P_IBYTES, P_NOW, P_DEL, P_N };
// P_ERR bits, after E_ORD_SLOT (order.hpp)
constexpr uint64_t EP_RANGE = 2;  // (bytes) one patch deletes 4 GiB or more

// BYTES: pos and del count UTF-8 bytes instead of items (crdt_hip.h, "byte offsets").  A compile-
// time parameter of every kernel below: the codepoint instantiation weighs an item as the constant
// 1 and keeps 32-bit prefixes.  A tile of 4,096 ranks holds at most 16 KiB, so the sums inside a
// tile fit 32 bits either way; the prefixes over the tiles do not in bytes (a replica may hold more
// than 2^32 visible bytes) and are 64-bit there.
template <bool BYTES>
using PosW = typename std::conditional<BYTES, uint64_t, uint32_t>::type;
template <bool BYTES>
__device__ __forceinline__ uint32_t item_w(uint32_t cpw) {
    if constexpr (BYTES) return utf8_len(cpw);
    else return 1u;
}

struct TileAgg {
    uint32_t now, del, ibytes, heads;  // counts inside the tile (heads: the decided ones)
    uint32_t first, last;              // class of the tile's first / last K, D or I item
};
template <bool BYTES>
struct TilePre {
    uint64_t ibytes;                   // exclusive prefixes over the tiles before this one
    PosW<BYTES> now, del;
    uint32_t heads;
    uint32_t carry;                    // class of the last K, D or I item before the tile
};

template <bool BYTES>
struct PatchArgs {
    const uint32_t* seq;   // rank -> slot, ranks 0..n (rank 0 = slot 0, the document start)
    const uint8_t* cp;     // 3-byte codepoint words of slots 0..n
    SelMark was;           // alive at the mark
    uint32_t n;
    uint32_t ntiles;
    TileAgg* agg;
    TilePre<BYTES>* pre;
    // write pass (sizes as the host read them)
    uint32_t npatch;
    uint64_t nibytes;
    uint64_t* hpos;        // per head: `now` items, D items (or their bytes), I bytes before it
    PosW<BYTES>* hdel;
    uint64_t* hib;
    PatchRec* out;
    uint8_t* ins;
    uint64_t* ctl;
};

__global__ void k_patch_init(uint64_t* ctl) {
    if (threadIdx.x < (uint32_t)P_N) ctl[threadIdx.x] = 0;
}

// ---- mark --------------------------------------------------------------------------------------
// Slots 0..64 * words - 1, one per thread (a wave covers one word): bit = tombstoned, or not an
// item (slot 0 and the slots past n).
__global__ __launch_bounds__(kJB) void k_mark_pack(const uint8_t* cp, uint32_t n, uint64_t* bits,
                                                   uint64_t words) {
    const uint64_t s = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    const bool set = s == 0 || s > n || (cp3_get(cp, s) & kDelBit) != 0;
    const uint64_t b = __ballot(set);
    if ((threadIdx.x & 63u) == 0 && (s >> 6) < words) bits[s >> 6] = b;
}

// ---- classify ----------------------------------------------------------------------------------
// The classes and codepoints of the thread's four ranks k0..k0 + 3 (ranks past n, rank 0 and
// slots that are no item: C_NONE).
template <bool BYTES>
__device__ __forceinline__ void patch_load(const PatchArgs<BYTES>& a, uint64_t k0, uint32_t cls[kOrdPer],
                                           uint32_t cpw[kOrdPer], uint64_t& err) {
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        cls[j] = C_NONE;
        cpw[j] = 0;
    }
    order_load4(a.seq, a.cp, a.n, k0, err, E_ORD_SLOT, [&](uint32_t j, uint32_t s, uint32_t c) {
        const bool now = SelNow{}(s, c), was = a.was(s, c);
        cls[j] = was ? (now ? C_K : C_D) : (now ? C_I : C_NONE);
        cpw[j] = c & kDeltaCpMask;
    });
}

// What a thread's four items add up to.  `heads` counts the D or I items whose previous K, D or I
// item lies in the same thread and is a K; the thread's first item is decided by what precedes
// the thread (patch_incoming).
struct ThreadSum {
    uint32_t now, del, ibytes, heads, first, last;
};
template <bool BYTES>
__device__ __forceinline__ ThreadSum patch_sum(const uint32_t cls[kOrdPer],
                                               const uint32_t cpw[kOrdPer]) {
    ThreadSum t{0, 0, 0, 0, C_NONE, C_NONE};
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        const uint32_t c = cls[j];
        if (c == C_NONE) continue;
        if (c != C_D) t.now += item_w<BYTES>(cpw[j]);
        if (c == C_D) t.del += item_w<BYTES>(cpw[j]);
        if (c == C_I) t.ibytes += utf8_len(cpw[j]);
        if (t.last == C_NONE) t.first = c;
        else if (c != C_K && t.last == C_K) t.heads++;
        t.last = c;
    }
    return t;
}

// The class of the last K, D or I item of the tile before this thread's items (C_NONE: the tile
// holds none before them).  wlast: kOrdW entries of LDS.  Called by every thread of the block.
__device__ __forceinline__ uint32_t patch_incoming(uint32_t last, uint32_t* wlast) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t has = __ballot(last != C_NONE);
    // the wave's last class: that of its highest lane that holds an item
    const uint32_t top = has ? 63u - (uint32_t)__clzll((long long)has) : 0u;
    const uint32_t wl = (uint32_t)__shfl((int)last, (int)top);
    if (lane == 0) wlast[w] = has ? wl : C_NONE;
    const uint64_t below = has & ((1ull << lane) - 1ull);
    const uint32_t src = below ? 63u - (uint32_t)__clzll((long long)below) : 0u;
    const uint32_t inwave = (uint32_t)__shfl((int)last, (int)src);
    __syncthreads();
    uint32_t carry = C_NONE;  // the last class of the nearest earlier wave that holds an item
#pragma unroll
    for (uint32_t i = 0; i < kOrdW; ++i) {
        const uint32_t x = wlast[i];
        if (i < w && x != C_NONE) carry = x;
    }
    __syncthreads();
    return below ? inwave : carry;
}

template <bool BYTES>
__global__ __launch_bounds__(kOrdT) void k_patch_classify(PatchArgs<BYTES> a) {
    __shared__ uint32_t red[kOrdW];
    __shared__ uint32_t wfirst[kOrdW];
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t cls[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    patch_load(a, k0, cls, cpw, err);
    ctl_or(&a.ctl[P_ERR], err);
    const ThreadSum t = patch_sum<BYTES>(cls, cpw);
    const uint32_t inc = patch_incoming(t.last, red);
    // the thread's first item: a head iff it is a D or an I behind a K (behind nothing: the
    // tile's first item, left to k_patch_top)
    const uint32_t heads = t.heads + (t.first >= C_D && inc == C_K ? 1u : 0u);
    // the tile's first class: that of the lowest thread that holds an item; its last class: what
    // a thread behind the last one would see coming in
    const uint64_t has = __ballot(t.first != C_NONE);
    const uint32_t low = has ? (uint32_t)__ffsll((long long)has) - 1u : 0u;
    const uint32_t wf = (uint32_t)__shfl((int)t.first, (int)low);
    if ((threadIdx.x & 63u) == 0) wfirst[threadIdx.x >> 6] = has ? wf : C_NONE;
    __syncthreads();
    uint32_t first = C_NONE, last = C_NONE;
    if (threadIdx.x == kOrdT - 1) {
        for (uint32_t i = kOrdW; i-- > 0;)
            if (wfirst[i] != C_NONE) first = wfirst[i];
        last = t.last != C_NONE ? t.last : inc;
    }
    __syncthreads();
    const uint32_t s_now = block_sum_t0<kOrdW>(t.now, red), s_del = block_sum_t0<kOrdW>(t.del, red);
    const uint32_t s_ib = block_sum_t0<kOrdW>(t.ibytes, red), s_h = block_sum_t0<kOrdW>(heads, red);
    if (threadIdx.x == 0 && blockIdx.x < a.ntiles) {
        a.agg[blockIdx.x].now = s_now;
        a.agg[blockIdx.x].del = s_del;
        a.agg[blockIdx.x].ibytes = s_ib;
        a.agg[blockIdx.x].heads = s_h;
    }
    if (threadIdx.x == kOrdT - 1 && blockIdx.x < a.ntiles) {
        a.agg[blockIdx.x].first = first;
        a.agg[blockIdx.x].last = last;
    }
}

// ---- top ---------------------------------------------------------------------------------------
// Exclusive max-scan over the block's threads; `total`: the block's max.
template <int NW>
__device__ __forceinline__ uint32_t block_excl_max(uint32_t x, uint32_t* lds, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= (uint32_t)o) inc = max(inc, y);
    }
    if (lane == 63) lds[w] = inc;
    const uint32_t prev = (uint32_t)__shfl_up((int)inc, 1);
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)NW; ++i) {
        const uint32_t t = lds[i];
        if (i < w) off = max(off, t);
        tot = max(tot, t);
    }
    __syncthreads();
    total = tot;
    return lane ? max(off, prev) : off;
}

template <bool BYTES>
__global__ __launch_bounds__(kOrdTop) void k_patch_top(PatchArgs<BYTES> a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    uint64_t c_now = 0, c_del = 0, c_ib = 0, c_heads = 0;
    uint32_t c_last = 0;  // (tile index + 1) << 2 | class of the last tile so far that holds an item
    for (uint32_t base = 0; base < a.ntiles; base += kOrdTop) {
        const uint32_t i = base + threadIdx.x;
        TileAgg g{0, 0, 0, 0, C_NONE, C_NONE};
        if (i < a.ntiles) g = a.agg[i];
        uint32_t tot;
        const uint32_t seen = max(c_last, block_excl_max<kOrdTop / 64>(g.last != C_NONE ? ((i + 1u) << 2) | g.last : 0u, lds, tot));
        c_last = max(c_last, tot);
        const uint32_t carry = seen & 3u;  // (C_NONE: the start of the document)
        const uint32_t heads = g.heads + (g.first >= C_D && (carry == C_K || carry == C_NONE) ? 1u : 0u);
        TilePre<BYTES> p;
        p.carry = carry;
        p.now = (PosW<BYTES>)c_now + block_excl_scan<kOrdTop / 64>(g.now, lds, tot);
        c_now += tot;
        p.del = (PosW<BYTES>)c_del + block_excl_scan<kOrdTop / 64>(g.del, lds, tot);
        c_del += tot;
        p.ibytes = c_ib + block_excl_scan<kOrdTop / 64>(g.ibytes, lds, tot);
        c_ib += tot;
        p.heads = (uint32_t)c_heads + block_excl_scan<kOrdTop / 64>(heads, lds, tot);
        c_heads += tot;
        if (i < a.ntiles) a.pre[i] = p;
    }
    if (threadIdx.x == 0) {
        a.ctl[P_PATCHES] = c_heads;
        a.ctl[P_IBYTES] = c_ib;
        a.ctl[P_NOW] = c_now;
        a.ctl[P_DEL] = c_del;
    }
}

// ---- write -------------------------------------------------------------------------------------
template <bool BYTES>
__global__ __launch_bounds__(kOrdT) void k_patch_write(PatchArgs<BYTES> a) {
    __shared__ uint32_t lds[kOrdW];
    if (blockIdx.x >= a.ntiles) return;
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t cls[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    patch_load(a, k0, cls, cpw, err);  // (k_patch_classify reported any error)
    const ThreadSum t = patch_sum<BYTES>(cls, cpw);
    const TilePre<BYTES> p = a.pre[blockIdx.x];
    uint32_t inc = patch_incoming(t.last, lds);
    // nothing before the thread in its tile: what the tiles before carry (the start of the
    // document opens a run like a K does)
    if (inc == C_NONE) inc = p.carry == C_NONE ? C_K : p.carry;
    const uint32_t heads = t.heads + (t.first >= C_D && inc == C_K ? 1u : 0u);
    uint32_t tot;
    uint64_t now = (uint64_t)p.now + block_excl_scan<kOrdW>(t.now, lds, tot);
    PosW<BYTES> del = p.del + block_excl_scan<kOrdW>(t.del, lds, tot);
    uint64_t ib = p.ibytes + block_excl_scan<kOrdW>(t.ibytes, lds, tot);
    uint32_t h = p.heads + block_excl_scan<kOrdW>(heads, lds, tot);
    uint32_t prev = inc;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        const uint32_t c = cls[j];
        if (c == C_NONE) continue;
        if (c != C_K && prev == C_K) {
            if (h < a.npatch) {
                a.hpos[h] = now;
                a.hdel[h] = del;
                a.hib[h] = ib;
            }
            ++h;
        }
        if (c == C_I) {
            const uint32_t v = cpw[j], len = utf8_len(v);
            if (ib + len <= a.nibytes) utf8_store(a.ins + ib, v, len);
            ib += len;
        }
        if (c == C_D) del += item_w<BYTES>(cpw[j]);
        else now += item_w<BYTES>(cpw[j]);
        prev = c;
    }
}

template <bool BYTES>
__global__ __launch_bounds__(kJB) void k_patch_finish(PatchArgs<BYTES> a, PosW<BYTES> total_del) {
    const uint32_t h = blockIdx.x * kJB + threadIdx.x;
    if (h >= a.npatch) return;
    const bool lastp = h + 1u == a.npatch;
    const PosW<BYTES> d1 = lastp ? total_del : a.hdel[h + 1u];
    const uint64_t b1 = lastp ? a.nibytes : a.hib[h + 1u];
    PatchRec r;
    r.pos = a.hpos[h];
    r.ins_off = a.hib[h];
    r.del = (uint32_t)(d1 - a.hdel[h]);
    if constexpr (BYTES) {  // del is a uint32_t: 4 GiB or more is an error, never a truncation
        if (d1 - a.hdel[h] >= (1ull << 32)) {
            ctl_or(&a.ctl[P_ERR], EP_RANGE);
            r.del = 0xFFFFFFFFu;
        }
    }
    r.ins_len = (uint32_t)(b1 - a.hib[h]);
    a.out[h] = r;
}

}  // namespace

// ---- host side ---------------------------------------------------------------------------------
DeviceMark::~DeviceMark() {
    if (bits) pool_free(bits);
}

int replica_mark(Engine& E, Replica& r, DeviceMark& m) {
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    const uint64_t words = ((uint64_t)r.n + 1 + 63) / 64;
    // slots 0..64 * words - 1 are read where they are at most n: inside the column
    if ((uint64_t)r.n + 1 > r.logs.cap_slots && r.n) {
        E.err = "mark: replica smaller than its item count";
        return CRDT_HIP_EINVAL;
    }
    if (m.bits) {
        pool_free(m.bits);
        m.bits = nullptr;
    }
    HIPTRY(E, dalloc(&m.bits, words), "hipMalloc mark");
    m.n = r.n;
    m.words = words;
    if (r.n == 0) {  // (an empty replica may have no columns yet)
        const uint64_t all = ~0ull;
        HIPTRY(E, hipMemcpy(m.bits, &all, 8, hipMemcpyHostToDevice), "mark");
        return CRDT_HIP_OK;
    }
    k_mark_pack<<<grid_for(words * 64, kJB), kJB, 0, E.stream>>>(r.logs.cp, r.n, m.bits, words);
    HIPTRY(E, hipGetLastError(), "mark kernel");
    HIPTRY(E, hipStreamSynchronize(E.stream), "mark sync");
    return CRDT_HIP_OK;
}

namespace {
template <bool BYTES>
int patches_since_impl(Engine& E, Replica& r, const DeviceMark& m, PatchRec* out, size_t cap,
                       size_t* out_n, uint8_t* ins, size_t ins_cap, size_t* out_ins,
                       PatchStats* stats) {
    if (stats) *stats = PatchStats{};
    *out_n = 0;
    *out_ins = 0;
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    if ((rc = mark_fits(E, r, m))) return rc;
    if (r.n == 0) return CRDT_HIP_OK;  // nothing held: nothing changed
    PatchArgs<BYTES> a{};
    rc = replica_kept_order(E, r, "patches", &a.seq, &a.ntiles);
    if (rc) return rc;
    hipStream_t s = E.stream;
    CallScratch sc(s);
    a.cp = r.logs.cp;
    a.was = SelMark{{m.bits, m.n, m.words}};
    a.n = r.n;
    HIPTRY(E, sc.counters(P_N), "hipMalloc patch counters");
    HIPTRY(E, sc.alloc(&a.agg, (uint64_t)a.ntiles), "hipMalloc patch tiles");
    HIPTRY(E, sc.alloc(&a.pre, (uint64_t)a.ntiles), "hipMalloc patch tiles");
    a.ctl = sc.ctl;
    HIPTRY(E, sc.time_begin(), "patch event");
    k_patch_init<<<1, 64, 0, s>>>(sc.ctl);
    k_patch_classify<BYTES><<<a.ntiles, kOrdT, 0, s>>>(a);
    k_patch_top<BYTES><<<1, kOrdTop, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "patch classify kernels");
    HIPTRY(E, sc.time_end(), "patch event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, P_N * 8, hipMemcpyDeviceToHost, s), "copy patch counters");
    HIPTRY(E, hipStreamSynchronize(s), "patch sync");  // the one wait: the sizes
    sc.time_add();
    if (sc.hctl[P_ERR]) {
        E.err = "patches: the kept document order names a slot that is no item";
        return CRDT_HIP_EBADLOG;
    }
    if (sc.hctl[P_NOW] != (BYTES ? r.vis_bytes : r.vis_cp)) {
        E.err = "patches: the visible items of the kept order disagree with the replica's counter";
        return CRDT_HIP_EBADLOG;
    }
    const uint64_t np = sc.hctl[P_PATCHES], nib = sc.hctl[P_IBYTES];
    if (stats) {
        stats->patches = np;
        stats->ins_bytes = nib;
        stats->ranks = r.n;
        stats->device_ns = sc.dev_ns;
    }
    if (np >= (1ull << 32) || nib >= (1ull << 32) || np > r.n || nib > 4ull * r.n) {
        E.err = "patches: 2^32 or more patches, or 4 GiB or more of inserted bytes";
        return CRDT_HIP_ERANGE;
    }
    *out_n = (size_t)np;
    *out_ins = (size_t)nib;
    if ((np && (!out || cap < np)) || (nib && (!ins || ins_cap < nib))) {
        E.err = "buffer too small";
        return CRDT_HIP_ESPACE;
    }
    if (np == 0) return CRDT_HIP_OK;
    a.npatch = (uint32_t)np;
    a.nibytes = nib;
    HIPTRY(E, sc.alloc(&a.hpos, np), "hipMalloc patch heads");
    HIPTRY(E, sc.alloc(&a.hdel, np), "hipMalloc patch heads");
    HIPTRY(E, sc.alloc(&a.hib, np), "hipMalloc patch heads");
    HIPTRY(E, sc.alloc(&a.out, np), "hipMalloc patches");
    HIPTRY(E, sc.alloc(&a.ins, nib), "hipMalloc patch text");
    HIPTRY(E, sc.time_begin(), "patch event");
    k_patch_write<BYTES><<<a.ntiles, kOrdT, 0, s>>>(a);
    k_patch_finish<BYTES><<<grid_for(np, kJB), kJB, 0, s>>>(a, (PosW<BYTES>)sc.hctl[P_DEL]);
    HIPTRY(E, hipGetLastError(), "patch write kernels");
    HIPTRY(E, sc.time_end(), "patch event");
    HIPTRY(E, hipMemcpyAsync(out, a.out, np * sizeof(PatchRec), hipMemcpyDeviceToHost, s), "copy patches");
    if (nib) HIPTRY(E, hipMemcpyAsync(ins, a.ins, nib, hipMemcpyDeviceToHost, s), "copy patch text");
    if (BYTES)  // (k_patch_finish may have raised EP_RANGE: the same wait brings it back)
        HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, 8, hipMemcpyDeviceToHost, s), "copy patch counters");
    HIPTRY(E, hipStreamSynchronize(s), "patch sync");
    sc.time_add();
    if (stats) stats->device_ns = sc.dev_ns;
    if (BYTES && sc.hctl[P_ERR]) {
        E.err = "patches: a patch deletes 4 GiB or more";
        return CRDT_HIP_ERANGE;
    }
    return CRDT_HIP_OK;
}
}  // namespace

int replica_patches_since(Engine& E, Replica& r, const DeviceMark& m, PatchRec* out, size_t cap,
                          size_t* out_n, uint8_t* ins, size_t ins_cap, size_t* out_ins,
                          PatchStats* stats) {
    return patches_since_impl<false>(E, r, m, out, cap, out_n, ins, ins_cap, out_ins, stats);
}
int replica_patches_since_bytes(Engine& E, Replica& r, const DeviceMark& m, PatchRec* out,
                                size_t cap, size_t* out_n, uint8_t* ins, size_t ins_cap,
                                size_t* out_ins, PatchStats* stats) {
    return patches_since_impl<true>(E, r, m, out, cap, out_n, ins, ins_cap, out_ins, stats);
}

}  // namespace crdt
