// anchor.hip — anchors on a device-resident replica (replica.hpp, crdt_hip_replica_anchors_at /
// _at_bytes / _resolve): cursor and selection positions named by the identity of the item next to
// the gap, so that they survive every sync and mean the same place on every peer.  The semantics
// are stated in crdt_hip.h, "anchors"; the host twins are OpLog::anchors_at and
// OpLog::anchors_resolve (oplog.cpp), and both sides return the same arrays byte for byte.
//
// Both directions work over the document order the replica keeps after a merge_inc
// (IncState::seq[cur], rank -> slot, tombstones included) and start with the count and scan of
// bytes.hip (bytes_count_enqueue): per tile of kOrderTile = 4,096 ranks the visible codepoints and
// their UTF-8 bytes, then the exclusive prefixes of both (64-bit for the bytes) and the totals.
//
// resolve (anchors -> positions)
//   k_anchor_init     counters; the identity table cleared; per anchor its id copied into a
//                     contiguous column and its slot set to "not found" (locate_clear)
//   k_locate_insert   (locate.hpp) the distinct identities of the batch into an open-addressing table
//                     of at least twice as many entries as anchors
//   k_locate_probe    (locate.hpp) a grid-stride pass over the key column: every item looks its
//                     identity up and, on a hit, records its slot for the entry
//   k_anchor_resolve  a wave per anchor: slot -> rank from the kept inverse order (locate_rank), the
//                     tile's exclusive prefixes, and the visible ranks of the tile before `rank`, 64
//                     ranks a step (view_walk: ballot and popcount for the codepoints, a wave sum for
//                     the bytes)
// create (positions -> anchors)
//   k_anchor_create   a wave per position: a binary search of the scanned prefixes for the tile that
//                     holds the first visible item whose inclusive prefix reaches the position (AFTER)
//                     or passes it (BEFORE), then a walk of that tile 64 ranks a step with a wave
//                     scan (seek_tile and seek_step, view.hpp); the item's lane writes
//                     jident(key[slot]).  In bytes an item whose prefix steps over the position
//                     without meeting it raises EA_INSIDE (EINVAL)
//
// Per position a search, not every visible item searching a sorted position table as
// k_edit_resolve does: positions come unsorted and repeated, a cursor batch is small, and a walk
// touches one tile per position where the table form would gather every rank's codepoint word a
// second time.
//
// No atomic decides an order (locate.hpp says why for the table's CAS and the slot's min; here an
// OR raises an error bit and one add per block counts the unknown); every slot, rank, tile and
// table index is checked against n and the sizes of the call before use and a bad value raises an
// A_ERR bit instead of becoming an address; every loop is bounded (a probe by the table size, a
// walk by the tile); no host copy of the replica's columns is made, and the host waits once.
//
// Known cost: a call streams every rank of the replica once (the count), and a resolve every key
// as well, however few the anchors; after a join or a delta it first pays inc_rebuild's ORDER-mode
// merge.
#include <cstring>
#include <vector>

#include "bytes.hpp"
#include "idtab.hpp"
#include "locate.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// device counters (u64), after the B_N of the count
enum ACtl { A_ERR = 0, A_UNKNOWN, A_N };
// A_ERR bits, after E_ORD_SLOT (order.hpp), EL_RANK and EL_TABLE (locate.hpp)
constexpr uint64_t EA_INSIDE = 8;  // a byte position inside a codepoint
constexpr uint64_t EA_WALK = 16;   // a position's item is not in the tile the prefixes name

constexpr uint32_t kAncW = kJB / 64;  // anchors (waves) per workgroup

struct AnchorArgs {
    OrderView v;
    uint32_t fugue;
    uint32_t m;              // anchors (resolve) or positions (create) of the call
    // resolve
    const AnchorRec* anc;
    IdLookup l;              // (ids: anc[i].id)
    AnchorPosRec* pout;
    // create
    const uint64_t* pos;
    const uint8_t* bias;     // (null: all AFTER)
    AnchorRec* aout;
    uint64_t* ctl;
};

__global__ __launch_bounds__(kJB) void k_anchor_init(AnchorArgs a, uint32_t resolve) {
    const uint64_t g = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    if (g < (uint64_t)A_N) a.ctl[g] = 0;
    if (!resolve) return;
    locate_clear(a.l, g);
    if (g < a.m) a.l.ids[g] = a.anc[g].id;
}

// A wave per anchor.  Everything that branches depends on the anchor alone, so a wave stays whole
// through the ballots and the wave sum.
__global__ __launch_bounds__(kJB) void k_anchor_resolve(AnchorArgs a) {
    __shared__ uint32_t unk[kAncW];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * kAncW + w;
    uint64_t err = 0;
    uint32_t unknown = 0;
    if (i < a.m) {
        const AnchorRec an = a.anc[i];
        AnchorPosRec o{0, 0, kAnchorLive, 0u};
        if (an.id == kAnchorEdge) {
            if (an.bias == kAnchorBefore) {
                o.pos = a.v.vis[0];
                o.pos_bytes = a.v.vis[1];
            }
        } else {
            uint32_t s, rk;
            const Loc at = locate_rank(a.l, a.v, (uint32_t)i, s, rk, err);
            if (at == Loc::Unknown) {
                o.state = kAnchorUnknown;
                unknown = 1;
            } else if (at == Loc::Found) {
                const uint32_t cw = cp3_get(a.v.cp, s);  // (whole, and in flight during the walk)
                view_walk(a.v, rk / kOrderTile, rk, lane, o.pos, o.pos_bytes, err);  // (rk <= n)
                const bool live = !(cw & kDelBit);
                const bool add = live && an.bias == kAnchorAfter;
                o.pos += add ? 1u : 0u;
                o.pos_bytes += add ? utf8_len(cw & kDeltaCpMask) : 0u;
                o.state = live ? kAnchorLive : kAnchorDead;
            }
        }
        if (lane == 0) a.pout[i] = o;
    }
    ctl_or(&a.ctl[A_ERR], err);
    if (lane == 0) unk[w] = unknown;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t j = 0; j < kAncW; ++j) t += unk[j];
        if (t) atomicAdd((unsigned long long*)&a.ctl[A_UNKNOWN], (unsigned long long)t);
    }
}

// A wave per position; an item weighs 1 (codepoints) or its UTF-8 length (BYTES).
template <bool BYTES>
__global__ __launch_bounds__(kJB) void k_anchor_create(AnchorArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kAncW + (threadIdx.x >> 6);
    if (i >= a.m) return;
    uint64_t err = 0;
    const uint64_t p = a.pos[i];
    const uint32_t b = a.bias ? (uint32_t)a.bias[i] : kAnchorAfter;
    const uint64_t total = a.v.vis[BYTES ? 1 : 0];
    AnchorRec o{kAnchorEdge, b, 0u};
    if (b == kAnchorAfter ? p == 0 : p >= total) {  // the document start, the document end
        if (lane == 0) a.aout[i] = o;
        return;
    }
    // the item: the first visible one whose inclusive prefix is at least thr (thr >= 1)
    // (seek_tile and seek_step of view.hpp, a step's loads as the walk goes: view_seek's chunks of
    // 16 steps take 69 / 72 VGPRs and 104 SGPRs here and the kernel to 7 waves a SIMD)
    const uint64_t thr = b == kAnchorAfter ? p : p + 1;
    Seek f = seek_tile(a.v, BYTES, thr);
    for (uint32_t st = 0; st < kOrderTile / 64u && !f.found; ++st) {
        uint32_t sl;
        const uint32_t len = order_len_at(a.v.seq, a.v.cp, a.v.n, SelNow{},
                                          (uint64_t)f.tile * kOrderTile + st * 64u + lane, sl, err);
        seek_step(f, BYTES, thr, lane, len, sl, [&](uint64_t inc_c, uint64_t inc_b, uint32_t l, uint32_t s) {
            // AFTER: the item ends at p.  BEFORE: it starts at p.  (In codepoints always so.)
            const uint64_t inc = BYTES ? inc_b : inc_c;
            if (b == kAnchorAfter ? inc == p : inc - (BYTES ? l : 1u) == p) {
                const uint64_t k = a.v.key[s];
                o.id = a.fugue ? jident<true>(k) : jident<false>(k);
                a.aout[i] = o;
            } else {
                err |= EA_INSIDE;
            }
        });
    }
    if (!f.found) err |= EA_WALK;
    ctl_or(&a.ctl[A_ERR], err);
}

// What both directions share: the kept order with its inverse, the scratch, the count and scan.
struct AnchorCall {
    CallScratch sc;
    BytesArgs b{};
    AnchorArgs a{};
    explicit AnchorCall(hipStream_t s) : sc(s) {}
};

int anchor_begin(Engine& E, Replica& r, AnchorCall& c, size_t m) {
    AnchorArgs& a = c.a;
    int rc = replica_kept_ranks(E, r, "anchors", &a.v.seq, &a.v.rank, &a.v.ntiles);
    if (rc) return rc;
    HIPTRY(E, c.sc.counters(B_N + A_N), "hipMalloc anchor counters");
    HIPTRY(E, bytes_count_args(c.b, c.sc, r, a.v.seq, a.v.ntiles, c.sc.ctl), "hipMalloc anchor tiles");
    a.v.cp = r.logs.cp;
    a.v.key = r.logs.key;
    a.v.n = r.n;
    a.v.tcount = c.b.tcount;
    a.v.tbpre = c.b.tbpre;
    a.v.vis = c.sc.ctl + B_VIS;
    static_assert(B_VISB == B_VIS + 1, "vis[1] is the visible bytes");
    a.fugue = r.logs.fugue ? 1u : 0u;
    a.m = (uint32_t)m;
    a.ctl = c.sc.ctl + B_N;
    return CRDT_HIP_OK;
}

// After the kernels: the counters and the results come back in the one wait; then every check.
template <class T>
int anchor_end(Engine& E, Replica& r, AnchorCall& c, const T* dev, std::vector<T>& host) {
    hipStream_t s = c.sc.stream;
    HIPTRY(E, hipGetLastError(), "anchor kernels");
    HIPTRY(E, c.sc.time_end(), "anchor event");
    HIPTRY(E, hipMemcpyAsync(c.sc.hctl, c.sc.ctl, (B_N + A_N) * 8, hipMemcpyDeviceToHost, s),
              "copy anchor counters");
    HIPTRY(E, hipMemcpyAsync(host.data(), dev, host.size() * sizeof(T), hipMemcpyDeviceToHost, s),
              "copy anchors");
    HIPTRY(E, hipStreamSynchronize(s), "anchor sync");  // the one wait
    c.sc.time_add();
    const uint64_t* h = c.sc.hctl;
    const uint64_t e = h[B_N + A_ERR];
    // (a slot that is no item: the count met it before any walk here did, and its check says so)
    if (int rc = bytes_count_check(E, r, h, "anchors", "items")) return rc;
    if (e & ~EA_INSIDE) {
        E.err = e & E_ORD_SLOT ? "anchors: the kept document order names a slot that is no item"
                : e & EL_RANK  ? "anchors: the kept inverse order disagrees with the order"
                : e & EL_TABLE ? "anchors: the identity table did not take every anchor"
                               : "anchors: a position's item is not where the tile prefixes say";
        return CRDT_HIP_EBADLOG;
    }
    if (e & EA_INSIDE) {
        E.err = "anchor position inside a codepoint";
        return CRDT_HIP_EINVAL;
    }
    return CRDT_HIP_OK;
}

}  // namespace

int replica_anchors_at(Engine& E, Replica& r, const uint64_t* pos, const uint8_t* bias, size_t n,
                       bool bytes, AnchorRec* out, AnchorStats* stats) {
    if (stats) *stats = AnchorStats{};
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    rc = anchor_check_at(pos, bias, n, bytes ? r.vis_bytes : r.vis_cp, E.err);
    if (rc || n == 0) return rc;
    if (stats) stats->anchors = n;
    if (r.n == 0) {  // nothing held: every position is 0, the start and the end at once
        for (size_t k = 0; k < n; ++k) out[k] = AnchorRec{kAnchorEdge, bias ? bias[k] : kAnchorAfter, 0u};
        return CRDT_HIP_OK;
    }
    AnchorCall c(E.stream);
    if ((rc = anchor_begin(E, r, c, n))) return rc;
    AnchorArgs& a = c.a;
    hipStream_t s = E.stream;
    uint64_t* dpos = nullptr;
    uint8_t* dbias = nullptr;
    HIPTRY(E, c.sc.alloc(&dpos, n), "hipMalloc anchor positions");
    if (bias) HIPTRY(E, c.sc.alloc(&dbias, n), "hipMalloc anchor positions");
    HIPTRY(E, c.sc.alloc(&a.aout, n), "hipMalloc anchors");
    a.pos = dpos;
    a.bias = dbias;
    // (the caller's arrays outlive the wait of anchor_end, so the uploads may read them until then)
    HIPTRY(E, hipMemcpyAsync(dpos, pos, n * 8, hipMemcpyHostToDevice, s), "upload anchor positions");
    if (bias) HIPTRY(E, hipMemcpyAsync(dbias, bias, n, hipMemcpyHostToDevice, s), "upload anchor biases");
    HIPTRY(E, c.sc.time_begin(), "anchor event");
    bytes_count_enqueue(c.b, s);
    k_anchor_init<<<1, kJB, 0, s>>>(a, 0u);
    if (bytes) k_anchor_create<true><<<grid_for(n, kAncW), kJB, 0, s>>>(a);
    else k_anchor_create<false><<<grid_for(n, kAncW), kJB, 0, s>>>(a);
    std::vector<AnchorRec> res(n);
    rc = anchor_end(E, r, c, a.aout, res);
    if (stats) {
        stats->ranks = r.n;
        stats->device_ns = c.sc.dev_ns;
    }
    if (rc) return rc;
    std::memcpy(out, res.data(), n * sizeof(AnchorRec));
    return CRDT_HIP_OK;
}

int replica_anchors_resolve(Engine& E, Replica& r, const AnchorRec* anc, size_t n, AnchorPosRec* out,
                            AnchorStats* stats) {
    if (stats) *stats = AnchorStats{};
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    rc = anchor_check_resolve(anc, n, E.err);
    if (rc || n == 0) return rc;
    if (stats) stats->anchors = n;
    if (r.n == 0) {  // nothing held: both edges lie at 0 and every identity is unknown
        uint64_t unknown = 0;
        for (size_t k = 0; k < n; ++k) {
            const bool edge = anc[k].id == kAnchorEdge;
            out[k] = AnchorPosRec{0, 0, edge ? kAnchorLive : kAnchorUnknown, 0u};
            unknown += edge ? 0u : 1u;
        }
        if (stats) stats->unknown = unknown;
        return CRDT_HIP_OK;
    }
    AnchorCall c(E.stream);
    if ((rc = anchor_begin(E, r, c, n))) return rc;
    AnchorArgs& a = c.a;
    hipStream_t s = E.stream;
    AnchorRec* danc = nullptr;
    HIPTRY(E, c.sc.alloc(&danc, n), "hipMalloc anchors");
    HIPTRY(E, locate_alloc(c.sc, a.l, a.m), "hipMalloc anchor table");
    const uint64_t cap = (uint64_t)a.l.mask + 1;
    HIPTRY(E, c.sc.alloc(&a.pout, n), "hipMalloc anchor positions");
    a.anc = danc;
    HIPTRY(E, hipMemcpyAsync(danc, anc, n * sizeof(AnchorRec), hipMemcpyHostToDevice, s), "upload anchors");
    HIPTRY(E, c.sc.time_begin(), "anchor event");
    bytes_count_enqueue(c.b, s);
    k_anchor_init<<<grid_for(cap, kJB), kJB, 0, s>>>(a, 1u);
    k_locate_insert<<<grid_for(n, kJB), kJB, 0, s>>>(a.l, &a.ctl[A_ERR]);
    if (a.fugue) k_locate_probe<true><<<grid_stride(r.n), kJB, 0, s>>>(a.l, a.v.key, r.n);
    else k_locate_probe<false><<<grid_stride(r.n), kJB, 0, s>>>(a.l, a.v.key, r.n);
    k_anchor_resolve<<<grid_for(n, kAncW), kJB, 0, s>>>(a);
    std::vector<AnchorPosRec> res(n);
    rc = anchor_end(E, r, c, a.pout, res);
    if (stats) {
        stats->ranks = r.n;
        stats->device_ns = c.sc.dev_ns;
    }
    if (rc) return rc;
    if (stats) stats->unknown = c.sc.hctl[B_N + A_UNKNOWN];
    std::memcpy(out, res.data(), n * sizeof(AnchorPosRec));
    return CRDT_HIP_OK;
}

}  // namespace crdt
