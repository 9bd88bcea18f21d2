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
//                     contiguous column (what tab_insert / tab_find compare through) and its slot set
//                     to "not found"
//   k_anchor_insert   the distinct identities of the batch into an open-addressing table of at least
//                     twice as many entries as anchors; a repeated identity shares the entry of the
//                     anchor that claimed it (canon[i])
//   k_anchor_probe    a grid-stride pass over the key column, 8 B per slot: every item looks its
//                     identity up and, on a hit, records its slot for the entry (atomicMin: of two
//                     slots of a malformed log that share an identity the lower, as on the host)
//   k_anchor_resolve  a wave per anchor: slot -> rank from the kept inverse order (checked against n
//                     and against seq[rank] == slot), the tile's exclusive prefixes, and the visible
//                     ranks of the tile before `rank`, 64 ranks a step (ballot and popcount for the
//                     codepoints, a wave sum for the bytes)
// create (positions -> anchors)
//   k_anchor_create   a wave per position: a binary search of the scanned prefixes for the tile that
//                     holds the first visible item whose inclusive prefix reaches the position (AFTER)
//                     or passes it (BEFORE), then a walk of that tile 64 ranks a step with a wave
//                     scan; the item's lane writes jident(key[slot]).  In bytes an item whose prefix
//                     steps over the position without meeting it raises EA_INSIDE (EINVAL)
//
// Per position a search, not every visible item searching a sorted position table as
// k_edit_resolve does: positions come unsorted and repeated, a cursor batch is small, and a walk
// touches one tile per position where the table form would gather every rank's codepoint word a
// second time.
//
// No atomic decides an order (a CAS claims a table entry, a min picks a slot, an OR raises an error
// bit, one add per block counts the unknown); every slot, rank, tile and table index is checked
// against n and the sizes of the call before use and a bad value raises an A_ERR bit instead of
// becoming an address; every loop is bounded (a probe by the table size, a walk by the tile); no
// host copy of the replica's columns is made, and the host waits once.
//
// Known cost: a call streams every rank of the replica once (the count), and a resolve every key
// as well, however few the anchors; after a join or a delta it first pays inc_rebuild's ORDER-mode
// merge.
#include <cstring>
#include <vector>

#include "bytes.hpp"
#include "idtab.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// device counters (u64), after the B_N of the count
enum ACtl { A_ERR = 0, A_UNKNOWN, A_N };
// A_ERR bits
constexpr uint64_t EA_SLOT = 1;    // the order names a slot that is no item of the replica
constexpr uint64_t EA_RANK = 2;    // the inverse order names no rank, or not the slot's
constexpr uint64_t EA_TABLE = 4;   // the identity table did not take an anchor
constexpr uint64_t EA_INSIDE = 8;  // a byte position inside a codepoint
constexpr uint64_t EA_WALK = 16;   // a position's item is not in the tile the prefixes name

constexpr uint32_t kAncW = kJB / 64;  // anchors (waves) per workgroup

struct AnchorArgs {
    const uint32_t* seq;     // rank -> slot, ranks 0..n
    const uint32_t* rank;    // slot -> rank, slots 0..n
    const uint8_t* cp;       // 3-byte codepoint words of slots 0..n
    const uint64_t* key;
    uint32_t n;              // items held
    uint32_t fugue;
    uint32_t ntiles;
    const uint32_t* tcount;  // per tile: visible items before it
    const uint64_t* tbpre;   //   and their UTF-8 bytes
    const uint64_t* vis;     // the visible items and bytes of the whole order (B_VIS, B_VISB)
    uint32_t m;              // anchors of the call
    // resolve
    const AnchorRec* anc;
    uint64_t* ids;           // anc[i].id, contiguous
    uint32_t* tab;           // identity table: anchor indices (kEmpty: free), mask + 1 entries
    uint32_t mask;
    uint32_t* canon;         // per anchor: the anchor that owns its identity's entry
    uint32_t* slot;          // per owning anchor: the slot that holds the identity (kEmpty: none)
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
    if (g <= a.mask) a.tab[g] = kEmpty;
    if (g < a.m) {
        a.ids[g] = a.anc[g].id;
        a.slot[g] = kEmpty;
    }
}

__global__ __launch_bounds__(kJB) void k_anchor_insert(AnchorArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    if (g >= a.m) return;
    uint32_t owner = (uint32_t)g;
    const uint64_t id = a.ids[g];
    if (id != kAnchorEdge) {
        bool full = false;
        const uint32_t d = tab_insert<false>(a.tab, a.mask, a.ids, (uint32_t)g, id, full);
        if (d != kEmpty) owner = d;
        if (full) ctl_or(&a.ctl[A_ERR], EA_TABLE);
    }
    a.canon[g] = owner;
}

template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_anchor_probe(AnchorArgs a) {
    for (uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x; s <= a.n;
         s += (uint64_t)gridDim.x * kJB) {
        const uint32_t e = tab_find<false>(a.tab, a.mask, a.ids, jident<FUGUE>(a.key[s]));
        if (e != kEmpty && e < a.m) atomicMin(&a.slot[e], (uint32_t)s);
    }
}

// The UTF-8 length of the visible item at rank k (0: rank 0, a rank past n, a tombstone, or a slot
// that is no item, which also raises EA_SLOT); sl: its slot.
__device__ __forceinline__ uint32_t anchor_len(const AnchorArgs& a, uint64_t k, uint32_t& sl,
                                               uint64_t& err) {
    sl = 0;
    if (k == 0 || k > a.n) return 0;
    sl = a.seq[k];
    if (sl == 0 || sl > a.n) {
        err |= EA_SLOT;
        sl = 0;
        return 0;
    }
    const uint32_t c = cp3_get(a.cp, sl);
    return c & kDelBit ? 0u : utf8_len(c & kDeltaCpMask);
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
                o.pos = a.vis[0];
                o.pos_bytes = a.vis[1];
            }
        } else {
            const uint32_t own = a.canon[i];
            const uint32_t s = own < a.m ? a.slot[own] : 0u;
            if (s == kEmpty) {
                o.state = kAnchorUnknown;
                unknown = 1;
            } else if (s == 0 || s > a.n) {
                err |= EA_TABLE;
            } else {
                const uint32_t rk = a.rank[s];
                if (rk == 0 || rk > a.n || a.seq[rk] != s) {
                    err |= EA_RANK;
                } else {
                    const uint32_t tile = rk / kOrderTile;  // (below ntiles: rk <= n)
                    uint32_t cnt = 0, by = 0;
                    for (uint32_t k0 = tile * kOrderTile; k0 < rk; k0 += 64u) {
                        uint32_t sl;
                        const uint32_t wt = k0 + lane < rk ? anchor_len(a, k0 + lane, sl, err) : 0u;
                        cnt += (uint32_t)__popcll(__ballot(wt != 0));
                        by += wt;
                    }
                    by = wave_sum(by);  // (a tile holds at most 16 KiB)
                    const uint32_t cw = cp3_get(a.cp, s);
                    const bool live = !(cw & kDelBit);
                    const bool add = live && an.bias == kAnchorAfter;
                    o.pos = (uint64_t)a.tcount[tile] + cnt + (add ? 1u : 0u);
                    o.pos_bytes = a.tbpre[tile] + by + (add ? utf8_len(cw & kDeltaCpMask) : 0u);
                    o.state = live ? kAnchorLive : kAnchorDead;
                }
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
    const uint64_t total = a.vis[BYTES ? 1 : 0];
    AnchorRec o{kAnchorEdge, b, 0u};
    if (b == kAnchorAfter ? p == 0 : p >= total) {  // the document start, the document end
        if (lane == 0) a.aout[i] = o;
        return;
    }
    // the item: the first visible one whose inclusive prefix is at least thr; its tile: the last
    // whose exclusive prefix is below thr (thr >= 1, and tile 0's is 0)
    const uint64_t thr = b == kAnchorAfter ? p : p + 1;
    auto pre = [&](uint32_t t) { return BYTES ? a.tbpre[t] : (uint64_t)a.tcount[t]; };
    uint32_t lo = 0, hi = a.ntiles;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre(mid) < thr) lo = mid;
        else hi = mid;
    }
    uint64_t run = pre(lo);
    bool found = false;
    for (uint32_t st = 0; st < kOrderTile / 64u && !found; ++st) {
        uint32_t sl;
        const uint32_t len = anchor_len(a, (uint64_t)lo * kOrderTile + st * 64u + lane, sl, err);
        const uint32_t wt = BYTES ? len : (len ? 1u : 0u);
        const uint32_t inw = wave_incl_scan(wt);
        const uint64_t inc = run + inw;
        const bool hit = wt != 0 && inc >= thr && inc - wt < thr;
        found = __ballot(hit) != 0;  // (at most one lane: the prefixes ascend strictly over items)
        if (hit) {
            // AFTER: the item ends at p.  BEFORE: it starts at p.  (In codepoints always so.)
            if (b == kAnchorAfter ? inc == p : inc - wt == p) {
                const uint64_t k = a.key[sl];
                o.id = a.fugue ? jident<true>(k) : jident<false>(k);
                a.aout[i] = o;
            } else {
                err |= EA_INSIDE;
            }
        }
        run += (uint32_t)__builtin_amdgcn_readlane((int)inw, 63);
    }
    if (!found) err |= EA_WALK;
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
    int rc = replica_kept_ranks(E, r, "anchors", &c.a.seq, &c.a.rank, &c.a.ntiles);
    if (rc) return rc;
    HIPTRY(E, c.sc.counters(B_N + A_N), "hipMalloc anchor counters");
    BytesArgs& b = c.b;
    b.seq = c.a.seq;
    b.cp = r.logs.cp;
    b.n = r.n;
    b.ntiles = c.a.ntiles;
    b.ctl = c.sc.ctl;
    HIPTRY(E, c.sc.alloc(&b.tcount, (uint64_t)b.ntiles), "hipMalloc anchor tiles");
    HIPTRY(E, c.sc.alloc(&b.tbytes, (uint64_t)b.ntiles), "hipMalloc anchor tiles");
    HIPTRY(E, c.sc.alloc(&b.tbpre, (uint64_t)b.ntiles), "hipMalloc anchor tiles");
    AnchorArgs& a = c.a;
    a.cp = r.logs.cp;
    a.key = r.logs.key;
    a.n = r.n;
    a.fugue = r.logs.fugue ? 1u : 0u;
    a.tcount = b.tcount;
    a.tbpre = b.tbpre;
    a.vis = c.sc.ctl + B_VIS;
    static_assert(B_VISB == B_VIS + 1, "vis[1] is the visible bytes");
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
    if (h[B_ERR] || (e & EA_SLOT)) {
        E.err = "anchors: the kept document order names a slot that is no item";
        return CRDT_HIP_EBADLOG;
    }
    if (h[B_VIS] != r.vis_cp || h[B_VISB] != r.vis_bytes) {
        E.err = "anchors: the visible items of the kept order disagree with the replica's counters";
        return CRDT_HIP_EBADLOG;
    }
    if (e & ~EA_INSIDE) {
        E.err = e & EA_RANK    ? "anchors: the kept inverse order disagrees with the order"
                : e & EA_TABLE ? "anchors: the identity table did not take every anchor"
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
    const uint64_t cap = pow2_at_least(2 * (uint64_t)n);  // (n < 2^31: at most 2^32 entries)
    a.mask = (uint32_t)(cap - 1);
    AnchorRec* danc = nullptr;
    HIPTRY(E, c.sc.alloc(&danc, n), "hipMalloc anchors");
    HIPTRY(E, c.sc.alloc(&a.ids, n), "hipMalloc anchor ids");
    HIPTRY(E, c.sc.alloc(&a.tab, cap), "hipMalloc anchor table");
    HIPTRY(E, c.sc.alloc(&a.canon, n), "hipMalloc anchor table");
    HIPTRY(E, c.sc.alloc(&a.slot, n), "hipMalloc anchor slots");
    HIPTRY(E, c.sc.alloc(&a.pout, n), "hipMalloc anchor positions");
    a.anc = danc;
    HIPTRY(E, hipMemcpyAsync(danc, anc, n * sizeof(AnchorRec), hipMemcpyHostToDevice, s), "upload anchors");
    HIPTRY(E, c.sc.time_begin(), "anchor event");
    bytes_count_enqueue(c.b, s);
    k_anchor_init<<<grid_for(cap, kJB), kJB, 0, s>>>(a, 1u);
    k_anchor_insert<<<grid_for(n, kJB), kJB, 0, s>>>(a);
    if (a.fugue) k_anchor_probe<true><<<grid_stride(r.n), kJB, 0, s>>>(a);
    else k_anchor_probe<false><<<grid_stride(r.n), kJB, 0, s>>>(a);
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
