// delta.hip — state-vector delta sync of device-resident replicas (replica.hpp,
// crdt_hip_replica_state_vector / encode_diff / apply_diff): two peers that diverged exchange
// only what the other lacks.
//
// Replaces the reference's Yrs Downstream (rope.rs:252-255, :265-268: state_vector() +
// encode_diff_v1(&sv) + apply_update), for the engine's own logs.  A join (join.hip) ships the
// peer's whole log; here a peer sends its state vector (per agent the largest lamport it holds),
// the other answers with the items the vector does not cover plus the tombstones of the items it
// does cover, as identity ranges, and the first applies that.  The wire layout and the host twin
// are in oplog.hpp / oplog.cpp (OpLog::state_vector, encode_diff, apply_diff): both produce the
// same bytes and the same resulting log, slot for slot.  Items are named by identity (the
// replica's key word without the Fugue side bit, idtab.hpp); the kernels that name items take the
// replica's kind as a template parameter.
//
// state vector
//   k_sv_max       one pass over the key column.  A log has few agents in long runs, and
//                  same-address atomics serialise at the L2, so: a wave whose lanes agree on the
//                  agent reduces its lamports first and sends one value; values go to a 64-entry
//                  per-block LDS table keyed by agent, and to the dense 65,536-entry device table
//                  (atomicMax) only when the LDS entry belongs to another agent, or when the block
//                  flushes its table at the end; a write to the dense table also sets the agent's
//                  bit in a 65,536-bit presence map
//   k_sv_compact   one workgroup: the present agents in agent order, found from the presence
//                  map (8 KiB) instead of a scan of the dense table (512 KiB through one CU)
// encode
//   k_enc_bound    the peer's vector into a dense per-agent bound table
//   k_enc_classify per slot: uncovered item, covered tombstone or neither; a covered tombstone is
//                  a range head when the slot before it is none or does not continue to it (key +
//                  1 << 16), a range end likewise with the slot after it; per-block counts
//   k_enc_top      one workgroup: exclusive scans of the block counts, the totals.  The host waits
//                  here, once: the totals size the output
//   k_enc_write    per-block ranks; items, range heads and range ends compact in slot order, so
//                  no atomic decides an order; a parent's identity is one gather of key[parent]
//   k_enc_counts   count of range k = k-th end - k-th head + 1 (heads and ends compact alike)
// apply (validate, then write: a rejected delta changes nothing)
//   k_dl_table     identity table over every slot of dst (a delta has no common prefix to skip)
//   k_dl_probe     per delta item: bounds of its words, a transient table over the delta's items
//                  (its own duplicates; parents that are new), the lookup in dst's table
//   k_dl_top/rank  new items take ids n_dst + 1 + rank, in the delta's order
//   k_dl_roff      one workgroup: exclusive scan of the range counts (the ranges flattened)
//   k_dl_check     per delta item: an item both hold agrees in codepoint, parent identity and
//                  side; a new item's parent is found in dst or earlier in the delta
//   k_dl_rcheck    per flattened range item (one lane each, the range by binary search of the
//                  scan): its identity is known to dst or new with the delta
//   k_dl_write     appended items (byte stores: one thread owns the bytes of its slot)
//   k_dl_tomb      tombstones of items both hold and of the ranges, by atomicOr on the aligned
//                  word that holds the flag's byte: ranges may overlap each other or the items,
//                  and each newly tombstoned item is counted once.  A kernel of its own, so that
//                  no byte store of k_dl_write shares a word with an atomic in flight.
// Every phase is a kernel of its own on the engine's stream; no host copy of the replica's
// columns is made.  The identity table over all of dst makes an apply O(items of dst) in
// streaming work however small the delta: what the delta saves is the bytes exchanged.
#include <algorithm>
#include <cstring>
#include <vector>

#include "idtab.hpp"
#include "oplog.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

constexpr uint32_t kAgents = 65536;
constexpr int kSvLds = 64;  // entries of the per-block agent table

// device counters (u64)
enum DCtl { D_ERR = 0, D_SV_N, D_ITEMS, D_RANGES, D_ADDED, D_TOMB, D_ADD_CP, D_ADD_B, D_DEL_B,
            D_KILL_CP, D_KILL_B,  // appended items that a range of the same delta tombstones
            D_N };
// D_ERR bits
constexpr uint64_t ED_DUP_DST = 1, ED_DUP_ITEM = 2, ED_CP = 4, ED_PARENT = 8, ED_CAUSAL = 16,
                   ED_BOUNDS = 32, ED_TABLE = 64, ED_SIDE = 128, ED_ITEM = 256, ED_NOPARENT = 512,
                   ED_RANGE = 1024, ED_FUGUE = 2048;

__global__ void k_dl_init(uint64_t* ctl) {
    if (threadIdx.x < (uint32_t)D_N) ctl[threadIdx.x] = 0;
}

// ---- state vector ------------------------------------------------------------------------------
// (present: one bit per agent with an item, so that the compaction reads 8 KiB, not the table)
__device__ __forceinline__ void sv_top(unsigned long long* top, uint32_t* present, uint32_t agent,
                                       unsigned long long v) {
    atomicMax(&top[agent], v);
    atomicOr(&present[agent >> 5], 1u << (agent & 31u));
}
__device__ __forceinline__ void sv_put(uint32_t* tag, unsigned long long* val, unsigned long long* top,
                                       uint32_t* present, uint32_t agent, unsigned long long v) {
    const uint32_t h = (agent * 0x9E3779B1u) >> 26;  // (kSvLds = 64 entries)
    const uint32_t old = atomicCAS(&tag[h], 0u, agent + 1u);
    if (old == 0u || old == agent + 1u) atomicMax(&val[h], v);
    else sv_top(top, present, agent, v);  // the entry is another agent's
}

// top[agent] = largest lamport + 1 among the agent's items (0: none); slots 1..n.
__global__ __launch_bounds__(kJB) void k_sv_max(const uint64_t* key, uint32_t n, unsigned long long* top,
                                                uint32_t* present) {
    __shared__ uint32_t tag[kSvLds];            // agent + 1 (0: free)
    __shared__ unsigned long long val[kSvLds];  // lamport + 1
    if (threadIdx.x < kSvLds) {
        tag[threadIdx.x] = 0;
        val[threadIdx.x] = 0;
    }
    __syncthreads();
    // (the loop bound is the block's, so every lane of a wave takes part in the shuffles)
    for (uint64_t s0 = 1 + (uint64_t)blockIdx.x * kJB; s0 <= n; s0 += (uint64_t)gridDim.x * kJB) {
        const uint64_t s = s0 + threadIdx.x;
        const bool active = s <= n;
        const uint64_t k = active ? key[s] : 0;
        const uint32_t agent = (uint32_t)k & 0xFFFFu;
        const unsigned long long v = active ? ((k >> 16) & 0xFFFFFFFFull) + 1ull : 0ull;
        // inactive lanes are the wave's last ones: lane 0 is active unless the whole wave is not
        const uint32_t a0 = (uint32_t)__shfl((int)agent, 0);
        if (__all(!active || agent == a0)) {
            const unsigned long long m = ~wave_min_u64(~v);
            if ((threadIdx.x & 63u) == 0 && m) sv_put(tag, val, top, present, a0, m);
        } else if (active) {
            sv_put(tag, val, top, present, agent, v);
        }
    }
    __syncthreads();
    if (threadIdx.x < kSvLds && tag[threadIdx.x]) sv_top(top, present, tag[threadIdx.x] - 1u, val[threadIdx.x]);
}

// One workgroup of 1024 threads, 64 agents (two words of the presence bits) each: the present
// agents in agent order.
__global__ __launch_bounds__(1024) void k_sv_compact(const unsigned long long* top, const uint32_t* present,
                                                     uint2* out, uint64_t* ctl) {
    __shared__ uint32_t lds[16];
    const uint32_t w0 = present[2u * threadIdx.x], w1 = present[2u * threadIdx.x + 1u];
    uint32_t tot;
    uint32_t e = block_excl_scan<16>((uint32_t)(__popc(w0) + __popc(w1)), lds, tot);
    for (uint32_t h = 0; h < 2u; ++h)
        for (uint32_t w = h ? w1 : w0; w; w &= w - 1u) {
            const uint32_t a = 64u * threadIdx.x + 32u * h + (uint32_t)(__ffs((int)w) - 1);
            out[e++] = make_uint2(a, (uint32_t)(top[a] - 1ull));
        }
    if (threadIdx.x == 0) ctl[D_SV_N] = tot;
}

// ---- encode ------------------------------------------------------------------------------------
struct EncArgs {
    const uint32_t* par;
    const uint64_t* key;
    const uint8_t* cp;
    uint32_t n;
    const unsigned long long* bound;  // per agent: lamport + 1 the peer covers (0: nothing)
    uint8_t* flag;                    // per slot s at [s - 1]: F_ITEM | F_HEAD | F_END
    uint32_t* blk_i;                  // per kJB slots: items, range heads, range ends (then prefixes)
    uint32_t* blk_h;
    uint32_t* blk_e;
    uint32_t nblk;
    uint32_t* hslot;  // k-th range head / end: its slot
    uint32_t* eslot;
    // the wire columns (oplog.hpp), in the output buffer behind the header
    uint64_t* okey;
    uint64_t* opkey;
    uint64_t* orkey;
    uint32_t* ocp;
    uint32_t* orcount;
    uint64_t* ctl;
};
constexpr uint32_t F_ITEM = 1, F_HEAD = 2, F_END = 4;

__global__ void k_enc_bound(const uint2* sv, uint32_t nsv, unsigned long long* bound) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    // (the host checked the agents: strictly ascending, below kAgents)
    if (i < nsv && sv[i].x < kAgents) bound[sv[i].x] = (unsigned long long)sv[i].y + 1ull;
}

// Slot s (1..n): 1 = not covered by the peer's vector, 2 = covered and tombstoned, 0 = neither.
template <bool FUGUE>
__device__ __forceinline__ uint32_t enc_class(const EncArgs& a, uint64_t s, uint64_t& ident) {
    ident = jident<FUGUE>(a.key[s]);
    if ((ident >> 16) >= a.bound[(uint32_t)ident & 0xFFFFu]) return 1u;
    return (cp3_get(a.cp, s) & kDelBit) ? 2u : 0u;
}

template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_enc_classify(EncArgs a) {
    const uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x;
    uint32_t f = 0;
    if (s <= a.n) {
        uint64_t k, kn;
        const uint32_t c = enc_class<FUGUE>(a, s, k);
        if (c == 1u) f = F_ITEM;
        else if (c == 2u) {
            // slot 0 is the document start and the slots past n are padding: neither is an item
            if (!(s > 1 && enc_class<FUGUE>(a, s - 1, kn) == 2u && k == kn + (1ull << 16))) f |= F_HEAD;
            if (!(s < a.n && enc_class<FUGUE>(a, s + 1, kn) == 2u && kn == k + (1ull << 16))) f |= F_END;
        }
        a.flag[s - 1] = (uint8_t)f;
    }
    __shared__ uint32_t red[kJB / 64];
    const uint32_t ti = block_sum_t0<kJB / 64>(f & F_ITEM ? 1u : 0u, red);
    const uint32_t th = block_sum_t0<kJB / 64>(f & F_HEAD ? 1u : 0u, red);
    const uint32_t te = block_sum_t0<kJB / 64>(f & F_END ? 1u : 0u, red);
    if (threadIdx.x == 0) {
        a.blk_i[blockIdx.x] = ti;
        a.blk_h[blockIdx.x] = th;
        a.blk_e[blockIdx.x] = te;
    }
}

__global__ __launch_bounds__(1024) void k_enc_top(EncArgs a) {
    __shared__ uint32_t lds[16];
    const uint32_t ti = (uint32_t)block_scan_counts<1024>(a.blk_i, a.nblk, lds);
    const uint32_t th = (uint32_t)block_scan_counts<1024>(a.blk_h, a.nblk, lds);
    (void)block_scan_counts<1024>(a.blk_e, a.nblk, lds);
    if (threadIdx.x == 0) {
        a.ctl[D_ITEMS] = ti;
        a.ctl[D_RANGES] = th;
    }
}

// (ni, nr: the totals the host read; every rank is below them by construction, and checked)
template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_enc_write(EncArgs a, uint32_t ni, uint32_t nr) {
    __shared__ uint32_t lds[kJB / 64];
    const uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x;
    const uint32_t f = s <= a.n ? a.flag[s - 1] : 0u;
    uint32_t tot;
    const uint32_t ri = a.blk_i[blockIdx.x] + block_excl_scan<kJB / 64>(f & F_ITEM ? 1u : 0u, lds, tot);
    const uint32_t rh = a.blk_h[blockIdx.x] + block_excl_scan<kJB / 64>(f & F_HEAD ? 1u : 0u, lds, tot);
    const uint32_t re = a.blk_e[blockIdx.x] + block_excl_scan<kJB / 64>(f & F_END ? 1u : 0u, lds, tot);
    if (!f) return;
    const uint64_t kraw = a.key[s], k = jident<FUGUE>(kraw);
    if ((f & F_ITEM) && ri < ni) {
        const uint32_t p = a.par[s];
        const uint32_t c = cp3_get(a.cp, s);
        a.okey[ri] = k;
        a.opkey[ri] = p && p <= a.n ? jident<FUGUE>(a.key[p]) : kDeltaStart;
        a.ocp[ri] = (c & kDeltaCpMask) | (c & kDelBit ? kDeltaTombBit : 0u) |
                    (FUGUE && (kraw & kLeftKey) ? kDeltaSideBit : 0u);
    }
    if ((f & F_HEAD) && rh < nr) {
        a.orkey[rh] = k;
        a.hslot[rh] = (uint32_t)s;
    }
    if ((f & F_END) && re < nr) a.eslot[re] = (uint32_t)s;
}

__global__ __launch_bounds__(kJB) void k_enc_counts(EncArgs a, uint32_t nr) {
    const uint32_t k = blockIdx.x * kJB + threadIdx.x;
    if (k < nr) a.orcount[k] = a.eslot[k] - a.hslot[k] + 1u;
}

// ---- apply -------------------------------------------------------------------------------------
struct ApplyArgs {
    // dst (written by k_dl_write and k_dl_tomb alone)
    uint32_t* dpar;
    uint64_t* dkey;
    uint8_t* dcp;
    uint32_t nd;
    uint64_t cap_slots;
    // the delta's columns in the uploaded buffer
    const uint64_t* ikey;
    const uint64_t* ipkey;
    const uint64_t* rkey;
    const uint32_t* icp;
    const uint32_t* rcount;
    uint32_t n, r;
    uint32_t total;   // sum of the range counts (the host summed the same bytes)
    uint32_t* dtab;   // table over dst's slots 1..nd
    uint32_t dmask;
    uint32_t* itab;   // table over the delta's items (entries: 0-based item index)
    uint32_t imask;
    uint32_t* map;    // per delta item: its dst id
    uint32_t* tpar;   // per new delta item: its parent's dst id
    uint32_t* blk;    // per kJB delta items: new items (then their prefix)
    uint32_t nblk;
    uint32_t* roff;   // r + 1: items of the ranges before range k
    uint32_t* rslot;  // per flattened range item: its dst id
    uint64_t* ctl;
};

template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_dl_table(ApplyArgs a) {
    // (no counter: a table without a duplicate holds every slot, and a duplicate is an error)
    uint64_t err = 0;
    for (uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x; s <= a.nd; s += (uint64_t)gridDim.x * kJB) {
        const uint64_t k = jident<FUGUE>(a.dkey[s]);
        if (a.dpar[s] >= s) err |= ED_CAUSAL;
        bool full = false;
        if (tab_insert<FUGUE>(a.dtab, a.dmask, a.dkey, (uint32_t)s, k, full) != kEmpty) err |= ED_DUP_DST;
        if (full) err |= ED_TABLE;
    }
    ctl_or(&a.ctl[D_ERR], err);
}

// Delta item i = block * kJB + thread: its words are checked before anything uses them.
template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_dl_probe(ApplyArgs a) {
    const uint32_t i = blockIdx.x * kJB + threadIdx.x;
    uint64_t err = 0;
    uint32_t isnew = 0;
    if (i < a.n) {
        const uint64_t k = a.ikey[i];
        const uint32_t reserved = ~(kDeltaCpMask | kDeltaTombBit | (FUGUE ? kDeltaSideBit : 0u));
        uint32_t d = kEmpty;
        if (k >= kDeltaKeyEnd || (a.icp[i] & reserved)) {
            err |= ED_ITEM;  // (not entered: the table holds identities below kDeltaKeyEnd only)
        } else {
            bool full = false;
            if (tab_insert<false>(a.itab, a.imask, a.ikey, i, k, full) != kEmpty) err |= ED_DUP_ITEM;
            if (full) err |= ED_TABLE;
            d = tab_find<FUGUE>(a.dtab, a.dmask, a.dkey, k);
        }
        a.map[i] = d;
        isnew = d == kEmpty ? 1u : 0u;
    }
    ctl_or(&a.ctl[D_ERR], err);
    __shared__ uint32_t red[kJB / 64];
    const uint32_t t = block_sum_t0<kJB / 64>(isnew, red);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = t;
}

__global__ __launch_bounds__(1024) void k_dl_top(ApplyArgs a) {
    __shared__ uint32_t lds[16];
    const uint32_t t = (uint32_t)block_scan_counts<1024>(a.blk, a.nblk, lds);
    if (threadIdx.x == 0) a.ctl[D_ADDED] = t;
}

__global__ __launch_bounds__(kJB) void k_dl_rank(ApplyArgs a) {
    const uint32_t i = blockIdx.x * kJB + threadIdx.x;
    rank_new(a.map, a.blk, a.nd + 1u, i, i < a.n);
}

// One workgroup: the range counts -> roff[k] = items of the ranges before k, roff[r] = the total.
__global__ __launch_bounds__(1024) void k_dl_roff(ApplyArgs a) {
    __shared__ uint32_t lds[16];
    // (a count so large that a 1024-range sum wraps: the sum differs from the host's total)
    const uint64_t c0 = block_scan_counts<1024>(a.rcount, a.roff, a.r, lds);
    if (threadIdx.x == 0) {
        a.roff[a.r] = a.total;
        if (c0 != a.total) atomicOr((unsigned long long*)&a.ctl[D_ERR], (unsigned long long)ED_RANGE);
    }
}

// The dst id that holds identity k after the items: an item of dst, or a new item of the delta
// (map is complete: k_dl_rank ran before).  `before`: only delta items below that index count.
template <bool FUGUE>
__device__ __forceinline__ uint32_t dl_resolve(const ApplyArgs& a, uint64_t k, uint32_t before) {
    if (k >= kDeltaKeyEnd) return kEmpty;
    const uint32_t d = tab_find<FUGUE>(a.dtab, a.dmask, a.dkey, k);
    if (d != kEmpty) return d;
    const uint32_t j = tab_find<false>(a.itab, a.imask, a.ikey, k);
    return j != kEmpty && j < before && j < a.n ? a.map[j] : kEmpty;
}

template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_dl_check(ApplyArgs a) {
    uint64_t err = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * kJB + threadIdx.x; x < a.n; x += (uint64_t)gridDim.x * kJB) {
        const uint32_t i = (uint32_t)x;
        const uint32_t d = a.map[i], c = a.icp[i];
        const uint64_t k = a.ikey[i], pk = a.ipkey[i];
        if (k >= kDeltaKeyEnd) continue;  // (k_dl_probe reported it)
        if (d <= a.nd) {  // both hold the item (d >= 1: the table holds slots 1..nd)
            const uint32_t p = a.dpar[d];
            if ((c ^ cp3_get(a.dcp, d)) & kDeltaCpMask) err |= ED_CP;
            if ((p && p <= a.nd ? jident<FUGUE>(a.dkey[p]) : kDeltaStart) != pk) err |= ED_PARENT;
            if (FUGUE && ((a.dkey[d] & kLeftKey) != 0) != ((c & kDeltaSideBit) != 0)) err |= ED_SIDE;
            continue;
        }
        if ((uint64_t)d >= a.cap_slots) {
            err |= ED_BOUNDS;
            continue;
        }
        if (FUGUE && ((k >> 16) == 0xFFFFFFFFull || ((c & kDeltaSideBit) && pk == kDeltaStart))) err |= ED_FUGUE;
        uint32_t tp = 0;
        if (pk != kDeltaStart) {
            tp = dl_resolve<FUGUE>(a, pk, i);
            if (tp == kEmpty || tp >= d) {  // (an earlier new item has a smaller id)
                err |= ED_NOPARENT;
                tp = 0;
            }
        }
        a.tpar[i] = tp;
    }
    ctl_or(&a.ctl[D_ERR], err);
}

template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_dl_rcheck(ApplyArgs a) {
    uint64_t err = 0;
    for (uint64_t f = (uint64_t)blockIdx.x * kJB + threadIdx.x; f < a.total; f += (uint64_t)gridDim.x * kJB) {
        // the range of flattened item f: the last k with roff[k] <= f (counts are >= 1, so the
        // offsets ascend strictly; a scan that disagreed with the total was reported)
        uint32_t lo = 0, hi = a.r;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (a.roff[mid] <= f) lo = mid;
            else hi = mid;
        }
        const uint64_t j = f - a.roff[lo];
        const uint64_t k0 = a.rkey[lo];
        uint32_t d = kEmpty;
        if (j < a.rcount[lo] && k0 < kDeltaKeyEnd) d = dl_resolve<FUGUE>(a, k0 + (j << 16), a.n);
        if (d == kEmpty || (uint64_t)d >= a.cap_slots) {
            err |= ED_RANGE;
            d = 0;
        }
        a.rslot[f] = d;
    }
    ctl_or(&a.ctl[D_ERR], err);
}

template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_dl_write(ApplyArgs a) {
    if (a.ctl[D_ERR]) return;
    uint32_t add_cp = 0, add_b = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * kJB + threadIdx.x; x < a.n; x += (uint64_t)gridDim.x * kJB) {
        const uint32_t d = a.map[x];
        if (d <= a.nd || (uint64_t)d >= a.cap_slots) continue;
        const uint32_t c = a.icp[x], tp = a.tpar[x];
        const bool left = FUGUE && (c & kDeltaSideBit);
        a.dpar[d] = tp;
        a.dkey[d] = a.ikey[x] | (left ? kLeftKey : 0ull);
        // the previous-slot flag follows the translated parent (a left child carries kLeftBit and
        // never the flag), as in k_join_apply
        cp3_put(a.dcp, d, (c & kDeltaCpMask) | (c & kDeltaTombBit ? kDelBit : 0u) |
                              (left ? kLeftBit : tp == d - 1u ? kSeqBit : 0u));
        if (!(c & kDeltaTombBit)) {
            add_cp += 1u;
            add_b += utf8_len(c & kDeltaCpMask);
        }
    }
    __shared__ uint32_t red[kJB / 64];
    const uint32_t t0 = block_sum_t0<kJB / 64>(add_cp, red), t1 = block_sum_t0<kJB / 64>(add_b, red);
    if (threadIdx.x == 0 && t0) {
        atomicAdd((unsigned long long*)&a.ctl[D_ADD_CP], (unsigned long long)t0);
        atomicAdd((unsigned long long*)&a.ctl[D_ADD_B], (unsigned long long)t1);
    }
}

// Work items 0..n-1: delta item x, if both hold it and the delta has it tombstoned; n..n+total-1:
// flattened range item x - n.
__global__ __launch_bounds__(kJB) void k_dl_tomb(ApplyArgs a) {
    if (a.ctl[D_ERR]) return;
    uint32_t tomb = 0, del_b = 0, kill = 0, kill_b = 0;
    const uint64_t work = (uint64_t)a.n + a.total;
    for (uint64_t x = (uint64_t)blockIdx.x * kJB + threadIdx.x; x < work; x += (uint64_t)gridDim.x * kJB) {
        uint32_t d = 0;
        if (x < a.n) {
            const uint32_t m = a.map[x];
            if (m <= a.nd && (a.icp[x] & kDeltaTombBit)) d = m;
        } else {
            d = a.rslot[x - a.n];
        }
        if (d == 0 || (uint64_t)d >= a.cap_slots) continue;
        // the flag is bit 7 of the slot's third byte; the column starts on a word boundary
        const uint64_t byte = 3ull * d + 2ull;
        uint32_t* w = reinterpret_cast<uint32_t*>(a.dcp + (byte & ~3ull));
        const uint32_t bit = 0x80u << (8u * (uint32_t)(byte & 3ull));
        if (atomicOr(w, bit) & bit) continue;  // was tombstoned already
        const uint32_t len = utf8_len(cp3_get(a.dcp, d) & kDeltaCpMask);  // (codepoint bits do not change here)
        if (d <= a.nd) {
            tomb += 1u;
            del_b += len;
        } else {
            kill += 1u;
            kill_b += len;
        }
    }
    __shared__ uint32_t red[kJB / 64];
    const uint32_t t0 = block_sum_t0<kJB / 64>(tomb, red), t1 = block_sum_t0<kJB / 64>(del_b, red);
    const uint32_t t2 = block_sum_t0<kJB / 64>(kill, red), t3 = block_sum_t0<kJB / 64>(kill_b, red);
    if (threadIdx.x == 0 && t0) {
        atomicAdd((unsigned long long*)&a.ctl[D_TOMB], (unsigned long long)t0);
        atomicAdd((unsigned long long*)&a.ctl[D_DEL_B], (unsigned long long)t1);
    }
    if (threadIdx.x == 0 && t2) {
        atomicAdd((unsigned long long*)&a.ctl[D_KILL_CP], (unsigned long long)t2);
        atomicAdd((unsigned long long*)&a.ctl[D_KILL_B], (unsigned long long)t3);
    }
}

// ---- host side ---------------------------------------------------------------------------------
int replica_ready(Engine& E, const Replica& r) {
    if (r.pending) {
        E.err = "replica has an unsettled decode";
        return CRDT_HIP_EINVAL;
    }
    return CRDT_HIP_OK;
}

template <bool FUGUE>
void enc_launch(const EncArgs& a, hipStream_t s) {
    k_enc_classify<FUGUE><<<a.nblk, kJB, 0, s>>>(a);
    k_enc_top<<<1, 1024, 0, s>>>(a);
}
// Grid of the lookup kernels: one element per thread while that fits.  A lookup is a chain of
// dependent loads (table entry, key gather, the next probe; the binary search of the ranges), so
// a thread that takes several elements in turn multiplies the chain's latency: with four per
// thread (grid_stride) the table build over 200 k slots took 86 us and the 8 k range items 48 us.
uint32_t grid_each(uint64_t n) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(1u << 16, grid_for(n, kJB)));
}

template <bool FUGUE>
void apply_launch(const ApplyArgs& a, hipStream_t s) {
    if (a.nd) k_dl_table<FUGUE><<<grid_each(a.nd), kJB, 0, s>>>(a);
    if (a.n) {
        k_dl_probe<FUGUE><<<a.nblk, kJB, 0, s>>>(a);
        k_dl_top<<<1, 1024, 0, s>>>(a);
        k_dl_rank<<<a.nblk, kJB, 0, s>>>(a);
        k_dl_check<FUGUE><<<grid_each(a.n), kJB, 0, s>>>(a);
    }
    if (a.r) {
        k_dl_roff<<<1, 1024, 0, s>>>(a);
        k_dl_rcheck<FUGUE><<<grid_each(a.total), kJB, 0, s>>>(a);
    }
    if (a.n) k_dl_write<FUGUE><<<grid_stride(a.n), kJB, 0, s>>>(a);
    k_dl_tomb<<<grid_each((uint64_t)a.n + a.total), kJB, 0, s>>>(a);
}

}  // namespace

int replica_state_vector(Engine& E, const Replica& r, std::vector<SvEntry>& out, DeltaStats* stats) {
    out.clear();
    if (stats) *stats = DeltaStats{};
    int rc = replica_ready(E, r);
    if (rc) return rc;
    if (r.n == 0) return CRDT_HIP_OK;
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    hipStream_t s = E.stream;
    CallScratch sc(s);
    HIPTRY(E, sc.counters(D_N), "hipMalloc delta counters");
    unsigned long long* top = nullptr;
    uint2* ent = nullptr;
    HIPTRY(E, sc.alloc(&top, (uint64_t)kAgents), "hipMalloc state vector table");
    HIPTRY(E, sc.alloc(&ent, (uint64_t)kAgents), "hipMalloc state vector");
    uint32_t* present = nullptr;
    HIPTRY(E, sc.alloc(&present, (uint64_t)kAgents / 32), "hipMalloc state vector bits");
    HIPTRY(E, hipMemsetAsync(top, 0, kAgents * 8ull, s), "memset state vector table");
    HIPTRY(E, hipMemsetAsync(present, 0, kAgents / 8, s), "memset state vector bits");
    HIPTRY(E, sc.time_begin(), "delta event");
    k_dl_init<<<1, 64, 0, s>>>(sc.ctl);
    k_sv_max<<<grid_stride(r.n), kJB, 0, s>>>(r.logs.key, r.n, top, present);
    k_sv_compact<<<1, 1024, 0, s>>>(top, present, ent, sc.ctl);
    HIPTRY(E, hipGetLastError(), "state vector kernels");
    HIPTRY(E, sc.time_end(), "delta event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, D_N * 8, hipMemcpyDeviceToHost, s), "copy delta counters");
    HIPTRY(E, hipStreamSynchronize(s), "delta sync");
    sc.time_add();
    const uint64_t m = std::min<uint64_t>(sc.hctl[D_SV_N], kAgents);
    out.resize(m);
    static_assert(sizeof(SvEntry) == sizeof(uint2), "state vector entry layout");
    if (m) HIPTRY(E, hipMemcpy(out.data(), ent, m * sizeof(SvEntry), hipMemcpyDeviceToHost), "copy state vector");
    if (stats) stats->device_ns = sc.dev_ns;
    return CRDT_HIP_OK;
}

int replica_encode_diff(Engine& E, const Replica& r, const SvEntry* sv, size_t nsv, uint8_t* buf,
                        size_t cap, size_t* out_len, DeltaStats* stats) {
    if (stats) *stats = DeltaStats{};
    for (size_t i = 0; i < nsv; ++i)
        if (sv[i].agent >= kAgents || (i && sv[i].agent <= sv[i - 1].agent)) {
            E.err = "state vector is not sorted strictly by agent, or names an agent above 65535";
            return CRDT_HIP_EINVAL;
        }
    int rc = replica_ready(E, r);
    if (rc) return rc;
    const bool fugue = r.logs.fugue;
    const uint32_t n = r.n;
    uint32_t ni = 0, nr = 0;
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    hipStream_t s = E.stream;
    CallScratch sc(s);
    EncArgs a{};
    if (n) {
        HIPTRY(E, sc.counters(D_N), "hipMalloc delta counters");
        unsigned long long* bound = nullptr;
        uint2* dsv = nullptr;
        a.par = r.logs.parent;
        a.key = r.logs.key;
        a.cp = r.logs.cp;
        a.n = n;
        a.nblk = grid_for(n, kJB);
        a.ctl = sc.ctl;
        HIPTRY(E, sc.alloc(&bound, (uint64_t)kAgents), "hipMalloc bound table");
        HIPTRY(E, sc.alloc(&dsv, (uint64_t)nsv), "hipMalloc state vector");
        HIPTRY(E, sc.alloc(&a.flag, (uint64_t)n), "hipMalloc delta flags");
        HIPTRY(E, sc.alloc(&a.blk_i, (uint64_t)a.nblk), "hipMalloc delta blocks");
        HIPTRY(E, sc.alloc(&a.blk_h, (uint64_t)a.nblk), "hipMalloc delta blocks");
        HIPTRY(E, sc.alloc(&a.blk_e, (uint64_t)a.nblk), "hipMalloc delta blocks");
        a.bound = bound;
        HIPTRY(E, hipMemsetAsync(bound, 0, kAgents * 8ull, s), "memset bound table");
        if (nsv) HIPTRY(E, hipMemcpyAsync(dsv, sv, nsv * sizeof(SvEntry), hipMemcpyHostToDevice, s), "upload state vector");
        HIPTRY(E, sc.time_begin(), "delta event");
        k_dl_init<<<1, 64, 0, s>>>(sc.ctl);
        if (nsv) k_enc_bound<<<grid_for(nsv, kJB), kJB, 0, s>>>(dsv, (uint32_t)nsv, bound);
        if (fugue) enc_launch<true>(a, s);
        else enc_launch<false>(a, s);
        HIPTRY(E, hipGetLastError(), "delta classify kernels");
        HIPTRY(E, sc.time_end(), "delta event");
        HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, D_N * 8, hipMemcpyDeviceToHost, s), "copy delta counters");
        HIPTRY(E, hipStreamSynchronize(s), "delta sync");  // the one wait: the sizes
        sc.time_add();
        ni = (uint32_t)std::min<uint64_t>(sc.hctl[D_ITEMS], n);
        nr = (uint32_t)std::min<uint64_t>(sc.hctl[D_RANGES], n);
    }
    const uint64_t bytes = 16 + 20ull * ni + 12ull * nr;
    if (bytes >= (1ull << 32)) {
        E.err = "delta too large";
        return CRDT_HIP_ERANGE;
    }
    if (stats) {
        stats->items = ni;
        stats->ranges = nr;
        stats->device_ns = sc.dev_ns;
    }
    *out_len = bytes;
    if (!buf || cap < bytes) {
        E.err = "buffer too small";
        return CRDT_HIP_ESPACE;
    }
    const uint32_t hdr[4] = {kDeltaMagic, fugue ? kDeltaVersionFugue : kDeltaVersion, ni, nr};
    std::memcpy(buf, hdr, 16);
    if (bytes == 16) return CRDT_HIP_OK;
    // the columns, in wire order behind the header (16 + 16 ni + 8 nr: every u64 column 8-aligned)
    uint8_t* out = nullptr;
    HIPTRY(E, sc.alloc(&out, bytes - 16), "hipMalloc delta");
    HIPTRY(E, sc.alloc(&a.hslot, (uint64_t)nr), "hipMalloc delta ranges");
    HIPTRY(E, sc.alloc(&a.eslot, (uint64_t)nr), "hipMalloc delta ranges");
    a.okey = reinterpret_cast<uint64_t*>(out);
    a.opkey = a.okey + ni;
    a.orkey = a.opkey + ni;
    a.ocp = reinterpret_cast<uint32_t*>(a.orkey + nr);
    a.orcount = a.ocp + ni;
    HIPTRY(E, sc.time_begin(), "delta event");
    if (fugue) k_enc_write<true><<<a.nblk, kJB, 0, s>>>(a, ni, nr);
    else k_enc_write<false><<<a.nblk, kJB, 0, s>>>(a, ni, nr);
    if (nr) k_enc_counts<<<grid_for(nr, kJB), kJB, 0, s>>>(a, nr);
    HIPTRY(E, hipGetLastError(), "delta write kernels");
    HIPTRY(E, sc.time_end(), "delta event");
    HIPTRY(E, hipMemcpyAsync(buf + 16, out, bytes - 16, hipMemcpyDeviceToHost, s), "copy delta");
    HIPTRY(E, hipStreamSynchronize(s), "delta sync");
    sc.time_add();
    if (stats) stats->device_ns = sc.dev_ns;
    return CRDT_HIP_OK;
}

int replica_apply_diff(Engine& E, Replica& dst, const uint8_t* buf, size_t len, uint32_t* added,
                       uint32_t* tombstoned, DeltaStats* stats) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    if (stats) *stats = DeltaStats{};
    const bool fugue = dst.logs.fugue;
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, dst);
    if (rc) return rc;
    const uint32_t nd = dst.n;
    DeltaFrame f;
    rc = delta_frame(buf, len, fugue, nd, f, E.err);
    if (rc) return rc;
    if (stats) {
        stats->items = f.n;
        stats->ranges = f.r;
    }
    if (f.n == 0 && f.r == 0) return CRDT_HIP_OK;
    // appended items: at most the delta's
    rc = replica_reserve(E, dst, (uint64_t)nd + f.n);
    if (rc) return rc;
    hipStream_t s = E.stream;
    CallScratch sc(s);
    HIPTRY(E, sc.counters(D_N), "hipMalloc delta counters");
    uint8_t* dbuf = nullptr;
    ApplyArgs a{};
    const uint64_t dcap = pow2_at_least(2ull * nd), icap = pow2_at_least(2ull * f.n);
    a.nblk = grid_for(f.n, kJB);
    HIPTRY(E, sc.alloc(&dbuf, (uint64_t)len), "hipMalloc delta");
    HIPTRY(E, sc.alloc(&a.dtab, dcap), "hipMalloc delta table");
    HIPTRY(E, sc.alloc(&a.itab, icap), "hipMalloc delta table");
    HIPTRY(E, sc.alloc(&a.map, (uint64_t)f.n), "hipMalloc delta map");
    HIPTRY(E, sc.alloc(&a.tpar, (uint64_t)f.n), "hipMalloc delta map");
    HIPTRY(E, sc.alloc(&a.blk, (uint64_t)a.nblk), "hipMalloc delta blocks");
    HIPTRY(E, sc.alloc(&a.roff, (uint64_t)f.r + 1), "hipMalloc delta ranges");
    HIPTRY(E, sc.alloc(&a.rslot, f.range_items), "hipMalloc delta ranges");
    HIPTRY(E, hipMemcpyAsync(dbuf, buf, len, hipMemcpyHostToDevice, s), "upload delta");
    HIPTRY(E, hipMemsetAsync(a.dtab, 0xFF, dcap * 4, s), "memset delta table");
    HIPTRY(E, hipMemsetAsync(a.itab, 0xFF, icap * 4, s), "memset delta table");
    a.dpar = dst.logs.parent;
    a.dkey = dst.logs.key;
    a.dcp = dst.logs.cp;
    a.nd = nd;
    a.cap_slots = dst.logs.cap_slots;
    a.ikey = reinterpret_cast<const uint64_t*>(dbuf + f.key);
    a.ipkey = reinterpret_cast<const uint64_t*>(dbuf + f.pkey);
    a.rkey = reinterpret_cast<const uint64_t*>(dbuf + f.rkey);
    a.icp = reinterpret_cast<const uint32_t*>(dbuf + f.cp);
    a.rcount = reinterpret_cast<const uint32_t*>(dbuf + f.rcount);
    a.n = f.n;
    a.r = f.r;
    a.total = (uint32_t)f.range_items;  // (at most nd + n: delta_frame)
    a.dmask = (uint32_t)(dcap - 1);
    a.imask = (uint32_t)(icap - 1);
    a.ctl = sc.ctl;
    HIPTRY(E, sc.time_begin(), "delta event");
    k_dl_init<<<1, 64, 0, s>>>(sc.ctl);
    if (fugue) apply_launch<true>(a, s);
    else apply_launch<false>(a, s);
    HIPTRY(E, hipGetLastError(), "delta apply kernels");
    HIPTRY(E, sc.time_end(), "delta event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, D_N * 8, hipMemcpyDeviceToHost, s), "copy delta counters");
    HIPTRY(E, hipStreamSynchronize(s), "delta sync");
    sc.time_add();
    const uint64_t* c = sc.hctl;
    if (stats) {
        stats->table_slots = nd;  // every slot of dst is entered
        stats->device_ns = sc.dev_ns;
    }
    if (c[D_ERR]) {
        const uint64_t e = c[D_ERR];
        E.err = e & ED_DUP_DST    ? "delta: two items of the replica share an identity (lamport, agent)"
                : e & ED_CAUSAL   ? "delta: an item's parent does not precede it"
                : e & ED_ITEM     ? "delta: malformed item"
                : e & ED_DUP_ITEM ? "delta: two items share an identity (lamport, agent)"
                : e & ED_CP       ? "delta: an item both hold has another codepoint in each"
                : e & ED_PARENT   ? "delta: an item both hold has another parent in each"
                : e & ED_SIDE     ? "delta: an item both hold has another side in each"
                : e & ED_FUGUE    ? "delta: Fugue item with lamport 0xFFFFFFFF, or a left child of the document start"
                : e & ED_NOPARENT ? "delta: an item's parent is unknown or does not precede it"
                : e & ED_RANGE    ? "delta: a tombstone range names an unknown item"
                : e & ED_TABLE    ? "delta: identity table overflow"
                                  : "delta writes outside the replica";
        return CRDT_HIP_EBADLOG;
    }
    if (added) *added = (uint32_t)c[D_ADDED];
    if (tombstoned) *tombstoned = (uint32_t)c[D_TOMB];
    if (c[D_ADDED] == 0 && c[D_TOMB] == 0) return CRDT_HIP_OK;  // dst already held everything
    dst.n = nd + (uint32_t)c[D_ADDED];
    dst.vis_cp = dst.vis_cp + c[D_ADD_CP] - c[D_KILL_CP] - c[D_TOMB];
    dst.vis_bytes = dst.vis_bytes + c[D_ADD_B] - c[D_KILL_B] - c[D_DEL_B];
    dst.version++;
    dst.inc.valid = false;  // the kept document order does not cover the delta's items
    return CRDT_HIP_OK;
}

}  // namespace crdt
