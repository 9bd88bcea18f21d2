// join.hip — state-based merge of two device-resident replicas: dst <- dst U src by item identity
// (replica.hpp, crdt_hip_replica_join).
//
// Replaces the reference's `Downstream for Automerge` apply_update(&mut self, other: &Self) =
// doc.merge(other) (rope.rs:234-236): two editors that forked from a common
// log and both appended exchange their whole state.  An item's identity is its sibling key
// (lamport << 16 | agent), the word the replica's key column already holds; slot numbers mean
// nothing across logs.  Fugue replicas (both, or neither: the kind is the replica's, set by the
// side column of the view it was made from) join too: a left child's key carries kLeftKey
// (bit 48) and its codepoint word kLeftBit, and the side is an attribute of the item, not part of
// its name, so the identity is key & ~kLeftKey.  The kernels that name items take the kind as a
// template parameter (the RGA instances mask nothing).  Same semantics as OpLog::join
// (oplog.cpp), slot for slot:
//   k_join_prefix  both logs, slots 1..min(n): the first slot whose keys differ (min-reduce), and
//                  in the same pass the first slot with equal keys but another codepoint or parent.
//                  Slots below the first difference are the forks' common prefix: they map to
//                  themselves and never touch the table.  The host waits once here: the prefix
//                  length sizes the tables and the reserve.  Whole key words are compared: a
//                  Fugue slot that differs in the side alone ends the prefix, and the side check
//                  behind the table rejects it.
//   k_join_pmax    the largest key of the prefix.  Prefix slots are in no table, so an item past
//                  the prefix is only known to be none of them when every key past the prefix (of
//                  both logs) is above it, as it is for forks that appended local edits (lamport =
//                  max + 1).  Otherwise the join is run again with an empty prefix.
//   k_join_table   open-addressing table over dst's slots past the prefix: an entry is the u32
//                  slot, claimed by atomicCAS on the empty marker, identity equality by gathering
//                  dst.key[slot]; an insert that meets its own identity at another slot is a
//                  duplicate (Fugue: two keys that differ in the side bit alone are one identity)
//   k_join_probe   one thread per src slot past the prefix: the same insert into a transient
//                  table over src (src's own duplicates), then the lookup in dst's table:
//                  map[s] = dst slot, or new; new items counted per block
//   k_join_top     one workgroup: exclusive scan of the block counts, the total
//   k_join_rank    new items: map[s] = n_dst + 1 + rank among src's new items (src's slot order)
//   k_join_apply   <false> validates (an item both hold has the same codepoint, the same
//                  translated parent and, Fugue, the same side; parents precede their items),
//                  <true> writes: appended items get the translated parent, the key (side bit
//                  included) and the codepoint word with the previous-slot flag recomputed from
//                  the translated parent (a left child gets kLeftBit and never the flag, as in
//                  k_upd_items) and src's tombstone; items both hold take src's tombstone.  map is injective, so one thread owns the three
//                  bytes of each codepoint word it stores (byte stores, no read-modify-write of a
//                  neighbour's bytes).  Does nothing once any check failed.
// Every phase is a kernel of its own on the engine's stream (what one phase writes the next reads
// after the kernel boundary; inside a kernel only the table words are shared, through atomics).
// No host copy of either log is made; the host waits twice (prefix length, final counters).
#include <algorithm>
#include <cstring>

#include "idtab.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

constexpr uint32_t kCpMaskJ = 0x001FFFFFu;
// device counters (u64)
enum JCtl { J_ERR = 0, J_FIRST,  // first slot whose keys differ (min(n) + 1: none)
            J_BADCP, J_BADPAR,   // first slot with equal keys and another codepoint / parent
            J_PMAX,              // largest key of the prefix
            J_MINPOST,           // smallest key past the prefix, of both logs
            J_ADDED, J_TOMB, J_ADD_CP, J_ADD_B, J_DEL_B,
            J_TAB_USED,          // entries of dst's table in use (reported by tools/join_time.py)
            J_N };
// J_ERR bits
constexpr uint64_t EJ_DUP_DST = 1, EJ_DUP_SRC = 2, EJ_CP = 4, EJ_PARENT = 8, EJ_CAUSAL = 16,
                   EJ_BOUNDS = 32, EJ_TABLE = 64, EJ_SIDE = 128;

struct JoinArgs {
    // dst (written by k_join_apply<true> alone) and src slot arrays
    uint32_t* dpar;
    uint64_t* dkey;
    uint8_t* dcp;
    const uint32_t* spar;
    const uint64_t* skey;
    const uint8_t* scp;
    uint32_t nd, ns;
    uint32_t P;          // slots 1..P-1 are the common prefix (P >= 1)
    uint64_t cap_slots;  // of dst
    uint32_t* dtab;      // table over dst slots P..nd
    uint32_t dmask;
    uint32_t* stab;      // table over src slots P..ns
    uint32_t smask;
    uint32_t* map;       // per src slot s >= P, at [s - P]: its dst id
    uint32_t* blk;       // per kJB src slots past the prefix: new items (then their prefix)
    uint32_t nblk;
    uint64_t* ctl;
};

__global__ void k_join_init(uint64_t* ctl, uint32_t m) {
    const uint32_t i = threadIdx.x;
    if (i >= (uint32_t)J_N) return;
    ctl[i] = i == J_FIRST ? (uint64_t)m + 1u
             : (i == J_BADCP || i == J_BADPAR || i == J_MINPOST) ? ~0ull
                                                                 : 0ull;
}

// Slots 1..m of both logs: the first key difference and, where the keys agree, the first slot
// that fails the shared-item check (the host compares the two once the prefix is known).
__global__ __launch_bounds__(kJB) void k_join_prefix(JoinArgs a, uint32_t m) {
    uint32_t first = kEmpty, badcp = kEmpty, badpar = kEmpty;
    for (uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x; s <= m; s += (uint64_t)gridDim.x * kJB) {
        if (a.dkey[s] != a.skey[s]) {
            first = min(first, (uint32_t)s);
            continue;
        }
        if ((cp3_get(a.dcp, s) ^ cp3_get(a.scp, s)) & kCpMaskJ) badcp = min(badcp, (uint32_t)s);
        const uint32_t p = a.dpar[s];
        // (inside the prefix a parent translates to itself only if it lies there too: p < s)
        if (p != a.spar[s] || p >= s) badpar = min(badpar, (uint32_t)s);
    }
    ctl_min(&a.ctl[J_FIRST], first == kEmpty ? ~0ull : first);
    ctl_min(&a.ctl[J_BADCP], badcp == kEmpty ? ~0ull : badcp);
    ctl_min(&a.ctl[J_BADPAR], badpar == kEmpty ? ~0ull : badpar);
}

// (identities on both sides of the comparison with J_MINPOST: a left child's raw key is above
// every right child's, whatever their lamports)
template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_join_pmax(JoinArgs a) {
    uint64_t mx = 0;
    for (uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x; s < a.P; s += (uint64_t)gridDim.x * kJB)
        mx = max(mx, jident<FUGUE>(a.dkey[s]));
    ctl_max(&a.ctl[J_PMAX], mx);
}

// dst's slots P..nd into dst's table.
template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_join_table(JoinArgs a) {
    uint64_t err = 0, mn = ~0ull;
    uint32_t used = 0;
    for (uint64_t s = a.P + (uint64_t)blockIdx.x * kJB + threadIdx.x; s <= a.nd; s += (uint64_t)gridDim.x * kJB) {
        const uint64_t k = jident<FUGUE>(a.dkey[s]);
        mn = min(mn, k);
        if (a.dpar[s] >= s) err |= EJ_CAUSAL;
        bool full = false;
        if (tab_insert<FUGUE>(a.dtab, a.dmask, a.dkey, (uint32_t)s, k, full) != kEmpty) err |= EJ_DUP_DST;
        else used += 1u;
        if (full) err |= EJ_TABLE;
    }
    ctl_or(&a.ctl[J_ERR], err);
    ctl_min(&a.ctl[J_MINPOST], mn);
    __shared__ uint32_t red[kJB / 64];
    const uint32_t u = block_sum_t0<kJB / 64>(used, red);
    if (threadIdx.x == 0 && u) atomicAdd((unsigned long long*)&a.ctl[J_TAB_USED], (unsigned long long)u);
}

// src's slots P..ns, block b the kJB slots from P + b kJB: src's own duplicates, the lookup in
// dst's table (complete: k_join_table ran before), new items per block.
template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_join_probe(JoinArgs a) {
    const uint64_t s = (uint64_t)a.P + (uint64_t)blockIdx.x * kJB + threadIdx.x;
    uint64_t err = 0, mn = ~0ull;
    uint32_t isnew = 0;
    if (s <= a.ns) {
        const uint64_t k = jident<FUGUE>(a.skey[s]);
        mn = k;
        bool full = false;
        if (tab_insert<FUGUE>(a.stab, a.smask, a.skey, (uint32_t)s, k, full) != kEmpty) err |= EJ_DUP_SRC;
        const uint32_t d = tab_find<FUGUE>(a.dtab, a.dmask, a.dkey, k);
        if (full) err |= EJ_TABLE;
        a.map[s - a.P] = d;
        isnew = d == kEmpty ? 1u : 0u;
    }
    ctl_or(&a.ctl[J_ERR], err);
    ctl_min(&a.ctl[J_MINPOST], mn);
    __shared__ uint32_t red[kJB / 64];
    const uint32_t t = block_sum_t0<kJB / 64>(isnew, red);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = t;
}

// One workgroup: block counts -> exclusive prefixes, the total.
__global__ __launch_bounds__(1024) void k_join_top(JoinArgs a) {
    __shared__ uint32_t l0[16];
    const uint32_t c0 = (uint32_t)block_scan_counts<1024>(a.blk, a.nblk, l0);
    if (threadIdx.x == 0) a.ctl[J_ADDED] = c0;
}

// New items take their dst ids, in src's slot order.
__global__ __launch_bounds__(kJB) void k_join_rank(JoinArgs a) {
    const uint64_t s = (uint64_t)a.P + (uint64_t)blockIdx.x * kJB + threadIdx.x;
    rank_new(a.map, a.blk, a.nd + 1u, s - a.P, s <= a.ns);
}

// The dst id of src's slot p (map is complete: k_join_rank ran before).
__device__ __forceinline__ uint32_t jmap(const JoinArgs& a, uint32_t p) {
    return p < a.P ? p : a.map[p - a.P];
}

template <bool WRITE, bool FUGUE>
__global__ __launch_bounds__(kJB) void k_join_apply(JoinArgs a) {
    // (a key past the prefix at or below the prefix's largest: the prefix is not proven disjoint
    // from the rest, the host joins again with an empty prefix)
    if (WRITE && (a.ctl[J_ERR] || (a.P > 1u && a.ctl[J_MINPOST] <= a.ctl[J_PMAX]))) return;
    uint64_t err = 0;
    uint32_t add_cp = 0, add_b = 0, tomb = 0, del_b = 0;
    // the check covers the slots past the prefix (k_join_prefix checked the prefix), the write
    // every slot: a prefix item may be tombstoned in src alone
    const uint64_t s0 = WRITE ? 1u : a.P;
    for (uint64_t s = s0 + (uint64_t)blockIdx.x * kJB + threadIdx.x; s <= a.ns; s += (uint64_t)gridDim.x * kJB) {
        const uint32_t d = jmap(a, (uint32_t)s);
        const uint32_t cs = cp3_get(a.scp, s);
        if (d <= a.nd) {  // both hold the item
            if (!WRITE) {
                const uint32_t par = a.spar[s];
                if (par >= s) {
                    err |= EJ_CAUSAL;
                    continue;
                }
                if ((cs ^ cp3_get(a.dcp, d)) & kCpMaskJ) err |= EJ_CP;
                if (jmap(a, par) != a.dpar[d]) err |= EJ_PARENT;
                if (FUGUE && ((a.skey[s] ^ a.dkey[d]) & kLeftKey)) err |= EJ_SIDE;
            } else if (cs & kDelBit) {
                const uint32_t cd = cp3_get(a.dcp, d);
                if (!(cd & kDelBit)) {  // newly tombstoned
                    cp3_put(a.dcp, d, cd | kDelBit);
                    tomb += 1u;
                    del_b += utf8_len(cd & kCpMaskJ);
                }
            }
            continue;
        }
        const uint32_t par = a.spar[s];
        if (par >= s) {
            err |= EJ_CAUSAL;
            continue;
        }
        if (!WRITE) continue;
        if ((uint64_t)d >= a.cap_slots) {
            err |= EJ_BOUNDS;
            continue;
        }
        const uint32_t tp = jmap(a, par);
        a.dpar[d] = tp;
        const uint64_t k = a.skey[s];
        a.dkey[d] = k;
        // the previous-slot flag follows the translated parent: adjacency changes with the ids
        // (Fugue: a left child carries kLeftBit and never the flag, whatever its parent's slot)
        const bool left = FUGUE && (k & kLeftKey);
        cp3_put(a.dcp, d, (cs & (kCpMaskJ | kDelBit)) | (left ? kLeftBit : tp == d - 1u ? kSeqBit : 0u));
        if (!(cs & kDelBit)) {
            add_cp += 1u;
            add_b += utf8_len(cs & kCpMaskJ);
        }
    }
    ctl_or(&a.ctl[J_ERR], err);
    if (WRITE) {
        __shared__ uint32_t red[kJB / 64];
        const uint32_t t0 = block_sum_t0<kJB / 64>(add_cp, red), t1 = block_sum_t0<kJB / 64>(add_b, red);
        const uint32_t t2 = block_sum_t0<kJB / 64>(tomb, red), t3 = block_sum_t0<kJB / 64>(del_b, red);
        if (threadIdx.x == 0 && t0) {
            atomicAdd((unsigned long long*)&a.ctl[J_ADD_CP], (unsigned long long)t0);
            atomicAdd((unsigned long long*)&a.ctl[J_ADD_B], (unsigned long long)t1);
        }
        if (threadIdx.x == 0 && t2) {
            atomicAdd((unsigned long long*)&a.ctl[J_TOMB], (unsigned long long)t2);
            atomicAdd((unsigned long long*)&a.ctl[J_DEL_B], (unsigned long long)t3);
        }
    }
}

// Everything after the prefix pass, with slots 1..P-1 taken as the common prefix.  Leaves the
// final counters in sc.hctl (after a wait).
template <bool FUGUE>
int join_run(Engine& E, Replica& dst, const Replica& src, CallScratch& sc, uint32_t P) {
    const uint32_t nd = dst.n, ns = src.n;
    hipStream_t s = E.stream;
    // appended items: at most src's slots past the prefix
    int rc = replica_reserve(E, dst, (uint64_t)nd + (ns >= P ? ns - P + 1u : 0u));
    if (rc) return rc;
    const uint64_t cd = nd >= P ? nd - P + 1ull : 0, cs = ns >= P ? ns - P + 1ull : 0;
    const uint64_t dcap = pow2_at_least(2 * cd), scap = pow2_at_least(2 * cs);
    const uint32_t nblk = grid_for(cs, kJB);
    sc.drop_arrays();  // (a second run: the first one's arrays; the stream is idle)
    JoinArgs a{};
    HIPTRY(E, sc.alloc(&a.dtab, dcap), "hipMalloc join table");
    HIPTRY(E, sc.alloc(&a.stab, scap), "hipMalloc join table");
    HIPTRY(E, sc.alloc(&a.map, cs), "hipMalloc join map");
    HIPTRY(E, sc.alloc(&a.blk, (uint64_t)nblk), "hipMalloc join blocks");
    HIPTRY(E, hipMemsetAsync(a.dtab, 0xFF, dcap * 4, s), "memset join table");
    HIPTRY(E, hipMemsetAsync(a.stab, 0xFF, scap * 4, s), "memset join table");
    a.dpar = dst.logs.parent;
    a.dkey = dst.logs.key;
    a.dcp = dst.logs.cp;
    // (a self-join: dst's arrays may just have been replaced by the reserve)
    const DeviceLogs& S = &src == &dst ? dst.logs : src.logs;
    a.spar = S.parent;
    a.skey = S.key;
    a.scp = S.cp;
    a.nd = nd;
    a.ns = ns;
    a.P = P;
    a.cap_slots = dst.logs.cap_slots;
    a.dmask = (uint32_t)(dcap - 1);
    a.smask = (uint32_t)(scap - 1);
    a.nblk = nblk;
    a.ctl = sc.ctl;
    HIPTRY(E, sc.time_begin(), "join event");
    k_join_init<<<1, 64, 0, s>>>(sc.ctl, 0);
    if (P > 1) k_join_pmax<FUGUE><<<grid_stride(P - 1), kJB, 0, s>>>(a);
    if (cd) k_join_table<FUGUE><<<grid_stride(cd), kJB, 0, s>>>(a);
    if (cs) {
        k_join_probe<FUGUE><<<nblk, kJB, 0, s>>>(a);
        k_join_top<<<1, 1024, 0, s>>>(a);
        k_join_rank<<<nblk, kJB, 0, s>>>(a);
        k_join_apply<false, FUGUE><<<grid_stride(cs), kJB, 0, s>>>(a);
    }
    k_join_apply<true, FUGUE><<<grid_stride(ns), kJB, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "join kernels");
    HIPTRY(E, sc.time_end(), "join event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, J_N * 8, hipMemcpyDeviceToHost, s), "copy join counters");
    HIPTRY(E, hipStreamSynchronize(s), "join sync");
    sc.time_add();
    return CRDT_HIP_OK;
}

}  // namespace

int replica_join(Engine& E, Replica& dst, const Replica& src, uint32_t* added,
                 uint32_t* tombstoned, JoinStats* stats) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    if (stats) *stats = JoinStats{};
    // (the kind is the replica's own, whatever its items; checked before every early return)
    if ((dst.logs.fugue != 0) != (src.logs.fugue != 0)) {
        E.err = "join of a Fugue replica with an RGA replica: both sides must be of one kind";
        return CRDT_HIP_EINVAL;
    }
    const bool fugue = dst.logs.fugue != 0;
    if (src.pending) {
        E.err = "replica has an unsettled decode";
        return CRDT_HIP_EINVAL;
    }
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, dst);
    if (rc) return rc;
    const uint32_t nd = dst.n, ns = src.n;
    if (ns == 0) return CRDT_HIP_OK;  // nothing to take
    hipStream_t s = E.stream;
    CallScratch sc(s);
    HIPTRY(E, sc.counters(J_N), "hipMalloc join counters");

    // ---- the common prefix ---------------------------------------------------------------------
    const uint32_t m = std::min(nd, ns);
    uint32_t P = 1;
    if (m) {
        JoinArgs a{};
        a.dpar = dst.logs.parent;
        a.dkey = dst.logs.key;
        a.dcp = dst.logs.cp;
        a.spar = src.logs.parent;
        a.skey = src.logs.key;
        a.scp = src.logs.cp;
        a.ctl = sc.ctl;
        HIPTRY(E, sc.time_begin(), "join event");
        k_join_init<<<1, 64, 0, s>>>(sc.ctl, m);
        k_join_prefix<<<grid_stride(m), kJB, 0, s>>>(a, m);
        HIPTRY(E, hipGetLastError(), "join prefix kernel");
        HIPTRY(E, sc.time_end(), "join event");
        HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, J_N * 8, hipMemcpyDeviceToHost, s), "copy join counters");
        HIPTRY(E, hipStreamSynchronize(s), "join sync");
        sc.time_add();
        P = (uint32_t)sc.hctl[J_FIRST];
        if (sc.hctl[J_BADCP] < P) {
            E.err = "join: an item both logs hold has another codepoint in each";
            return CRDT_HIP_EBADLOG;
        }
        if (sc.hctl[J_BADPAR] < P) {
            E.err = "join: an item both logs hold has another parent in each";
            return CRDT_HIP_EBADLOG;
        }
    }
    // ---- table, probe, validate, write ---------------------------------------------------------
    rc = fugue ? join_run<true>(E, dst, src, sc, P) : join_run<false>(E, dst, src, sc, P);
    if (rc) return rc;
    if (P > 1 && !sc.hctl[J_ERR] && sc.hctl[J_MINPOST] <= sc.hctl[J_PMAX]) {
        // some key past the prefix does not exceed every prefix key (a log that took older items
        // in an earlier join): every slot goes through the table
        P = 1;
        rc = fugue ? join_run<true>(E, dst, src, sc, P) : join_run<false>(E, dst, src, sc, P);
        if (rc) return rc;
    }
    const uint64_t* c = sc.hctl;
    if (c[J_ERR]) {
        const uint64_t e = c[J_ERR];
        E.err = e & EJ_DUP_DST  ? "join: two items of the destination share an identity (lamport, agent)"
                : e & EJ_DUP_SRC ? "join: two items of the source share an identity (lamport, agent)"
                : e & EJ_CAUSAL  ? "join: an item's parent does not precede it"
                : e & EJ_CP      ? "join: an item both logs hold has another codepoint in each"
                : e & EJ_PARENT  ? "join: an item both logs hold has another parent in each"
                : e & EJ_SIDE    ? "join: an item both logs hold has another side in each"
                : e & EJ_TABLE   ? "join: identity table overflow"
                                 : "join writes outside the replica";
        return CRDT_HIP_EBADLOG;
    }
    if (stats) {
        stats->prefix = P - 1;
        stats->table_slots = c[J_TAB_USED];
        stats->table_cap = pow2_at_least(2 * (nd >= P ? nd - P + 1ull : 0));
        stats->device_ns = sc.dev_ns;
    }
    if (added) *added = (uint32_t)c[J_ADDED];
    if (tombstoned) *tombstoned = (uint32_t)c[J_TOMB];
    if (c[J_ADDED] == 0 && c[J_TOMB] == 0) return CRDT_HIP_OK;  // dst already held everything
    dst.n = nd + (uint32_t)c[J_ADDED];
    dst.vis_cp = dst.vis_cp + c[J_ADD_CP] - c[J_TOMB];
    dst.vis_bytes = dst.vis_bytes + c[J_ADD_B] - c[J_DEL_B];
    dst.version++;
    dst.inc.valid = false;  // the kept document order does not cover the joined items
    return CRDT_HIP_OK;
}

}  // namespace crdt
