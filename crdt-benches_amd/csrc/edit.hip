// edit.hip — local edits on a device-resident replica (replica.hpp, crdt_hip_replica_apply_patches
// / crdt_hip_replica_replace): a set of positional patches, the reference's TestPatch(pos, del, ins)
// applied as Upstream::replace (rope.rs:21-32), resolved to item identities where the replica lies.
// The inverse of patch.hip.  The semantics are stated in crdt_hip.h; the host twin is
// OpLog::apply_patches (oplog.cpp), a loop of remove + insert, and both give the same log slot for
// slot.
//
// The patches of one call never touch (pos[k + 1] > pos[k] + codepoints(ins[k])), so in the
// coordinates of the document before the call every patch has its own surviving left neighbour
// and its own delete range: the whole set resolves in one pass over the document
// order the replica keeps after a merge_inc (IncState::seq[cur], rank -> slot, tombstones
// included), the same count, scan and select as patch.hip.
//
//   k_edit_init     counters, and the anchors of every patch set to "not found"
//   k_edit_slots    one pass over the slots 1..n: the largest lamport held (block reduction, one
//                   atomicMax per block) and, for a Fugue replica, the "has a right child" bit
//                   plane (atomicOr of the parent's bit for every item that is no left child;
//                   slot 0 included).  The plane is rebuilt by every call: it is a function of two
//                   columns and costs one pass that is needed for the lamport anyway
//   k_edit_count    a workgroup per tile of kOrderTile = 4,096 consecutive ranks, four ranks per
//                   thread (one 16-byte load of the order), the codepoint word gathered per rank:
//                   the tile's visible items
//   k_edit_top      one workgroup scans the tile counts
//   k_edit_resolve  each tile recomputes the visible rank v of its items (no per-rank array is
//                   stored) and every visible item, and rank 0 as v = 0, binary-searches the patch
//                   table (sorted by old position) for the last patch with old_pos <= v.
//                   v == old_pos: the item is that patch's left neighbour and records its slot and
//                   its successor in the full order, seq[rank + 1] (which may lie in the next
//                   tile).  old_pos < v <= old_pos + del: the item is deleted, and its id goes to
//                   entry del0 + (v - old_pos - 1) of the update's delete list: the deleted ids
//                   come out in document order without a compaction, because the index follows
//                   from the visible rank alone
//   k_edit_emit     one thread per inserted codepoint writes the new item's parent, lamport,
//                   codepoint word (Fugue: with the side bit) and agent into the update
//
// What the kernels write is one wire update (OpLog::encode_from's format) in device memory, which
// replica_decode_enqueue(resident = true) then applies: the state change (n, the visible counters,
// the version, the capacity, the tombstone bits, `inc` left valid for the old n) is the decode's
// own and cannot drift from it, and a set that fails any check is never handed over.
//
// No atomic decides an order (the atomics are an OR into a bit plane, a max and counts); every
// slot, rank, patch and id is checked against n and the buffer sizes before use and a bad value
// raises ECtl::E_ERR instead of becoming an address; no host copy of the replica's columns is made.
// The host waits once before the decode, for the counters: the largest lamport (the ERANGE check)
// and the integrity counts (visible items, anchors found, ids deleted).
//
// The byte-offset entry point (crdt_hip_replica_apply_patches_bytes; crdt_hip.h, "byte offsets")
// shares everything after "the patch table is known" (edit_run): its table is built on the device
// by the translation kernels of bytes.hip, after which it waits once more (the boundary check and
// the number of deleted items, which sizes the update).
//
// Known cost: a call streams every slot and every rank of the replica, even for one keystroke, and
// after a join or a delta it also pays inc_rebuild's ORDER-mode merge.
#include <algorithm>
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

// device counters (u64)
enum ECtl { E_ERR = 0, E_MAXLAM, E_VIS, E_LEFTS, E_DELS, E_N };
// E_ERR bits
constexpr uint64_t EE_SLOT = 1;    // the order names a slot that is no item of the replica
constexpr uint64_t EE_PARENT = 2;  // a parent outside the replica
constexpr uint64_t EE_TABLE = 4;   // a patch table entry disagrees with the sizes of the call
constexpr uint64_t EE_ANCHOR = 8;  // a patch without a left neighbour, or (Fugue) without the
                                   //   successor its left-child anchor needs

struct EditArgs {
    const uint32_t* seq;     // rank -> slot, ranks 0..n (rank 0 = slot 0, the document start)
    const uint8_t* cp;       // 3-byte codepoint words of slots 0..n
    const uint64_t* key;
    const uint32_t* parent;
    uint32_t n;              // items held before the call
    uint32_t fugue;
    uint32_t ntiles;
    uint32_t* tcount;        // per tile: visible items, then their exclusive prefix
    uint32_t* hasr;          // (Fugue) bit s: slot s has a right child; (n + 32) / 32 words
    const EditPatch* tab;    // the patches, by old position
    uint32_t np;
    uint32_t* left;          // per patch: slot of its left neighbour (NIL: not found)
    uint32_t* succ;          //   and that slot's successor in the full order (NIL: none)
    const uint32_t* cps;     // the inserted codepoints
    uint32_t ncp, ndel;
    uint32_t agent;
    uint32_t* wire;          // the update: 6 header words, parent, origin_right, lamport, cp (ncp
    uint64_t wire_words;     //   each), agents (u16, padded to a word), deleted ids (ndel)
    uint64_t* woff;          // its two byte offsets
    uint64_t* ctl;
};

__device__ __forceinline__ uint64_t wire_dels(const EditArgs& a) {
    return 6ull + 4ull * a.ncp + (2ull * a.ncp + 3ull) / 4ull;
}

__global__ __launch_bounds__(kJB) void k_edit_init(EditArgs a, uint32_t empty) {
    const uint32_t g = blockIdx.x * kJB + threadIdx.x;
    if (g < (uint32_t)E_N) a.ctl[g] = (g == (uint32_t)E_LEFTS && empty && a.np) ? 1u : 0u;
    // (an empty replica has no order to stream: its one patch is anchored to the document start)
    if (g < a.np) {
        a.left[g] = empty && g == 0 ? 0u : NIL;
        a.succ[g] = NIL;
    }
}

__global__ __launch_bounds__(kJB) void k_edit_slots(EditArgs a) {
    uint64_t mx = 0, err = 0;
    for (uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x; s <= a.n;
         s += (uint64_t)gridDim.x * kJB) {
        const uint64_t k = a.key[s];
        const uint64_t lam = (k & ~kLeftKey) >> 16;
        mx = lam > mx ? lam : mx;
        if (a.fugue && !(k & kLeftKey)) {
            const uint32_t p = a.parent[s];
            if (p > a.n) err |= EE_PARENT;
            else atomicOr(&a.hasr[p >> 5], 1u << (p & 31u));
        }
    }
    ctl_or(&a.ctl[E_ERR], err);
    ctl_max(&a.ctl[E_MAXLAM], mx);
}

// The slots of the thread's four ranks k0..k0 + 3 and whether each holds a visible item (ranks
// past n, rank 0, tombstones and slots that are no item: not visible).
__device__ __forceinline__ void edit_load(const EditArgs& a, uint64_t k0, uint32_t sl[kOrdPer],
                                          bool vis[kOrdPer], uint64_t& err) {
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        sl[j] = 0;
        vis[j] = false;
    }
    order_load4(a.seq, a.cp, a.n, k0, err, EE_SLOT, [&](uint32_t j, uint32_t s, uint32_t c) {
        sl[j] = s;
        vis[j] = !(c & kDelBit);
    });
}

__global__ __launch_bounds__(kOrdT) void k_edit_count(EditArgs a) {
    __shared__ uint32_t red[kOrdW];
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t sl[kOrdPer];
    bool vis[kOrdPer];
    uint64_t err = 0;
    edit_load(a, k0, sl, vis, err);
    ctl_or(&a.ctl[E_ERR], err);
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) c += vis[j] ? 1u : 0u;
    const uint32_t t = block_sum_t0<kOrdW>(c, red);
    if (threadIdx.x == 0 && blockIdx.x < a.ntiles) a.tcount[blockIdx.x] = t;
}

__global__ __launch_bounds__(kOrdTop) void k_edit_top(EditArgs a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    const uint64_t c = block_scan_counts<kOrdTop>(a.tcount, a.ntiles, lds);  // (at most n < 2^31)
    if (threadIdx.x == 0) a.ctl[E_VIS] = c;
}

__global__ __launch_bounds__(kOrdT) void k_edit_resolve(EditArgs a) {
    __shared__ uint32_t lds[kOrdW];
    if (blockIdx.x >= a.ntiles) return;
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t sl[kOrdPer];
    bool vis[kOrdPer];
    uint64_t err = 0;
    edit_load(a, k0, sl, vis, err);  // (k_edit_count reported any bad slot)
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) c += vis[j] ? 1u : 0u;
    uint32_t tot;
    uint32_t v = a.tcount[blockIdx.x] + block_excl_scan<kOrdW>(c, lds, tot);  // visible before
    uint32_t lefts = 0, dels = 0;
    const uint64_t dbase = wire_dels(a);
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        const uint64_t rank = k0 + j;
        if (!vis[j] && rank != 0) continue;
        if (vis[j]) ++v;  // this item's visible rank (the document start: 0)
        const uint32_t k = last_at_most(a.np, v, [&](uint32_t i) { return a.tab[i].old_pos; });
        if (k >= a.np) continue;
        const EditPatch e = a.tab[k];
        if (e.old_pos == v) {
            a.left[k] = sl[j];
            uint32_t nx = NIL;
            if (rank + 1 <= a.n) {
                nx = a.seq[rank + 1];
                if (nx == 0 || nx > a.n) {
                    err |= EE_SLOT;
                    nx = NIL;
                }
            }
            a.succ[k] = nx;
            ++lefts;
        } else if (v - e.old_pos <= e.del) {
            const uint64_t idx = (uint64_t)e.del0 + (v - e.old_pos - 1u);
            if (idx >= a.ndel || dbase + idx >= a.wire_words) {
                err |= EE_TABLE;
                continue;
            }
            a.wire[dbase + idx] = sl[j];
            ++dels;
        }
    }
    ctl_or(&a.ctl[E_ERR], err);
    const uint32_t s0 = block_sum_t0<kOrdW>(lefts, lds), s1 = block_sum_t0<kOrdW>(dels, lds);
    if (threadIdx.x == 0) {
        if (s0) atomicAdd((unsigned long long*)&a.ctl[E_LEFTS], (unsigned long long)s0);
        if (s1) atomicAdd((unsigned long long*)&a.ctl[E_DELS], (unsigned long long)s1);
    }
}

__global__ __launch_bounds__(kJB) void k_edit_emit(EditArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    const uint64_t dbase = wire_dels(a);
    if (dbase + a.ndel != a.wire_words) {
        if (j == 0) ctl_or(&a.ctl[E_ERR], EE_TABLE);
        return;
    }
    if (j == 0) {
        a.wire[0] = kUpdateMagic;
        a.wire[1] = a.fugue ? kUpdateVersionFugue : kUpdateVersion;
        a.wire[2] = a.n + 1u;
        a.wire[3] = a.ncp;
        a.wire[4] = 0u;
        a.wire[5] = a.ndel;
        a.woff[0] = 0;
        a.woff[1] = a.wire_words * 4ull;
        if (a.ncp & 1u)  // the padding of the agent column
            reinterpret_cast<uint16_t*>(a.wire + 6ull + 4ull * a.ncp)[a.ncp] = 0;
    }
    if (j >= a.ncp) return;
    // the patch of codepoint j: the last one whose codepoints start at or before j (patches
    // without text share their start with the next one that has some)
    uint32_t lo = 0, hi = a.np;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.tab[mid].cp0 <= j) lo = mid;
        else hi = mid;
    }
    uint64_t err = 0;
    uint32_t par = 0, side = 0;
    const uint32_t id = a.n + 1u + (uint32_t)j;
    if (a.np == 0 || a.tab[lo].cp0 > j || j - a.tab[lo].cp0 >= a.tab[lo].ncp) {
        err |= EE_TABLE;
    } else if (j > a.tab[lo].cp0) {
        par = id - 1u;  // a right child of the codepoint before it
    } else {
        const uint32_t l = a.left[lo];
        if (l > a.n) {
            err |= EE_ANCHOR;
        } else if (a.fugue && ((a.hasr[l >> 5] >> (l & 31u)) & 1u)) {
            // the left neighbour has a right child: a left child of its successor
            const uint32_t nx = a.succ[lo];
            if (nx == 0 || nx > a.n) err |= EE_ANCHOR;
            else {
                par = nx;
                side = 1;
            }
        } else {
            par = l;
        }
    }
    ctl_or(&a.ctl[E_ERR], err);
    const uint64_t lam = a.ctl[E_MAXLAM] + 1ull + j;  // (the host checks the bound before the decode)
    uint32_t* w = a.wire + 6;
    w[j] = par;
    w[(uint64_t)a.ncp + j] = NIL;  // origin_right is not carried, as after a delta
    w[2ull * a.ncp + j] = (uint32_t)lam;
    w[3ull * a.ncp + j] = (a.cps[j] & kDeltaCpMask) | (side ? kUpdateSideBit : 0u);
    reinterpret_cast<uint16_t*>(w + 4ull * a.ncp)[j] = (uint16_t)a.agent;
}

}  // namespace

// ---- host side ---------------------------------------------------------------------------------
namespace {

// 32-bit words of the update that ncp new items and ndel deleted ids make.
uint64_t edit_words(uint64_t ncp, uint64_t ndel) { return 6 + 4 * ncp + (2 * ncp + 3) / 4 + ndel; }

// Everything after "the patch table is known": shared by the codepoint entry point, which uploads
// the table edit_plan made (host_tab), and the byte entry point, whose table bytes.hip built on the
// device (dev_tab).  a: seq and ntiles set (an empty replica: neither).  cps: every inserted
// codepoint.  The lamport bound is checked here, after everything else.
int edit_run(Engine& E, Replica& r, CallScratch& sc, EditArgs& a, const std::vector<uint32_t>& cpsv,
             const EditPatch* host_tab, EditPatch* dev_tab, uint64_t np, uint64_t ndel,
             uint32_t* added, uint32_t* tombstoned, EditStats* stats) {
    const uint64_t ncp = cpsv.size(), words = edit_words(ncp, ndel);
    const bool empty = r.n == 0;
    hipStream_t s = sc.stream;
    a.cp = r.logs.cp;
    a.key = r.logs.key;
    a.parent = r.logs.parent;
    a.n = r.n;
    a.fugue = r.logs.fugue ? 1u : 0u;
    a.np = (uint32_t)np;
    a.ncp = (uint32_t)ncp;
    a.ndel = (uint32_t)ndel;
    a.agent = r.agent;
    a.wire_words = words;
    const uint64_t hasr_words = ((uint64_t)r.n + 32) / 32;
    EditPatch* tab = dev_tab;
    uint32_t* cps = nullptr;
    if (!sc.ctl) HIPTRY(E, sc.counters(E_N), "hipMalloc edit counters");
    a.ctl = sc.ctl;
    HIPTRY(E, sc.alloc(&a.tcount, (uint64_t)a.ntiles), "hipMalloc edit tiles");
    HIPTRY(E, sc.alloc(&a.hasr, hasr_words), "hipMalloc edit right-child bits");
    if (host_tab) HIPTRY(E, sc.alloc(&tab, np), "hipMalloc edit patches");
    HIPTRY(E, sc.alloc(&a.left, np), "hipMalloc edit anchors");
    HIPTRY(E, sc.alloc(&a.succ, np), "hipMalloc edit anchors");
    HIPTRY(E, sc.alloc(&cps, ncp), "hipMalloc edit codepoints");
    HIPTRY(E, sc.alloc(&a.wire, words), "hipMalloc edit update");
    HIPTRY(E, sc.alloc(&a.woff, 2), "hipMalloc edit update");
    a.tab = tab;
    a.cps = cps;
    // (the caller's plan outlives the wait below, so the uploads may read it until then)
    if (host_tab)
        HIPTRY(E, hipMemcpyAsync(tab, host_tab, np * sizeof(EditPatch), hipMemcpyHostToDevice, s),
                  "upload edit patches");
    if (ncp) HIPTRY(E, hipMemcpyAsync(cps, cpsv.data(), ncp * 4, hipMemcpyHostToDevice, s), "upload edit text");
    HIPTRY(E, sc.time_begin(), "edit event");
    k_edit_init<<<grid_for(std::max<uint64_t>(np, E_N), kJB), kJB, 0, s>>>(a, empty ? 1u : 0u);
    if (!empty) {
        if (a.fugue) HIPTRY(E, hipMemsetAsync(a.hasr, 0, hasr_words * 4, s), "clear right-child bits");
        k_edit_slots<<<grid_stride(r.n), kJB, 0, s>>>(a);
        k_edit_count<<<a.ntiles, kOrdT, 0, s>>>(a);
        k_edit_top<<<1, kOrdTop, 0, s>>>(a);
        k_edit_resolve<<<a.ntiles, kOrdT, 0, s>>>(a);
    } else if (a.fugue) {
        HIPTRY(E, hipMemsetAsync(a.hasr, 0, hasr_words * 4, s), "clear right-child bits");
    }
    k_edit_emit<<<grid_for(std::max<uint64_t>(ncp, 1), kJB), kJB, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "edit kernels");
    HIPTRY(E, sc.time_end(), "edit event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl, a.ctl, E_N * 8, hipMemcpyDeviceToHost, s), "copy edit counters");
    HIPTRY(E, hipStreamSynchronize(s), "edit sync");  // the one wait before anything changes
    sc.time_add();
    const uint64_t* c = sc.hctl;
    if (c[E_ERR]) {
        E.err = c[E_ERR] & EE_SLOT     ? "edit: the kept document order names a slot that is no item"
                : c[E_ERR] & EE_PARENT ? "edit: a parent outside the replica"
                : c[E_ERR] & EE_ANCHOR ? "edit: a patch found no anchor"
                                       : "edit: the patch table disagrees with the call's sizes";
        return CRDT_HIP_EBADLOG;
    }
    if (!empty && c[E_VIS] != r.vis_cp) {
        E.err = "edit: the visible items of the kept order disagree with the replica's counter";
        return CRDT_HIP_EBADLOG;
    }
    if (c[E_LEFTS] != np || c[E_DELS] != ndel) {
        E.err = "edit: not every patch resolved";
        return CRDT_HIP_EBADLOG;
    }
    if (c[E_MAXLAM] + ncp >= 0xFFFFFFFFull) {
        E.err = "lamports would reach 0xFFFFFFFF";
        return CRDT_HIP_ERANGE;
    }
    // the update is whole and checked: the decode applies it (and validates it once more)
    const uint32_t n0 = r.n;
    const uint64_t vis0 = r.vis_cp;
    HIPTRY(E, sc.time_begin(), "edit event");
    int rc = replica_decode_enqueue(E, r, reinterpret_cast<const uint8_t*>(a.wire), words * 4, a.woff, 1,
                                true, ncp ? (uint32_t)(n0 + ncp) : 0u, true);
    if (rc) return rc;
    HIPTRY(E, sc.time_end(), "edit event");
    rc = replica_settle(E, r);
    if (rc) return rc;
    sc.time_add();
    if (r.n != n0 + ncp || r.vis_cp != vis0 + ncp - ndel) {
        E.err = "edit: the decode disagrees with the patches";
        return CRDT_HIP_EBADLOG;
    }
    if (added) *added = (uint32_t)ncp;
    if (tombstoned) *tombstoned = (uint32_t)ndel;
    if (stats) {
        stats->patches = np;
        stats->items = ncp;
        stats->tombstones = ndel;
        stats->ranks = n0;
        stats->device_ns = sc.dev_ns;
    }
    return CRDT_HIP_OK;
}

}  // namespace

int replica_apply_patches(Engine& E, Replica& r, const PatchRec* p, size_t n, const uint8_t* ins,
                          size_t ins_len, uint32_t* added, uint32_t* tombstoned, EditStats* stats) {
    if (stats) *stats = EditStats{};
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    if (n == 0) return CRDT_HIP_OK;
    if (!p) {
        E.err = "null patch array";
        return CRDT_HIP_EINVAL;
    }
    // everything the arguments and the replica's own counters can tell, before any device work
    EditPlan plan;
    rc = edit_plan(p, n, ins, ins_len, r.vis_cp, r.n, plan, E.err);
    if (rc) return rc;
    if (edit_words(plan.cps.size(), plan.ndel) * 4 >= (1ull << 32) - 16) {
        E.err = "edit of 4 GiB or more";
        return CRDT_HIP_ERANGE;
    }
    EditArgs a{};  // (an empty replica has no order: seq null, no tiles)
    if (r.n != 0 && (rc = replica_kept_order(E, r, "edit", &a.seq, &a.ntiles))) return rc;
    CallScratch sc(E.stream);
    return edit_run(E, r, sc, a, plan.cps, plan.patch.data(), nullptr, plan.patch.size(), plan.ndel,
                    added, tombstoned, stats);
}

// The byte-offset reading (crdt_hip.h, "byte offsets"): edit_plan_bytes, the translation kernels
// of bytes.hip, one more wait (the boundary check, and the number of deleted items, which sizes the
// update), then edit_run on the table the device built.  Two host waits before the decode where
// the codepoint call makes one.
int replica_apply_patches_bytes(Engine& E, Replica& r, const PatchRec* p, size_t n,
                                const uint8_t* ins, size_t ins_len, uint32_t* added,
                                uint32_t* tombstoned, EditStats* stats) {
    if (stats) *stats = EditStats{};
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    if (n == 0) return CRDT_HIP_OK;
    if (!p) {
        E.err = "null patch array";
        return CRDT_HIP_EINVAL;
    }
    EditPlanBytes plan;
    rc = edit_plan_bytes(p, n, ins, ins_len, r.vis_bytes, r.n, plan, E.err);
    if (rc) return rc;
    const uint64_t np = plan.patch.size(), ncp = plan.cps.size();
    EditArgs a{};
    if (r.n == 0) {
        // nothing to translate: the checks left one patch, at byte 0 of an empty document
        if (np != 1 || plan.patch[0].old_pos_b || plan.patch[0].del_b) {
            E.err = "edit: a patch set beyond an empty replica passed the checks";
            return CRDT_HIP_EBADLOG;
        }
        if (edit_words(ncp, 0) * 4 >= (1ull << 32) - 16) {
            E.err = "edit of 4 GiB or more";
            return CRDT_HIP_ERANGE;
        }
        const EditPatch one{0u, 0u, 0u, (uint32_t)ncp, 0u, 0u};
        CallScratch sc(E.stream);
        return edit_run(E, r, sc, a, plan.cps, &one, nullptr, 1, 0, added, tombstoned, stats);
    }
    if ((rc = replica_kept_order(E, r, "edit", &a.seq, &a.ntiles))) return rc;
    hipStream_t s = E.stream;
    CallScratch sc(s);
    HIPTRY(E, sc.counters(E_N + B_N), "hipMalloc edit counters");
    BytesArgs b{};
    HIPTRY(E, bytes_count_args(b, sc, r, a.seq, a.ntiles, sc.ctl + E_N), "hipMalloc byte tiles");
    b.np = (uint32_t)np;
    BytePatch* btab = nullptr;
    HIPTRY(E, sc.alloc(&btab, np), "hipMalloc byte patches");
    HIPTRY(E, sc.alloc(&b.cp_start, np), "hipMalloc byte patches");
    HIPTRY(E, sc.alloc(&b.cp_end, np), "hipMalloc byte patches");
    HIPTRY(E, sc.alloc(&b.tab, np), "hipMalloc edit patches");
    b.btab = btab;
    HIPTRY(E, hipMemcpyAsync(btab, plan.patch.data(), np * sizeof(BytePatch), hipMemcpyHostToDevice, s),
              "upload byte patches");
    HIPTRY(E, sc.time_begin(), "edit event");
    bytes_translate_enqueue(b, s);
    HIPTRY(E, hipGetLastError(), "byte translation kernels");
    HIPTRY(E, sc.time_end(), "edit event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl + E_N, b.ctl, B_N * 8, hipMemcpyDeviceToHost, s), "copy byte counters");
    HIPTRY(E, hipStreamSynchronize(s), "byte translation sync");  // the wait the byte form adds
    sc.time_add();
    const uint64_t* c = sc.hctl + E_N;
    if (c[B_ERR] == EB_TABLE) {  // (with E_ORD_SLOT too, the check below names the slot first)
        E.err = "edit: a patch ends before it starts";
        return CRDT_HIP_EBADLOG;
    }
    if ((rc = bytes_count_check(E, r, c, "edit", "bytes"))) return rc;
    if (c[B_STARTS] < np || c[B_ENDS] < np) {
        E.err = "patch boundary inside a codepoint";
        return CRDT_HIP_EINVAL;
    }
    const uint64_t ndel = c[B_NDEL];
    if (c[B_STARTS] != np || c[B_ENDS] != np || ndel > r.vis_cp) {
        E.err = "edit: the translated patches disagree with the replica's counters";
        return CRDT_HIP_EBADLOG;
    }
    if (edit_words(ncp, ndel) * 4 >= (1ull << 32) - 16) {
        E.err = "edit of 4 GiB or more";
        return CRDT_HIP_ERANGE;
    }
    return edit_run(E, r, sc, a, plan.cps, nullptr, b.tab, np, ndel, added, tombstoned, stats);
}

}  // namespace crdt
