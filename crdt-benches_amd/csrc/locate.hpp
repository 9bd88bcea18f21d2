// locate.hpp — what the kernels that turn the identities of a batch (anchors, format ends) into
// positions share (anchor.hip, format.hip): the view of the kept document order with its walk and
// seek (view.hpp, which text.hip takes alone) and the identity lookup of a batch: the init part, the
// insert and probe kernels, and "anchor -> rank".
// Header-only, internal linkage (the library has no relocatable device code).
//
// No atomic here decides an order.  k_locate_insert claims a table entry with a CAS: which of the
// anchors that share an identity owns the entry differs from run to run, what canon[] -> slot[]
// yields does not.  k_locate_probe picks a slot with a min: of two slots of a malformed log that
// share an identity the lower, as on the host.  An error bit is raised with an OR.
#pragma once
#include <cstdint>

#include "idtab.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "view.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// error bits, the same in A_ERR (anchor.hip) and F_ERR (format.hip), after E_ORD_SLOT (order.hpp)
constexpr uint64_t EL_RANK = 2;   // the inverse order names no rank, or not the slot's
constexpr uint64_t EL_TABLE = 4;  // the identity table did not take an anchor

// The identities a batch of m anchors names, and where the replica holds them.
struct IdLookup {
    uint64_t* ids;    // the anchors' ids, contiguous (what tab_insert / tab_find compare through)
    uint32_t* tab;    // identity table: anchor indices (kEmpty: free), mask + 1 entries
    uint32_t mask;
    uint32_t* canon;  // per anchor: the anchor that owns its identity's entry
    uint32_t* slot;   // per owning anchor: the slot that holds the identity (kEmpty: none)
    uint32_t m;
};

// The five arrays, the table of at least twice as many entries as anchors (m < 2^31).
inline hipError_t locate_alloc(CallScratch& sc, IdLookup& l, uint32_t m) {
    const uint64_t cap = pow2_at_least(2 * (uint64_t)m);
    l.m = m;
    l.mask = (uint32_t)(cap - 1);
    hipError_t rc = sc.alloc(&l.ids, m);
    if (rc == hipSuccess) rc = sc.alloc(&l.tab, cap);
    if (rc == hipSuccess) rc = sc.alloc(&l.canon, m);
    if (rc == hipSuccess) rc = sc.alloc(&l.slot, m);
    return rc;
}

// Thread g's part of the caller's init kernel (which also copies ids[g]): the table cleared, every
// anchor's slot "not found".
__device__ __forceinline__ void locate_clear(const IdLookup& l, uint64_t g) {
    if (g <= l.mask) l.tab[g] = kEmpty;
    if (g < l.m) l.slot[g] = kEmpty;
}

// The distinct identities of the batch into the table; a repeated identity shares the entry of the
// anchor that claimed it (canon[i]).  ctl_err: the caller's error word.
__global__ __launch_bounds__(kJB) void k_locate_insert(IdLookup l, uint64_t* ctl_err) {
    const uint64_t g = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    if (g >= l.m) return;
    uint32_t owner = (uint32_t)g;
    const uint64_t id = l.ids[g];
    if (id != kAnchorEdge) {
        bool full = false;
        const uint32_t d = tab_insert<false>(l.tab, l.mask, l.ids, (uint32_t)g, id, full);
        if (d != kEmpty) owner = d;
        if (full) ctl_or(ctl_err, EL_TABLE);
    }
    l.canon[g] = owner;
}

// A grid-stride pass over the key column, 8 B per slot: every item looks its identity up and, on a
// hit, records its slot for the entry.
template <bool FUGUE>
__global__ __launch_bounds__(kJB) void k_locate_probe(IdLookup l, const uint64_t* key, uint32_t n) {
    for (uint64_t s = 1 + (uint64_t)blockIdx.x * kJB + threadIdx.x; s <= n;
         s += (uint64_t)gridDim.x * kJB) {
        const uint32_t e = tab_find<false>(l.tab, l.mask, l.ids, jident<FUGUE>(key[s]));
        if (e != kEmpty && e < l.m) atomicMin(&l.slot[e], (uint32_t)s);
    }
}

// Where the identity of anchor idx lies: its slot s and its rank rk from the kept inverse order,
// checked against n and against seq[rk] == s.
enum class Loc { Found, Unknown /* no item holds it */, Bad /* with EL_TABLE or EL_RANK */ };
__device__ __forceinline__ Loc locate_rank(const IdLookup& l, const OrderView& v, uint32_t idx,
                                           uint32_t& s, uint32_t& rk, uint64_t& err) {
    const uint32_t own = l.canon[idx];
    s = own < l.m ? l.slot[own] : 0u;
    rk = 0;
    if (s == kEmpty) return Loc::Unknown;
    if (s == 0 || s > v.n) {
        err |= EL_TABLE;
        return Loc::Bad;
    }
    rk = v.rank[s];
    if (rk == 0 || rk > v.n || v.seq[rk] != s) {
        err |= EL_RANK;
        return Loc::Bad;
    }
    return Loc::Found;
}

}  // namespace
}  // namespace crdt
