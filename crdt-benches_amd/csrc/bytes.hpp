// bytes.hpp — what edit.hip hands to the translation kernels of bytes.hip: byte-offset patches
// (crdt_hip.h, "byte offsets") turned into the codepoint patch table k_edit_resolve and
// k_edit_emit take, where the replica lies; and the count and scan at its start, which anchor.hip
// and format.hip run alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "oplog.hpp"
#include "replica.hpp"
#include "wave.hpp"

namespace crdt {

// device counters (u64) of a translation
enum BCtl { B_ERR = 0, B_VIS, B_VISB, B_STARTS, B_ENDS, B_NDEL, B_N };
// B_ERR bits, after E_ORD_SLOT (order.hpp)
constexpr uint64_t EB_TABLE = 2;  // a patch whose end was found before its start

// Device pointers only; the caller owns every array.
struct BytesArgs {
    const uint32_t* seq;     // rank -> slot, ranks 0..n (replica_kept_order)
    const uint8_t* cp;       // 3-byte codepoint words of slots 0..n
    uint32_t n;              // items held
    uint32_t ntiles;         // tiles of kOrderTile ranks
    uint32_t* tcount;        // per tile: visible items, then their exclusive prefix
    uint32_t* tbytes;        // per tile: visible UTF-8 bytes (at most 16 KiB)
    uint64_t* tbpre;         //   and their exclusive prefix, which may pass 2^32
    const BytePatch* btab;   // the patches in bytes, by old byte position
    uint32_t np;
    uint32_t* cp_start;      // per patch: visible items before it (NIL: no item ends there)
    uint32_t* cp_end;        //   and before the end of its delete range
    EditPatch* tab;          // out: the table in codepoints, del0 filled in
    uint64_t* ctl;           // B_N counters
};

// Enqueues init, count and top alone: the counters cleared, tcount and tbpre the exclusive prefixes
// of the tiles' visible items and bytes, B_VIS and B_VISB their totals.  With np == 0 nothing of a
// patch is touched (anchor.hip and format.hip count and scan with it).
void bytes_count_enqueue(const BytesArgs& a, hipStream_t s);
// What the count needs of a replica whose kept order is seq, in ntiles tiles (replica_kept_order):
// its columns, the B_N counters at ctl and the three tile arrays, from the call's scratch.
inline hipError_t bytes_count_args(BytesArgs& a, CallScratch& sc, const Replica& r, const uint32_t* seq,
                                   uint32_t ntiles, uint64_t* ctl) {
    a.seq = seq;
    a.cp = r.logs.cp;
    a.n = r.n;
    a.ntiles = ntiles;
    a.ctl = ctl;
    hipError_t rc = sc.alloc(&a.tcount, (uint64_t)ntiles);
    if (rc == hipSuccess) rc = sc.alloc(&a.tbytes, (uint64_t)ntiles);
    if (rc == hipSuccess) rc = sc.alloc(&a.tbpre, (uint64_t)ntiles);
    return rc;
}
// After the wait, c: the host copy of the count's counters.  EBADLOG, as "<who>: ...", if the order
// named a slot that is no item or the totals are not the replica's visible items and bytes.
int bytes_count_check(Engine& E, const Replica& r, const uint64_t* c, const char* who, const char* what);
// Enqueues the translation on `s`: init, count, top, translate, table.  The caller then waits
// for ctl: B_STARTS or B_ENDS below np means a boundary inside a codepoint.
void bytes_translate_enqueue(const BytesArgs& a, hipStream_t s);

}  // namespace crdt
