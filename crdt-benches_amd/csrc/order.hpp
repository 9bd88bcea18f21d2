// order.hpp — how patch.hip, edit.hip and bytes.hip stream the document order a replica keeps after
// a merge_inc (IncState::seq[cur], rank -> slot, ranks 0..n, tombstones included; obtained and
// checked by replica_kept_order, incr.hip): a workgroup per tile of consecutive ranks, four ranks
// per thread, and one workgroup over the tiles' aggregates.  anchor.hip and format.hip walk single
// tiles of the same size a wave at a time (locate.hpp); incr.hip sizes the tiles.  Header-only,
// internal linkage.
#pragma once
#include <cstdint>

#include "engine.hpp"

namespace crdt {
namespace {

constexpr uint32_t kOrderTile = 4096;             // consecutive ranks per workgroup
constexpr uint32_t kOrdT = 1024;                  // threads of a tile's workgroup
constexpr uint32_t kOrdPer = kOrderTile / kOrdT;  // consecutive ranks per thread
static_assert(kOrdPer == 4, "a thread loads its ranks as one uint4");
constexpr uint32_t kOrdW = kOrdT / 64;            // waves per workgroup
constexpr int kOrdTop = 256;  // threads of the kernel that scans the tiles (an aggregate each)

// item(j, slot, codepoint word) for each of the thread's four ranks k0 + j (k0 a multiple of 4)
// that names an item: not for rank 0 (the document start), a rank past n or a slot outside 1..n;
// the last also raises `bit` in err.  The uint4 load needs seq to hold ranks 0..n and the gather
// cp to hold slots 0..n, which is what replica_kept_order checks.  (A callback, not arrays of
// slots and words with 0 for "refused": the callers' code then runs under the loader's own
// branches instead of testing the slot again.)
template <class F>
__device__ __forceinline__ void order_load4(const uint32_t* seq, const uint8_t* cp, uint32_t n,
                                            uint64_t k0, uint64_t& err, uint64_t bit, F&& item) {
    uint32_t sl[kOrdPer];
    if (k0 + kOrdPer - 1 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(seq + k0);
        sl[0] = v.x;
        sl[1] = v.y;
        sl[2] = v.z;
        sl[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kOrdPer; ++j) sl[j] = k0 + j <= n ? seq[k0 + j] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        if (k0 + j == 0 || k0 + j > n) continue;
        if (sl[j] == 0 || sl[j] > n) {
            err |= bit;
            continue;
        }
        item(j, sl[j], cp3_get(cp, sl[j]));
    }
}

}  // namespace
}  // namespace crdt
