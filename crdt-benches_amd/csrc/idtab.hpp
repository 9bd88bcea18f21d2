// idtab.hpp — what the kernels that name items by identity share (join.hip, delta.hip, and through
// locate.hpp anchor.hip and format.hip): the identity of a key word, the open-addressing identity
// table (u32 entries claimed by atomicCAS, identity equality by gathering the key column) and the
// ids of the items new to dst; and, for patch.hip, edit.hip and bytes.hip too, the block reductions
// that keep device counters to one atomic per block.  Header-only, internal linkage.
#pragma once
#include <algorithm>
#include <cstdint>

#include "engine.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

constexpr int kJB = 256;  // threads per block
constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // table: free entry; map: the item is new to dst
constexpr uint32_t kMaxGridJ = 2048;      // grid-stride kernels: one counter atomic per block

// An item's identity in its key word: a Fugue left child's side bit is not part of its name.
template <bool FUGUE>
__device__ __forceinline__ uint64_t jident(uint64_t k) {
    return FUGUE ? k & ~kLeftKey : k;
}

__device__ __forceinline__ uint32_t jhash(uint64_t k) {
    k ^= k >> 29;
    k *= 0x9E3779B97F4A7C15ull;
    return (uint32_t)(k >> 32);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, o);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), o);
        const uint64_t y = ((uint64_t)hi << 32) | lo;
        x = y < x ? y : x;
    }
    return x;
}
// Min of x over the block, valid in thread 0.
__device__ __forceinline__ uint64_t block_min_t0(uint64_t x) {
    __shared__ uint64_t lds[kJB / 64];
    x = wave_min_u64(x);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    uint64_t t = ~0ull;
    if (threadIdx.x == 0)
        for (int i = 0; i < kJB / 64; ++i) t = lds[i] < t ? lds[i] : t;
    __syncthreads();
    return t;
}
// One device atomic per block, and only from blocks that have something to say: same-address
// atomics serialise at the L2 (one per wave of a 180 k-slot prefix cost k_join_pmax 33 us).
__device__ __forceinline__ void ctl_min(uint64_t* p, uint64_t x) {
    x = block_min_t0(x);
    if (threadIdx.x == 0 && x != ~0ull) atomicMin((unsigned long long*)p, (unsigned long long)x);
}
__device__ __forceinline__ void ctl_max(uint64_t* p, uint64_t x) {
    x = ~block_min_t0(~x);
    if (threadIdx.x == 0 && x) atomicMax((unsigned long long*)p, (unsigned long long)x);
}
__device__ __forceinline__ void ctl_or(uint64_t* p, uint64_t e) {
    if (e) atomicOr((unsigned long long*)p, (unsigned long long)e);
}

// Claim an entry for slot s of the log whose key column is `key`; returns the other slot that
// already holds identity k (a duplicate), kEmpty if none.  The table has at least twice as
// many entries as slots, so the probe ends; `full` reports a table that did not (never expected).
template <bool FUGUE>
__device__ __forceinline__ uint32_t tab_insert(uint32_t* tab, uint32_t mask, const uint64_t* key,
                                               uint32_t s, uint64_t k, bool& full) {
    uint32_t h = jhash(k) & mask;
    for (uint32_t it = 0; it <= mask; ++it) {
        const uint32_t old = atomicCAS(&tab[h], kEmpty, s);
        if (old == kEmpty) return kEmpty;
        if (jident<FUGUE>(key[old]) == k) return old;  // (the key column is not written by this kernel)
        h = (h + 1u) & mask;
    }
    full = true;
    return kEmpty;
}
// The slot holding identity k in a table that is complete (built by an earlier kernel), or kEmpty.
template <bool FUGUE>
__device__ __forceinline__ uint32_t tab_find(const uint32_t* tab, uint32_t mask, const uint64_t* key,
                                             uint64_t k) {
    uint32_t h = jhash(k) & mask;
    for (uint32_t it = 0; it <= mask; ++it) {
        const uint32_t e = tab[h];
        if (e == kEmpty) return kEmpty;
        if (jident<FUGUE>(key[e]) == k) return e;
        h = (h + 1u) & mask;
    }
    return kEmpty;
}

// The items new to dst (map[i] == kEmpty; `in`: i is an item) take the ids base + their rank
// among the new items, in index order.  blk: the exclusive prefixes of the blocks' counts of new
// items.  Called by every thread of a block of kJB.
__device__ __forceinline__ void rank_new(uint32_t* map, const uint32_t* blk, uint32_t base, uint64_t i,
                                         bool in) {
    __shared__ uint32_t lds[kJB / 64];
    const bool isnew = in && map[i] == kEmpty;
    uint32_t tot;
    const uint32_t e = block_excl_scan<kJB / 64>(isnew ? 1u : 0u, lds, tot);
    if (isnew) map[i] = base + blk[blockIdx.x] + e;
}

// Grid of a grid-stride kernel over n slots: four slots per thread (a quarter of the counter
// atomics of one slot per thread), at most kMaxGridJ blocks.
inline uint32_t grid_stride(uint64_t n) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kMaxGridJ, grid_for(n, 4 * kJB)));
}
inline uint64_t pow2_at_least(uint64_t x) {
    uint64_t c = 64;
    while (c < x) c <<= 1;
    return c;
}

}  // namespace
}  // namespace crdt
