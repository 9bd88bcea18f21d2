// view.hpp — what the kernels that go between positions and ranks a wave at a time share
// (anchor.hip, format.hip, text.hip): a read-only view of the document order a replica keeps after a
// merge_inc with the tile prefixes of a count and scan (order.hpp), the walk of one tile of it up to
// a rank (view_walk), and the seek of the item at which a position falls (seek_tile, seek_step,
// view_seek).  Header-only, internal linkage (the library has no relocatable device code).
#pragma once
#include <cstdint>

#include "order.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

struct OrderView {
    const uint32_t* seq;     // rank -> slot, ranks 0..n
    const uint32_t* rank;    // slot -> rank, slots 0..n
    const uint8_t* cp;       // 3-byte codepoint words of slots 0..n
    const uint64_t* key;
    uint32_t n;              // items held
    uint32_t ntiles;         // tiles of kOrderTile ranks (and gaps)
    const uint32_t* tcount;  // per tile: visible (text.hip: selected) items before it
    const uint64_t* tbpre;   //   and their UTF-8 bytes
    const uint64_t* vis;     // the visible items and bytes of the whole order (B_VIS, B_VISB)
};

// The visible codepoints and UTF-8 bytes at the ranks below `end`: the prefixes of `tile` (below
// ntiles, and end at most its last rank + 1: the caller's) and a walk of the tile's ranks before
// `end`, 64 a step (a lane at or past `end` loads rank 0, which holds no item).  Called by a whole
// wave.
__device__ __forceinline__ void view_walk(const OrderView& v, uint32_t tile, uint32_t end, uint32_t lane,
                                          uint64_t& pos, uint64_t& posb, uint64_t& err) {
    const uint64_t pre = v.tcount[tile], preb = v.tbpre[tile];  // (in flight during the walk)
    uint32_t cnt = 0, by = 0;
    for (uint32_t k0 = tile * kOrderTile; k0 < end; k0 += 64u) {
        uint32_t sl;
        const uint32_t wt = order_len_at(v.seq, v.cp, v.n, SelNow{}, k0 + lane < end ? k0 + lane : 0u, sl, err);
        cnt += (uint32_t)__popcll(__ballot(wt != 0));
        by += wt;
    }
    by = wave_sum(by);  // (a tile holds at most 16 KiB)
    pos = pre + cnt;
    posb = preb + by;
}

// Where a threshold falls: the first selected item whose inclusive prefix, in codepoints or in
// UTF-8 bytes, is at least thr (0 < thr <= the version's total, in that unit).
// A whole wave seeks it with a wave-uniform thr: seek_tile, then seek_step over the tile's ranks, 64
// a step, until found.  The one lane that holds the item calls item(inc_c, inc_b, len, slot): the
// selected codepoints up to and including it and their UTF-8 bytes, its UTF-8 length and its slot.
// (A callback, as order_load4's: the caller's few lines run inside the step, under its branch, and
// nothing of the item is carried through the steps in registers.)
struct Seek {
    uint32_t tile;   // the last tile whose exclusive prefix is below thr (tile 0's is 0)
    uint64_t run_c;  // the selected codepoints before the next step's ranks
    uint64_t run_b;  //   and their UTF-8 bytes
    bool found;      // some lane held the item (the same in every lane); not after the tile's last
                     // step: the item is not in the tile the prefixes name (the caller's *_WALK error)
};
// The binary search of the scanned tile prefixes (v.tcount, v.tbpre: of the selected items).
__device__ __forceinline__ Seek seek_tile(const OrderView& v, bool bytes, uint64_t thr) {
    auto pre = [&](uint32_t t) { return bytes ? v.tbpre[t] : (uint64_t)v.tcount[t]; };
    uint32_t lo = 0, hi = v.ntiles;  // (not last_at_most: a strict <, and tile 0 always qualifies)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre(mid) < thr) lo = mid;
        else hi = mid;
    }
    return Seek{lo, v.tcount[lo], v.tbpre[lo], false};
}
// One step: len and slot are the lane's of order_len_at for the step's rank.
template <class F>
__device__ __forceinline__ void seek_step(Seek& r, bool bytes, uint64_t thr, uint32_t lane, uint32_t len,
                                          uint32_t slot, F&& item) {
    const uint64_t on = __ballot(len != 0);
    const uint32_t inc_c = (uint32_t)__popcll(on & (~0ull >> (63u - lane)));
    const uint32_t inc_b = wave_incl_scan(len);
    const uint64_t inc = bytes ? r.run_b + inc_b : r.run_c + inc_c;
    const uint32_t wt = bytes ? len : 1u;
    const bool hit = len != 0 && inc >= thr && inc - wt < thr;
    r.found = __ballot(hit) != 0;  // (at most one lane: the prefixes ascend strictly over items)
    if (hit) item(r.run_c + inc_c, r.run_b + inc_b, len, slot);
    r.run_c += (uint32_t)__popcll(on);
    r.run_b += (uint32_t)__builtin_amdgcn_readlane((int)inc_b, 63);
}

constexpr uint32_t kWalkChunk = 16;  // steps of 64 ranks whose loads are issued together
// The whole seek, under the selector sel; false: not found.
template <class Sel, class F>
__device__ __forceinline__ bool view_seek(const OrderView& v, const Sel& sel, bool bytes, uint64_t thr,
                                          uint32_t lane, uint64_t& err, F&& item) {
    Seek r = seek_tile(v, bytes, thr);
    // in chunks of kWalkChunk steps, a chunk's loads first: the steps' gathers are independent of
    // one another, and a walk that loads as it goes pays one dependent round trip (order, then
    // codepoint word) per step.  A chunk, not the whole tile, keeps the registers of the loads in
    // flight to kWalkChunk and lets a walk end after the chunk that holds the item.
    constexpr uint32_t kSteps = kOrderTile / 64u;
    static_assert(kSteps % kWalkChunk == 0, "a tile is a whole number of chunks");
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < kSteps && !r.found; c0 += kWalkChunk) {
        uint32_t lens[kWalkChunk], sls[kWalkChunk];
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st)
            lens[st] = order_len_at(v.seq, v.cp, v.n, sel,
                                    (uint64_t)r.tile * kOrderTile + (c0 + st) * 64u + lane, sls[st], err);
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st)
            if (!r.found) seek_step(r, bytes, thr, lane, lens[st], sls[st], item);  // (wave-uniform)
    }
    return r.found;
}

}  // namespace
}  // namespace crdt
