// order.hpp — how patch.hip, edit.hip, bytes.hip and text.hip stream the document order a replica
// keeps after a merge_inc (IncState::seq[cur], rank -> slot, ranks 0..n, tombstones included;
// obtained and checked by replica_kept_order, incr.hip): a workgroup per tile of consecutive ranks,
// four ranks per thread, and one workgroup over the tiles' aggregates.  Here: the two ways a version
// selects items (not tombstoned now, alive at a mark), the loaders of four ranks and of one, the
// tiles' count and scan of the selected codepoints and their UTF-8 bytes, and the UTF-8 store.
// anchor.hip, format.hip and text.hip walk single tiles of the same size a wave at a time
// (view.hpp); incr.hip sizes the tiles.  Header-only, internal linkage.
#pragma once
#include <cstdint>

#include "engine.hpp"
#include "idtab.hpp"
#include "oplog.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

constexpr uint32_t kOrderTile = 4096;             // consecutive ranks per workgroup
constexpr uint32_t kOrdT = 1024;                  // threads of a tile's workgroup
constexpr uint32_t kOrdPer = kOrderTile / kOrdT;  // consecutive ranks per thread
static_assert(kOrdPer == 4, "a thread loads its ranks as one uint4");
constexpr uint32_t kOrdW = kOrdT / 64;            // waves per workgroup
constexpr int kOrdTop = 256;  // threads of the kernel that scans the tiles (an aggregate each)

// Bit 1 of every error word a pass over the order raises: the order names a slot that is no item
// of the replica.
constexpr uint64_t E_ORD_SLOT = 1;

// A version selects items: the ones that are not tombstoned now, or the ones a mark saw alive.
// sel(s, c): whether it selects slot s (any value) with codepoint word c.  sel(s, c, ok, v): v if ok
// and it does, else 0.  (A value, not a flag: returned as a flag, the 16 steps of a chunked walk keep
// 16 lane masks in SGPR pairs until the lengths are chosen, and k_text_top at a mark spills 50.)
struct SelNow {
    __device__ __forceinline__ uint32_t operator()(uint32_t, uint32_t c, bool ok, uint32_t v) const {
        return ok && !(c & kDelBit) ? v : 0u;
    }
    __device__ __forceinline__ bool operator()(uint32_t s, uint32_t c) const {
        return (*this)(s, c, true, 1u);
    }
};
struct MarkPlane {
    const uint64_t* bits;  // bit s = slot s was tombstoned at the mark, or is not an item
    uint32_t n_mark;       // items the replica held at the mark
    uint64_t words;        // words of bits (at least one: slot 0)
};
struct SelMark {
    MarkPlane m;
    // The plane is never read for a slot above n_mark or a word at or past `words`: such a slot
    // reads word 0 instead, so that no load sits behind a branch.
    __device__ __forceinline__ uint32_t operator()(uint32_t s, uint32_t, bool ok, uint32_t v) const {
        const bool in = s <= m.n_mark && (uint64_t)(s >> 6) < m.words;
        const uint64_t w = m.bits[in ? s >> 6 : 0u];
        return ok && in && !((w >> (s & 63u)) & 1ull) ? v : 0u;
    }
    __device__ __forceinline__ bool operator()(uint32_t s, uint32_t c) const {
        return (*this)(s, c, true, 1u);
    }
};

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

// The UTF-8 lengths (0: not selected, rank 0, a rank past n, a slot that is no item, which also
// raises E_ORD_SLOT) and the codepoints of the thread's four ranks k0..k0 + 3.
template <class Sel>
__device__ __forceinline__ void order_lens4(const uint32_t* seq, const uint8_t* cp, uint32_t n,
                                            const Sel& sel, uint64_t k0, uint32_t len[kOrdPer],
                                            uint32_t cpw[kOrdPer], uint64_t& err) {
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        len[j] = 0;
        cpw[j] = 0;
    }
    order_load4(seq, cp, n, k0, err, E_ORD_SLOT, [&](uint32_t j, uint32_t s, uint32_t c) {
        if (sel(s, c)) {
            cpw[j] = c & kDeltaCpMask;
            len[j] = utf8_len(cpw[j]);
        }
    });
}

// The same length for the single rank k (a walk's lane), and the slot sl it names (0: none).  No
// load sits behind a branch: a rank or a slot that is refused reads entry 0 of its array instead
// (rank 0, slot 0 and mark word 0 always exist), so that the loads of a chunk of a walk's steps can
// all be in flight at once.
template <class Sel>
__device__ __forceinline__ uint32_t order_len_at(const uint32_t* seq, const uint8_t* cp, uint32_t n,
                                                 const Sel& sel, uint64_t k, uint32_t& sl,
                                                 uint64_t& err) {
    const bool inr = k != 0 && k <= n;
    const uint32_t s = seq[inr ? k : 0];
    const bool item = inr && s != 0 && s <= n;
    err |= inr && !item ? E_ORD_SLOT : 0;
    sl = item ? s : 0u;
    const uint32_t c = cp3_get(cp, sl);
    return sel(sl, c, item, utf8_len(c & kDeltaCpMask));
}

// The count of a tile's workgroup (kOrdT threads, block b = tile b): the selected items of its
// ranks into tcount[b] and their UTF-8 bytes (at most 16 KiB) into tbytes[b]; a bad slot raises
// E_ORD_SLOT in *errw.  red: kOrdW entries of LDS.
template <class Sel>
__device__ __forceinline__ void order_tile_count(const uint32_t* seq, const uint8_t* cp, uint32_t n,
                                                 const Sel& sel, uint32_t ntiles, uint32_t* tcount,
                                                 uint32_t* tbytes, uint64_t* errw, uint32_t* red) {
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t w[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    order_lens4(seq, cp, n, sel, k0, w, cpw, err);
    ctl_or(errw, err);
    uint32_t c = 0, b = 0;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        c += w[j] ? 1u : 0u;
        b += w[j];
    }
    const uint32_t tc = block_sum_t0<kOrdW>(c, red), tb = block_sum_t0<kOrdW>(b, red);
    if (threadIdx.x == 0 && blockIdx.x < ntiles) {
        tcount[blockIdx.x] = tc;
        tbytes[blockIdx.x] = tb;
    }
}

// The scan of one workgroup of kOrdTop threads over the tiles' counts: tcount becomes its own
// exclusive prefix, tbpre that of tbytes, which is 64-bit (a tile holds at most 16 KiB, a replica
// may hold more than 2^32 bytes); vis and visb: the totals, in every thread.  The prefixes are
// written by this workgroup: one that reads them afterwards synchronises first.  lds: kOrdTop / 64
// entries.
__device__ __forceinline__ void order_tile_scan(uint32_t ntiles, uint32_t* tcount,
                                                const uint32_t* tbytes, uint64_t* tbpre,
                                                uint32_t* lds, uint64_t& vis, uint64_t& visb) {
    uint64_t c_vis = 0, c_b = 0;
    for (uint32_t base = 0; base < ntiles; base += kOrdTop) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < ntiles ? tcount[i] : 0u, b = i < ntiles ? tbytes[i] : 0u;
        uint32_t tot;
        const uint32_t ec = block_excl_scan<kOrdTop / 64>(c, lds, tot);
        if (i < ntiles) tcount[i] = (uint32_t)c_vis + ec;  // (at most n < 2^31)
        c_vis += tot;
        const uint32_t eb = block_excl_scan<kOrdTop / 64>(b, lds, tot);  // (a round: at most 4 MiB)
        if (i < ntiles) tbpre[i] = c_b + eb;
        c_b += tot;
    }
    vis = c_vis;
    visb = c_b;
}

// The UTF-8 of codepoint v, len = utf8_len(v) bytes at o.
__device__ __forceinline__ void utf8_store(uint8_t* o, uint32_t v, uint32_t len) {
    if (len == 1) {
        o[0] = (uint8_t)v;
    } else if (len == 2) {
        o[0] = (uint8_t)(0xC0u | (v >> 6));
        o[1] = (uint8_t)(0x80u | (v & 63u));
    } else if (len == 3) {
        o[0] = (uint8_t)(0xE0u | (v >> 12));
        o[1] = (uint8_t)(0x80u | ((v >> 6) & 63u));
        o[2] = (uint8_t)(0x80u | (v & 63u));
    } else {
        o[0] = (uint8_t)(0xF0u | (v >> 18));
        o[1] = (uint8_t)(0x80u | ((v >> 12) & 63u));
        o[2] = (uint8_t)(0x80u | ((v >> 6) & 63u));
        o[3] = (uint8_t)(0x80u | (v & 63u));
    }
}

}  // namespace
}  // namespace crdt
