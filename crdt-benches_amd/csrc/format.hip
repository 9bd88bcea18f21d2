// format.hip — formats on a device-resident replica (replica.hpp, crdt_hip_replica_spans):
// rich-text attribute ranges between two anchors, last-writer-wins per key by op identity, with
// removal ops, flattened into the non-overlapping spans an editor paints.  The semantics are
// stated in crdt_hip.h, "formats"; the host twin is OpLog::spans (oplog.cpp), and both sides return
// the same span array, attr array and pending count byte for byte.
//
// The call works over the document order the replica keeps after a merge_inc (IncState::seq[cur],
// rank -> slot, tombstones included, and its inverse) and starts with the count and scan of
// bytes.hip (bytes_count_enqueue): per tile of kOrderTile = 4,096 ranks the visible codepoints and
// their UTF-8 bytes, then the exclusive prefixes of both and the totals.  The host has checked the
// formats (format_check) and uploads them sorted by (key, op): within a key the last format that
// covers an item wins it.
//
//   k_fmt_init      counters; the identity table and the bit plane cleared; the 2n anchor ids copied
//                   into a contiguous column (start of format i at 2i, its end at 2i + 1)
//   k_locate_insert (locate.hpp) the distinct identities into an open-addressing table of at least
//                   twice as many entries as anchors
//   k_locate_probe  (locate.hpp) a grid-stride pass over the key column: every item looks its
//                   identity up and, on a hit, records its slot for the entry
//   k_fmt_gaps      a thread per format: slot -> rank from the kept inverse order (locate_rank), the
//                   two gaps, the pending flag; a format that covers something sets its two gaps in a
//                   bit plane over the gaps 0..n (atomicOr)
//   k_fmt_bcount    a wave per tile of the plane (4,096 gaps, a word per lane): its set bits
//   k_fmt_btop      one workgroup scans the tiles' counts: the boundaries B, the segments B - 1
//   k_fmt_bcompact  a wave per tile: its set bits, in order, into the sorted boundary array
//   k_fmt_bpos      a wave per boundary: the visible codepoints and bytes at the ranks up to its gap,
//                   from the tile prefixes and a walk of the tile 64 ranks a step (view_walk)
//   k_fmt_live      one workgroup: the segments (boundary j, boundary j + 1] that hold a visible item,
//                   compacted in order (a scan); the others are dropped
//   k_fmt_count     a thread per such segment: one walk over the formats, the index the same in every
//                   lane, that finds per key the winner for this segment and for the one before it:
//                   the size of its attribute set, whether the two sets are equal, and from both the
//                   head flag (a set that is not empty and differs from its predecessor's)
//   k_fmt_scan      one workgroup: exclusive scans of the head flags and of the heads' set sizes: the
//                   span and attr offsets and the totals (the sizes the host waits for)
//   k_fmt_emit      a thread per head: its span record and, by the same walk, its attributes
//   k_fmt_close     a thread per segment that ends a run (its successor is a head, has an empty set,
//                   or does not exist): the span's len and len_bytes from the boundary prefixes
//
// No atomic decides an order: locate.hpp says why for the table's CAS and the slot's min; here an
// OR sets a bit of the plane or an error bit, one add per block counts the pending; the boundaries
// come out sorted because the plane is compacted in rank order, not by when a bit was set.
// Every slot, rank, tile, table, boundary and segment index is checked against n and the sizes of
// the call before it becomes an address, and a bad one raises an F_ERR bit (EBADLOG) instead;
// every loop is bounded (a probe by the table size, a walk by the tile or the format count, a
// word's bits by 64).  No host copy of the replica's columns is made; the host waits twice, for the
// sizes and for the result.
//
// Known cost: a call streams every rank and every key of the replica once, however few the
// formats; k_fmt_count and k_fmt_emit are O(segments * formats); after a join or a delta the call
// first pays inc_rebuild's ORDER-mode merge.
#include <cstring>
#include <vector>

#include "bytes.hpp"
#include "idtab.hpp"
#include "locate.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// device counters (u64), after the B_N of the count
enum FCtl { F_ERR = 0, F_PENDING, F_BOUNDS, F_SEGS, F_LIVE, F_SPANS, F_ATTRS, F_N };
// F_ERR bits, after E_ORD_SLOT (order.hpp), EL_RANK and EL_TABLE (locate.hpp)
constexpr uint64_t EF_BOUND = 8;  // a boundary, segment, span or attr index outside its array
constexpr uint64_t EF_RANGE = 16;  // 2^32 or more attributes

constexpr uint32_t kFmtW = kJB / 64;      // waves per workgroup
constexpr uint32_t kPlaneTile = kOrderTile / 64;  // plane words per tile: one per lane
static_assert(kPlaneTile == 64, "a wave holds a tile of the plane, a word per lane");

struct FmtDev {  // a format on the device: its gaps (covers nothing: 1, 0) and what it sets
    uint32_t gs, ge;
    uint32_t key, flags;
    uint64_t value;
};

struct FmtArgs {
    OrderView v;
    uint32_t nf;             // formats of the call
    const FormatRec* fmt;    // the formats by (key, op)
    IdLookup l;              // their anchors; l.m = 2 * nf: also the capacity of every per-boundary array
    FmtDev* fd;
    uint64_t* plane;         // a bit per gap, ntiles * kPlaneTile words
    uint32_t* tb;            // per tile: its boundaries, then their exclusive prefix
    uint32_t* bounds;        // the distinct gaps named, ascending
    uint64_t* bpos;          // per boundary: visible codepoints at the ranks up to it
    uint64_t* bposb;         //   and their UTF-8 bytes
    uint32_t* live;          // the segments with a visible item, ascending
    uint32_t* cnt;           // per live segment: its attributes if it is a head, else 0
    uint32_t* flg;           //   bit 0: its set is not empty; bit 1: it is a head
    uint32_t* sidx;          //   heads before it
    uint32_t* aoff;          //   attributes of the heads before it
    SpanRec* out;
    SpanAttrRec* attrs;
    uint32_t nspans;
    uint64_t nattrs;
    uint64_t* ctl;
};

__global__ __launch_bounds__(kJB) void k_fmt_init(FmtArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    if (g < (uint64_t)F_N) a.ctl[g] = 0;
    locate_clear(a.l, g);
    if (g < (uint64_t)a.v.ntiles * kPlaneTile) a.plane[g] = 0;
    if (g < a.l.m) {
        const FormatRec& f = a.fmt[g >> 1];
        a.l.ids[g] = g & 1u ? f.end.id : f.start.id;
    }
}

// The gap of anchor `idx` (0..n); false: its identity is not held (or, with an error bit, its
// table entry or rank is bad).
__device__ __forceinline__ bool fmt_gap(const FmtArgs& a, const AnchorRec& an, uint32_t idx,
                                        uint32_t& gap, uint64_t& err) {
    gap = 0;
    if (an.id == kAnchorEdge) {
        gap = an.bias == kAnchorAfter ? 0u : a.v.n;
        return true;
    }
    uint32_t s, rk;
    if (locate_rank(a.l, a.v, idx, s, rk, err) != Loc::Found) return false;
    gap = an.bias == kAnchorAfter ? rk : rk - 1u;
    return true;
}

__global__ __launch_bounds__(kJB) void k_fmt_gaps(FmtArgs a) {
    __shared__ uint32_t red[kFmtW];
    const uint64_t i = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    uint64_t err = 0;
    uint32_t pend = 0;
    if (i < a.nf) {
        const FormatRec f = a.fmt[i];
        uint32_t gs, ge;
        const bool ks = fmt_gap(a, f.start, (uint32_t)(2 * i), gs, err);
        const bool ke = fmt_gap(a, f.end, (uint32_t)(2 * i + 1), ge, err);
        pend = ks && ke ? 0u : 1u;
        FmtDev d{1u, 0u, f.key, f.flags, f.value};
        if (ks && ke && gs < ge) {  // (ge <= n: inside the plane)
            d.gs = gs;
            d.ge = ge;
            atomicOr((unsigned long long*)&a.plane[gs >> 6], 1ull << (gs & 63u));
            atomicOr((unsigned long long*)&a.plane[ge >> 6], 1ull << (ge & 63u));
        }
        a.fd[i] = d;
    }
    ctl_or(&a.ctl[F_ERR], err);
    const uint32_t t = block_sum_t0<kFmtW>(pend, red);
    if (threadIdx.x == 0 && t) atomicAdd((unsigned long long*)&a.ctl[F_PENDING], (unsigned long long)t);
}

// A wave per tile of the plane; the branch depends on the tile alone, so a wave stays whole.
__global__ __launch_bounds__(kJB) void k_fmt_bcount(FmtArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * kFmtW + (threadIdx.x >> 6);
    if (t >= a.v.ntiles) return;
    const uint32_t c = wave_sum((uint32_t)__popcll(a.plane[t * kPlaneTile + lane]));
    if (lane == 0) a.tb[t] = c;
}

__global__ __launch_bounds__(kOrdTop) void k_fmt_btop(FmtArgs a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    const uint64_t b = block_scan_counts<kOrdTop>(a.tb, a.v.ntiles, lds);
    if (threadIdx.x == 0) {
        if (b > a.l.m) ctl_or(&a.ctl[F_ERR], EF_BOUND);  // (at most two gaps a format)
        a.ctl[F_BOUNDS] = b;
        a.ctl[F_SEGS] = b ? b - 1 : 0;
    }
}

__global__ __launch_bounds__(kJB) void k_fmt_bcompact(FmtArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * kFmtW + (threadIdx.x >> 6);
    if (t >= a.v.ntiles) return;
    uint64_t w = a.plane[t * kPlaneTile + lane];
    const uint32_t c = (uint32_t)__popcll(w);
    const uint64_t base = (uint64_t)a.tb[t] + wave_incl_scan(c) - c;
    uint64_t err = 0;
    for (uint32_t q = 0; q < 64u && w; ++q) {
        const uint32_t bit = (uint32_t)__ffsll((long long)w) - 1u;
        w &= w - 1;
        const uint64_t gap = t * kOrderTile + lane * 64u + bit;
        if (base + q < a.l.m && gap <= a.v.n) a.bounds[base + q] = (uint32_t)gap;
        else err |= EF_BOUND;
    }
    ctl_or(&a.ctl[F_ERR], err);
}

// The boundaries and the segments of the call, as the earlier kernels left them, held to the
// capacity of the arrays.
__device__ __forceinline__ uint32_t fmt_nbounds(const FmtArgs& a) {
    const uint64_t b = a.ctl[F_BOUNDS];
    return b < a.l.m ? (uint32_t)b : a.l.m;
}
__device__ __forceinline__ uint32_t fmt_nlive(const FmtArgs& a) {
    const uint64_t l = a.ctl[F_LIVE];
    return l < a.l.m ? (uint32_t)l : a.l.m;
}

// A wave per boundary.  Everything that branches depends on the boundary alone, so a wave stays
// whole through the ballots and the wave sum.
__global__ __launch_bounds__(kJB) void k_fmt_bpos(FmtArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kFmtW + (threadIdx.x >> 6);
    if (i >= fmt_nbounds(a)) return;
    uint64_t err = 0;
    const uint32_t g = a.bounds[i];
    uint64_t pos = 0, posb = 0;
    if (g > a.v.n) {
        err |= EF_BOUND;
    } else {  // the ranks up to and including g, in g's own tile (below ntiles: g <= n)
        view_walk(a.v, g / kOrderTile, g + 1u, lane, pos, posb, err);
    }
    if (lane == 0) {
        a.bpos[i] = pos;
        a.bposb[i] = posb;
    }
    ctl_or(&a.ctl[F_ERR], err);
}

__global__ __launch_bounds__(kOrdT) void k_fmt_live(FmtArgs a) {
    __shared__ uint32_t lds[kOrdW];
    const uint32_t nb = fmt_nbounds(a), ns = nb ? nb - 1u : 0u;
    uint32_t c = 0;  // (at most m < 2^18)
    uint64_t err = 0;
    for (uint32_t base = 0; base < ns; base += kOrdT) {
        const uint32_t j = base + threadIdx.x;
        uint32_t lv = 0;
        if (j < ns) {
            const uint64_t p0 = a.bpos[j], p1 = a.bpos[j + 1];
            if (p1 < p0 || a.bposb[j + 1] < a.bposb[j]) err |= EF_BOUND;
            lv = p1 > p0 ? 1u : 0u;
        }
        uint32_t tot;
        const uint32_t e = block_excl_scan<kOrdW>(lv, lds, tot);
        if (lv) a.live[c + e] = j;  // (c + e < ns < m)
        c += tot;
    }
    ctl_or(&a.ctl[F_ERR], err);
    if (threadIdx.x == 0) a.ctl[F_LIVE] = c;
}

// The attribute set of the ranks (lo, hi] between two neighbouring boundaries: per key group of the
// sorted formats the last one that covers them wins, and set(key, value) is called for a winner
// that is no REMOVE.  With PREV the same for (plo, phi], and `equal` tells whether the two sets are
// the same.  The index is the same in every lane: the loads of a format are uniform.
template <bool PREV, class F>
__device__ __forceinline__ void fmt_walk(const FmtArgs& a, uint32_t lo, uint32_t hi, uint32_t plo,
                                         uint32_t phi, bool& equal, F&& set) {
    bool w1 = false, w2 = false;
    uint64_t v1 = 0, v2 = 0;
    uint32_t key = 0;
    equal = true;
    auto close = [&] {
        if (w1) set(key, v1);
        if (PREV) equal = equal && w1 == w2 && (!w1 || v1 == v2);
        w1 = w2 = false;
    };
    for (uint32_t i = 0; i < a.nf; ++i) {
        const FmtDev d = a.fd[i];
        if (i && d.key != key) close();
        key = d.key;
        if (d.gs <= lo && hi <= d.ge) {
            w1 = !(d.flags & kFormatRemove);
            v1 = d.value;
        }
        if (PREV && d.gs <= plo && phi <= d.ge) {
            w2 = !(d.flags & kFormatRemove);
            v2 = d.value;
        }
    }
    close();
}

// The boundaries of live segment m (false, with EF_BOUND: it is none).
__device__ __forceinline__ bool fmt_segment(const FmtArgs& a, uint32_t m, uint32_t& j, uint32_t& lo,
                                            uint32_t& hi, uint64_t& err) {
    j = a.live[m];
    if ((uint64_t)j + 1 >= fmt_nbounds(a)) {
        err |= EF_BOUND;
        return false;
    }
    lo = a.bounds[j];
    hi = a.bounds[j + 1];
    return true;
}

__global__ __launch_bounds__(kJB) void k_fmt_count(FmtArgs a) {
    const uint64_t m = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    if (m >= fmt_nlive(a)) return;
    uint64_t err = 0;
    uint32_t j, lo, hi, pj, plo = 1, phi = 0, count = 0;
    bool equal = false;
    if (fmt_segment(a, (uint32_t)m, j, lo, hi, err)) {
        const auto one = [&](uint32_t, uint64_t) { ++count; };
        if (m && fmt_segment(a, (uint32_t)m - 1u, pj, plo, phi, err)) {
            fmt_walk<true>(a, lo, hi, plo, phi, equal, one);
        } else {
            fmt_walk<false>(a, lo, hi, plo, phi, equal, one);
            equal = false;
        }
    }
    const bool head = count != 0 && !equal;
    a.flg[m] = (count ? 1u : 0u) | (head ? 2u : 0u);
    a.cnt[m] = head ? count : 0u;
    ctl_or(&a.ctl[F_ERR], err);
}

__global__ __launch_bounds__(kOrdT) void k_fmt_scan(FmtArgs a) {
    __shared__ uint32_t lds[kOrdW];
    const uint32_t nl = fmt_nlive(a);
    uint64_t c_s = 0, c_a = 0;
    for (uint32_t base = 0; base < nl; base += kOrdT) {
        const uint32_t m = base + threadIdx.x;
        const uint32_t h = m < nl && (a.flg[m] & 2u) ? 1u : 0u, c = m < nl ? a.cnt[m] : 0u;
        uint32_t tot;
        const uint32_t es = block_excl_scan<kOrdW>(h, lds, tot);
        if (m < nl) a.sidx[m] = (uint32_t)c_s + es;
        c_s += tot;
        const uint32_t ea = block_excl_scan<kOrdW>(c, lds, tot);  // (a round: at most 2^26)
        if (m < nl) a.aoff[m] = (uint32_t)(c_a + ea);
        c_a += tot;
    }
    if (threadIdx.x == 0) {
        if (c_a >= (1ull << 32)) ctl_or(&a.ctl[F_ERR], EF_RANGE);
        a.ctl[F_SPANS] = c_s;
        a.ctl[F_ATTRS] = c_a;
    }
}

__global__ __launch_bounds__(kJB) void k_fmt_emit(FmtArgs a) {
    const uint64_t m = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    if (m >= fmt_nlive(a) || !(a.flg[m] & 2u)) return;
    uint64_t err = 0;
    uint32_t j, lo, hi;
    const uint32_t k = a.sidx[m], n_at = a.cnt[m];
    const uint64_t off = a.aoff[m];
    if (k >= a.nspans || off + n_at > a.nattrs || !fmt_segment(a, (uint32_t)m, j, lo, hi, err)) {
        ctl_or(&a.ctl[F_ERR], err | EF_BOUND);
        return;
    }
    a.out[k] = SpanRec{a.bpos[j], a.bposb[j], 0, 0, (uint32_t)off, n_at};
    uint32_t q = 0;
    bool equal;
    fmt_walk<false>(a, lo, hi, 1u, 0u, equal, [&](uint32_t key, uint64_t value) {
        if (q < n_at) a.attrs[off + q] = SpanAttrRec{value, key, 0u};
        ++q;
    });
    if (q != n_at) err |= EF_BOUND;
    ctl_or(&a.ctl[F_ERR], err);
}

__global__ __launch_bounds__(kJB) void k_fmt_close(FmtArgs a) {
    const uint64_t m = (uint64_t)blockIdx.x * kJB + threadIdx.x;
    const uint32_t nl = fmt_nlive(a);
    if (m >= nl) return;
    const uint32_t f = a.flg[m];
    if (!(f & 1u)) return;
    if (m + 1 < nl) {  // the run goes on through a successor that has a set and is no head
        const uint32_t nx = a.flg[m + 1];
        if ((nx & 1u) && !(nx & 2u)) return;
    }
    uint64_t err = 0;
    uint32_t j, lo, hi;
    const uint32_t s = a.sidx[m];  // heads before m: the run's own head included unless m is it
    if ((!(f & 2u) && s == 0) || !fmt_segment(a, (uint32_t)m, j, lo, hi, err)) {
        ctl_or(&a.ctl[F_ERR], err | EF_BOUND);
        return;
    }
    const uint32_t k = f & 2u ? s : s - 1u;
    if (k >= a.nspans) {
        ctl_or(&a.ctl[F_ERR], EF_BOUND);
        return;
    }
    // (k_fmt_emit, an earlier kernel, wrote pos and pos_bytes; this thread alone writes the lengths)
    a.out[k].len = a.bpos[j + 1] - a.out[k].pos;
    a.out[k].len_bytes = a.bposb[j + 1] - a.out[k].pos_bytes;
}

int fmt_fail(Engine& E, uint64_t e) {
    if (e & EF_RANGE) {
        E.err = "spans: 2^32 or more span attributes";
        return CRDT_HIP_ERANGE;
    }
    E.err = e & E_ORD_SLOT ? "spans: the kept document order names a slot that is no item"
            : e & EL_RANK  ? "spans: the kept inverse order disagrees with the order"
            : e & EL_TABLE ? "spans: the identity table did not take every anchor"
                           : "spans: a boundary or a segment lies outside the call's arrays";
    return CRDT_HIP_EBADLOG;
}

}  // namespace

int replica_spans(Engine& E, Replica& r, const FormatRec* f, size_t n, SpanRec* out, size_t cap,
                  size_t* out_n, SpanAttrRec* attrs, size_t attr_cap, size_t* out_attrs,
                  size_t* pending, FormatStats* stats) {
    if (stats) *stats = FormatStats{};
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    std::vector<uint32_t> by;
    rc = format_check(f, n, by, E.err);
    if (rc) return rc;
    if (stats) stats->formats = n;
    if (n == 0 || r.n == 0) {  // nothing held: no span, and every identity is unknown
        size_t pend = 0;
        for (size_t k = 0; k < n; ++k)
            pend += f[k].start.id != kAnchorEdge || f[k].end.id != kAnchorEdge ? 1u : 0u;
        *out_n = 0;
        *out_attrs = 0;
        *pending = pend;
        if (stats) stats->pending = pend;
        return CRDT_HIP_OK;
    }
    std::vector<FormatRec> sorted(n);  // (outlives the scratch, whose release waits for the stream)
    for (size_t k = 0; k < n; ++k) sorted[k] = f[by[k]];
    FmtArgs a{};
    rc = replica_kept_ranks(E, r, "spans", &a.v.seq, &a.v.rank, &a.v.ntiles);
    if (rc) return rc;
    hipStream_t s = E.stream;
    CallScratch sc(s);
    HIPTRY(E, sc.counters(B_N + F_N), "hipMalloc format counters");
    BytesArgs b{};
    HIPTRY(E, bytes_count_args(b, sc, r, a.v.seq, a.v.ntiles, sc.ctl), "hipMalloc format tiles");
    a.v.cp = r.logs.cp;
    a.v.key = r.logs.key;
    a.v.n = r.n;
    a.v.tcount = b.tcount;
    a.v.tbpre = b.tbpre;
    a.v.vis = sc.ctl + B_VIS;
    a.nf = (uint32_t)n;
    a.ctl = sc.ctl + B_N;
    const uint64_t m = 2 * (uint64_t)n, words = (uint64_t)a.v.ntiles * kPlaneTile;  // (n <= 65,536)
    FormatRec* dfmt = nullptr;
    HIPTRY(E, sc.alloc(&dfmt, n), "hipMalloc formats");
    HIPTRY(E, locate_alloc(sc, a.l, (uint32_t)m), "hipMalloc format table");
    const uint64_t tcap = (uint64_t)a.l.mask + 1;
    HIPTRY(E, sc.alloc(&a.fd, n), "hipMalloc formats");
    HIPTRY(E, sc.alloc(&a.plane, words), "hipMalloc format plane");
    HIPTRY(E, sc.alloc(&a.tb, (uint64_t)a.v.ntiles), "hipMalloc format tiles");
    HIPTRY(E, sc.alloc(&a.bounds, m), "hipMalloc format boundaries");
    HIPTRY(E, sc.alloc(&a.bpos, m), "hipMalloc format boundaries");
    HIPTRY(E, sc.alloc(&a.bposb, m), "hipMalloc format boundaries");
    HIPTRY(E, sc.alloc(&a.live, m), "hipMalloc format segments");
    HIPTRY(E, sc.alloc(&a.cnt, m), "hipMalloc format segments");
    HIPTRY(E, sc.alloc(&a.flg, m), "hipMalloc format segments");
    HIPTRY(E, sc.alloc(&a.sidx, m), "hipMalloc format segments");
    HIPTRY(E, sc.alloc(&a.aoff, m), "hipMalloc format segments");
    a.fmt = dfmt;
    HIPTRY(E, hipMemcpyAsync(dfmt, sorted.data(), n * sizeof(FormatRec), hipMemcpyHostToDevice, s),
              "upload formats");
    HIPTRY(E, sc.time_begin(), "format event");
    bytes_count_enqueue(b, s);
    k_fmt_init<<<grid_for(std::max<uint64_t>(std::max<uint64_t>(tcap, words), F_N), kJB), kJB, 0, s>>>(a);
    k_locate_insert<<<grid_for(m, kJB), kJB, 0, s>>>(a.l, &a.ctl[F_ERR]);
    if (r.logs.fugue) k_locate_probe<true><<<grid_stride(r.n), kJB, 0, s>>>(a.l, a.v.key, r.n);
    else k_locate_probe<false><<<grid_stride(r.n), kJB, 0, s>>>(a.l, a.v.key, r.n);
    k_fmt_gaps<<<grid_for(n, kJB), kJB, 0, s>>>(a);
    k_fmt_bcount<<<grid_for(a.v.ntiles, kFmtW), kJB, 0, s>>>(a);
    k_fmt_btop<<<1, kOrdTop, 0, s>>>(a);
    k_fmt_bcompact<<<grid_for(a.v.ntiles, kFmtW), kJB, 0, s>>>(a);
    k_fmt_bpos<<<grid_for(m, kFmtW), kJB, 0, s>>>(a);
    k_fmt_live<<<1, kOrdT, 0, s>>>(a);
    k_fmt_count<<<grid_for(m, kJB), kJB, 0, s>>>(a);
    k_fmt_scan<<<1, kOrdT, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "format kernels");
    HIPTRY(E, sc.time_end(), "format event");
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, (B_N + F_N) * 8, hipMemcpyDeviceToHost, s),
              "copy format counters");
    HIPTRY(E, hipStreamSynchronize(s), "format sync");  // the first wait: the sizes
    sc.time_add();
    const uint64_t* h = sc.hctl;
    if (stats) {
        stats->ranks = r.n;
        stats->device_ns = sc.dev_ns;
    }
    if ((rc = bytes_count_check(E, r, h, "spans", "items"))) return rc;
    if (h[B_N + F_ERR]) return fmt_fail(E, h[B_N + F_ERR]);
    const uint64_t nsp = h[B_N + F_SPANS], nat = h[B_N + F_ATTRS], pend = h[B_N + F_PENDING];
    if (nsp > m || nat < nsp || pend > n) return fmt_fail(E, EF_BOUND);
    if (stats) {
        stats->pending = pend;
        stats->segments = h[B_N + F_SEGS];
        stats->spans = nsp;
    }
    if (nsp && (!out || cap < nsp || !attrs || attr_cap < nat)) {
        *out_n = (size_t)nsp;
        *out_attrs = (size_t)nat;
        E.err = "buffer too small";
        return CRDT_HIP_ESPACE;
    }
    std::vector<SpanRec> hs((size_t)nsp);
    std::vector<SpanAttrRec> ha((size_t)nat);
    if (nsp) {
        a.nspans = (uint32_t)nsp;
        a.nattrs = nat;
        HIPTRY(E, sc.alloc(&a.out, nsp), "hipMalloc spans");
        HIPTRY(E, sc.alloc(&a.attrs, nat), "hipMalloc span attributes");
        HIPTRY(E, sc.time_begin(), "format event");
        k_fmt_emit<<<grid_for(m, kJB), kJB, 0, s>>>(a);
        k_fmt_close<<<grid_for(m, kJB), kJB, 0, s>>>(a);
        HIPTRY(E, hipGetLastError(), "format write kernels");
        HIPTRY(E, sc.time_end(), "format event");
        HIPTRY(E, hipMemcpyAsync(hs.data(), a.out, nsp * sizeof(SpanRec), hipMemcpyDeviceToHost, s),
                  "copy spans");
        HIPTRY(E, hipMemcpyAsync(ha.data(), a.attrs, nat * sizeof(SpanAttrRec), hipMemcpyDeviceToHost, s),
                  "copy span attributes");
        HIPTRY(E, hipMemcpyAsync(sc.hctl, a.ctl, 8, hipMemcpyDeviceToHost, s), "copy format counters");
        HIPTRY(E, hipStreamSynchronize(s), "format sync");  // the second wait: the result
        sc.time_add();
        if (stats) stats->device_ns = sc.dev_ns;
        if (sc.hctl[0]) return fmt_fail(E, sc.hctl[0]);
        std::memcpy(out, hs.data(), (size_t)nsp * sizeof(SpanRec));
        std::memcpy(attrs, ha.data(), (size_t)nat * sizeof(SpanAttrRec));
    }
    *out_n = (size_t)nsp;
    *out_attrs = (size_t)nat;
    *pending = (size_t)pend;
    return CRDT_HIP_OK;
}

}  // namespace crdt
