// utf16.hip — UTF-16 positions on a device-resident replica (replica.hpp, crdt_hip_replica_units_of
// and the *_utf16 edits and patches): a gap position translated between codepoints, UTF-8 bytes
// and UTF-16 code units, now or at a mark.  The semantics are stated in crdt_hip_utf16.h; the host
// twin is OpLog::units_of (oplog.cpp), and both sides return the same arrays byte for byte.
//
// As lines.hip, over the document order the replica keeps after a merge_inc (IncState::seq[cur],
// rank -> slot, tombstones included) under the version's selector (SelNow or SelMark, order.hpp),
// the one template parameter of every kernel here.  A third weight rides beside the codepoints and
// their UTF-8 bytes: the UTF-16 code units, 2 for a selected item of UTF-8 length 4 and else 1, so
// the loaders of order.hpp carry it already.
//
//   k_unit_count  a workgroup per tile of kOrderTile = 4,096 consecutive ranks, four ranks per
//                 thread as a uint4 (order_lens4); per tile the selected codepoints, their UTF-8
//                 bytes and their UTF-16 code units.  SelMark never reads the plane for a slot above
//                 n_mark or a word at or past its words.
//   k_unit_top    one workgroup scans the three tile aggregates into exclusive prefixes, in rounds of
//                 kOrdTop tiles with a carry (order_tile_scan: 32-bit for the codepoints, 64-bit for
//                 the bytes; block_scan_counts: 32-bit for the UTF-16 code units, which are at most
//                 two per item and so at most 2 n < 2^32 with n < 2^31 items; the carry and the total
//                 are 64-bit), and writes the version's totals.
//   k_unit_seek   a wave per position p in the unit asked.  0 and the version's length come from the
//                 totals; otherwise a binary search of that unit's prefixes for the last tile whose
//                 exclusive prefix is below p (strict, as seek_tile: a tile with nothing selected
//                 shares its prefix with its neighbours) and a walk of that tile, 64 ranks a step,
//                 to the first selected item whose inclusive prefix in the unit reaches p.  An item
//                 that steps over p (a byte inside a codepoint, the second unit of a pair) raises
//                 EU_INSIDE; otherwise lane 0 writes the item's three inclusive prefixes.  The
//                 walk's loads are issued in chunks of kWalkChunk steps through order_len_at, which
//                 puts no load behind a branch.
// No atomic decides a value (an OR raises an error bit); every rank, slot, tile, mark word and query
// index is checked against n, n_mark, the mark's words, ntiles and the query count before use; every
// loop is bounded (a search by the tiles, a walk by the tile).  A query that fails writes no record;
// the host waits once, runs the checks of crdt_hip_utf16.h from the totals and the error bits,
// verifies every record against its query and copies the n records out in one transfer.
//
// The *_utf16 edits and patches at the end of the file are compositions: one translation of the
// patches' boundaries by the kernels here, and the codepoint call (edit.hip, patch.hip) untouched.
// Each pays one more pass over the order and one more host wait than its codepoint call.
//
// Known cost: a call streams every rank of the replica once (the count), however few the
// positions, and after a join or a delta it also pays inc_rebuild's ORDER-mode merge.
#include <cstring>
#include <type_traits>
#include <vector>

#include "idtab.hpp"
#include "oplog.hpp"
#include "order.hpp"
#include "replica.hpp"
#include "util.hpp"
#include "view.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

// device counters (u64): what the host reads after its one wait
enum UCtl { U_ERR = 0, U_LEN, U_LENB, U_LEN16, U_N };
// U_ERR bits, after E_ORD_SLOT (order.hpp)
constexpr uint64_t EU_BEYOND = 2;  // a position beyond the version
constexpr uint64_t EU_INSIDE = 4;  // a position inside a codepoint (bytes) or a pair (UTF-16)
constexpr uint64_t EU_WALK = 8;    // a query's item is not in the tile the prefixes name

constexpr uint32_t kUnitW = kJB / 64;  // queries (waves) per workgroup

template <class Sel>
struct UnitArgs {
    OrderView v;        // the kept order and the version's codepoint and byte prefixes
    Sel sel;            // the version
    uint32_t* tcount;   // v.tcount and v.tbpre as the count and the scan write them
    uint32_t* tbytes;   // per tile: the selected UTF-8 bytes (at most 16 KiB)
    uint64_t* tbpre;
    uint32_t* t16;      // per tile: the selected UTF-16 code units (at most 8,192), then those before the tile
    const uint64_t* q;  // the positions, in `unit`
    uint32_t m;         // their number
    uint32_t unit;      // kUnitCodepoints, kUnitBytes or kUnitUtf16
    UnitPos* out;       // m records
    uint64_t* ctl;
};

__global__ void k_unit_init(uint64_t* ctl) {
    if (threadIdx.x < (uint32_t)U_N) ctl[threadIdx.x] = 0;
}

// ---- count -------------------------------------------------------------------------------------
template <class Sel>
__global__ __launch_bounds__(kOrdT) void k_unit_count(UnitArgs<Sel> a) {
    __shared__ uint32_t red[kOrdW];
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t len[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    order_lens4(a.v.seq, a.v.cp, a.v.n, a.sel, k0, len, cpw, err);
    ctl_or(&a.ctl[U_ERR], err);
    uint32_t c = 0, b = 0, u = 0;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        c += len[j] ? 1u : 0u;
        b += len[j];
        u += len[j] ? utf16_units(len[j]) : 0u;
    }
    const uint32_t tc = block_sum_t0<kOrdW>(c, red), tb = block_sum_t0<kOrdW>(b, red),
                   tu = block_sum_t0<kOrdW>(u, red);
    if (threadIdx.x == 0 && blockIdx.x < a.v.ntiles) {
        a.tcount[blockIdx.x] = tc;
        a.tbytes[blockIdx.x] = tb;
        a.t16[blockIdx.x] = tu;
    }
}

// ---- top ---------------------------------------------------------------------------------------
template <class Sel>
__global__ __launch_bounds__(kOrdTop) void k_unit_top(UnitArgs<Sel> a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    uint64_t c_cnt, c_by;
    order_tile_scan(a.v.ntiles, a.tcount, a.tbytes, a.tbpre, lds, c_cnt, c_by);
    // (32-bit prefixes: at most two code units per item, 2 n < 2^32 with n < 2^31 items)
    const uint64_t c_16 = block_scan_counts<kOrdTop>(a.t16, a.v.ntiles, lds);
    if (threadIdx.x == 0) {
        a.ctl[U_LEN] = c_cnt;
        a.ctl[U_LENB] = c_by;
        a.ctl[U_LEN16] = c_16;
    }
}

// ---- seek --------------------------------------------------------------------------------------
// The seek of one item by a whole wave, with a wave-uniform unit and thr (0 < thr < the version's
// length in that unit): the first selected item whose inclusive prefix in the unit is at least
// thr.  On true, in every lane: the selected codepoints up to and including that item, their UTF-8
// bytes and their UTF-16 code units.  false: no lane of the tile the prefixes name held it (the
// caller's EU_WALK).
template <class Sel>
__device__ __forceinline__ bool unit_walk(const UnitArgs<Sel>& a, uint32_t unit, uint64_t thr,
                                          uint32_t lane, uint64_t& err, uint64_t& inc_c, uint64_t& inc_b,
                                          uint64_t& inc_u) {
    auto pre = [&](uint32_t t) {
        return unit == kUnitUtf16 ? (uint64_t)a.t16[t] : unit == kUnitBytes ? a.tbpre[t] : (uint64_t)a.tcount[t];
    };
    uint32_t tile = 0;  // the last tile whose exclusive prefix is below thr (tile 0's is 0)
    for (uint32_t hi = a.v.ntiles; hi - tile > 1u;) {
        const uint32_t mid = (tile + hi) >> 1;
        if (pre(mid) < thr) tile = mid;
        else hi = mid;
    }
    uint64_t run_c = a.tcount[tile], run_b = a.tbpre[tile], run_u = a.t16[tile];
    const uint64_t le = ~0ull >> (63u - lane);  // this lane and the ones below
    bool found = false;
    constexpr uint32_t kSteps = kOrderTile / 64u;
    static_assert(kSteps % kWalkChunk == 0, "a tile is a whole number of chunks");
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < kSteps && !found; c0 += kWalkChunk) {
        uint32_t wts[kWalkChunk];
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st) {
            uint32_t sl;
            wts[st] = order_len_at(a.v.seq, a.v.cp, a.v.n, a.sel,
                                   (uint64_t)tile * kOrderTile + (c0 + st) * 64u + lane, sl, err);
        }
#pragma unroll
        for (uint32_t st = 0; st < kWalkChunk; ++st) {
            if (found) continue;  // (wave-uniform)
            const uint32_t len = wts[st];
            const uint64_t on = __ballot(len != 0), wide = __ballot(len == 4u);
            const uint32_t lc = (uint32_t)__popcll(on & le), lu = lc + (uint32_t)__popcll(wide & le);
            const uint32_t lb = wave_incl_scan(len);
            const uint64_t inc = unit == kUnitUtf16 ? run_u + lu : unit == kUnitBytes ? run_b + lb : run_c + lc;
            const uint32_t wt = unit == kUnitUtf16 ? utf16_units(len) : unit == kUnitBytes ? len : 1u;
            const bool hit = len != 0 && inc >= thr && inc - wt < thr;
            const uint64_t hm = __ballot(hit);  // (at most one lane: the prefixes ascend over items)
            if (hm) {
                const int src = (int)__builtin_ctzll(hm);
                inc_c = run_c + (uint32_t)__shfl((int)lc, src);
                inc_b = run_b + (uint32_t)__shfl((int)lb, src);
                inc_u = run_u + (uint32_t)__shfl((int)lu, src);
                found = true;
            } else {
                run_c += (uint32_t)__popcll(on);
                run_b += (uint32_t)__builtin_amdgcn_readlane((int)lb, 63);
                run_u += (uint32_t)(__popcll(on) + __popcll(wide));
            }
        }
    }
    return found;
}

// A wave per query.  Everything that branches depends on the query alone, so a wave stays whole
// through the ballots and the wave scans.
template <class Sel>
__global__ __launch_bounds__(kJB) void k_unit_seek(UnitArgs<Sel> a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kUnitW + (threadIdx.x >> 6);
    if (i >= a.m) return;
    const uint64_t len = a.ctl[U_LEN], lenb = a.ctl[U_LENB], len16 = a.ctl[U_LEN16];
    const uint64_t total = a.unit == kUnitUtf16 ? len16 : a.unit == kUnitBytes ? lenb : len;
    const uint64_t p = a.q[i];
    uint64_t err = 0, rc = 0, rb = 0, ru = 0;
    bool done = true;
    if (p > total) {
        err |= EU_BEYOND;
        done = false;
    } else if (p == total) {  // the end of the version (the start too, of an empty one)
        rc = len;
        rb = lenb;
        ru = len16;
    } else if (p != 0) {
        if (a.v.ntiles == 0 || !unit_walk(a, a.unit, p, lane, err, rc, rb, ru)) {
            err |= EU_WALK;
            done = false;
        } else if ((a.unit == kUnitUtf16 ? ru : a.unit == kUnitBytes ? rb : rc) != p) {
            err |= EU_INSIDE;
            done = false;
        }
    }
    if (done && lane == 0) a.out[i] = UnitPos{rc, rb, ru};
    ctl_or(&a.ctl[U_ERR], err);  // (E_ORD_SLOT is a lane's own)
}

template <class Sel>
int units_impl(Engine& E, Replica& r, const OrderView& v, const Sel& sel, uint32_t unit, const uint64_t* q,
               size_t n, UnitPos* out, UnitInfo* info, UnitStats* stats) {
    hipStream_t s = E.stream;
    CallScratch sc(s);
    const uint32_t ntiles = v.ntiles;
    UnitArgs<Sel> a{};
    a.v = v;
    a.sel = sel;
    a.unit = unit;
    a.m = (uint32_t)n;
    uint64_t* dq = nullptr;
    HIPTRY(E, sc.counters(U_N), "hipMalloc unit counters");
    HIPTRY(E, sc.alloc(&a.tcount, (uint64_t)ntiles), "hipMalloc unit tiles");
    HIPTRY(E, sc.alloc(&a.tbytes, (uint64_t)ntiles), "hipMalloc unit tiles");
    HIPTRY(E, sc.alloc(&a.tbpre, (uint64_t)ntiles), "hipMalloc unit tiles");
    HIPTRY(E, sc.alloc(&a.t16, (uint64_t)ntiles), "hipMalloc unit tiles");
    HIPTRY(E, sc.alloc(&dq, n), "hipMalloc unit queries");
    HIPTRY(E, sc.alloc(&a.out, n), "hipMalloc unit records");
    a.v.tcount = a.tcount;
    a.v.tbpre = a.tbpre;
    a.q = dq;
    a.ctl = sc.ctl;
    // (the caller's array outlives the wait below, so the upload may read it until then)
    if (n) HIPTRY(E, hipMemcpyAsync(dq, q, n * 8, hipMemcpyHostToDevice, s), "upload unit queries");
    HIPTRY(E, sc.time_begin(), "unit event");
    k_unit_init<<<1, 64, 0, s>>>(sc.ctl);
    k_unit_count<<<ntiles, kOrdT, 0, s>>>(a);
    k_unit_top<<<1, kOrdTop, 0, s>>>(a);
    if (n) k_unit_seek<<<grid_for(n, kUnitW), kJB, 0, s>>>(a);
    HIPTRY(E, hipGetLastError(), "unit kernels");
    HIPTRY(E, sc.time_end(), "unit event");
    std::vector<UnitPos> res(n);
    HIPTRY(E, hipMemcpyAsync(sc.hctl, sc.ctl, U_N * 8, hipMemcpyDeviceToHost, s), "copy unit counters");
    if (n)
        HIPTRY(E, hipMemcpyAsync(res.data(), a.out, n * sizeof(UnitPos), hipMemcpyDeviceToHost, s),
               "copy unit records");
    HIPTRY(E, hipStreamSynchronize(s), "unit sync");  // the one wait
    sc.time_add();
    if (stats) {
        stats->queries = n;
        stats->ranks = r.n;
        stats->device_ns = sc.dev_ns;
    }
    const uint64_t* h = sc.hctl;
    const uint64_t e = h[U_ERR];
    if (e & E_ORD_SLOT) {
        E.err = "units: the kept document order names a slot that is no item";
        return CRDT_HIP_EBADLOG;
    }
    bool off;
    if constexpr (std::is_same<Sel, SelMark>::value) off = h[U_LEN] > sel.m.n_mark;
    else off = h[U_LEN] != r.vis_cp || h[U_LENB] != r.vis_bytes;
    // (an item of two code units has four bytes: at most (bytes - codepoints) / 3 of them)
    if (off || h[U_LENB] < h[U_LEN] || h[U_LENB] > 4 * h[U_LEN] || h[U_LEN16] < h[U_LEN] ||
        3 * (h[U_LEN16] - h[U_LEN]) > h[U_LENB] - h[U_LEN]) {
        E.err = "units: the selected items of the kept order disagree with the replica's counters";
        return CRDT_HIP_EBADLOG;
    }
    if (int rc = unit_check_version(unit, (e & EU_BEYOND) != 0, (e & EU_INSIDE) != 0, E.err)) return rc;
    // what the kernels found is what was asked for
    bool ok = !(e & EU_WALK);
    for (size_t k = 0; k < n && ok; ++k) {
        const UnitPos& p = res[k];
        ok = (unit == kUnitUtf16 ? p.utf16 : unit == kUnitBytes ? p.bytes : p.cp) == q[k] &&
             p.cp <= h[U_LEN] && p.bytes <= h[U_LENB] && p.utf16 <= h[U_LEN16] && p.cp <= p.utf16 &&
             p.utf16 <= p.bytes;
    }
    if (!ok) {
        E.err = "units: a position's item is not where the tile prefixes say";
        return CRDT_HIP_EBADLOG;
    }
    if (n) std::memcpy(out, res.data(), n * sizeof(UnitPos));
    if (info) *info = UnitInfo{h[U_LEN], h[U_LENB], h[U_LEN16]};
    return CRDT_HIP_OK;
}

}  // namespace

int replica_units(Engine& E, Replica& r, const DeviceMark* m, uint32_t unit, const uint64_t* q, size_t n,
                  UnitPos* out, UnitInfo* info, UnitStats* stats, uint64_t bound) {
    if (stats) *stats = UnitStats{};
    HIPTRY(E, hipSetDevice(E.device), "hipSetDevice");
    int rc = replica_settle(E, r);
    if (rc) return rc;
    if (m && (rc = mark_fits(E, r, *m))) return rc;
    if ((rc = unit_check(q, n, unit, out, E.err, bound))) return rc;
    if (r.n == 0) {  // nothing held: every version is empty, and its one gap is 0 in every unit
        bool beyond = false;
        for (size_t k = 0; k < n; ++k) beyond |= q[k] != 0;
        if ((rc = unit_check_version(unit, beyond, false, E.err))) return rc;
        for (size_t k = 0; k < n; ++k) out[k] = UnitPos{0, 0, 0};
        if (info) *info = UnitInfo{0, 0, 0};
        if (stats) stats->queries = n;
        return CRDT_HIP_OK;
    }
    OrderView v{};
    if ((rc = replica_kept_order(E, r, "units", &v.seq, &v.ntiles))) return rc;
    v.cp = r.logs.cp;
    v.n = r.n;
    if (!m) return units_impl(E, r, v, SelNow{}, unit, q, n, out, info, stats);
    return units_impl(E, r, v, SelMark{{m->bits, m->n, m->words}}, unit, q, n, out, info, stats);
}

// ---- the compositions ----------------------------------------------------------------------------
int replica_apply_patches_utf16(Engine& E, Replica& r, const PatchRec* p, size_t n, const uint8_t* ins,
                                size_t ins_len, uint32_t* added, uint32_t* tombstoned, EditStats* stats,
                                UnitStats* ustats) {
    if (added) *added = 0;
    if (tombstoned) *tombstoned = 0;
    if (n == 0) return CRDT_HIP_OK;
    EditPlanUtf16 plan;
    std::string err_plan;
    const int rc_plan = edit_plan_utf16(p, n, ins, ins_len, plan, err_plan);
    std::vector<UnitPos> tr(plan.bounds.size());
    // (nothing to translate: the first patch was refused, and no range check comes before it)
    const int rc_units = plan.bounds.empty()
                             ? CRDT_HIP_OK
                             : replica_units(E, r, nullptr, kUnitUtf16, plan.bounds.data(), plan.bounds.size(),
                                             tr.data(), nullptr, ustats, 1ull << 32);
    std::vector<PatchRec> q;
    if (int rc = edit_patches_utf16(plan, rc_plan, err_plan, rc_units, p, n, tr.data(), q, E.err)) return rc;
    return replica_apply_patches(E, r, q.data(), n, ins, ins_len, added, tombstoned, stats);
}

int replica_patches_since_utf16(Engine& E, Replica& r, const DeviceMark& m, PatchRec* out, size_t cap,
                                size_t* out_n, uint8_t* ins, size_t ins_cap, size_t* out_ins,
                                PatchStats* stats, UnitStats* ustats) {
    // (ESPACE leaves here with the two counts written: they are those of the codepoint call)
    if (int rc = replica_patches_since(E, r, m, out, cap, out_n, ins, ins_cap, out_ins, stats)) return rc;
    const size_t n = *out_n;
    if (n == 0) return CRDT_HIP_OK;
    std::vector<uint64_t> bounds;
    since_bounds(out, n, ins, bounds);
    std::vector<UnitPos> tr(bounds.size());
    if (int rc = replica_units(E, r, &m, kUnitCodepoints, bounds.data(), bounds.size(), tr.data(), nullptr,
                               ustats, 1ull << 32)) {
        if (rc != CRDT_HIP_ERANGE && rc != CRDT_HIP_EINVAL) return rc;
        E.err = "patches since: a patch boundary lies outside the mark's version";
        return CRDT_HIP_EBADLOG;
    }
    return since_utf16(out, n, ins, tr.data(), E.err);
}

}  // namespace crdt
