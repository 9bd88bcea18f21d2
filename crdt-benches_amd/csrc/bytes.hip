// bytes.hip — the byte-offset reading of local edits on a device-resident replica
// (crdt_hip_replica_apply_patches_bytes; semantics in crdt_hip.h, "byte offsets"): a translation
// pre-pass that turns patches whose pos and del count UTF-8 bytes into the codepoint patch table
// edit.hip resolves.  The host twin is OpLog::apply_patches_bytes (oplog.cpp).  The byte form of
// patches since a mark needs no kernel of its own: it is the BYTES instantiation of patch.hip.
//
// The host has checked what the arguments alone can tell (edit_plan_bytes) and uploads, per patch,
// its byte position in the document before the call and the bytes it deletes.  In those
// coordinates the patches do not touch (old_pos_b[k + 1] > old_pos_b[k] + del_b[k], DESIGN.md
// §6g), so a byte offset is the start or the end of at most one patch, and every visible item,
// which knows the byte offset at which it ends, is the only writer of the entries it decides.
//
//   k_bytes_init       counters, and the boundaries of every patch set to "not found"
//   k_bytes_count      a workgroup per tile of kOrderTile = 4,096 consecutive ranks, four ranks per
//                      thread: the tile's visible items and their UTF-8 bytes (order_tile_count)
//   k_bytes_top        one workgroup scans both (order_tile_scan); the byte prefixes are 64-bit (a
//                      tile holds at most 16 KiB, a replica may hold more than 2^32 bytes)
//   k_bytes_translate  each tile recomputes, per visible item, its visible rank v and the byte end
//                      b of the document up to and including it (rank 0, the document start:
//                      (0, 0)), binary-searches the byte table for the last patch with
//                      old_pos_b <= b and stores cp_start[k] = v if b == old_pos_b[k] and
//                      cp_end[k] = v if b == old_pos_b[k] + del_b[k]
//   k_bytes_table      one workgroup of 1,024, a patch per thread in rounds: old_pos = cp_start,
//                      del = cp_end - cp_start, the exclusive scan of del (del0) and its total, and
//                      how many starts and ends were found.  Fewer than the patches: a boundary
//                      falls inside a codepoint, which the host reports as EINVAL
//
// No atomic decides an order (the only atomic is the OR of an error bit); every slot, rank and
// patch index is checked against n and np before use; no host copy of the replica's columns is
// made and nothing is handed to the decoder here.
#include "bytes.hpp"

#include "idtab.hpp"
#include "order.hpp"
#include "wave.hpp"

namespace crdt {
namespace {

__global__ __launch_bounds__(kJB) void k_bytes_init(BytesArgs a) {
    const uint32_t g = blockIdx.x * kJB + threadIdx.x;
    if (g < (uint32_t)B_N) a.ctl[g] = 0;
    if (g < a.np) {
        a.cp_start[g] = NIL;
        a.cp_end[g] = NIL;
    }
}

__global__ __launch_bounds__(kOrdT) void k_bytes_count(BytesArgs a) {
    __shared__ uint32_t red[kOrdW];
    order_tile_count(a.seq, a.cp, a.n, SelNow{}, a.ntiles, a.tcount, a.tbytes, &a.ctl[B_ERR], red);
}

__global__ __launch_bounds__(kOrdTop) void k_bytes_top(BytesArgs a) {
    __shared__ uint32_t lds[kOrdTop / 64];
    uint64_t vis, visb;
    order_tile_scan(a.ntiles, a.tcount, a.tbytes, a.tbpre, lds, vis, visb);
    if (threadIdx.x == 0) {
        a.ctl[B_VIS] = vis;
        a.ctl[B_VISB] = visb;
    }
}

__global__ __launch_bounds__(kOrdT) void k_bytes_translate(BytesArgs a) {
    __shared__ uint32_t lds[kOrdW];
    if (blockIdx.x >= a.ntiles) return;
    const uint64_t k0 = (uint64_t)blockIdx.x * kOrderTile + (uint64_t)threadIdx.x * kOrdPer;
    uint32_t w[kOrdPer], cpw[kOrdPer];
    uint64_t err = 0;
    order_lens4(a.seq, a.cp, a.n, SelNow{}, k0, w, cpw, err);  // (k_bytes_count reported any bad slot)
    uint32_t c = 0, bs = 0;
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        c += w[j] ? 1u : 0u;
        bs += w[j];
    }
    uint32_t tot;
    uint32_t v = a.tcount[blockIdx.x] + block_excl_scan<kOrdW>(c, lds, tot);   // visible before
    uint64_t b = a.tbpre[blockIdx.x] + block_excl_scan<kOrdW>(bs, lds, tot);   // and their bytes
#pragma unroll
    for (uint32_t j = 0; j < kOrdPer; ++j) {
        if (!w[j] && k0 + j != 0) continue;
        if (w[j]) {  // this item's visible rank and the byte at which it ends (the start: 0, 0)
            ++v;
            b += w[j];
        }
        const uint32_t k = last_at_most(a.np, b, [&](uint32_t i) { return a.btab[i].old_pos_b; });
        if (k >= a.np) continue;
        const BytePatch e = a.btab[k];
        if (b == e.old_pos_b) a.cp_start[k] = v;
        if (b == e.old_pos_b + e.del_b) a.cp_end[k] = v;
    }
}

__global__ __launch_bounds__(kOrdT) void k_bytes_table(BytesArgs a) {
    __shared__ uint32_t lds[kOrdW];
    uint64_t c_del = 0, err = 0;
    uint32_t n_s = 0, n_e = 0;  // this thread's starts and ends found (np < 2^31)
    for (uint32_t base = 0; base < a.np; base += kOrdT) {
        const uint32_t i = base + threadIdx.x;
        uint32_t s = NIL, e = NIL, d = 0;
        if (i < a.np) {
            s = a.cp_start[i];
            e = a.cp_end[i];
            n_s += s != NIL ? 1u : 0u;
            n_e += e != NIL ? 1u : 0u;
            if (s != NIL && e != NIL) {
                if (e < s) err |= EB_TABLE;
                else d = e - s;
            }
        }
        uint32_t tot;
        const uint32_t d0 = block_excl_scan<kOrdW>(d, lds, tot);  // (deleted items: below 2^31)
        if (i < a.np) {
            const BytePatch bp = a.btab[i];
            a.tab[i] = EditPatch{s, d, bp.cp0, bp.ncp, (uint32_t)c_del + d0, 0u};
        }
        c_del += tot;
    }
    ctl_or(&a.ctl[B_ERR], err);
    const uint32_t t_s = block_sum_t0<kOrdW>(n_s, lds), t_e = block_sum_t0<kOrdW>(n_e, lds);
    if (threadIdx.x == 0) {
        a.ctl[B_NDEL] = c_del;
        a.ctl[B_STARTS] = t_s;
        a.ctl[B_ENDS] = t_e;
    }
}

}  // namespace

void bytes_count_enqueue(const BytesArgs& a, hipStream_t s) {
    k_bytes_init<<<grid_for(std::max<uint64_t>(a.np, B_N), kJB), kJB, 0, s>>>(a);
    k_bytes_count<<<a.ntiles, kOrdT, 0, s>>>(a);
    k_bytes_top<<<1, kOrdTop, 0, s>>>(a);
}

int bytes_count_check(Engine& E, const Replica& r, const uint64_t* c, const char* who, const char* what) {
    if (c[B_ERR] & E_ORD_SLOT) {
        E.err = std::string(who) + ": the kept document order names a slot that is no item";
        return CRDT_HIP_EBADLOG;
    }
    if (c[B_VIS] != r.vis_cp || c[B_VISB] != r.vis_bytes) {
        E.err = std::string(who) + ": the visible " + what +
                " of the kept order disagree with the replica's counters";
        return CRDT_HIP_EBADLOG;
    }
    return CRDT_HIP_OK;
}

void bytes_translate_enqueue(const BytesArgs& a, hipStream_t s) {
    bytes_count_enqueue(a, s);
    k_bytes_translate<<<a.ntiles, kOrdT, 0, s>>>(a);
    k_bytes_table<<<1, kOrdT, 0, s>>>(a);
}

}  // namespace crdt
