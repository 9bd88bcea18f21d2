// replica.hpp — Downstream on the device: an op log resident in HBM that receives encoded
// updates and is merged where it lies.
//
// Replaces diamond-types' OpLog::decode_and_add (the Dt Downstream adapter,
// /root/reference/src/rope.rs:222-224) for the bench's downstream group
// (/root/reference/src/main.rs:63-69: clone the initial replica, apply every update, len()).
// Updates use the wire format of OpLog::encode_from (oplog.cpp); a batch of them is decoded by
// the kernels in replica.hip straight into the replica's slot arrays, and the replica is then
// merged by the engine like any resident document (one document, slot k = item id k).
#pragma once
#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace crdt {

// Incremental merge state of a replica (incr.hip, crdt_hip_replica_merge_inc): the document
// order of the items 0..n it covers (tombstones included; rank 0 = the document start), its
// inverse, and the merged text.
constexpr uint32_t kIncMax = 4096;  // most items a fast-path merge appends
struct IncState {
    bool valid = false;
    uint32_t n = 0;                  // items the order covers
    uint64_t cap = 0;                // entries of seq[0], seq[1], rank[0], rank[1]
    uint32_t* seq[2] = {nullptr, nullptr};  // rank -> slot (ping-pong: seq[cur] is current)
    int cur = 0;
    // slot -> rank, ping-pong like seq: a merge reads the old ranks of the new roots' parents in
    // every workgroup while the splices of other workgroups write the new ranks, so they are
    // two arrays (rank[cur] read, rank[cur ^ 1] written)
    uint32_t* rank[2] = {nullptr, nullptr};
    // (Fugue replicas) 1 bit per slot: the item has a left child (a new left child of an old
    // item goes right before it only while it has none)
    uint32_t* hasl = nullptr;
    // per new item (kIncMax): the anchor rank found by k_inc_search for a root whose key is not
    // above every old key (0xFFFFFFFF: the search ran out of range)
    uint64_t* hanc = nullptr;
    uint32_t* lb_flag = nullptr;     // per tile of the order: look-back status, aggregate and
    uint64_t* lb_agg = nullptr;      //   inclusive prefix of the text (incr.hip inc_lookback)
    uint64_t* lb_inc = nullptr;
    uint64_t lb_cap = 0;
    uint8_t* text = nullptr;
    uint64_t text_cap = 0;
    uint64_t* ctl = nullptr;         // device counters (incr.hip ICtl)
    uint64_t* hres = nullptr;        // host-mapped result block (written by the last phase)
    uint64_t* dres = nullptr;        //   (its device address)
    uint64_t calls = 0;              // calls made (stamps the result block)
    std::vector<uint32_t> hseq;      // (rebuild staging)
    // (CRDT_INC_PROFILE) this state's profile events and phase timestamps
    hipEvent_t pev[2] = {nullptr, nullptr};
    uint64_t* tsp = nullptr;
    IncState() = default;
    IncState(const IncState&) = delete;
    IncState& operator=(const IncState&) = delete;
    ~IncState();
};

struct Replica {
    DeviceLogs logs;          // one document: slot 0 = document start, slot k = item k
    uint32_t n = 0;           // items present (ids 1..n)
    uint64_t vis_cp = 0;      // visible codepoints (Upstream::len, rope.rs:16-19)
    uint64_t vis_bytes = 0;   // visible UTF-8 bytes (= merged length)
    // update staging, grown on demand
    uint8_t* ubuf = nullptr;
    uint64_t ubuf_cap = 0;
    uint64_t* uoff = nullptr;  // n + 1 byte offsets
    uint4* uhdr = nullptr;     // per update {first id, items, deletes, data word offset}
    uint4* uscan = nullptr;    // per update {item offset, delete offset, known before, known after}
    uint64_t ucap = 0;
    uint4* ublk = nullptr;     // per 256-update block aggregates
    uint64_t ublk_cap = 0;
    uint32_t* imap = nullptr;  // per flattened item / delete of a batch: its update
    uint32_t* dmap = nullptr;
    uint64_t imap_cap = 0, dmap_cap = 0;
    uint64_t* uctl = nullptr;  // device counters (see replica.hip)
    uint64_t* hctl = nullptr;  // pinned host copy
    bool pending = false;      // a decode was enqueued and its counters not yet applied
    uint64_t gen = 0;          // bumped by every (re)allocation of the replica's device arrays
    uint64_t version = 0;      // bumped by every change of the contents
    uint16_t agent = 0;        // agent id of the replica's own edits (edit.hip); a clone keeps it
    std::vector<void*> graveyard;  // arrays replaced by a regrow, freed at the next wait
    IncState inc;              // incremental merge state (invalid until the first merge_inc)

    Replica() = default;
    Replica(const Replica&) = delete;
    Replica& operator=(const Replica&) = delete;
    ~Replica();
};

// A batch of encoded updates resident in HBM (uploaded once, applied to any replica of the
// context without a PCIe transfer).
struct UpdateBatch {
    uint8_t* buf = nullptr;   // the updates, concatenated (each 4-aligned)
    uint64_t* off = nullptr;  // n + 1 byte offsets
    uint64_t len = 0;
    uint32_t n = 0;
    uint32_t max_id = 0;      // largest item id the batch carries (read from the headers on the
                              // host at upload; 0 = unknown): sizes a replica before the decode

    UpdateBatch() = default;
    UpdateBatch(const UpdateBatch&) = delete;
    UpdateBatch& operator=(const UpdateBatch&) = delete;
    ~UpdateBatch();
};

int updates_upload(Engine& E, UpdateBatch& ub, const uint8_t* buf, uint64_t len,
                   const uint64_t* offsets, uint32_t n);
// As replica_apply, with the batch already in HBM.
int replica_apply_resident(Engine& E, Replica& r, const UpdateBatch& ub);
// The decode itself: buf/offsets are host pointers (uploaded first) or, if resident, device ones.
int replica_decode(Engine& E, Replica& r, const uint8_t* buf, uint64_t len,
                   const uint64_t* offsets, uint32_t n, bool resident);

// Room for ids 0..items (slot arrays grow by doubling; new slots are padding).
int replica_reserve(Engine& E, Replica& r, uint64_t items);
// Initial contents (Downstream's initial CRDT; may be empty).
int replica_upload(Engine& E, Replica& r, const crdt_hip_oplog_view* v);
// dst = src, device to device (Downstream: Clone, main.rs:64).
int replica_copy(Engine& E, const Replica& src, Replica& dst);
// Decode and apply updates i = 0..n-1, update i = buf[offsets[i], offsets[i+1]), in order, with
// OpLog::apply_update's semantics.  A batch that fails validation changes nothing.
int replica_apply(Engine& E, Replica& r, const uint8_t* buf, uint64_t len,
                  const uint64_t* offsets, uint32_t n);
// The decode without the wait: counters are copied to r.hctl in stream order (copy_counters)
// and applied by replica_settle.  max_id: the batch's largest id if known (0: bound from len).
int replica_decode_enqueue(Engine& E, Replica& r, const uint8_t* buf, uint64_t len,
                           const uint64_t* offsets, uint32_t n, bool resident, uint32_t max_id,
                           bool copy_counters);
// Wait for an enqueued decode and apply its counters (errors: the batch changed nothing).
int replica_settle(Engine& E, Replica& r);

// The downstream closure (main.rs:63-69: clone the initial replica, apply every update, len())
// in one call: `work` receives a copy of `init`, the resident batch is decoded into it and it is
// merged.  The merge is planned with the sizes the previous replay of the same init and batch
// produced, enqueued right behind the decode (one wait for the whole closure); a device check
// compares those sizes with the decode's counters, and on a mismatch the host merges again with
// the real ones.
// Once the sizes are known the whole closure (copy, decode, check, merge, result copies) is
// captured as a hipGraph and replayed while nothing it points to is reallocated.
struct ReplayState {
    Replica work;
    const Replica* init = nullptr;
    const UpdateBatch* ub = nullptr;
    uint64_t init_version = 0;
    bool known = false;
    uint32_t n_after = 0;
    uint64_t bytes_after = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<uint64_t> key;  // what the graph was captured with
    ReplayState() = default;
    ReplayState(const ReplayState&) = delete;
    ReplayState& operator=(const ReplayState&) = delete;
    ~ReplayState();
};
int replica_replay(Engine& E, const Replica& init, const UpdateBatch& ub, ReplayState& st,
                   uint64_t* cps, uint64_t* bytes, uint64_t* digest);

// Merge the replica's document (text may be null: length and digest only; cps: codepoints of
// the merged text, counted on the device).
int replica_merge(Engine& E, Replica& r, std::vector<uint8_t>* text, uint64_t* len,
                  uint64_t* digest, crdt_hip_stats* st, uint64_t* cps = nullptr);

// What the last join observed (crdt_hip_join_stats; tools/join_time.py reports it).
struct JoinStats {
    uint64_t prefix = 0;       // slots of the common prefix (mapped to themselves, in no table)
    uint64_t table_slots = 0;  // dst slots past the prefix, the entries of the identity table
    uint64_t table_cap = 0;    // its capacity (a power of two >= twice the entries)
    uint64_t device_ns = 0;    // summed device time of the join's kernels (HIP events)
};
// State-based merge (join.hip): dst <- dst U src by item identity (lamport, agent), the
// reference's `Downstream for Automerge` apply_update(&mut self, other: &Self) = doc.merge(other)
// (rope.rs:234-236).  Items of src that dst lacks are appended in src's slot
// order with their parents translated to dst's ids; an item both hold is tombstoned if either
// has it tombstoned.  *added: items appended; *tombstoned: items dst held that the join
// tombstoned.  Validated first: a rejected join (EBADLOG) changes nothing.  Two RGA replicas or
// two Fugue replicas (identity = key & ~kLeftKey; an appended item keeps its side, an item both
// hold must have the same side in each); a mixed pair is EINVAL.
int replica_join(Engine& E, Replica& dst, const Replica& src, uint32_t* added,
                 uint32_t* tombstoned, JoinStats* stats = nullptr);

// State-vector delta sync (delta.hip; wire layout and host twin in oplog.hpp / oplog.cpp): the
// reference's Yrs Downstream state_vector() + encode_diff_v1(&sv) + apply_update
// (rope.rs:252-255, :265-268) for replicas that diverged.  Same bytes and same resulting log as
// OpLog::state_vector / encode_diff / apply_diff.
struct DeltaStats {  // what the last device encode or apply observed (crdt_hip_delta_stats)
    uint64_t items = 0;        // items of the delta
    uint64_t ranges = 0;       // tombstone ranges of the delta
    uint64_t table_slots = 0;  // apply: dst slots entered into the identity table (all of them)
    uint64_t device_ns = 0;    // summed device time of the call's kernels (HIP events)
};
struct SvEntry;
// Per agent with an item, its largest lamport, by agent ascending.
int replica_state_vector(Engine& E, const Replica& r, std::vector<SvEntry>& out,
                         DeltaStats* stats = nullptr);
// The items of r that `sv` does not cover, in slot order, and the tombstones of the items it
// covers as identity ranges.  *out_len: the delta's size; ESPACE when buf is null or cap short.
int replica_encode_diff(Engine& E, const Replica& r, const SvEntry* sv, size_t nsv, uint8_t* buf,
                        size_t cap, size_t* out_len, DeltaStats* stats = nullptr);
// dst <- dst U delta, validated first: a rejected delta (EINVAL, EBADLOG, ERANGE) changes nothing.
int replica_apply_diff(Engine& E, Replica& dst, const uint8_t* buf, size_t len, uint32_t* added,
                       uint32_t* tombstoned, DeltaStats* stats = nullptr);

// Patches since a mark (patch.hip; semantics in crdt_hip.h, host twin OpLog::patches_since): what
// changed in the replica's document between a mark and now, as positional edits.
// A version of one replica: its item count and a device bit plane of n + 1 bits, 1 = the slot was
// tombstoned or is not an item (slot 0, and the padding of the last word).  Owns the buffer.
struct DeviceMark {
    uint32_t n = 0;
    uint64_t words = 0;
    uint64_t* bits = nullptr;
    DeviceMark() = default;
    DeviceMark(const DeviceMark&) = delete;
    DeviceMark& operator=(const DeviceMark&) = delete;
    ~DeviceMark();
};
// What every call that reads a mark asks of it first (r settled): a mark of this replica's past, with
// the plane its item count needs.  EINVAL otherwise.
inline int mark_fits(Engine& E, const Replica& r, const DeviceMark& m) {
    if (r.n < m.n || !m.bits || m.words != ((uint64_t)m.n + 1 + 63) / 64) {
        E.err = "the replica holds fewer items than the mark";
        return CRDT_HIP_EINVAL;
    }
    return CRDT_HIP_OK;
}
struct PatchStats {  // what the last device patches_since observed (crdt_hip_patch_stats)
    uint64_t patches = 0;    // patches found
    uint64_t ins_bytes = 0;  // their inserted UTF-8 bytes
    uint64_t ranks = 0;      // ranks of the document order streamed (the items held)
    uint64_t device_ns = 0;  // summed device time of the call's kernels (HIP events)
};
struct PatchRec;
// Settles a pending decode, then packs the tombstone bits of slots 0..n (k_mark_pack).
int replica_mark(Engine& E, Replica& r, DeviceMark& m);
// Brings r.inc up to date as replica_merge_inc does (so a call leaves the replica as a merge_inc
// would), then classifies, scans and compacts over the kept order.  *out_n / *out_ins: patches
// and inserted bytes; ESPACE (before the write pass) when out / ins are null or short.  EINVAL
// when the replica holds fewer items than the mark, ERANGE for 4 GiB or more of inserted bytes.
int replica_patches_since(Engine& E, Replica& r, const DeviceMark& m, PatchRec* out, size_t cap,
                          size_t* out_n, uint8_t* ins, size_t ins_cap, size_t* out_ins,
                          PatchStats* stats = nullptr);

// Local edits (edit.hip; semantics in crdt_hip.h, host twin OpLog::apply_patches): a set of
// positional patches in the patches_since convention, resolved against the kept document order and
// applied as items and tombstones under r.agent.
struct EditStats {  // what the last device apply_patches observed (crdt_hip_edit_stats)
    uint64_t patches = 0;     // patches applied
    uint64_t items = 0;       // items appended
    uint64_t tombstones = 0;  // items tombstoned
    uint64_t ranks = 0;       // ranks of the document order streamed (the items held before)
    uint64_t device_ns = 0;   // summed device time of the call's kernels, the decode of the
                              //   update they write included (HIP events; not the order update)
};
// Validates everything first (EINVAL / ERANGE as OpLog::apply_patches; a rejected call changes
// nothing), brings r.inc up to date as replica_merge_inc does, resolves the patches in kernels
// into one wire update in device memory and hands it to replica_decode_enqueue: the replica is
// left as replica_decode of that update leaves it.  *added / *tombstoned may be null.
int replica_apply_patches(Engine& E, Replica& r, const PatchRec* p, size_t n, const uint8_t* ins,
                          size_t ins_len, uint32_t* added, uint32_t* tombstoned,
                          EditStats* stats = nullptr);
// The byte-offset reading of both (crdt_hip.h, "byte offsets"): pos and del count UTF-8 bytes of
// the visible document.  patches_since_bytes is the BYTES instantiation of patch.hip's kernels
// (64-bit prefixes over the tiles; ERANGE also when one patch deletes 4 GiB or more).
// apply_patches_bytes translates the boundaries to codepoint ranks in the kernels of bytes.hip (a
// boundary inside a codepoint: EINVAL, after every other check but the lamport bound), then runs
// the resolve, emit and decode of edit.hip unchanged; it waits for the host twice before the decode.
int replica_patches_since_bytes(Engine& E, Replica& r, const DeviceMark& m, PatchRec* out,
                                size_t cap, size_t* out_n, uint8_t* ins, size_t ins_cap,
                                size_t* out_ins, PatchStats* stats = nullptr);
int replica_apply_patches_bytes(Engine& E, Replica& r, const PatchRec* p, size_t n,
                                const uint8_t* ins, size_t ins_len, uint32_t* added,
                                uint32_t* tombstoned, EditStats* stats = nullptr);

// The document order of every item r holds, as a merge_inc leaves it (and leaving r as a merge_inc
// does): *seq = rank -> slot for ranks 0..n, *ntiles = its tiles of kOrderTile ranks (order.hpp).
// Checked here, once, for the kernels that stream it: the order covers exactly the replica's
// items and both it and the slot arrays hold n + 1 entries, so a uint4 load of four ranks at or
// below n and the gather of their slots stay inside.  EBADLOG "<who>: the kept document order
// does not cover the replica" otherwise.
int replica_kept_order(Engine& E, Replica& r, const char* who, const uint32_t** seq,
                       uint32_t* ntiles);

// replica_kept_order, and the inverse order with it: *rank = slot -> rank for slots 0..n, the array
// the same merge_inc leaves (its splice writes a rank for every rank it writes a slot for).  Only
// the sizes are checked here; a kernel that reads rank[s] checks the value against n and, where it
// holds the slot anyway, seq[rank[s]] == s.
int replica_kept_ranks(Engine& E, Replica& r, const char* who, const uint32_t** seq,
                       const uint32_t** rank, uint32_t* ntiles);

// Anchors (anchor.hip; semantics in crdt_hip.h, host twin OpLog::anchors_at / anchors_resolve).
struct AnchorStats {  // what the last device anchors call observed (crdt_hip_anchor_stats)
    uint64_t anchors = 0;    // anchors of the call
    uint64_t unknown = 0;    // resolve: those whose identity the replica does not hold
    uint64_t ranks = 0;      // ranks of the document order streamed (the items held)
    uint64_t device_ns = 0;  // summed device time of the call's kernels (HIP events)
};
struct AnchorRec;
struct AnchorPosRec;
// Both settle a pending decode, check the arguments on the host (anchor_check_*), bring r.inc up to
// date as replica_merge_inc does and wait once; `out` is written only by a call that succeeds.
// bytes: pos counts UTF-8 bytes (a position inside a codepoint: EINVAL, found on the device).
int replica_anchors_at(Engine& E, Replica& r, const uint64_t* pos, const uint8_t* bias, size_t n,
                       bool bytes, AnchorRec* out, AnchorStats* stats = nullptr);
int replica_anchors_resolve(Engine& E, Replica& r, const AnchorRec* a, size_t n, AnchorPosRec* out,
                            AnchorStats* stats = nullptr);

// Formats (format.hip; semantics in crdt_hip.h, host twin OpLog::spans).
struct FormatStats {  // what the last device spans call observed (crdt_hip_format_stats)
    uint64_t formats = 0;    // formats of the call
    uint64_t pending = 0;    // those with an anchor whose identity the replica does not hold
    uint64_t segments = 0;   // segments between two named gaps, before equal neighbours merge
    uint64_t spans = 0;      // spans found
    uint64_t ranks = 0;      // ranks of the document order streamed (the items held)
    uint64_t device_ns = 0;  // summed device time of the call's kernels (HIP events)
};
struct FormatRec;
struct SpanRec;
struct SpanAttrRec;
// Settles a pending decode, checks the arguments on the host (format_check), brings r.inc up to
// date as replica_merge_inc does and waits twice: for the sizes, then for the result.  *out_n /
// *out_attrs / *pending are written by a call that succeeds, the first two also with ESPACE (out
// or attrs null or short, before the write pass); out and attrs only by a call that succeeds.
int replica_spans(Engine& E, Replica& r, const FormatRec* f, size_t n, SpanRec* out, size_t cap,
                  size_t* out_n, SpanAttrRec* attrs, size_t attr_cap, size_t* out_attrs,
                  size_t* pending, FormatStats* stats = nullptr);

// Text windows (text.hip; semantics in crdt_hip.h, host twin OpLog::text_at).
struct TextStats {  // what the last device text_at observed (crdt_hip_text_stats)
    uint64_t ranks = 0;          // ranks of the document order streamed (the items held)
    uint64_t tiles_written = 0;  // tiles the write pass launched a workgroup for
    uint64_t bytes = 0;          // bytes returned
    uint64_t device_ns = 0;      // summed device time of the call's kernels (HIP events)
};
struct TextInfo;
// Settles a pending decode, runs the checks of crdt_hip.h in their order (m null: the version now),
// brings r.inc up to date as replica_merge_inc does, counts and scans under the version's predicate,
// waits once for the totals and the window, and writes only the tiles the window overlaps.
// *out_len and *info are written by a call that succeeds and with ESPACE (before the write pass);
// out only by a call that succeeds.
int replica_text_at(Engine& E, Replica& r, const DeviceMark* m, uint64_t start, uint64_t end,
                    uint32_t flags, uint8_t* out, size_t cap, size_t* out_len, TextInfo* info,
                    TextStats* stats = nullptr);

// The line index (lines.hip; semantics in crdt_hip_lines.h, host twins OpLog::line_starts and
// OpLog::lines_of).
struct LineStats {  // what the last device line_starts / lines_of observed (crdt_hip_line_stats)
    uint64_t queries = 0;    // line numbers or positions of the call
    uint64_t ranks = 0;      // ranks of the document order streamed (the items held)
    uint64_t device_ns = 0;  // summed device time of the call's kernels (HIP events)
};
struct LinePos;
struct LineInfo;
// Both calls: q holds n line numbers (positions false; flags ignored) or n gap positions, in
// codepoints or with kTextBytes in UTF-8 bytes.  Settles a pending decode, runs the checks of
// crdt_hip_lines.h in their order (m null: the version now), brings r.inc up to date as
// replica_merge_inc does, counts and scans codepoints, bytes and line breaks under the version's
// predicate, seeks every query with a wave and waits once.  out and *info are written only by a
// call that succeeds.
int replica_lines(Engine& E, Replica& r, const DeviceMark* m, bool positions, const uint64_t* q, size_t n,
                  uint32_t flags, LinePos* out, LineInfo* info, LineStats* stats = nullptr);

// UTF-16 positions (utf16.hip; semantics in crdt_hip_utf16.h, host twin OpLog::units_of).
struct UnitStats {  // what the last device translation observed (crdt_hip_unit_stats)
    uint64_t queries = 0;    // positions of the call
    uint64_t ranks = 0;      // ranks of the document order streamed (the items held)
    uint64_t device_ns = 0;  // summed device time of the call's kernels (HIP events)
};
struct UnitPos;
struct UnitInfo;
// q holds n gap positions in `unit` (kUnit*, oplog.hpp).  Settles a pending decode, runs the checks
// of crdt_hip_utf16.h in their order (m null: the version now; bound: unit_check's), brings r.inc up
// to date as replica_merge_inc does, counts and scans codepoints, bytes and UTF-16 code units under
// the version's predicate, seeks every position with a wave and waits once.  out and *info are
// written only by a call that succeeds.
int replica_units(Engine& E, Replica& r, const DeviceMark* m, uint32_t unit, const uint64_t* q, size_t n,
                  UnitPos* out, UnitInfo* info, UnitStats* stats = nullptr, uint64_t bound = 1ull << 31);
// The UTF-16 reading of apply_patches and patches_since (crdt_hip_utf16.h): compositions of one
// replica_units call over the patches' boundaries and the codepoint call, which runs unchanged.
// Each pays one more pass over the order and one more host wait than its codepoint call.  The
// checks and the arithmetic are the host's (edit_plan_utf16, edit_patches_utf16, since_bounds,
// since_utf16; oplog.hpp).  patches_since_utf16 writes out only with a code of 0 or ESPACE, except
// that a call refused after the codepoint pass may leave codepoint patches in it.
int replica_apply_patches_utf16(Engine& E, Replica& r, const PatchRec* p, size_t n, const uint8_t* ins,
                                size_t ins_len, uint32_t* added, uint32_t* tombstoned,
                                EditStats* stats = nullptr, UnitStats* ustats = nullptr);
int replica_patches_since_utf16(Engine& E, Replica& r, const DeviceMark& m, PatchRec* out, size_t cap,
                                size_t* out_n, uint8_t* ins, size_t ins_cap, size_t* out_ins,
                                PatchStats* stats = nullptr, UnitStats* ustats = nullptr);

// Incremental merge (incr.hip): the merged text (may be null), its UTF-8 bytes and codepoints;
// *path = 1 when only the items appended since the previous merge_inc were ranked, 0 for a
// full merge (the first call, a concurrent update, more than kIncMax new items, Fugue).
int replica_merge_inc(Engine& E, Replica& r, std::vector<uint8_t>* text, uint64_t* bytes,
                      uint64_t* cps, uint32_t* path);

}  // namespace crdt
