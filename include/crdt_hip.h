/*
 * crdt_hip.h — C ABI of the MI355X-native merge engine (libcrdt_hip.so).
 *
 * This is the drop-in boundary for the replay-and-merge path of noib3/crdt-benches.  The
 * reference binds CRDT engines through two Rust traits:
 *   trait Upstream   /root/reference/src/rope.rs:6-33   (from_str, insert, remove, len, replace)
 *   trait Downstream /root/reference/src/rope.rs:185-191 (upstream_updates, apply_update)
 * and registers them in the bench at /root/reference/src/main.rs:43-46 and :78.  A Rust
 * `crdt-hip-sys` crate binds exactly the entry points below; the
 * `impl Upstream/Downstream for HipMerge` maps:
 *   from_str(s)          -> crdt_hip_oplog_new + crdt_hip_oplog_insert(0, s)   (rope.rs:113-121)
 *   insert(at, s)        -> crdt_hip_oplog_insert                               (rope.rs:124-126)
 *   remove(a..b)         -> crdt_hip_oplog_remove                               (rope.rs:129-131)
 *   len()                -> crdt_hip_merge  (replaces OpLog::checkout_tip().len(), rope.rs:134-136)
 *   upstream_updates     -> crdt_hip_oplog_version + crdt_hip_oplog_encode_from (rope.rs:196-220)
 *   apply_update(u)      -> crdt_hip_oplog_apply_update (replaces decode_and_add, rope.rs:222-224),
 *                           or on the device: crdt_hip_replica_apply_updates (batched)
 *   clone()              -> crdt_hip_oplog_clone (the device context is shared, never copied)
 *   apply_update(&other) -> crdt_hip_oplog_join, or on the device crdt_hip_replica_join: the
 *                           state-based Downstream of the Automerge adapter, doc.merge(other)
 *                           (rope.rs:234-236), for logs that diverged (two RGA logs or two
 *                           Fugue logs)
 *   state_vector / encode_diff_v1 / apply_update (the Yrs adapter, rope.rs:252-255)
 *                        -> crdt_hip_oplog_state_vector / _encode_diff / _apply_diff, or on the
 *                           device crdt_hip_replica_state_vector / _encode_diff / _apply_diff:
 *                           divergent logs exchange only what the other lacks ("delta sync")
 *   TestPatch(pos, del, ins) / replace (rope.rs:21-32), the other way round
 *                        -> crdt_hip_oplog_mark + crdt_hip_oplog_patches_since, or on the device
 *                           crdt_hip_replica_mark + crdt_hip_replica_patches_since: what an update,
 *                           a join or a delta changed in the document, as positional edits for an
 *                           editor that keeps a text buffer beside the log ("patches since a mark")
 *   insert / remove / replace on the device (Upstream for a resident replica)
 *                        -> crdt_hip_replica_replace / crdt_hip_replica_apply_patches ("local
 *                           edits"): positions resolved to identities in HIP kernels
 *   EDITS_USE_BYTE_OFFSETS = true (rope.rs:8,16-19; the cola and yrs adapters)
 *                        -> the *_bytes twins of replace, apply_patches and patches_since, on the
 *                           host and on the device ("byte offsets"): positions in UTF-8 bytes
 *   a cursor or selection end that survives sync (cola's Anchor, yrs' StickyIndex, automerge's
 *   cursors; no trait of the bench)
 *                        -> crdt_hip_oplog_anchors_at / _anchors_resolve, or on the device
 *                           crdt_hip_replica_anchors_at / _anchors_resolve ("anchors")
 *   attribute ranges that converge (Peritext, yrs' Text::format, automerge's marks; no trait of
 *   the bench)
 *                        -> crdt_hip_oplog_spans, or on the device crdt_hip_replica_spans
 *                           ("formats")
 *
 * Conventions
 *   - Every function returns int status: 0 = ok, < 0 = error (CRDT_HIP_E*).  Nothing throws or
 *     aborts across the ABI.  crdt_hip_last_error(ctx) returns the message of the last failure
 *     on that context (ctx == NULL: the last failure of a context-free call on this thread).
 *   - Host pointers are BORROWED for the duration of the call only.
 *   - Positions are Unicode codepoints (EDITS_USE_BYTE_OFFSETS = false, rope.rs:8,16-19), except
 *     in the functions named *_bytes ("byte offsets"), which take and report UTF-8 bytes.
 *   - A context is bound to one HIP device and must be used by one host thread at a time; calls
 *     are synchronous at the ABI (the work runs on the context's own HIP stream).
 *   - Op log ids: items are 1..n in creation order; id 0 is the document start (origin of an
 *     insert at position 0).
 */
#ifndef CRDT_HIP_H
#define CRDT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRDT_HIP_ABI_VERSION 2

enum {
    CRDT_HIP_OK = 0,
    CRDT_HIP_EINVAL = -1,   /* bad argument */
    CRDT_HIP_ERANGE = -2,   /* position / id out of range */
    CRDT_HIP_ENOMEM = -3,   /* host or device allocation failed */
    CRDT_HIP_EDEVICE = -4,  /* HIP runtime error (no device, launch failure, ...) */
    CRDT_HIP_EBADLOG = -5,  /* malformed op log (bad parent, cycle) detected on device */
    CRDT_HIP_ESPACE = -6,   /* caller's output buffer too small (*out_len says how much) */
    CRDT_HIP_EIO = -7,      /* file / decompression / parse error */
    CRDT_HIP_ECOMM = -8     /* RCCL error */
};

typedef struct crdt_hip_ctx crdt_hip_ctx;
typedef struct crdt_hip_oplog crdt_hip_oplog;
typedef struct crdt_hip_trace crdt_hip_trace;
typedef struct crdt_hip_batch crdt_hip_batch;
typedef struct crdt_hip_replica crdt_hip_replica;
typedef struct crdt_hip_updates crdt_hip_updates;
typedef struct crdt_hip_logfile crdt_hip_logfile;

/* Anchor op log, structure of arrays (borrowed view).  Item k (0-based) has id k+1.
 * parent = origin_left id (0 = document start).  Document order (RGA): pre-order of the tree
 * parent -> children, siblings by (lamport, agent) descending.  cp = Unicode codepoint. */
typedef struct {
    uint32_t n;
    const uint32_t* parent;
    const uint32_t* origin_right; /* optional (may be NULL); not used by the RGA merge */
    const uint32_t* lamport;
    const uint16_t* agent;
    const uint8_t* deleted;
    const uint32_t* cp;
    /* optional (NULL: RGA).  Fugue order (SURVEY.md §8(a) s0 "side u8 (Fugue)"): side[k] != 0
     * makes item k a LEFT child of parent[k]; the document is then the in-order walk (left
     * children, the item, right children; each side by (lamport, agent) descending).  An RGA
     * log is the Fugue log without left children.  lamport must stay below 0xFFFFFFFF (a Fugue
     * log with lamport 0xFFFFFFFF, or with a left child of the document start, is malformed:
     * CRDT_HIP_EBADLOG on every path that takes a view).
     * ABI 2 added this field at the end of the struct: a caller written against ABI 1 must
     * zero-initialise the whole view (`crdt_hip_oplog_view v = {0};`) and check
     * crdt_hip_abi_version() == CRDT_HIP_ABI_VERSION, or a garbage `side` makes its log a Fugue
     * log. */
    const uint8_t* side;
} crdt_hip_oplog_view;

/* Per-stage device time of the last merge (HIP events on the context's stream), in ns,
 * summed over every wave of the call, plus work counters. */
typedef struct {
    uint64_t items;        /* op-log items merged */
    uint64_t docs;         /* documents merged */
    uint64_t text_bytes;   /* merged bytes produced */
    uint64_t runs;         /* runs (unary chains of consecutive items) the items collapsed to */
    uint32_t waves;        /* device waves the call was split into */
    uint32_t nstages;      /* valid entries in stage_ns / stage_launches */
    uint64_t stage_ns[16];
    uint32_t stage_launches[16];
    uint64_t total_ns;     /* first event to last event of the call */
} crdt_hip_stats;

/* Stage indices of crdt_hip_stats.stage_ns (one HIP-event interval per kernel group). */
enum {
    CRDT_HIP_STAGE_CLASSIFY = 0, /* level 0: seq/jump bits, weights, per-tile UTF-8           */
    CRDT_HIP_STAGE_RUNS = 1,     /* level 0: head bitvector, tile scan, run records, text     */
    CRDT_HIP_STAGE_SORTB = 2,    /* level 1 (radix): sort of the (run, next sibling) pairs by
                                    run id, and the run records in run order                  */
    CRDT_HIP_STAGE_COUNT = 3,    /* level 1: child counts (counting) or the digit histograms
                                    of the sort by parent run (radix)                         */
    CRDT_HIP_STAGE_SCAN = 4,     /* level 1: segment starts / radix bucket starts             */
    CRDT_HIP_STAGE_PLACE = 5,    /* level 1: runs grouped by parent run: placement (counting)
                                    or LDS-staged onesweep radix passes                       */
    CRDT_HIP_STAGE_LINK = 6,     /* level 1: sibling order of each group, first children      */
    CRDT_HIP_STAGE_WALK1 = 7,    /* level 1: Euler-tour sublist sums and each run's offset in
                                    its sublist (text mode: each sublist's text staged in walk
                                    order instead)                                            */
    CRDT_HIP_STAGE_RANK = 8,     /* level 1: ranking of the splitter lists                    */
    CRDT_HIP_STAGE_WALK2 = 9,    /* level 1: per-document totals (text mode: and the staged
                                    sublist texts copied to their documents)                  */
    CRDT_HIP_STAGE_EXPAND = 10,  /* runs copy their UTF-8 to their document offset (global
                                    level 1: offset in the sublist + the sublist's prefix)    */
    CRDT_HIP_STAGE_DIGEST = 11,  /* per-document tree digest                                  */
    CRDT_HIP_STAGE_DOCTREE = 12, /* level 1 in LDS: whole run tree of a document per workgroup
                                    (replaces stages 3-9 when every document fits)           */
    CRDT_HIP_STAGE_TEXT = 13,    /* text scatter after a k_doctree in scatter mode: the tiles'
                                    slot-order text to the documents (k_tscatter)            */
    CRDT_HIP_STAGE_ENCODE = 14,  /* raw SoA mode (crdt_hip_batch_raw): the input encoding derived
                                    from the raw columns inside the merge (k_raw_encode + the
                                    compact nsq list)                                        */
    CRDT_HIP_NSTAGES = 15
};

/* ---- library / context ----------------------------------------------------------------- */
int crdt_hip_abi_version(void);
int crdt_hip_device_count(int* out);
int crdt_hip_init(int device, crdt_hip_ctx** out);
int crdt_hip_destroy(crdt_hip_ctx* ctx);
const char* crdt_hip_last_error(const crdt_hip_ctx* ctx);
/* Tuning: "splitter_stride" of the global list ranking (power of two, 16..4096; default 16),
 * "max_wave_slots" per device wave (4096..2^31, default 2^30), and "level1": 0 = per-document LDS merge of
 * the run tree whenever every document of a wave fits a workgroup's LDS (default), 1 = always
 * the global (multi-kernel) level-1 path, and "lanes" (1..8, default 2): waves of a multi-wave
 * merge run concurrently on that many streams, each with its own scratch (1 = one after the
 * other), "lane_gate" (default 1: lanes take turns at the HBM-bound level 0), "plan_cache"
 * (default 1: a merge of logs merged before enqueues every wave with the launch plan the earlier
 * merge learnt, checked on the device, and waits once instead of after each wave's level 0),
 * "l1_split" (default 0; 1: such enqueued waves run level 1 on a low-priority stream of their
 * lane, so that the next wave's level 0 is favoured when the two compete for the CUs),
 * "tail_wave_div" (0..64, default 0; k: a merge of several waves ends with a wave of at most
 * max_wave_slots / k slots), "xcd_order" (default 1: XCD-aware tile order in level 0),
 * "group_docs" (replica batches: 1 = documents placed in slots base by base, each base's
 * replicas in waves of their own, so that only the waves of a base whose run trees exceed the
 * per-document LDS level 1 take the global one; results stay in the caller's order; default 0),
 * "runs_slots" (k_runs slots per thread, 16, 32 or 64; default 32),
 * "stile_text" (default 2: the per-document merge stages text from the per-tile segments by
 * LDS-DMA, tile by tile; 1: by loads and shifts into one contiguous image; 0: from the slot-order
 * text k_runs then writes),
 * "nsq_list" (the compact list of the parents and keys of the items without the previous-slot
 * flag: 1 (default) = resident batches, and replicas of at least 2^22 slots, whose merges rebuild
 * it; 2 = every replica too; 0 = never), "static_jumps" (default 1: RGA logs with that list keep
 * their jump bits, a function of the parent column alone, with it, and the merges only read them;
 * 0 = every merge rebuilds the bits), "dead_skip" (default 1: such logs also keep the tombstone
 * and previous-slot flags as bit planes of their own, one bit per slot each, built with the list,
 * and text merges fetch the codepoints only of 16-slot groups that hold a visible character;
 * every merge still reads every slot's tombstone; 0 = the flags are read from the codepoint word
 * of every slot), "plain_tiles" (default 1: resident batches on that path also keep a list of
 * their plain 4096-slot tiles, the inside of one typed run, a function of the parent column alone;
 * such a tile takes a thread of k_runs instead of a workgroup; 0 = a workgroup per tile),
 * "contraction" (run contraction of RGA waves, decided
 * when a batch is built or logs are uploaded: 0 = by the input (default: no contraction when at
 * least 3/4 of a wave's items lack the previous-slot flag), 1 = always, 2 = never; replica
 * merges, which count no flags, contract under 0 and 1 and never under 2), "l1_group"
 * (sibling grouping of the global level 1: 0 = by counting when the wave's largest document has
 * at most 2^16 runs or the wave at most 2^23, else by radix sorts (default), 1 = always
 * counting, 2 = always radix sorts), "rs_digit_bits" (digit width of the radix sort by parent:
 * 0 = 10 bits where that takes fewer passes than 8 (default), 8, 10),
 * "text_scatter" (default 0; 1: the text of such plans is written by a kernel of its own after the
 * per-document merge), "doctree_k32" (default 0; 1: every per-document merge on 32-bit sibling
 * keys).  A value outside a parameter's range is CRDT_HIP_EINVAL; the switches take 0 or 1.
 * Hooks for tests and experiments, any value, nonzero = on: "fuse_text" (default 1),
 * "doctree_lds_max", "glds_late", "plan_shrink" (default 0).  Results never depend on these. */
int crdt_hip_set_param(crdt_hip_ctx* ctx, const char* key, uint64_t value);

/* ---- op log: host-side resolver (positional patch -> anchor op) ---------------------------- */
int crdt_hip_oplog_new(crdt_hip_oplog** out);
/* Fugue anchors for every later insert (only on an empty log): an insert after left neighbour a
 * becomes a right child of a if a has none yet, else a left child of a's full-list successor.
 * A Fugue log's updates are wire version 2 (bit 31 of each cp word = left child); only Fugue
 * logs and Fugue replicas (crdt_hip_replica_new from a Fugue log's view, empty or not) take
 * them.  Version-1 (RGA) updates apply to either kind. */
int crdt_hip_oplog_set_fugue(crdt_hip_oplog* log, int on);
/* The agent id of this log's later local inserts (default 0).  Editors that exchange updates
 * need distinct agents: (lamport, agent) identifies an item. */
int crdt_hip_oplog_set_agent(crdt_hip_oplog* log, uint16_t agent);
int crdt_hip_oplog_clone(const crdt_hip_oplog* src, crdt_hip_oplog** out);
void crdt_hip_oplog_free(crdt_hip_oplog* log);
/* insert `nbytes` of UTF-8 at codepoint position `pos` (Upstream::insert). */
int crdt_hip_oplog_insert(crdt_hip_oplog* log, size_t pos, const char* utf8, size_t nbytes);
/* delete codepoints [start, end) (Upstream::remove). */
int crdt_hip_oplog_remove(crdt_hip_oplog* log, size_t start, size_t end);
/* Upstream::replace default (rope.rs:21-32): remove if end > start, then insert if non-empty. */
int crdt_hip_oplog_replace(crdt_hip_oplog* log, size_t start, size_t end, const char* utf8,
                           size_t nbytes);
/* Visible codepoints tracked by the resolver (host side; NOT the merged result). */
size_t crdt_hip_oplog_visible_len(const crdt_hip_oplog* log);
/* Borrowed SoA view, valid until the next mutation of `log`. */
int crdt_hip_oplog_get_view(const crdt_hip_oplog* log, crdt_hip_oplog_view* out);
/* Version token (items and delete ops so far) for encode_from. */
uint64_t crdt_hip_oplog_version(const crdt_hip_oplog* log);
/* Encode every op after `version` as one update (Downstream::upstream_updates, rope.rs:210-216).
 * If buf is NULL or cap too small, *out_len gets the needed size and ESPACE is returned. */
int crdt_hip_oplog_encode_from(const crdt_hip_oplog* log, uint64_t version, uint8_t* buf,
                               size_t cap, size_t* out_len);
/* Decode and append an update (Downstream::apply_update / decode_and_add, rope.rs:222-224). */
int crdt_hip_oplog_apply_update(crdt_hip_oplog* log, const uint8_t* buf, size_t len);
/* State-based merge of two divergent logs (the reference's `Downstream for Automerge`:
 * apply_update(&mut self, other: &Self) = doc.merge(other), rope.rs:234-236).
 * dst <- dst U src by item identity (lamport, agent): editors that forked from a common log and
 * both appended (each under its own agent, crdt_hip_oplog_set_agent) exchange their whole state.
 *   - every item of src whose identity dst lacks is appended, in src's slot order (new id =
 *     items of dst + 1 + rank among src's new items), parent and origin_right translated to dst's
 *     ids; an item both hold becomes deleted if either has it deleted;
 *   - *added: items appended; *tombstoned: items dst already held that the join deleted (either
 *     may be NULL);
 *   - validated first, and a rejected join changes nothing: CRDT_HIP_EBADLOG when two items of
 *     one log share an identity, when an item both hold differs in codepoint, translated
 *     parent or (Fugue) side, or when a parent does not precede its item; CRDT_HIP_ERANGE when
 *     the result would exceed the op-log size limit;
 *   - Fugue: two Fugue logs join like two RGA logs.  The identity stays (lamport, agent): the
 *     side is an attribute of the item, so two items of one log that differ in side alone share
 *     an identity, and an appended item keeps its side.  src is a caller's view, so it is also
 *     held to the rules of crdt_hip_oplog_view (lamport 0xFFFFFFFF or a left child of the
 *     document start: CRDT_HIP_EBADLOG).  The kind of a log is the presence of its side column
 *     (dst set Fugue by crdt_hip_oplog_set_fugue; src->side non-NULL), never its contents, and
 *     both must be of one kind: a Fugue log with an RGA log is CRDT_HIP_EINVAL, also when the
 *     Fugue one has no left child or either is empty;
 *   - joining a log with itself, or with one it already contains, changes nothing.
 * crdt_hip_oplog_version / encode_from keep their local meaning: a joined log ships its ops to
 * downstream replicas of that log as before (ids are the log's own); a join is not a wire update.
 * Positional edits after a join rebuild the resolver index first, as for a loaded log (Fugue:
 * an insert after an item that gained a right child through the join becomes a left child of
 * that item's successor). */
int crdt_hip_oplog_join(crdt_hip_oplog* dst, const crdt_hip_oplog_view* src, uint32_t* added,
                        uint32_t* tombstoned);

/* ---- delta sync: exchange only what the peer lacks ------------------------------------------
 * The Downstream of the reference's Yrs adapter (rope.rs:252-255, :265-268: state_vector() +
 * encode_diff_v1(&sv) + apply_update) for two logs that diverged.  A join ships the other side's
 * whole log; here the receiver sends its state vector, the sender answers with a delta, and the
 * receiver applies it:  dst.apply_diff(src.encode_diff(dst.state_vector())).
 *
 * State vector: for every agent that has at least one item, the largest lamport among its items,
 * sorted by agent ascending.  An item is covered by a vector when its agent has an entry and its
 * lamport is <= that entry's (an agent whose only item has lamport 0 still has an entry; an
 * empty vector covers nothing).
 *
 * Delta (little-endian; n items, r tombstone ranges; 16 + 20 n + 12 r bytes, below 4 GiB):
 *   header    4 x u32: magic 0x44445243 ("CRDD"), version (1 RGA, 2 Fugue), n, r
 *   key[n]    u64  identity lamport << 16 | agent
 *   pkey[n]   u64  the parent's identity, 0xFFFFFFFFFFFFFFFF for the document start
 *   rkey[r]   u64  identity of a range's first item
 *   cp[n]     u32  bits 0-20 codepoint, bit 30 tombstone, bit 31 side (version 2 only)
 *   rcount[r] u32  items of the range, >= 1
 * Items: every item the vector does not cover, in the log's slot order; parents are named by
 * identity because slot numbers mean nothing across logs.  Ranges: every tombstoned item the
 * vector covers (the peer holds it and may not know it is deleted), as maximal runs of consecutive
 * slots that are all tombstoned and covered and whose identities ascend by 1 << 16 (one agent,
 * consecutive lamports; a Fugue item's identity has no side bit).  origin_right is not carried
 * (no merge reads it): appended items get origin_right = NIL, as in a join from a view without
 * that column.
 *
 * Apply: dst <- dst U delta, validated first; a rejected delta changes nothing.  A delta item dst
 * lacks is appended in the delta's order (new id = items of dst + 1 + rank among the new items),
 * its parent looked up by identity in dst or among earlier delta items, side and tombstone kept;
 * one dst holds (a stale vector, a delta sent twice) must agree in codepoint, parent identity and
 * side, and its tombstone is OR-ed in; every identity of every range must be known to dst after
 * the items, and those items become tombstoned.  *added / *tombstoned as for the join (either may
 * be NULL); the same delta applied again gives (0, 0).
 *   CRDT_HIP_EINVAL  bad magic or version; a buffer shorter or longer than its header says; a
 *                    range count of 0; a version-2 delta into an RGA log or replica, or version 1
 *                    into a Fugue one (the kind is the presence of the side column, as for a join)
 *   CRDT_HIP_EBADLOG two delta items share an identity; an identity of 2^48 or more, or reserved
 *                    bits set in a cp word; a parent identity that is unknown or does not precede
 *                    its item in the delta; an item both hold that differs in codepoint, parent or
 *                    side; a range that names an unknown identity (ranges that together name more
 *                    items than dst and the delta hold do); Fugue: lamport 0xFFFFFFFF or a left
 *                    child of the document start
 *   CRDT_HIP_ERANGE  the result would exceed the op-log size limit
 *
 * Precondition: dst.apply_diff(src.encode_diff(dst.state_vector())) leaves dst equal, slot for
 * slot, to dst joined with src (origin_right absent) whenever both logs are per-agent
 * prefix-closed: each holds every item of an agent up to the largest lamport it holds of that
 * agent.  Every log built from local edits, wire updates, joins and deltas is.  A violation that
 * can be seen (a parent that is missing, a range over an unknown item) is CRDT_HIP_EBADLOG with
 * nothing changed; one that cannot (a gap below the vector's entry that no delta item refers to)
 * leaves the gap.
 *
 * Output buffers follow crdt_hip_oplog_encode_from: a NULL or short buffer sets *out_len / *out_n
 * to the need and returns CRDT_HIP_ESPACE.  A vector that is not sorted strictly by agent, or has
 * an agent above 65535, is CRDT_HIP_EINVAL.  The host and the device calls produce the same bytes
 * and the same resulting log.  The host apply marks the resolver index stale and appends newly
 * tombstoned ids to the log's delete ops, as crdt_hip_oplog_join does. */
typedef struct {
    uint32_t agent;
    uint32_t lamport;
} crdt_hip_sv_entry;
int crdt_hip_oplog_state_vector(const crdt_hip_oplog* log, crdt_hip_sv_entry* out, size_t cap,
                                size_t* out_n);
int crdt_hip_oplog_encode_diff(const crdt_hip_oplog* log, const crdt_hip_sv_entry* sv, size_t nsv,
                               uint8_t* buf, size_t cap, size_t* out_len);
int crdt_hip_oplog_apply_diff(crdt_hip_oplog* log, const uint8_t* buf, size_t len,
                              uint32_t* added, uint32_t* tombstoned);

/* ---- patches since a mark: what a sync changed, as positional edits ---------------------------
 * After an update, a join or a delta the log is right, but an editor that keeps a text buffer
 * beside it needs the remote change in the reference's own unit, TestPatch(pos, del, ins) applied
 * as Upstream::replace (rope.rs:21-32).  The resolver turns positions into identities; this turns
 * identities back into positions, on the host (crdt_hip_oplog_*) and in HIP kernels on the device
 * (crdt_hip_replica_*, below), with identical results.
 *
 * A mark remembers a version of one log or one replica: the item count n_mark and, for every item
 * 1..n_mark, whether it was deleted.  Slots are append-only and tombstones are only ever set, so
 * that describes the earlier version in full.
 *
 * Patches since a mark are defined over the current document order of all items held, tombstones
 * included (RGA pre-order or Fugue in-order).  For item s:
 *   was = s <= n_mark and not deleted at the mark;   now = not deleted now.
 * Items that are neither are dropped.  The rest are K = was and now, D = was and not now,
 * I = not was and now (tombstones never clear, so I implies s > n_mark).  A patch is a maximal
 * run of consecutive non-K items of that filtered sequence:
 *   pos = the now items (K or I) before the run, in codepoints;
 *   del = the D items of the run;
 *   ins = the UTF-8 of the run's I items, in order.
 * Patches come out ascending in pos.  Applied in that order, each as replace(pos..pos + del, ins),
 * to the document at the mark, they give the current document.  Hence:
 *   - an item inserted and deleted after the mark appears in no patch;
 *   - a run that interleaves D and I items is one patch (one side deleted a stretch, the other
 *     typed inside it);
 *   - two patches never touch: pos[k + 1] > pos[k] + codepoints(ins[k]);
 *   - nothing changed means zero patches.
 *
 * ins_off / ins_len are bytes into `ins`; ins_off ascends and the pieces are contiguous.  Output
 * buffers follow crdt_hip_oplog_encode_from: a NULL or short `out` or `ins` sets *out_n (patches)
 * and *out_ins (bytes) to the need and returns CRDT_HIP_ESPACE.
 * A mark belongs to the log or replica it was taken from and stays valid across every later
 * update, join, delta and local edit of that owner; several marks may be alive at once; taking or
 * using one changes no log contents (a host call neither reads nor disturbs the resolver index).
 * Free a mark with crdt_hip_mark_free (before the context of a replica mark is destroyed).
 *   CRDT_HIP_EINVAL  a mark of another owner (a clone is another owner); a host mark passed to a
 *                    replica call or the reverse; a replica of another context; an owner with
 *                    fewer items than the mark
 *   CRDT_HIP_ERANGE  2^32 or more patches, or 4 GiB or more of inserted bytes */
typedef struct crdt_hip_mark crdt_hip_mark;
typedef struct {
    uint64_t pos;     /* codepoints before the patch in the current document */
    uint64_t ins_off; /* byte offset of the inserted text in `ins` */
    uint32_t del;     /* codepoints deleted at pos */
    uint32_t ins_len; /* bytes inserted at pos */
} crdt_hip_patch;
int crdt_hip_oplog_mark(const crdt_hip_oplog* log, crdt_hip_mark** out);
void crdt_hip_mark_free(crdt_hip_mark* m);
int crdt_hip_oplog_patches_since(crdt_hip_oplog* log, const crdt_hip_mark* m, crdt_hip_patch* out,
                                 size_t cap, size_t* out_n, uint8_t* ins, size_t ins_cap,
                                 size_t* out_ins);

/* ---- text windows: a range of the document, now or at a mark -----------------------------------
 * An editor paints a viewport, not the document, and every system this project models itself on
 * can read an old version (diamond-types' checkout(version), yrs' snapshots, automerge's
 * text_at(heads)).  One read call takes a version (now, or a mark) and a window and returns that
 * UTF-8 and nothing else, on the host (crdt_hip_oplog_text_at) and in HIP kernels on the device
 * (crdt_hip_replica_text_at), with identical bytes and identical `info`.
 *
 * Everything is defined over the document order of all items held, tombstones included (RGA
 * pre-order or Fugue in-order, as for patches_since and anchors).
 *
 * Versions.  m == NULL is the version now: item s is selected iff it is not tombstoned.  With a
 * mark, s is selected iff s <= n_mark and it was not deleted at the mark.  The version's text is the
 * UTF-8 of the selected items in document order.  Later items never reorder earlier ones, so
 * text_at(mark) is byte for byte the text the owner had when the mark was taken, whatever updates,
 * joins, deltas and local edits came since; and for every mark, applying patches_since(mark) to
 * text_at(mark) gives the text now.
 *
 * Window.  [start, end) of that version, in codepoints, or in UTF-8 bytes with
 * CRDT_HIP_TEXT_BYTES; end == CRDT_HIP_TEXT_END is the version's end.  `info` may be NULL; it
 * reports the whole version and the window in both units, which is a position translation for
 * free.  An empty window, an empty version and an empty log are all ok and give *out_len = 0 (and
 * need no buffer: `out` may then be NULL).
 *
 * Checks, in this order.  On any error but ESPACE, `out`, *out_len and *info are untouched;
 * nothing in the log or the replica ever changes.
 *   1. CRDT_HIP_EINVAL  a mark of another owner (a clone is another owner); a host mark passed to
 *                       the replica call or the reverse; a replica of another context; an owner
 *                       with fewer items than the mark (the patches_since rules)
 *   2. CRDT_HIP_EINVAL  flags other than 0 or CRDT_HIP_TEXT_BYTES; out_len == NULL
 *   3. CRDT_HIP_EINVAL  start > end, when end is not CRDT_HIP_TEXT_END
 *   4. CRDT_HIP_ERANGE  start, or an end that is not CRDT_HIP_TEXT_END, beyond the version's length
 *                       in the unit asked
 *   5. CRDT_HIP_EINVAL  (bytes) a start or end inside a codepoint of that version
 *   6. CRDT_HIP_ERANGE  a window of 4 GiB or more
 *   7. CRDT_HIP_ESPACE  a window of n_bytes > 0 with `out` NULL or cap < n_bytes: *out_len and
 *                       *info are set and `out` is untouched
 *
 * The host call is the definition, not a product path: it takes the order from the log itself per
 * call, O(items), and neither reads nor disturbs the resolver index; a malformed log is
 * CRDT_HIP_EBADLOG.  The device call is the product.  It settles a pending decode and brings the
 * kept document order up to date exactly as crdt_hip_replica_patches_since does (so a call leaves
 * the replica as a merge_inc would), and makes no host copy of the replica's columns.  It counts the
 * selected codepoints and bytes per tile of 4,096 ranks under the version's predicate (the mark's
 * bit plane is never read for a slot above n_mark), scans the tile aggregates in one workgroup
 * (64-bit prefixes), which also finds the tiles of `start` and `end` and walks each, a wave per
 * boundary, to the boundary's codepoints and bytes; the host waits here once, runs checks 4 to 7
 * (ESPACE comes before the write pass) and launches the write pass over the tiles the window
 * overlaps only; the result is copied out in one transfer.  Known cost: a call streams every rank
 * of the replica once, however small the window; after a join or a delta it first pays the full
 * ORDER-mode rebuild. */
#define CRDT_HIP_TEXT_END 0xFFFFFFFFFFFFFFFFull      /* `end`: the end of the version */
enum { CRDT_HIP_TEXT_BYTES = 1 };                    /* flags: start/end count UTF-8 bytes */
typedef struct {
    uint64_t len, len_bytes;      /* the whole version: visible codepoints / UTF-8 bytes */
    uint64_t start, start_bytes;  /* the window's start in both units */
    uint64_t n, n_bytes;          /* the window's codepoints / bytes (n_bytes == *out_len) */
} crdt_hip_text_info;
int crdt_hip_oplog_text_at(crdt_hip_oplog* log, const crdt_hip_mark* m, uint64_t start, uint64_t end,
                           uint32_t flags, uint8_t* out, size_t cap, size_t* out_len,
                           crdt_hip_text_info* info);
int crdt_hip_replica_text_at(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                             uint64_t start, uint64_t end, uint32_t flags, uint8_t* out, size_t cap,
                             size_t* out_len, crdt_hip_text_info* info);
/* What the context's last crdt_hip_replica_text_at observed (each may be NULL): ranks of the
 * document order streamed (the items held), tiles the write pass launched a workgroup for, bytes
 * returned, and the summed device time of the call's own kernels in ns (HIP events; the order
 * update is not included). */
int crdt_hip_text_stats(const crdt_hip_ctx* ctx, uint64_t* ranks, uint64_t* tiles_written,
                        uint64_t* bytes, uint64_t* device_ns);

/* ---- local edits: positional patches into a log or a replica ----------------------------------
 * The inverse of patches_since: a set of positional patches applied as local edits, on the host
 * (crdt_hip_oplog_apply_patches) or, in HIP kernels, to a replica where it lies
 * (crdt_hip_replica_apply_patches), under the replica's own agent (crdt_hip_replica_set_agent,
 * default 0; a clone keeps it).  With it a device replica is a full peer: it edits, syncs and
 * reports, and needs no host twin (`impl Upstream` for the device replica).
 *
 * A patch array reads in the patches_since convention: patch k is
 * replace(pos..pos + del, ins[ins_off, +ins_len)), applied in array order, pos counted in the
 * document as the earlier patches of the array left it.  The result is defined by the host: the
 * log that crdt_hip_oplog_replace, called once per patch in order, produces on a log that holds
 * the same items and has the same local agent, slot for slot: ids (n + 1 ... in patch order, then
 * codepoint order), parents, lamports (largest lamport held + 1, + 2, ...), agent, tombstones and
 * (Fugue) sides.  The device log carries no origin_right, as after a delta.
 *
 * Everything is validated before anything changes, and a rejected call changes nothing; n == 0 is
 * ok and changes nothing.
 *   CRDT_HIP_EINVAL  a patch with del == 0 and ins_len == 0; patches that are not ascending and
 *                    non-touching (the rule is pos[k + 1] > pos[k] + codepoints(ins[k]), what
 *                    patches_since guarantees); a piece [ins_off, ins_off + ins_len) outside
 *                    `ins`; a piece that is not UTF-8 by the rule of crdt_hip_oplog_insert; a
 *                    replica of another context
 *   CRDT_HIP_ERANGE  pos[k] + del[k] beyond the document as the earlier patches left it; an item
 *                    count that would reach the op-log limit; lamports that would reach
 *                    0xFFFFFFFF
 * *added: items appended; *tombstoned: items deleted (either may be NULL).
 *
 * The device call checks the arguments on the host against the visible length the replica tracks,
 * brings the kept document order up to date exactly as crdt_hip_replica_patches_since does, then
 * counts the visible items per tile of 4,096 ranks, scans the tile counts, and resolves: every
 * visible item finds its patch by its visible rank, becomes a patch's left neighbour or one of its
 * deleted items, and one thread per inserted codepoint emits the new item.  The kernels write one
 * wire update in device memory that the replica's own decoder applies, so a call leaves the
 * replica as crdt_hip_replica_apply_updates of that update would; the host waits once before the
 * decode (the largest lamport held and the integrity counts).  No host copy of the replica's
 * columns is made.  Known cost: a call streams every slot and every rank of the replica, even for
 * a single keystroke.
 * crdt_hip_replica_replace is one patch with Upstream::replace's reading (rope.rs:21-32): remove
 * if end > start, insert if nbytes > 0, nothing otherwise. */
int crdt_hip_oplog_apply_patches(crdt_hip_oplog* log, const crdt_hip_patch* p, size_t n,
                                 const uint8_t* ins, size_t ins_len, uint32_t* added,
                                 uint32_t* tombstoned);
int crdt_hip_replica_set_agent(crdt_hip_replica* r, uint16_t agent);
int crdt_hip_replica_apply_patches(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_patch* p,
                                   size_t n, const uint8_t* ins, size_t ins_len, uint32_t* added,
                                   uint32_t* tombstoned);
int crdt_hip_replica_replace(crdt_hip_ctx* ctx, crdt_hip_replica* r, size_t start, size_t end,
                             const char* utf8, size_t nbytes);
/* What the context's last crdt_hip_replica_apply_patches observed (each may be NULL): patches
 * applied, items appended, items tombstoned, ranks of the document order streamed (the items held
 * before the call), and the summed device time of the call's kernels in ns, the decode of the
 * update they write included (HIP events; the order update is not included). */
int crdt_hip_edit_stats(const crdt_hip_ctx* ctx, uint64_t* patches, uint64_t* items,
                        uint64_t* tombstones, uint64_t* ranks, uint64_t* device_ns);

/* ---- byte offsets: the same patches with pos and del in UTF-8 bytes ----------------------------
 * For a caller that keeps its text as UTF-8 (EDITS_USE_BYTE_OFFSETS = true, rope.rs:8,16-19: the
 * cola and yrs adapters; a Rust String, a rope of bytes): the *_bytes twins of the two sections
 * above take and report positions in UTF-8 bytes of the visible document, so no text is kept
 * beside the log or the replica to translate them.  The same crdt_hip_patch struct: pos and del are
 * bytes, ins_off and ins_len were bytes already.  Every codepoint function and its results are
 * unchanged.  crdt_hip_oplog_visible_bytes: the visible UTF-8 bytes of a log (walks the columns;
 * a replica reports them in crdt_hip_replica_info).
 *
 * Local edits, *_apply_patches_bytes.  The array reads in the patches_since convention, in bytes:
 * patch k is replace(pos..pos + del, ins[ins_off, +ins_len)), pos counted in the document as the
 * earlier patches of the array left it.  The result is defined through the codepoint call:
 * translate every patch through the text of the document before the call (codepoint pos = the
 * codepoints in its first pos bytes, codepoint del = the codepoints in the del bytes that follow);
 * the log is then, slot for slot, the log crdt_hip_oplog_apply_patches gives for the translated
 * array.  *added and *tombstoned stay item counts.  Everything is validated before anything
 * changes, and a rejected call changes nothing; n == 0 is ok and changes nothing.  The checks run
 * in array order and, within a patch, in this order:
 *   CRDT_HIP_EINVAL  del == 0 and ins_len == 0
 *   CRDT_HIP_EINVAL  a piece [ins_off, ins_off + ins_len) outside `ins`
 *   CRDT_HIP_EINVAL  a piece that is not UTF-8 by the rule of crdt_hip_oplog_insert
 *   CRDT_HIP_EINVAL  unless pos[k + 1] > pos[k] + ins_len[k]
 *   CRDT_HIP_ERANGE  pos + del beyond the visible bytes, as the earlier patches left them
 *   CRDT_HIP_ERANGE  an item count that would reach the op-log limit
 * then, only when every patch passed them,
 *   CRDT_HIP_EINVAL  a pos or a pos + del that falls inside a codepoint of the document (Rust's
 *                    String::replace_range panics on the same condition)
 * and after that
 *   CRDT_HIP_ERANGE  lamports that would reach 0xFFFFFFFF
 * *_replace_bytes is one patch with Upstream::replace's reading (rope.rs:21-32): remove if
 * end > start, insert if nbytes > 0, nothing otherwise.
 *
 * Patches since a mark, *_patches_since_bytes.  The same runs of D and I items as patches_since:
 * pos = the UTF-8 bytes of the `now` items before the run, del = the UTF-8 bytes of the run's D
 * items; ins, ins_off and ins_len are unchanged.  Applied in order to the UTF-8 of the document at
 * the mark, each as a splice of bytes, the patches give the UTF-8 of the current document, and
 * they never touch: pos[k + 1] > pos[k] + ins_len[k].  CRDT_HIP_ERANGE also when one patch deletes
 * 4 GiB or more (del is a uint32_t and is never truncated).  Everything else is as for
 * patches_since: the mark's owner and lifetime, the ESPACE sizing, and a device call leaves the
 * replica as a merge_inc would.  Host and device return the same array and the same bytes.
 *
 * The host calls are the definition, not a product path: crdt_hip_oplog_apply_patches_bytes takes
 * the document order from the log itself and builds a table of visible byte ends per call, so a
 * call costs O(items) and a keystroke loop O(n^2).  The device calls are the product: patches_since
 * in bytes is the same classification, scan and compaction with UTF-8 lengths as weights (64-bit
 * prefixes over the tiles); apply_patches in bytes adds one streaming pass over the kept order that
 * gives every visible item its byte end, lets it find the patch boundary it is, and builds the
 * codepoint patch table on the device, then resolves, emits and decodes exactly as the codepoint
 * call does.  It waits for the host twice before the decode (the boundary check and the number of
 * deleted items, then the codepoint call's own wait).  crdt_hip_edit_stats and
 * crdt_hip_patch_stats report the byte calls too (the translation kernels included).
 * crdt_hip_trace_resolve keeps refusing a trace that went through chars_to_bytes. */
int crdt_hip_oplog_visible_bytes(const crdt_hip_oplog* log, uint64_t* out);
int crdt_hip_oplog_apply_patches_bytes(crdt_hip_oplog* log, const crdt_hip_patch* p, size_t n,
                                       const uint8_t* ins, size_t ins_len, uint32_t* added,
                                       uint32_t* tombstoned);
int crdt_hip_oplog_replace_bytes(crdt_hip_oplog* log, size_t start, size_t end, const char* utf8,
                                 size_t nbytes);
int crdt_hip_oplog_patches_since_bytes(crdt_hip_oplog* log, const crdt_hip_mark* m,
                                       crdt_hip_patch* out, size_t cap, size_t* out_n, uint8_t* ins,
                                       size_t ins_cap, size_t* out_ins);
int crdt_hip_replica_apply_patches_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_patch* p, size_t n, const uint8_t* ins,
                                         size_t ins_len, uint32_t* added, uint32_t* tombstoned);
int crdt_hip_replica_replace_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r, size_t start, size_t end,
                                   const char* utf8, size_t nbytes);
int crdt_hip_replica_patches_since_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_mark* m, crdt_hip_patch* out, size_t cap,
                                         size_t* out_n, uint8_t* ins, size_t ins_cap,
                                         size_t* out_ins);

/* ---- anchors: cursor and selection positions that survive sync ----------------------------------
 * A cursor, a selection end or a comment range is not an offset but a place in the text: it must
 * keep pointing at the same place while every peer inserts and deletes around it, and mean the same
 * place on every peer (cola's Anchor, yrs' StickyIndex, automerge's cursors).  An anchor names the
 * item next to the gap by its identity, the 48-bit value of the delta layout (key[n] above), with a
 * bias: AFTER is the gap right after the item, BEFORE the gap right before it.  EDGE with AFTER is
 * the document start, EDGE with BEFORE the document end.  An anchor is 16 plain bytes and may be
 * shipped to another peer as it is.
 *
 * Everything is defined over the document order of all items held, tombstones included (RGA
 * pre-order or Fugue in-order, as for patches_since).  len = the visible codepoints.
 *
 * *_anchors_at: gap positions 0 <= p <= len of the current visible document -> anchors.  AFTER
 * names the p-th visible item (p == 0: EDGE), BEFORE the (p + 1)-th (p == len: EDGE).
 * *_anchors_at_bytes reads p in UTF-8 bytes: AFTER names the visible item whose inclusive UTF-8
 * prefix equals p, BEFORE the one whose exclusive prefix equals p, the edges against the visible
 * bytes.  bias == NULL means all AFTER.  Positions come in any order and may repeat.  Everything is
 * validated before `out` is written (on an error it is untouched); n == 0 is ok.  The checks run in
 * array order, per position the bias before the range, then, only when every position passed,
 * the boundary check of the byte reading:
 *   CRDT_HIP_EINVAL  a bias other than 0 or 1
 *   CRDT_HIP_ERANGE  p beyond the document
 *   CRDT_HIP_EINVAL  (bytes) p inside a codepoint
 *
 * *_anchors_resolve: anchors, made here or on any other peer -> where each lies now.  For an anchor
 * on item x: pos = the visible items at ranks strictly before rank(x), plus 1 if the bias is AFTER
 * and x is visible; pos_bytes the same with UTF-8 lengths as weights; state LIVE or DEAD by x's
 * tombstone.  A DEAD anchor lies where its item was, the same place under either bias.
 * EDGE / AFTER gives (0, 0, LIVE), EDGE / BEFORE (len, visible bytes, LIVE).  An identity the log
 * does not hold is no error: it gives (0, 0, UNKNOWN), since a remote cursor may arrive before the
 * update that carries its item, and the caller resolves it again after the next sync.  Anchors
 * come in any order and may repeat.
 *   CRDT_HIP_EINVAL  an id of 2^48 or more that is not EDGE; a bias above 1; pad != 0; a replica of
 *                    another context
 * Hence resolve(anchors_at(p, b)) == p; after an insert of k codepoints at the very gap p an AFTER
 * anchor stays at p and a BEFORE anchor moves to p + k; after the anchored item is deleted the
 * anchor is DEAD at the same pos; and two logs that hold the same items resolve an anchor alike,
 * whatever their slot numbering.
 *
 * The host calls are the definition, not a product path: they take the order from the log itself
 * per call, O(items), and neither read nor disturb the resolver index; a malformed log is
 * CRDT_HIP_EBADLOG.  The device calls are the product, with byte-identical results.  They settle a
 * pending decode and bring the kept document order up to date exactly as
 * crdt_hip_replica_patches_since does (so a call leaves the replica as a merge_inc would), make no
 * host copy of the replica's columns, wait for the host once and change no log contents.  Both
 * count the visible codepoints and UTF-8 bytes per tile of 4,096 ranks and scan the tile aggregates
 * (64-bit byte prefixes).  Resolve then enters the batch's distinct identities into a hash table,
 * probes it with every key of the replica, and per anchor (a wave each) takes the item's rank from
 * the kept inverse order and counts the visible ranks of its tile before it.  Create searches the
 * scanned prefixes for each position's tile and walks that tile, a wave per position, to the item.
 * Known cost: a call streams every rank of the replica once, and for a resolve every key as well,
 * however few the anchors; after a join or a delta it first pays the full ORDER-mode rebuild. */
#define CRDT_HIP_ANCHOR_EDGE 0xFFFFFFFFFFFFFFFFull
enum { CRDT_HIP_ANCHOR_AFTER = 0, CRDT_HIP_ANCHOR_BEFORE = 1 };
enum { CRDT_HIP_ANCHOR_LIVE = 0, CRDT_HIP_ANCHOR_DEAD = 1, CRDT_HIP_ANCHOR_UNKNOWN = 2 };
typedef struct {
    uint64_t id;    /* identity lamport << 16 | agent (no Fugue side bit), or CRDT_HIP_ANCHOR_EDGE */
    uint32_t bias;  /* AFTER: the gap right after the item; BEFORE: the gap right before it */
    uint32_t pad;   /* 0 */
} crdt_hip_anchor;
typedef struct {
    uint64_t pos;        /* codepoints before the anchor in the visible document */
    uint64_t pos_bytes;  /* UTF-8 bytes before it */
    uint32_t state;      /* LIVE, DEAD (the item is tombstoned), UNKNOWN (the log lacks the item) */
    uint32_t pad;        /* 0 */
} crdt_hip_anchor_pos;
int crdt_hip_oplog_anchors_at(crdt_hip_oplog* log, const uint64_t* pos, const uint8_t* bias, size_t n,
                              crdt_hip_anchor* out);
int crdt_hip_oplog_anchors_at_bytes(crdt_hip_oplog* log, const uint64_t* pos, const uint8_t* bias,
                                    size_t n, crdt_hip_anchor* out);
int crdt_hip_oplog_anchors_resolve(crdt_hip_oplog* log, const crdt_hip_anchor* a, size_t n,
                                   crdt_hip_anchor_pos* out);
int crdt_hip_replica_anchors_at(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint64_t* pos,
                                const uint8_t* bias, size_t n, crdt_hip_anchor* out);
int crdt_hip_replica_anchors_at_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint64_t* pos,
                                      const uint8_t* bias, size_t n, crdt_hip_anchor* out);
int crdt_hip_replica_anchors_resolve(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_anchor* a,
                                     size_t n, crdt_hip_anchor_pos* out);
/* What the context's last device anchors call observed (each may be NULL): anchors of the call,
 * those that resolved UNKNOWN (0 for a create), ranks of the document order streamed (the items
 * held), and the summed device time of the call's own kernels in ns (HIP events; the order update
 * is not included). */
int crdt_hip_anchor_stats(const crdt_hip_ctx* ctx, uint64_t* anchors, uint64_t* unknown,
                          uint64_t* ranks, uint64_t* device_ns);

/* ---- formats: rich-text attribute ranges on anchors, flattened into spans ------------------------
 * Bold, a colour, a link: an attribute over a range of the text that must keep covering the same
 * characters while every peer edits, and that converges when peers set and clear it concurrently
 * (Peritext, yrs' Text::format, automerge's marks).  "Mark" already means a version here
 * (crdt_hip_mark), so the ops are called formats and the result spans.  A format is a range
 * between two anchors with a key, a value and the identity of the op that made it.  Formats are
 * not stored in a log or a replica and travel in no update, delta or join: like anchors they are
 * plain bytes (56 each) that the caller ships and unions itself, by `op`.
 *
 * Gaps and coverage.  Everything is defined over the document order of all items held, tombstones
 * included, at ranks 1..N (RGA pre-order or Fugue in-order, as for anchors and patches_since).
 * Gap g (0..N) lies right after the item of rank g: EDGE / AFTER is gap 0, EDGE / BEFORE gap N,
 * item x with AFTER gap rank(x), with BEFORE gap rank(x) - 1.  Format f covers the item of rank k
 * iff gap(f.start) < k <= gap(f.end).  Tombstones play no part in coverage, so two logs that hold
 * the same items agree on it, whatever their slot numbering and whatever was deleted where.  A
 * format with gap(start) >= gap(end) covers nothing, which is no error.  A format with an anchor
 * whose identity the log does not hold is pending: it covers nothing and is counted in *pending,
 * and the caller asks again after the next sync, as for UNKNOWN anchors.
 * The biases are the expansion rule: an end AFTER the last character does not take text typed at
 * the end, an end BEFORE the next character does; mirrored at the start.
 *
 * Attributes and spans.  For a visible item and a key K, of the formats of key K that are not
 * pending and cover it, the one with the largest `op` wins.  If it is a REMOVE, or there is none,
 * the item does not have K; otherwise it has (K, value).  An item's attribute set is these pairs,
 * ascending by key.  A span is a maximal run of consecutive items of the visible document whose
 * sets are equal, key for key and value for value, and not empty: tombstones between two visible
 * items do not break a run, a visible item with an empty set does.  Spans come out ascending in
 * pos and never overlap; their pieces of `attrs` are contiguous, attr_off ascends, and each span's
 * attributes ascend by key.
 *
 * Everything is checked before any output is written: on an error `out`, `attrs` and the counts
 * are untouched and nothing in the log or the replica changes.  The per-format checks run in array
 * order, the duplicate check once they all passed:
 *   CRDT_HIP_ERANGE  more than 65,536 formats
 *   CRDT_HIP_EINVAL  a malformed start or end anchor (as *_anchors_resolve); op >= 2^48; flags
 *                    other than 0 or REMOVE; two formats with the same op (the caller's union by op
 *                    removes duplicates); a replica of another context
 *   CRDT_HIP_ESPACE  `out` or `attrs` NULL or short: *out_n and *out_attrs are set to the need
 *   CRDT_HIP_EBADLOG a malformed log (host); a kept order that disagrees with the replica (device)
 * n == 0 is ok and gives no span; an empty log gives no span and every format on an item identity
 * is pending.
 *
 * The host call is the definition, not a product path: the order comes from the log itself per
 * call, O(items + work over the formats), and the resolver index is neither read nor disturbed.
 * The device call is the product, with byte-identical spans, attrs and pending count.  It settles a
 * pending decode and brings the kept document order up to date as the anchors calls do (so a call
 * leaves the replica as a merge_inc would), makes no host copy of the replica's columns, changes
 * no log contents and waits for the host twice (the sizes, then the result).  It counts the
 * visible codepoints and bytes per tile of 4,096 ranks, finds the anchors' items through a hash
 * table probed by every key, marks the gaps the formats name in a bit plane over the ranks and
 * compacts it into the sorted boundaries, takes each boundary's visible prefix (a wave each), and
 * per segment between two boundaries (a thread each) walks the formats, sorted by (key, op) on the
 * host, for the segment's attribute set; equal neighbours are merged by head flags and a scan.
 * Known cost: a call streams every rank and every key once, however few the formats; the
 * attribute pass is O(segments * formats); after a join or a delta it first pays the full
 * ORDER-mode rebuild. */
enum { CRDT_HIP_FORMAT_REMOVE = 1 };
typedef struct {
    crdt_hip_anchor start, end;  /* the two gaps the range lies between */
    uint64_t op;     /* identity of this format op: lamport << 16 | agent, below 2^48 */
    uint64_t value;  /* opaque payload (a colour, 1 for bold, an index into the caller's table) */
    uint32_t key;    /* attribute name, opaque */
    uint32_t flags;  /* 0, or CRDT_HIP_FORMAT_REMOVE (value is ignored) */
} crdt_hip_format;                      /* 56 bytes */
typedef struct {
    uint64_t pos, pos_bytes;   /* visible codepoints / UTF-8 bytes before the span */
    uint64_t len, len_bytes;   /* visible codepoints / UTF-8 bytes of the span, len >= 1 */
    uint32_t attr_off, attr_n; /* its attributes: attrs[attr_off, +attr_n), attr_n >= 1 */
} crdt_hip_span;                        /* 40 bytes */
typedef struct { uint64_t value; uint32_t key; uint32_t pad; } crdt_hip_span_attr;  /* 16 bytes */
/* f may be NULL when n == 0; out_n, out_attrs and pending must not be NULL. */
int crdt_hip_oplog_spans(crdt_hip_oplog* log, const crdt_hip_format* f, size_t n,
                         crdt_hip_span* out, size_t cap, size_t* out_n,
                         crdt_hip_span_attr* attrs, size_t attr_cap, size_t* out_attrs,
                         size_t* pending);
int crdt_hip_replica_spans(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_format* f,
                           size_t n, crdt_hip_span* out, size_t cap, size_t* out_n,
                           crdt_hip_span_attr* attrs, size_t attr_cap, size_t* out_attrs,
                           size_t* pending);
/* What the context's last device spans call observed (each may be NULL): formats of the call,
 * those pending, segments between two named gaps before equal neighbours were merged, spans,
 * ranks of the document order streamed (the items held), and the summed device time of the call's
 * own kernels in ns (HIP events; the order update is not included). */
int crdt_hip_format_stats(const crdt_hip_ctx* ctx, uint64_t* formats, uint64_t* pending,
                          uint64_t* segments, uint64_t* spans, uint64_t* ranks, uint64_t* device_ns);

/* ---- trace loader (crdt-testdata load_testing_data / chars_to_bytes, main.rs:19-23) ---------- */
int crdt_hip_trace_load(const char* path, crdt_hip_trace** out);
void crdt_hip_trace_free(crdt_hip_trace* t);
/* Number of patches (TestData::len, main.rs:25) / txns. */
size_t crdt_hip_trace_len(const crdt_hip_trace* t);
size_t crdt_hip_trace_txns(const crdt_hip_trace* t);
/* Patch i: codepoint position, deleted codepoints, inserted UTF-8 (borrowed). */
int crdt_hip_trace_patch(const crdt_hip_trace* t, size_t i, size_t* pos, size_t* del,
                         const char** ins, size_t* ins_len);
int crdt_hip_trace_start_content(const crdt_hip_trace* t, const char** s, size_t* len);
int crdt_hip_trace_end_content(const crdt_hip_trace* t, const char** s, size_t* len);
/* Rewrite every patch from codepoint to UTF-8 byte offsets (TestData::chars_to_bytes). */
int crdt_hip_trace_chars_to_bytes(crdt_hip_trace* t);
/* Replay every patch into a fresh op log (the upstream loop body of main.rs:29-34). */
int crdt_hip_trace_resolve(const crdt_hip_trace* t, crdt_hip_oplog** out);
/* The same replay with Fugue anchors (crdt_hip_oplog_set_fugue). */
int crdt_hip_trace_resolve_fugue(const crdt_hip_trace* t, crdt_hip_oplog** out);
/* crdt_hip_trace_resolve of n traces on up to `threads` host threads (0: one per trace, capped
 * by the hardware), documents being independent.  out[i] receives trace
 * i's op log; on an error every out[i] is null and the first error is reported. */
int crdt_hip_trace_resolve_many(const crdt_hip_trace* const* traces, uint32_t n, uint32_t threads,
                                crdt_hip_oplog** out);

/* ---- binary files (skip gunzip + JSON; map resolved logs) ------------
 * Trace cache: the parsed trace in one flat file; crdt_hip_trace_load reads either format
 * (recognised by the file's magic), so a cache is a drop-in for the .json.gz path of
 * load_testing_data (main.rs:19,52).  Op-log file: the resolved anchor log as 64-byte-aligned
 * SoA arrays (a Fugue log's file is version 2 and adds its side column; its view has `side`).
 * Files are written to `path`.tmp and renamed. */
int crdt_hip_trace_save(const crdt_hip_trace* t, const char* path);
int crdt_hip_oplog_save(const crdt_hip_oplog* log, const char* path);
/* An editable op log read from a file (positional edits rebuild the resolver index first). */
int crdt_hip_oplog_load(const char* path, crdt_hip_oplog** out);
/* Map an op-log file read-only: *view points into the mapping (no copy) and stays valid until
 * crdt_hip_logfile_close.  The view can be passed to crdt_hip_merge*, crdt_hip_batch_create and
 * crdt_hip_replica_new. */
int crdt_hip_logfile_open(const char* path, crdt_hip_logfile** out, crdt_hip_oplog_view* view);
int crdt_hip_logfile_close(crdt_hip_logfile* f);

/* ---- synthetic op logs -------------------------------- */
/* 64-agent concurrent interleaved edits; `n_items` inserts, ~20% deletes, splitmix64 seed. */
int crdt_hip_synth_agents(uint32_t n_items, uint32_t agents, uint64_t seed, crdt_hip_oplog** out);
/* single document: parent of item i is i-1 with probability p_chain_pct/100, else uniform in
 * [0, i-1]; deleted ~ Bernoulli(del_pct/100); cp = 'a' + h % 26; lamport = i; agent = i % 64. */
int crdt_hip_synth_tree(uint32_t n_items, uint32_t p_chain_pct, uint32_t del_pct, uint64_t seed,
                        crdt_hip_oplog** out);
/* Visible items (= merged bytes) of that log, counted without building it. */
int crdt_hip_synth_tree_visible(uint32_t n_items, uint32_t del_pct, uint64_t seed, uint64_t* out);

/* ---- merge (device) --------------------------------------------------------------------- */
/* Merge one op log to its document: UTF-8 into out[0..cap), byte length in *out_len, tree
 * digest in *digest (either may be NULL).  If out is NULL only length/digest are produced. */
int crdt_hip_merge(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* log, uint8_t* out, size_t cap,
                   size_t* out_len, uint64_t* digest);
/* Upstream::len (rope.rs:16-19, 133-136) without copying the document back: merge one op log on
 * the device and return the merged text's codepoints (counted on the device from the merged
 * bytes), its UTF-8 length and its tree digest (each may be NULL). */
int crdt_hip_merge_len(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* log, uint64_t* codepoints,
                       uint64_t* bytes, uint64_t* digest);
/* Merge n independent op logs; digests[i], lens[i] per log.  stats may be NULL. */
int crdt_hip_merge_batch(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* logs, uint32_t n,
                         uint64_t* digests, uint64_t* lens, crdt_hip_stats* stats);
/* Pre-order of every item (tombstones included), ids 1..n, into order[0..n) (test hook for
 * the Euler-tour + list-ranking kernels). */
int crdt_hip_merge_order(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* log, uint32_t* order);

/* ---- device-resident replica batches (bench config 3) ------------------------------------- */
/* Upload `nbases` base logs once, then materialise `replicas` independent HBM copies of each
 * (document r uses base r % nbases).  relabel: 0 = ids kept, 1 = per-replica rotation of item
 * ids (locality kept), 2 = per-replica pseudo-random permutation of item ids (seeded by seed
 * and the replica index).  Parents are relabelled; lamport/agent kept, so every replica of a
 * base must merge to the base's document. */
int crdt_hip_batch_create(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* bases, uint32_t nbases,
                          uint32_t replicas, uint32_t relabel, uint64_t seed,
                          crdt_hip_batch** out);
/* A one-document batch generated on the device: crdt_hip_synth_tree's log (same parameters,
 * same items) without a host copy, for the 1 G-item config. */
int crdt_hip_batch_synth_tree(crdt_hip_ctx* ctx, uint32_t n_items, uint32_t p_chain_pct,
                              uint32_t del_pct, uint64_t seed, crdt_hip_batch** out);
int crdt_hip_batch_free(crdt_hip_batch* b);
int crdt_hip_batch_info(const crdt_hip_batch* b, uint64_t* docs, uint64_t* items,
                        uint64_t* device_bytes);
/* Merge every document of the batch (resident inputs); digests/lens sized to docs (may be
 * NULL). */
int crdt_hip_batch_merge(crdt_hip_ctx* ctx, crdt_hip_batch* b, uint64_t* digests,
                         uint64_t* lens, crdt_hip_stats* stats);
/* Raw SoA mode of a resident RGA batch (the companion line that prices the input encoding): keep
 * the reference-shaped columns (lamport u32, agent u16, deleted u8, codepoint u32 per item, beside
 * the parent column) and derive the engine's input format from them on the device at every
 * crdt_hip_batch_merge: the sibling key, the 3-byte codepoint word with its tombstone and
 * previous-slot flags, and the compact list of the items without that flag (stage
 * CRDT_HIP_STAGE_ENCODE).  on = 0 leaves the mode (the columns are kept until the batch is freed).
 * Replaces no reference interface: the reference's op log is its own in-memory format
 * (rope.rs:116-130 builds it). */
int crdt_hip_batch_raw(crdt_hip_ctx* ctx, crdt_hip_batch* b, int on);

/* ---- device-resident replicas: Downstream on the device ------------------------------------
 * A replica is an op log resident in HBM that receives encoded updates and is merged where it
 * lies.  Replaces diamond-types' decode_and_add (Dt Downstream, rope.rs:222-224) for the
 * downstream bench group (main.rs:63-69: clone the initial CRDT, apply every update, len()).
 * Updates are in the wire format of crdt_hip_oplog_encode_from; they are decoded on the device,
 * a whole batch per call, with crdt_hip_oplog_apply_update's semantics (ids already known are
 * skipped; an update must be causally ready: its first id <= known ids + 1).  Unlike the
 * host decoder, a batch that fails validation changes nothing.  A replica belongs to the
 * context that created it. */
/* New replica holding `init` (NULL: empty, = Downstream's from_str("")). */
int crdt_hip_replica_new(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* init,
                         crdt_hip_replica** out);
/* Device-to-device copy (Downstream: Clone, main.rs:64). */
int crdt_hip_replica_clone(crdt_hip_ctx* ctx, const crdt_hip_replica* src,
                           crdt_hip_replica** out);
int crdt_hip_replica_free(crdt_hip_replica* r);
/* Apply updates i = 0..n-1, update i = buf[offsets[i], offsets[i+1]) (n + 1 offsets, each a
 * multiple of 4, offsets[n] <= len < 4 GiB), in order (apply_update, rope.rs:222-224).
 * Same validation as crdt_hip_oplog_apply_update, with one documented difference: the device
 * replica keeps tombstone bits, not the host log's ordered list of delete ops (which
 * encode_from re-sends by index), so it does not refuse an update whose first delete index lies
 * beyond the deletes it has seen ("missing deletes" on the host).  Tombstoning a known item is
 * order-free, so the documents agree once both have every update
 * (tests/test_gpu_replica.py::test_gap_in_deletes_host_rejects_device_accepts). */
int crdt_hip_replica_apply_updates(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint8_t* buf,
                                   size_t len, const uint64_t* offsets, uint32_t n);
/* A batch of encoded updates (layout as crdt_hip_replica_apply_updates) uploaded to HBM once:
 * Downstream's `updates` vector held on the device (main.rs:58), so that applying it to a fresh
 * clone every iteration (main.rs:64-67) moves no bytes over PCIe. */
int crdt_hip_updates_upload(crdt_hip_ctx* ctx, const uint8_t* buf, size_t len,
                            const uint64_t* offsets, uint32_t n, crdt_hip_updates** out);
int crdt_hip_updates_free(crdt_hip_updates* u);
/* crdt_hip_replica_apply_updates with a resident batch (same semantics and validation). */
int crdt_hip_replica_apply_resident(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                    const crdt_hip_updates* u);
/* crdt_hip_oplog_join on the device (rope.rs:234-236): dst <- dst U src by item identity, both
 * replicas of `ctx` (another context's: CRDT_HIP_EINVAL), with the same semantics, validation and
 * error codes, and the same resulting log slot for slot.  Runs in HIP kernels on the context's
 * stream; no host copy of either log is made.  The forks' common prefix (equal keys slot by slot)
 * maps to itself; only the slots past it go through an identity hash table.  src is unchanged.
 * Two RGA replicas or two Fugue replicas (crdt_hip_replica_new from a Fugue log's view, empty or
 * not); a mixed pair is CRDT_HIP_EINVAL.  A Fugue item's identity is its key without the side
 * bit; an appended item keeps its side, an item both hold must have the same side in each.
 * After a join the next crdt_hip_replica_merge_inc of dst merges in full (*path == 0). */
int crdt_hip_replica_join(crdt_hip_ctx* ctx, crdt_hip_replica* dst,
                          const crdt_hip_replica* src, uint32_t* added, uint32_t* tombstoned);
/* What the context's last crdt_hip_replica_join observed (each may be NULL): slots of the common
 * prefix, dst slots entered into the identity table, the table's capacity, and the summed device
 * time of the join's kernels in ns (HIP events). */
int crdt_hip_join_stats(const crdt_hip_ctx* ctx, uint64_t* prefix_slots, uint64_t* table_slots,
                        uint64_t* table_capacity, uint64_t* device_ns);
/* Delta sync on the device (see "delta sync" above): crdt_hip_oplog_state_vector / encode_diff /
 * apply_diff for a replica of `ctx` (another context's: CRDT_HIP_EINVAL), with the same bytes,
 * the same validation and error codes and the same resulting log slot for slot.  HIP kernels on
 * the context's stream; no host copy of the replica's columns is made (encode_diff waits once for
 * the delta's size, then copies its bytes; apply_diff uploads the bytes and waits once).  An apply
 * builds an identity table over every item of dst, so its device work is O(items of dst) however
 * small the delta: what a delta saves is the bytes exchanged.  After an apply_diff the next
 * crdt_hip_replica_merge_inc merges in full (*path == 0), as after a join. */
int crdt_hip_replica_state_vector(crdt_hip_ctx* ctx, const crdt_hip_replica* r,
                                  crdt_hip_sv_entry* out, size_t cap, size_t* out_n);
int crdt_hip_replica_encode_diff(crdt_hip_ctx* ctx, const crdt_hip_replica* r,
                                 const crdt_hip_sv_entry* sv, size_t nsv, uint8_t* buf, size_t cap,
                                 size_t* out_len);
int crdt_hip_replica_apply_diff(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint8_t* buf,
                                size_t len, uint32_t* added, uint32_t* tombstoned);
/* What the context's last device encode_diff or apply_diff observed (each may be NULL): items and
 * tombstone ranges of the delta, dst slots entered into the identity table (apply; 0 for an
 * encode), and the summed device time of the call's kernels in ns (HIP events). */
int crdt_hip_delta_stats(const crdt_hip_ctx* ctx, uint64_t* items, uint64_t* ranges,
                         uint64_t* table_slots, uint64_t* device_ns);
/* Patches since a mark on the device (see "patches since a mark" above): the same patch array and
 * the same `ins` bytes as the host calls, from HIP kernels on the context's stream; no host copy
 * of the replica's columns is made.  crdt_hip_replica_mark settles a pending decode, then packs
 * the tombstone bits of the replica into a device bit plane the mark owns.
 * crdt_hip_replica_patches_since first brings the replica's kept document order up to date exactly
 * as crdt_hip_replica_merge_inc does (the incremental path where it applies, a full ORDER-mode
 * merge otherwise, as after a join or a delta), so a call leaves the replica as a merge_inc would.
 * It then classifies every rank of that order (each workgroup a tile of at most 4,096 consecutive
 * ranks), scans the tile aggregates in one workgroup, waits once for the totals that size the
 * outputs (CRDT_HIP_ESPACE is returned here, before the write pass), and compacts the patches and
 * their text in order.  Known cost: a call streams every rank of the replica however small the
 * change. */
int crdt_hip_replica_mark(crdt_hip_ctx* ctx, crdt_hip_replica* r, crdt_hip_mark** out);
int crdt_hip_replica_patches_since(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                                   crdt_hip_patch* out, size_t cap, size_t* out_n, uint8_t* ins,
                                   size_t ins_cap, size_t* out_ins);
/* What the context's last crdt_hip_replica_patches_since observed (each may be NULL): patches
 * found, their inserted bytes, ranks of the document order streamed (the items held), and the
 * summed device time of the call's own kernels in ns (HIP events; the order update is not
 * included). */
int crdt_hip_patch_stats(const crdt_hip_ctx* ctx, uint64_t* patches, uint64_t* ins_bytes,
                         uint64_t* ranks, uint64_t* device_ns);
/* Items held, visible codepoints (Upstream::len, rope.rs:16-19) and visible UTF-8 bytes. */
int crdt_hip_replica_info(const crdt_hip_replica* r, uint64_t* items,
                          uint64_t* visible_codepoints, uint64_t* visible_bytes);
/* Merge the replica to its document (as crdt_hip_merge: out may be NULL). */
int crdt_hip_replica_merge(crdt_hip_ctx* ctx, crdt_hip_replica* r, uint8_t* out, size_t cap,
                           size_t* out_len, uint64_t* digest);

/* The downstream closure (main.rs:63-69) in one call: a copy of `init` (clone, :64) receives
 * every update of the resident batch `u` (apply_update, :65-67) and is merged (len(), :68).
 * Returns the merged text's codepoints, UTF-8 bytes and tree digest; `init` is unchanged.  The
 * context keeps a work replica per (init, u) and the sizes the last replay produced: the merge
 * is planned with them and enqueued right behind the decode (one host wait for the closure), a
 * device check compares them with the decode's counters, and on a mismatch the replica is merged
 * again with the real sizes.  A batch that fails validation returns EBADLOG. */
int crdt_hip_replica_replay(crdt_hip_ctx* ctx, const crdt_hip_replica* init,
                            const crdt_hip_updates* u, uint64_t* codepoints, uint64_t* bytes,
                            uint64_t* digest);
/* Downstream's len() (main.rs:68 asserts it; rope.rs:135 materialises): merge the replica and
 * return the merged text's codepoints (counted on the device), UTF-8 bytes and tree digest. */
int crdt_hip_replica_merge_len(crdt_hip_ctx* ctx, crdt_hip_replica* r, uint64_t* codepoints,
                               uint64_t* bytes, uint64_t* digest);

/* Incremental len(): the replica keeps its document order and text between
 * calls, and the items appended since the previous call are ranked alone when every one of them
 * with an old parent has a key (lamport, agent) above every older item's (local edits; updates
 * that race no older op), at most 4096 of them; deletes only re-weigh.  Anything else merges in
 * full (engine ORDER mode) and rebuilds the state.  Returns the merged text (out may be NULL),
 * its UTF-8 bytes and codepoints; *path = 1 for the incremental path, 0 for a full merge.
 * Replaces the from-scratch checkout_tip of Dt::len (rope.rs:135) for a caller that asks for the
 * length every K patches (main.rs:35 / :68 with len() inside the loop). */
int crdt_hip_replica_merge_inc(crdt_hip_ctx* ctx, crdt_hip_replica* r, uint8_t* out, size_t cap,
                               size_t* out_len, uint64_t* codepoints, uint32_t* path);

/* ---- multi-GPU (RCCL over xGMI): digest/counter exchange only ----------------------------- */
int crdt_hip_comm_unique_id(uint8_t id[128]);
int crdt_hip_comm_init(crdt_hip_ctx* ctx, int nranks, int rank, const uint8_t id[128]);
/* All-gather `count` u64 from every rank into recv[nranks * count] (rank-major). */
int crdt_hip_allgather_u64(crdt_hip_ctx* ctx, const uint64_t* send, size_t count,
                           uint64_t* recv);
int crdt_hip_comm_destroy(crdt_hip_ctx* ctx);

/* ---- helpers ------------------------------------------------------------------------------ */
uint64_t crdt_hip_xxh64(const void* data, size_t len, uint64_t seed);
uint64_t crdt_hip_tree_digest(const uint8_t* text, size_t len);

#ifdef __cplusplus
}
#endif
#endif
