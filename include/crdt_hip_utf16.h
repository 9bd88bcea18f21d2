/*
 * crdt_hip_utf16.h — UTF-16 positions for libcrdt_hip.so: a gap position translated between
 * codepoints, UTF-8 bytes and UTF-16 code units, and edits and patches in UTF-16 code units, on a
 * host log and in HIP kernels on a device replica.  An extension of crdt_hip.h: it adds nine
 * functions and changes nothing there.
 *
 * A JavaScript string, Monaco, CodeMirror, the Yjs and automerge-js text types and the default
 * `character` of the Language Server Protocol count UTF-16 code units.  Every position crdt_hip.h
 * takes or returns is a codepoint or a UTF-8 byte; with the translation below such a caller uses
 * every call there without a copy of the document, and the edits and patches_since get UTF-16
 * twins as they got *_bytes ones.
 *
 * Everything is defined over the document order of all items held, tombstones included (RGA
 * pre-order or Fugue in-order), as for text_at.  A version is the version now (m == NULL) or a
 * mark, with the selection rule of text_at ("text windows", crdt_hip.h).
 *
 * Weight.  A selected item weighs 2 UTF-16 code units if its codepoint is U+10000 or above, else
 * 1: 1 + (its UTF-8 length == 4).  The rule is by value alone: a log built from raw arrays that
 * holds a codepoint in U+D800..DFFF weighs it 1.
 *
 * Units.  CRDT_HIP_UNIT_CODEPOINTS (0) and CRDT_HIP_UNIT_BYTES (1) have the values of the text_at
 * flags; CRDT_HIP_UNIT_UTF16 is 2.
 *
 * crdt_hip_*_units_of takes n gap positions in `unit`, in any order, repeats allowed, and writes
 * for each the same gap in all three units; *info gets the version's length in all three.  `info`
 * may be NULL.  n == 0 is ok and writes only `info`.  Nothing in the log or the replica changes.
 *
 * Checks, in this order.  On any error `out` and *info are untouched.
 *   1. CRDT_HIP_EINVAL  the mark rules of patches_since and text_at: a mark of another owner, a
 *                       host mark passed to a replica call or the reverse, a replica of another
 *                       context, an owner with fewer items than the mark
 *   2. CRDT_HIP_EINVAL  a unit other than 0, 1 or 2; n > 0 with a NULL `pos` or a NULL `out`;
 *      CRDT_HIP_ERANGE  then n of 2^31 or more (as for crdt_hip_replica_anchors_at)
 *   3. CRDT_HIP_ERANGE  a position beyond the version's length in the unit asked
 *   4. CRDT_HIP_EINVAL  a byte position inside a codepoint, or a UTF-16 position between the two
 *                       code units of one item; checked only when every position passed check 3
 *
 * Local edits, *_apply_patches_utf16 and *_replace_utf16.  The arguments of the *_bytes twins
 * (crdt_hip.h, "byte offsets"); pos and del count UTF-16 code units of the visible document, `ins`
 * stays UTF-8.  The result is defined through the codepoint call: translate every patch through
 * the text of the document before the call; the log is then, slot for slot, the log
 * crdt_hip_oplog_apply_patches gives for the translated array.  Everything is validated before
 * anything changes, and a rejected call changes nothing; n == 0 is ok and changes nothing.  The
 * checks run in array order and, within a patch, in this order:
 *   CRDT_HIP_EINVAL  del == 0 and ins_len == 0
 *   CRDT_HIP_EINVAL  a piece [ins_off, ins_off + ins_len) outside `ins`
 *   CRDT_HIP_EINVAL  a piece that is not UTF-8 by the rule of crdt_hip_oplog_insert
 *   CRDT_HIP_EINVAL  unless pos[k + 1] > pos[k] + the UTF-16 code units of ins[k]
 *   CRDT_HIP_ERANGE  pos + del beyond the visible UTF-16 code units, as the earlier patches left
 *                    them
 * then, only when every patch passed them,
 *   CRDT_HIP_EINVAL  a pos or a pos + del between the two code units of one item
 * and after that, as the codepoint call states them,
 *   CRDT_HIP_ERANGE  an item count that would reach the op-log limit; lamports that would reach
 *                    0xFFFFFFFF
 *
 * Patches since a mark, *_patches_since_utf16.  The arguments and the ESPACE convention of
 * *_patches_since_bytes.  The same runs of D and I items as patches_since, so the same number of
 * patches and the same ins, ins_off and ins_len (UTF-8); pos = the UTF-16 code units of the `now`
 * items before the run, del = those of the run's D items.  Spliced in order into the UTF-16 of the
 * document at the mark, the patches give the UTF-16 of the current document.  CRDT_HIP_ERANGE also
 * when one patch's del reaches 2^32.
 *
 * The host calls are the definition, not a product path: one walk of the log's own document order
 * per call, O(items + n log items).  The device calls are the product (utf16.hip):
 * crdt_hip_replica_units_of settles a pending decode and brings the kept document order up to date
 * as crdt_hip_replica_text_at does (a call leaves the replica as a merge_inc would), counts the
 * selected codepoints, bytes and UTF-16 code units per tile of 4,096 ranks, scans the three
 * aggregates in one workgroup, and answers each position with one wave: a binary search of the
 * tile prefixes and a walk of one tile.  The host waits once and copies the n records out in one
 * transfer; it makes no copy of the replica's columns.  The device *_utf16 edits and patches are
 * compositions inside the library: one such translation of the patches' boundaries, and the
 * codepoint call untouched.  Each pays one more pass over the order and one more host wait than
 * its codepoint call.  Known cost: a call streams every rank of the replica once, however few the
 * positions; after a join or a delta it first pays the full ORDER-mode rebuild.
 */
#ifndef CRDT_HIP_UTF16_H
#define CRDT_HIP_UTF16_H

#include "crdt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CRDT_HIP_UNIT_CODEPOINTS = 0, CRDT_HIP_UNIT_BYTES = 1, CRDT_HIP_UNIT_UTF16 = 2 };

typedef struct {
    uint64_t cp, bytes, utf16;  /* one gap: the selected codepoints, UTF-8 bytes and UTF-16 code units before it */
} crdt_hip_unit_pos;            /* 24 bytes */

typedef struct {
    uint64_t len, len_bytes, len_utf16;  /* of the whole version */
} crdt_hip_unit_info;

int crdt_hip_oplog_units_of(crdt_hip_oplog* log, const crdt_hip_mark* m, const uint64_t* pos, size_t n,
                            uint32_t unit, crdt_hip_unit_pos* out, crdt_hip_unit_info* info);
int crdt_hip_replica_units_of(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                              const uint64_t* pos, size_t n, uint32_t unit, crdt_hip_unit_pos* out,
                              crdt_hip_unit_info* info);

int crdt_hip_oplog_apply_patches_utf16(crdt_hip_oplog* log, const crdt_hip_patch* p, size_t n,
                                       const uint8_t* ins, size_t ins_len, uint32_t* added,
                                       uint32_t* tombstoned);
int crdt_hip_oplog_replace_utf16(crdt_hip_oplog* log, size_t start, size_t end, const char* utf8,
                                 size_t nbytes);
int crdt_hip_oplog_patches_since_utf16(crdt_hip_oplog* log, const crdt_hip_mark* m,
                                       crdt_hip_patch* out, size_t cap, size_t* out_n, uint8_t* ins,
                                       size_t ins_cap, size_t* out_ins);
int crdt_hip_replica_apply_patches_utf16(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_patch* p, size_t n, const uint8_t* ins,
                                         size_t ins_len, uint32_t* added, uint32_t* tombstoned);
int crdt_hip_replica_replace_utf16(crdt_hip_ctx* ctx, crdt_hip_replica* r, size_t start, size_t end,
                                   const char* utf8, size_t nbytes);
int crdt_hip_replica_patches_since_utf16(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_mark* m, crdt_hip_patch* out, size_t cap,
                                         size_t* out_n, uint8_t* ins, size_t ins_cap,
                                         size_t* out_ins);
/* What the context's last device translation observed, one made inside a *_utf16 call included
 * (each may be NULL): positions of the call, ranks of the document order streamed (the items
 * held), and the summed device time of the translation's own kernels in ns (HIP events; the order
 * update is not included). */
int crdt_hip_unit_stats(const crdt_hip_ctx* ctx, uint64_t* queries, uint64_t* ranks,
                        uint64_t* device_ns);

#ifdef __cplusplus
}
#endif
#endif
