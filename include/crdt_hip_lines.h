/*
 * crdt_hip_lines.h — the line index of libcrdt_hip.so: line numbers -> line starts, and positions
 * -> (line, column), on a host log and in HIP kernels on a device replica.  An extension of
 * crdt_hip.h: it adds five functions and changes nothing there.
 *
 * An editor knows lines: it paints lines 4,100 to 4,160, a language server reports (line, column),
 * "go to line" is a line number.  crdt_hip_*_text_at takes a window in codepoints or UTF-8 bytes;
 * these calls supply the translation without a copy of the document (ropey's and crop's
 * line_of_byte / byte_of_line, the ropes under diamond-types).
 *
 * Everything is defined over the document order of all items held, tombstones included (RGA
 * pre-order or Fugue in-order), as for text_at.  A version is the version now (m == NULL) or a
 * mark, with the selection rule of text_at ("text windows", crdt_hip.h); its text is T.
 *
 * Line breaks.  A line break is a selected item whose codepoint is U+000A, and nothing else: CR,
 * U+2028 and the rest are ordinary characters.
 *
 * Lines.  With L selected line breaks the version has lines = L + 1 lines; the empty version has
 * one, "a\n" has two, the last one empty.  Line k (0-based, 0 <= k <= L) starts right after the
 * k-th line break, line 0 at position 0.  Line k ends, its own line break included, where line
 * k + 1 starts; the last line ends at the end of the version.
 *
 * crdt_hip_*_line_starts turns line numbers into line starts.  A line number may be any k in
 * [0, L + 1]; k == L + 1 is the end of the version (start = len, start_bytes = len_bytes,
 * line = L + 1), so [start(k), start(k + 1)) is always the extent of line k.  Numbers come in any
 * order and may repeat.  col and col_bytes are 0.
 *
 * crdt_hip_*_lines_of turns gap positions 0 <= p <= len into lines and columns; with
 * CRDT_HIP_TEXT_BYTES (crdt_hip.h; no other flag exists) positions are UTF-8 bytes.  `line` is the
 * number of selected line breaks among the items before the gap: the gap right after a '\n' is
 * column 0 of the next line, the gap right before it belongs to the line it ends.  start and
 * start_bytes are the start of that line, col and col_bytes the distance from it, so start + col
 * and start_bytes + col_bytes are the position in both units.
 *
 * `info` may be NULL.  n == 0 is ok and writes only `info`.  Nothing in the log or the replica
 * changes.
 *
 * Checks, in this order.  On any error `out` and *info are untouched.
 *   1. CRDT_HIP_EINVAL  the mark rules of patches_since and text_at: a mark of another owner, a
 *                       host mark passed to a replica call or the reverse, a replica of another
 *                       context, an owner with fewer items than the mark
 *   2. CRDT_HIP_EINVAL  flags other than 0 or CRDT_HIP_TEXT_BYTES; n > 0 with a NULL input array
 *                       or a NULL `out`
 *   3. CRDT_HIP_ERANGE  a line number above L + 1, or a position beyond the version's length in
 *                       the unit asked (and, as for crdt_hip_replica_anchors_at, n of 2^31 or more)
 *   4. CRDT_HIP_EINVAL  (bytes) a position inside a codepoint of that version; checked only when
 *                       every position passed check 3
 *
 * The host calls are the definition, not a product path: they take the order from the log itself
 * per call, O(items), and neither read nor disturb the resolver index; a malformed log is
 * CRDT_HIP_EBADLOG.  The device calls are the product (lines.hip): they settle a pending decode
 * and bring the kept document order up to date as crdt_hip_replica_text_at does (a call leaves the
 * replica as a merge_inc would), count the selected codepoints, bytes and line breaks per tile of
 * 4,096 ranks, scan the three aggregates in one workgroup, and answer each query with one wave: a
 * binary search of the tile prefixes and a walk of one tile.  The host waits once and copies the n
 * records out in one transfer; it makes no copy of the replica's columns.  Known cost: a call
 * streams every rank of the replica once, however few the queries; after a join or a delta it
 * first pays the full ORDER-mode rebuild.
 */
#ifndef CRDT_HIP_LINES_H
#define CRDT_HIP_LINES_H

#include "crdt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t line;                /* 0-based line */
    uint64_t start, start_bytes;  /* where that line starts, in codepoints / UTF-8 bytes of the version */
    uint64_t col, col_bytes;      /* the position's distance from the line start, in both units (0 for line_starts) */
} crdt_hip_line_pos;              /* 40 bytes */

typedef struct {
    uint64_t lines, len, len_bytes;  /* of the whole version */
} crdt_hip_line_info;

int crdt_hip_oplog_line_starts(crdt_hip_oplog* log, const crdt_hip_mark* m, const uint64_t* lines,
                               size_t n, crdt_hip_line_pos* out, crdt_hip_line_info* info);
int crdt_hip_oplog_lines_of(crdt_hip_oplog* log, const crdt_hip_mark* m, const uint64_t* pos, size_t n,
                            uint32_t flags, crdt_hip_line_pos* out, crdt_hip_line_info* info);
int crdt_hip_replica_line_starts(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                                 const uint64_t* lines, size_t n, crdt_hip_line_pos* out,
                                 crdt_hip_line_info* info);
int crdt_hip_replica_lines_of(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                              const uint64_t* pos, size_t n, uint32_t flags, crdt_hip_line_pos* out,
                              crdt_hip_line_info* info);
/* What the context's last crdt_hip_replica_line_starts / _lines_of observed (each may be NULL):
 * queries of the call, ranks of the document order streamed (the items held), and the summed
 * device time of the call's own kernels in ns (HIP events; the order update is not included). */
int crdt_hip_line_stats(const crdt_hip_ctx* ctx, uint64_t* queries, uint64_t* ranks,
                        uint64_t* device_ns);

#ifdef __cplusplus
}
#endif
#endif
