// oplog.hpp — host-side resolver: positional patches -> anchor op log (SoA).
//
// Replaces the positional half of diamond-types' OpLog::add_insert / add_delete_without_content
// (called from the Dt adapter, /root/reference/src/rope.rs:116-131).  Conventions (SURVEY.md
// §4.2): an insert at visible codepoint position p is anchored to the p-th visible item
// (origin_left; id 0 = document start) and placed immediately after it, before any tombstones
// that follow it; origin_right = the item that followed origin_left (tombstones included, NIL
// at the end); char k > 0 of a multi-char insert is anchored to char k-1; every deleted
// codepoint is tombstoned exactly once.  lamport = max lamport seen + 1 per item, agent =
// the log's local agent.  With RGA ordering (siblings by (lamport, agent) descending) the
// resolver's sequence equals the merged document order at every step.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace crdt {

struct Patch;  // trace.hpp

// Op-log columns: vectors whose growth leaves new elements default-initialised (uninitialised
// for these integer types) instead of zero-filled: the resolver sizes every column once to the
// trace's bound and writes each item by index (OpLog::replay), so a zero fill would be a second
// pass over the columns.
template <class T>
struct DefaultInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = DefaultInitAlloc<U>;
    };
    DefaultInitAlloc() = default;
    template <class U>
    DefaultInitAlloc(const DefaultInitAlloc<U>&) noexcept {}
    template <class U>
    void construct(U* p) noexcept {
        ::new (static_cast<void*>(p)) U;
    }
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};
template <class T>
using Column = std::vector<T, DefaultInitAlloc<T>>;

// Update wire format (OpLog::encode_from / apply_update, decoded on the device by replica.hip).
constexpr uint32_t kUpdateMagic = 0x55445243u;  // "CRDU"
constexpr uint32_t kUpdateVersion = 1;
// A Fugue log's updates: the same layout, with bit 31 of cp[k] = side[k] (1: left child).
// Only Fugue logs and replicas accept them.
constexpr uint32_t kUpdateVersionFugue = 2;
constexpr uint32_t kUpdateSideBit = 0x80000000u;

// Delta wire format (OpLog::encode_diff / apply_diff, and the kernels of delta.hip), little-endian:
//   header  4 x u32: kDeltaMagic, version (1 RGA, 2 Fugue), n items, r tombstone ranges
//   key[n]  u64  identity lamport << 16 | agent          pkey[n] u64  the parent's identity
//   rkey[r] u64  identity of a range's first item        (kDeltaStart: the document start)
//   cp[n]   u32  bits 0-20 codepoint, bit 30 tombstone, bit 31 side (version 2 only)
//   rcount[r] u32  items of the range (>= 1): identities rkey, rkey + (1 << 16), ...
// 16 + 20 n + 12 r bytes, below 4 GiB.  Items are named by identity: slot numbers mean nothing
// across logs.
constexpr uint32_t kDeltaMagic = 0x44445243u;  // "CRDD"
constexpr uint32_t kDeltaVersion = 1, kDeltaVersionFugue = 2;
constexpr uint64_t kDeltaStart = ~0ull;
constexpr uint32_t kDeltaCpMask = 0x001FFFFFu, kDeltaTombBit = 0x40000000u, kDeltaSideBit = 0x80000000u;
constexpr uint64_t kDeltaKeyEnd = 1ull << 48;  // identities are below it
struct SvEntry {
    uint32_t agent, lamport;
};
// The columns of a delta inside its buffer (byte offsets from its start).
struct DeltaFrame {
    uint32_t version = 0, n = 0, r = 0;
    uint64_t key = 0, pkey = 0, rkey = 0, cp = 0, rcount = 0, bytes = 0;
    uint64_t range_items = 0;  // sum of the range counts
};
// The checks of apply_diff that need no log, shared by the host and the device path: magic,
// version against the log's kind, the exact size, no range count of 0 (CRDT_HIP_EINVAL); ranges
// that name more identities than the log and the delta together can hold name an unknown one
// (CRDT_HIP_EBADLOG).  `held`: items of the destination.
int delta_frame(const uint8_t* buf, size_t len, bool fugue, uint64_t held, DeltaFrame& f,
                std::string& err);

// Patches since a mark (crdt_hip.h, "patches since a mark"; the device twin is patch.hip).
// A mark is a version of one log: its item count and every item's tombstone at that time.
struct LogMark {
    uint32_t n = 0;
    std::vector<uint8_t> deleted;  // n entries
};
// One positional edit, layout of crdt_hip_patch: replace(pos..pos + del, ins[ins_off, +ins_len)).
struct PatchRec {
    uint64_t pos, ins_off;
    uint32_t del, ins_len;
};

// Local edits as positional patches (crdt_hip.h, "local edits"; the device twin is edit.hip).
// What the checks that need no log leave behind, shared by the host and the device path: per patch
// its position in the document before the call (old-document coordinates), the range it deletes,
// and where its codepoints and its deleted ids start in the call's flattened lists.
struct EditPatch {
    uint32_t old_pos;  // visible items before the patch in the document before the call
    uint32_t del;      // items of old visible rank old_pos + 1 .. old_pos + del are deleted
    uint32_t cp0;      // first of its codepoints in EditPlan::cps (new id = items held + 1 + cp0)
    uint32_t ncp;      // codepoints it inserts
    uint32_t del0;     // deleted items of the patches before it
    uint32_t pad;
};
struct EditPlan {
    std::vector<EditPatch> patch;
    std::vector<uint32_t> cps;  // every inserted codepoint, patch after patch
    uint64_t ndel = 0;          // items the call deletes
};
// Validates a patch array against a document of `visible` codepoints and `items` items, in the
// order and with the codes crdt_hip.h states (everything but the lamport bound, which needs the
// log), and fills the plan.  CRDT_HIP_OK, EINVAL or ERANGE with `err` set.
int edit_plan(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len, uint64_t visible,
              uint64_t items, EditPlan& plan, std::string& err);
// The byte-offset reading (crdt_hip.h, "byte offsets"; the device twin is bytes.hip): pos and del
// count UTF-8 bytes of the visible document.  The same checks in the same order, in bytes, against
// `visible_bytes`; what they cannot tell is whether a boundary falls inside a codepoint, which
// needs the document.  Per patch its byte position in the document before the call,
// old_pos_b = pos - sum over the earlier patches of (ins_len - del): the patches do not touch
// there either, old_pos_b[k + 1] > old_pos_b[k] + del_b[k].
struct BytePatch {
    uint64_t old_pos_b;  // visible bytes before the patch in the document before the call
    uint32_t del_b;      // bytes old_pos_b .. old_pos_b + del_b of that document are deleted
    uint32_t cp0, ncp;   // as EditPatch
    uint32_t pad = 0;
};
struct EditPlanBytes {
    std::vector<BytePatch> patch;
    std::vector<uint32_t> cps;
};
int edit_plan_bytes(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                    uint64_t visible_bytes, uint64_t items, EditPlanBytes& plan, std::string& err);

// Text windows (crdt_hip.h, "text windows"; the device twin is text.hip).  Layout of
// crdt_hip_text_info.
constexpr uint64_t kTextEnd = ~0ull;
constexpr uint32_t kTextBytes = 1;
struct TextInfo {
    uint64_t len, len_bytes, start, start_bytes, n, n_bytes;
};
// The checks of a text_at call that need no document, shared by the host and the device path, in
// their order: flags other than 0 or kTextBytes, out_len null, start > end (EINVAL).
int text_check(uint64_t start, uint64_t end, uint32_t flags, const size_t* out_len, std::string& err);
// And those that need the version's lengths and the boundaries, in their order: start or end
// beyond `total` (the version's length in the unit asked; ERANGE), a byte boundary inside a
// codepoint (EINVAL), a window of 4 GiB or more (ERANGE), then ESPACE with *out_len and *info set.
// On success *out_len and *info are set too.  end: already resolved (kTextEnd -> total).
int text_check_window(uint64_t start, uint64_t end, uint64_t total, bool inside, const TextInfo& w,
                      const uint8_t* out, size_t cap, size_t* out_len, TextInfo* info, std::string& err);

// The line index (crdt_hip_lines.h; the device twin is lines.hip).  Layouts of crdt_hip_line_pos
// and crdt_hip_line_info.
constexpr uint32_t kLineBreak = 0x0A;  // the one codepoint that ends a line
struct LinePos {
    uint64_t line, start, start_bytes, col, col_bytes;
};
struct LineInfo {
    uint64_t lines, len, len_bytes;
};
// The checks of a line_starts / lines_of call that need no document, shared by the host and the
// device path, in their order: flags other than 0 or kTextBytes, n > 0 with a null input array or
// a null out (EINVAL); 2^31 or more queries (ERANGE, the bound of anchor_check_at).
int line_check(const uint64_t* in, size_t n, uint32_t flags, const LinePos* out, std::string& err);
// And those that need the version, in their order: `beyond` (a line number above L + 1, or a
// position beyond the version in the unit asked; ERANGE), then `inside` (a byte position inside a
// codepoint; EINVAL).
int line_check_version(bool lines, bool beyond, bool inside, std::string& err);

// UTF-16 positions (crdt_hip_utf16.h; the device twin is utf16.hip).  Layouts of crdt_hip_unit_pos
// and crdt_hip_unit_info; the units have the values of CRDT_HIP_UNIT_*.
constexpr uint32_t kUnitCodepoints = 0, kUnitBytes = 1, kUnitUtf16 = 2;
struct UnitPos {
    uint64_t cp, bytes, utf16;
};
struct UnitInfo {
    uint64_t len, len_bytes, len_utf16;
};
// An item's UTF-16 code units from its UTF-8 length (1..4): by value alone, 2 from U+10000 on.
constexpr uint32_t utf16_units(uint32_t utf8_length) { return 1u + (utf8_length == 4u ? 1u : 0u); }
// The checks of a units_of call that need no document, shared by the host and the device path, in
// their order: a unit other than 0, 1, 2, n > 0 with a null pos or a null out (EINVAL); `bound` or
// more positions (ERANGE; 2^31 at the boundary, the bound of anchor_check_at; the *_utf16 calls
// translate two boundaries per patch of fewer than 2^31 patches).
int unit_check(const uint64_t* pos, size_t n, uint32_t unit, const UnitPos* out, std::string& err,
               uint64_t bound = 1ull << 31);
// And those that need the version, in their order: `beyond` (a position beyond the version in the
// unit asked; ERANGE), then `inside` (a byte position inside a codepoint, a UTF-16 position inside
// a pair; EINVAL).
int unit_check_version(uint32_t unit, bool beyond, bool inside, std::string& err);

// Local edits in UTF-16 code units (crdt_hip_utf16.h), shared by the host and the device path.
// The checks of a patch array that need no document, in array order and with the codes the header
// states: all but the range, which the translation of `bounds` answers.  bounds: per patch that
// passed, the two ends of the range it deletes in UTF-16 code units of the document before the call,
// a = pos - sum over the earlier patches of (ins - del) and a + del; ncp: the codepoints it inserts.
// A refusal is to be reported only if the translation finds none of `bounds` beyond the document
// (the range check of an earlier patch comes first).
struct EditPlanUtf16 {
    std::vector<uint64_t> bounds;
    std::vector<uint32_t> ncp;
};
int edit_plan_utf16(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                    EditPlanUtf16& plan, std::string& err);
// What follows the translation of plan.bounds (rc_units and tr: what units_of answered for them in
// kUnitUtf16; rc_plan and err_plan: what edit_plan_utf16 answered): ERANGE for a range beyond the
// document, then the plan's own refusal, then EINVAL for a boundary inside a pair; otherwise q,
// the n patches in codepoints for apply_patches.
int edit_patches_utf16(const EditPlanUtf16& plan, int rc_plan, const std::string& err_plan, int rc_units,
                       const PatchRec* p, size_t n, const UnitPos* tr, std::vector<PatchRec>& q,
                       std::string& err);
// Patches since a mark in UTF-16 code units, shared the same way.  since_bounds: per codepoint
// patch of patches_since the two ends of what it deletes in codepoints of the mark's version (the
// running shift undone).  since_utf16: with tr, their translation by units_of at the mark, pos and
// del rewritten in place in UTF-16 code units; ERANGE when one patch's del reaches 2^32 (then p is
// unchanged).
void since_bounds(const PatchRec* p, size_t n, const uint8_t* ins, std::vector<uint64_t>& bounds);
int since_utf16(PatchRec* p, size_t n, const uint8_t* ins, const UnitPos* tr, std::string& err);

// Anchors (crdt_hip.h, "anchors"; the device twin is anchor.hip): a place in the text named by the
// identity of the item next to it.  Layouts of crdt_hip_anchor and crdt_hip_anchor_pos.
constexpr uint64_t kAnchorEdge = ~0ull;
constexpr uint32_t kAnchorAfter = 0, kAnchorBefore = 1;
constexpr uint32_t kAnchorLive = 0, kAnchorDead = 1, kAnchorUnknown = 2;
struct AnchorRec {
    uint64_t id;
    uint32_t bias, pad;
};
struct AnchorPosRec {
    uint64_t pos, pos_bytes;
    uint32_t state, pad;
};
// The checks of the two calls that need no document, shared by the host and the device path, in
// array order.  Create: per position a bias above 1 (EINVAL), then a position beyond `visible`
// (codepoints or bytes, as pos counts; ERANGE).  Resolve: an id of 2^48 or more that is not the
// edge, a bias above 1, pad != 0 (EINVAL).
int anchor_check_at(const uint64_t* pos, const uint8_t* bias, size_t n, uint64_t visible,
                    std::string& err);
int anchor_check_resolve(const AnchorRec* a, size_t n, std::string& err);

// Formats (crdt_hip.h, "formats"; the device twin is format.hip): attribute ranges between two
// anchors, flattened into spans.  Layouts of crdt_hip_format, crdt_hip_span, crdt_hip_span_attr.
constexpr uint32_t kFormatRemove = 1;
constexpr size_t kFormatMax = 65536;  // formats of one call
struct FormatRec {
    AnchorRec start, end;
    uint64_t op, value;
    uint32_t key, flags;
};
struct SpanRec {
    uint64_t pos, pos_bytes, len, len_bytes;
    uint32_t attr_off, attr_n;
};
struct SpanAttrRec {
    uint64_t value;
    uint32_t key, pad;
};
// The checks of a spans call that need no document, shared by the host and the device path: more
// than kFormatMax formats (ERANGE); then per format, in array order, a malformed start or end
// anchor (anchor_check_resolve), an op of 2^48 or more, flags other than 0 or REMOVE (EINVAL);
// then, when every format passed, two formats with one op (EINVAL).  On success `sorted` holds the
// indices 0..n-1 ordered by (key, op): within a key the last format that covers an item wins it.
int format_check(const FormatRec* f, size_t n, std::vector<uint32_t>& sorted, std::string& err);

class OpLog {
public:
    // ---- SoA (index k holds item id k+1) ----
    Column<uint32_t> parent, oright, lamport, cp;
    Column<uint16_t> agent;
    Column<uint8_t> deleted;
    Column<uint32_t> del_ops;  // target id of every delete op, in op order
    // Fugue mode (set on an empty log): side[k] = 1 if item k+1 is a LEFT child of parent[k].
    // An insert after left neighbour a (full-list successor b) is a right child of a when a has
    // no right child yet, else a left child of b (the leftmost node of a's right subtree): the
    // resolver's sequence is then the Fugue in-order at every step.  Empty in RGA mode.
    std::vector<uint8_t> side;
    bool fugue = false;
    uint16_t local_agent = 0;
    uint32_t max_lamport = 0;

    OpLog();
    uint32_t size() const { return (uint32_t)parent.size(); }
    // An item's identity, its name in every log that holds it (a Fugue item's side is no part of it).
    uint64_t ident(uint32_t id) const { return ((uint64_t)lamport[id - 1] << 16) | agent[id - 1]; }
    uint64_t visible() const { return nvis_; }
    uint64_t visible_bytes() const;  // UTF-8 bytes of the visible items (walks the columns)

    // Upstream::insert / remove (codepoint offsets).  Return "" or an error message.
    std::string insert(uint64_t pos, const uint32_t* cps, size_t k);
    std::string insert_utf8(uint64_t pos, const char* s, size_t nbytes);
    std::string remove(uint64_t start, uint64_t end);

    // The upstream loop of one editing trace (main.rs:28-36: replace = remove then insert per
    // patch, rope.rs:21-32) as one call: a trace's patches (trace.hpp: pos and del in codepoints),
    // ins the concatenated inserted UTF-8 (ins_total bytes: every patch's text lies inside).
    // RGA logs run a fused loop over columns sized once; Fugue (or stale) logs take insert /
    // remove per patch.  "" or an error message.
    std::string replay(const Patch* patches, size_t n, const char* ins, size_t ins_total);

    // Downstream wire format (see oplog.cpp for the layout).
    uint64_t version() const { return ((uint64_t)size() << 32) | (uint32_t)del_ops.size(); }
    std::vector<uint8_t> encode_from(uint64_t version) const;
    std::string apply_update(const uint8_t* buf, size_t len);

    // State-based merge: this <- this U src by item identity (lamport, agent; a Fugue item's side
    // is an attribute, not part of its name), the reference's
    // `Downstream for Automerge` apply_update(&mut self, other: &Self) = doc.merge(other)
    // (rope.rs:234-236).  Every item of src whose identity this log lacks is
    // appended in src's slot order (new id = size() + 1 + its rank among src's new items) with
    // parent and origin_right translated to this log's ids; an item both hold becomes deleted if
    // either has it deleted (newly tombstoned ids go to del_ops).  Everything is validated first
    // and a rejected join changes nothing.  Returns 0, or a CRDT_HIP_E* code with `err` set:
    // EBADLOG (two items of one log share an identity; an item both hold differs in codepoint,
    // translated parent or side; a parent that does not precede its item; a Fugue src with
    // lamport 0xFFFFFFFF or a left child of the document start), ERANGE (result too large),
    // EINVAL (a Fugue log joined with an RGA log: the kind is the presence of the side column,
    // s_side non-null, never its contents, and both must be of one kind).  Appended Fugue items
    // keep their side.  version() / encode_from keep their local meaning: a joined log ships its
    // later ops to downstream replicas of that log, as before.
    // src arrays as in crdt_hip_oplog_view (origin_right may be null; side null: RGA).
    int join(uint32_t n, const uint32_t* s_parent, const uint32_t* s_oright,
             const uint32_t* s_lamport, const uint16_t* s_agent, const uint8_t* s_deleted,
             const uint32_t* s_cp, const uint8_t* s_side, uint32_t* added, uint32_t* tombstoned,
             std::string& err);

    // State-vector delta sync (crdt_hip.h, "delta sync"): what a peer lacks, by item identity.
    // state_vector: per agent with an item its largest lamport, by agent ascending.
    // encode_diff: the delta against a peer's vector (wire layout at kDeltaMagic), CRDT_HIP_EINVAL
    // for a vector not strictly sorted by agent or with an agent above 65535, ERANGE for a delta
    // of 4 GiB or more.  apply_diff: this <- this U delta, validated first (a rejected delta
    // changes nothing); appended items get origin_right = NIL, newly tombstoned ids go to del_ops
    // and the positional index is marked stale, as by join.
    std::vector<SvEntry> state_vector() const;
    int encode_diff(const SvEntry* sv, size_t nsv, std::vector<uint8_t>& out, std::string& err) const;
    int apply_diff(const uint8_t* buf, size_t len, uint32_t* added, uint32_t* tombstoned,
                   std::string& err);

    // Patches since a mark: what changed in the document between the mark and now, as positional
    // edits in ascending position (the semantics are stated in crdt_hip.h).  The document order
    // comes from the log itself (document_order), never from the positional index, which a call
    // neither reads nor touches.  CRDT_HIP_EINVAL when the log holds fewer items than the mark,
    // EBADLOG for a malformed log, ERANGE for 4 GiB or more of inserted bytes.
    LogMark mark() const;
    int patches_since(const LogMark& m, std::vector<PatchRec>& out, std::vector<uint8_t>& ins,
                      std::string& err) const;
    // The same runs with pos and del in UTF-8 bytes (crdt_hip.h, "byte offsets"); also ERANGE when
    // one patch deletes 4 GiB or more.
    int patches_since_bytes(const LogMark& m, std::vector<PatchRec>& out, std::vector<uint8_t>& ins,
                            std::string& err) const;
    // A window of a version's text (crdt_hip.h, "text windows"): the version now (m null) or at a
    // mark, [start, end) in codepoints or, with kTextBytes, in UTF-8 bytes (kTextEnd: the version's
    // end).  The definition the device path (text.hip) is held to: the order comes from
    // document_order per call, O(items); the positional index is neither read nor touched.  The
    // checks run in the order crdt_hip.h states, from "fewer items than the mark" on; on any error
    // but ESPACE out, *out_len and *info are untouched.  out_len may be null only to be refused.
    int text_at(const LogMark* m, uint64_t start, uint64_t end, uint32_t flags, uint8_t* out,
                size_t cap, size_t* out_len, TextInfo* info, std::string& err) const;
    // The line index of a version (crdt_hip_lines.h): line numbers 0..L + 1 -> where each line
    // starts, and gap positions (codepoints, or UTF-8 bytes with kTextBytes) -> line, line start
    // and column.  The definition the device path (lines.hip) is held to: the order comes from
    // document_order per call, O(items); the positional index is neither read nor touched.  The
    // checks run in the order crdt_hip_lines.h states, from "fewer items than the mark" on; on any
    // error out and *info are untouched.  info may be null; n == 0 writes only *info.
    int line_starts(const LogMark* m, const uint64_t* lines, size_t n, LinePos* out, LineInfo* info,
                    std::string& err) const;
    int lines_of(const LogMark* m, const uint64_t* pos, size_t n, uint32_t flags, LinePos* out,
                 LineInfo* info, std::string& err) const;
    // Local edits as a set of positional patches in the patches_since convention (crdt_hip.h,
    // "local edits"): validated up front (edit_plan, then the lamport bound and the positional
    // index), and a rejected call changes nothing; then remove + insert per patch, in order, which
    // is the definition the device path (edit.hip) is held to.  *added: items appended,
    // *tombstoned: items deleted (either may be null).
    int apply_patches(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                      uint32_t* added, uint32_t* tombstoned, std::string& err);
    // The same with pos and del in UTF-8 bytes: edit_plan_bytes, then every boundary is translated
    // to a codepoint rank through the visible byte ends of document_order (a boundary inside a
    // codepoint: EINVAL) and the translated array goes to apply_patches.  The definition the device
    // path is held to, not a product path: a call walks the whole document.
    int apply_patches_bytes(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                            uint32_t* added, uint32_t* tombstoned, std::string& err);
    // UTF-16 positions (crdt_hip_utf16.h).  units_of: n gap positions of a version in `unit` ->
    // the same gaps in codepoints, UTF-8 bytes and UTF-16 code units, by one walk of
    // document_order under the version's selector, O(items + n log items); the positional index is
    // neither read nor touched.  The definition the device path (utf16.hip) is held to.  The checks
    // run in the order crdt_hip_utf16.h states, from "fewer items than the mark" on (`bound`:
    // unit_check's); on any error out and *info are untouched.  apply_patches_utf16 and
    // patches_since_utf16 are built on it: edit_plan_utf16, the translation of the boundaries,
    // edit_patches_utf16 and apply_patches; patches_since, since_bounds, the translation at the
    // mark and since_utf16.
    int units_of(const LogMark* m, const uint64_t* pos, size_t n, uint32_t unit, UnitPos* out,
                 UnitInfo* info, std::string& err, uint64_t bound = 1ull << 31) const;
    int apply_patches_utf16(const PatchRec* p, size_t n, const uint8_t* ins, size_t ins_len,
                            uint32_t* added, uint32_t* tombstoned, std::string& err);
    int patches_since_utf16(const LogMark& m, std::vector<PatchRec>& out, std::vector<uint8_t>& ins,
                            std::string& err) const;
    // Anchors (crdt_hip.h, "anchors"): gap positions of the visible document -> identity-based
    // anchors (pos in codepoints, or with `bytes` in UTF-8 bytes; bias null: all AFTER), and
    // anchors -> where each lies now.  The definition the device path (anchor.hip) is held to: the
    // order comes from document_order per call, O(items); the positional index is neither read nor
    // touched.  Everything is validated before `out` is written.  EINVAL, ERANGE as crdt_hip.h
    // states, EBADLOG for a malformed log.
    int anchors_at(const uint64_t* pos, const uint8_t* bias, size_t n, bool bytes, AnchorRec* out,
                   std::string& err) const;
    int anchors_resolve(const AnchorRec* a, size_t n, AnchorPosRec* out, std::string& err) const;
    // Formats (crdt_hip.h, "formats"): attribute ranges on anchors -> the non-overlapping spans of
    // the visible document with their attribute sets, and the formats whose anchors name an item
    // the log does not hold.  The definition the device path (format.hip) is held to: the order
    // comes from document_order per call, O(items + segments * formats); the positional index is
    // neither read nor touched.  EINVAL, ERANGE as format_check, EBADLOG for a malformed log,
    // ERANGE for 2^32 or more attributes.
    int spans(const FormatRec* f, size_t n, std::vector<SpanRec>& out, std::vector<SpanAttrRec>& attrs,
              uint64_t& pending, std::string& err) const;
    // Every item id in document order, tombstones included (RGA pre-order or Fugue in-order): the
    // sibling sort and walk that rebuild_index / rebuild_index_fugue build their index from.
    std::string document_order(std::vector<uint32_t>& order) const;

    // Append a fully-specified item (synthetic generators / decoding); marks the positional
    // index stale.
    void push_item(uint32_t par, uint32_t orr, uint32_t lam, uint16_t ag, uint8_t del,
                   uint32_t c, uint8_t sd = 0);
    void mark_deleted(uint32_t id);
    // For bulk builders that fill the SoA directly.
    void mark_stale() { stale_ = true; }
    void reset_visible(uint64_t v) { nvis_ = v; }
    void reserve(size_t items, size_t dels = 0);

private:
    int patches_walk(const LogMark& m, bool bytes, std::vector<PatchRec>& out,
                     std::vector<uint8_t>& ins, std::string& err) const;
    // RGA positional index: the visible items in document order as a gap buffer of spans (runs
    // of consecutive ids; typing extends the span before the gap), the gap at the last edit and
    // the visible items before it (gvis_), so an edit next to the previous one moves nothing and a
    // jump moves the spans in between, not the items; and the full-list successor of every item
    // (tombstones included; nxt_[0] = the first item) for origin_right.  Fugue logs use the span
    // index below: an insert there needs to know whether its left neighbour has a right child.
    struct GSpan {
        uint32_t id, len;
    };
    Column<GSpan> gb_;             // gap [g0_, g1_)
    size_t g0_ = 0, g1_ = 0;
    uint64_t gvis_ = 0;            // visible items in gb_[0, g0_)
    Column<uint32_t> nxt_;         // per id 0..n: next item in the full list (NIL: last)
    void gb_move(uint64_t pos);    // the gap at visible position pos (a span split if needed)
    void gb_reserve(size_t k);
    std::string insert_rga(uint64_t pos, const uint32_t* cps, size_t k);
    std::string remove_rga(uint64_t start, uint64_t end);
    std::string rebuild_index_rga(const std::vector<uint32_t>& order);

    // Positional index (Fugue): the document sequence (tombstones included) as spans of consecutive
    // item ids that are also consecutive in document order and share one deleted state, packed
    // into chunks of at most kSpanMax spans with a Fenwick tree over the chunks' visible counts.
    struct Span {
        uint32_t id;  // first item id
        uint32_t n;   // bit 31: deleted; low 31 bits: length
        uint32_t len() const { return n & 0x7FFFFFFFu; }
        bool del() const { return (n >> 31) != 0; }
    };
    struct Chunk {
        std::vector<Span> s;
        uint32_t vis = 0;
    };
    std::vector<Chunk> chunks_;
    // Fenwick tree over chunks_[i].vis; a chunk split shifts every later chunk, so the tree is
    // rebuilt lazily, at the next lookup that misses the hints (not at every split)
    mutable std::vector<int64_t> fen_;
    mutable bool fen_dirty_ = false;
    std::vector<uint32_t> cps_;  // scratch for insert_utf8
    std::vector<uint8_t> hasright_;  // Fugue: item (id) already has a right child
    uint64_t nvis_ = 0;
    // Chunk of the last lookup and the visible items before it.  Edits only change counts at or
    // after the chunk they start in and splits append after it, so the hint stays exact.
    mutable size_t hint_c_ = SIZE_MAX;
    mutable uint64_t hint_base_ = 0;
    // Span of the last lookup inside hint_c_ and the visible items of the chunk before it: edits
    // change spans only at or after it (tombstone spans merging into it count 0), so a lookup at
    // or after it scans on from there.  Dropped when a split moves it to another chunk.
    mutable size_t hint_si_ = SIZE_MAX;
    mutable uint64_t hint_vb_ = 0;
    bool stale_ = false;  // positional index must be rebuilt (after remote items arrived)

    void fen_build() const;
    void fen_add(size_t i, int64_t d);
    size_t fen_find(uint64_t& p) const;  // chunk holding the p-th visible item (p >= 1)
    Chunk new_chunk() const;
    bool split_chunk(size_t c);  // true if chunk c was split in two
    std::string rebuild_index();
    std::string rebuild_index_fugue();
    std::string order_rga(std::vector<uint32_t>& order) const;
    std::string order_fugue(std::vector<uint32_t>& order) const;
    void index_append(uint32_t v);
    // p-th visible item (p >= 1): chunk c, span si, offset off inside the span.
    bool find_visible(uint64_t p, size_t& c, size_t& si, uint32_t& off) const;
    uint32_t first_id_from(size_t c, size_t si) const;  // first item at or after (c, si), or NIL
    size_t delete_in_span(Chunk& ch, size_t si, uint32_t off, uint32_t take);
};

}  // namespace crdt
