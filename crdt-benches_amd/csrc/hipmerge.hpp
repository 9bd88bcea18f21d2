// hipmerge.hpp — C++ mirror of the reference's per-CRDT adapter interface for the GPU engine,
// written against the C ABI only (include/crdt_hip.h), exactly as the Rust `impl Upstream /
// Downstream for HipMerge` in INTEGRATION.md is.
//
//   trait Upstream   /root/reference/src/rope.rs:6-33
//   trait Downstream /root/reference/src/rope.rs:185-191
//   Dt adapter it sits beside: /root/reference/src/rope.rs:105-137, :193-225
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "crdt_hip.h"
#include "crdt_hip_lines.h"
#include "crdt_hip_utf16.h"

namespace hipmerge {

// Panic on error, matching the harness's unwrap/assert style (rope.rs:53, main.rs:35).
inline void check(int rc, const crdt_hip_ctx* ctx, const char* what) {
    if (rc != CRDT_HIP_OK) {
        std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, crdt_hip_last_error(ctx));
        std::abort();
    }
}

// One device context shared by every clone (clones never copy device buffers).
struct Device {
    crdt_hip_ctx* ctx = nullptr;
    explicit Device(int dev) { check(crdt_hip_init(dev, &ctx), nullptr, "crdt_hip_init"); }
    ~Device() { crdt_hip_destroy(ctx); }
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    // The process-wide device, never destroyed: a static destructor would run crdt_hip_destroy
    // after the HIP runtime's own teardown at exit (the process exit releases the device).
    static std::shared_ptr<Device> shared() {
        static std::shared_ptr<Device>* d = new std::shared_ptr<Device>(std::make_shared<Device>(0));
        return *d;
    }
};

// One positional edit, the reference's TestPatch applied as Upstream::replace (rope.rs:21-32):
// replace(pos..pos + del, ins), positions in codepoints.
struct Patch {
    size_t pos, del;
    std::string ins;
};
// A version of one HipMerge or HipDownstream (crdt_hip_mark): valid for the object it was taken
// from (a clone is another owner), across its later edits, updates, joins and deltas.
struct MarkFree {
    void operator()(crdt_hip_mark* m) const { crdt_hip_mark_free(m); }
};
using Mark = std::unique_ptr<crdt_hip_mark, MarkFree>;
// call(out, cap, out_n, ins, ins_cap, out_ins) under the ESPACE convention -> the patches.
// (cap0, ins0: first capacities to try; a device call streams the document order every time)
template <class Call>
std::vector<Patch> patches_get(Call&& call, crdt_hip_ctx* ctx, size_t cap0, size_t ins0) {
    std::vector<crdt_hip_patch> p(cap0);
    std::string text(ins0, '\0');
    size_t n = 0, nb = 0;
    int rc = call(p.data(), p.size(), &n, reinterpret_cast<uint8_t*>(text.data()), text.size(), &nb);
    if (rc == CRDT_HIP_ESPACE) {
        p.resize(n);
        text.resize(nb);
        rc = call(p.data(), p.size(), &n, reinterpret_cast<uint8_t*>(text.data()), text.size(), &nb);
    }
    check(rc, ctx, "patches_since");
    std::vector<Patch> out;
    out.reserve(n);
    for (size_t k = 0; k < n; ++k)
        out.push_back(Patch{(size_t)p[k].pos, p[k].del, text.substr((size_t)p[k].ins_off, p[k].ins_len)});
    return out;
}

// call(start, end, flags, out, cap, out_len, info) under the ESPACE convention -> the window's UTF-8
// (crdt_hip.h, "text windows").  cap0: the first capacity to try (a device call streams the
// document order every time); end == npos is the version's end.
template <class Call>
std::string text_get(Call&& call, crdt_hip_ctx* ctx, size_t start, size_t end, bool bytes, size_t cap0) {
    const uint64_t e = end == std::string::npos ? CRDT_HIP_TEXT_END : (uint64_t)end;
    const uint32_t flags = bytes ? CRDT_HIP_TEXT_BYTES : 0u;
    std::string out(cap0, '\0');
    size_t n = 0;
    int rc = call(start, e, flags, reinterpret_cast<uint8_t*>(out.data()), out.size(), &n, nullptr);
    if (rc == CRDT_HIP_ESPACE) {
        out.resize(n);
        rc = call(start, e, flags, reinterpret_cast<uint8_t*>(out.data()), out.size(), &n, nullptr);
    }
    check(rc, ctx, "text_at");
    out.resize(n);
    return out;
}

// The line index (crdt_hip_lines.h): where lines start, and the line and column of positions.
using LinePos = crdt_hip_line_pos;
// call(queries, n, out, info) -> the n records.  `beyond`: where a query beyond the version
// (CRDT_HIP_ERANGE) is reported instead of being fatal (text_lines clips then).
template <class Call>
std::vector<LinePos> lines_get(Call&& call, crdt_hip_ctx* ctx, const std::vector<uint64_t>& q,
                               crdt_hip_line_info* info = nullptr, bool* beyond = nullptr) {
    std::vector<LinePos> out(q.size());
    const int rc = call(q.data(), q.size(), out.data(), info);
    if (beyond) *beyond = rc == CRDT_HIP_ERANGE;
    if (!(beyond && *beyond)) check(rc, ctx, "lines");
    return out;
}
// Lines first .. first + count of a version as UTF-8, line breaks included, clipped to the version:
// starts(lines, info, beyond) is line_starts, window(start_bytes, end_bytes) the byte window.
template <class Starts, class Window>
std::string text_lines_get(Starts&& starts, Window&& window, size_t first, size_t count) {
    bool beyond = false;
    std::vector<LinePos> s = starts({(uint64_t)first, (uint64_t)first + count}, nullptr, &beyond);
    if (beyond) {
        crdt_hip_line_info info{};
        starts({}, &info, nullptr);
        s = starts({std::min<uint64_t>(first, info.lines), std::min<uint64_t>((uint64_t)first + count, info.lines)},
                   nullptr, nullptr);
    }
    return window((size_t)s[0].start_bytes, (size_t)s[1].start_bytes);
}

// UTF-16 positions (crdt_hip_utf16.h): a gap in codepoints, UTF-8 bytes and UTF-16 code units.
using UnitPos = crdt_hip_unit_pos;
// call(positions, n, out, info) -> the n records.
template <class Call>
std::vector<UnitPos> units_get(Call&& call, crdt_hip_ctx* ctx, const std::vector<uint64_t>& q,
                               crdt_hip_unit_info* info = nullptr) {
    std::vector<UnitPos> out(q.size());
    check(call(q.data(), q.size(), out.data(), info), ctx, "units_of");
    return out;
}

// A cursor, a selection end: a place in the text that survives every edit and sync and means the
// same on every peer (crdt_hip_anchor; 16 plain bytes, shipped as they are).
using Anchor = crdt_hip_anchor;
// Where an anchor lies now (codepoints; HipDownstreamBytes: bytes), or nothing while the item it
// names has not arrived (CRDT_HIP_ANCHOR_UNKNOWN): resolve again after the next sync.
struct AnchorAt {
    bool known;
    size_t pos;
};
inline std::vector<AnchorAt> anchors_known(const std::vector<crdt_hip_anchor_pos>& p, bool bytes) {
    std::vector<AnchorAt> out;
    out.reserve(p.size());
    for (const crdt_hip_anchor_pos& x : p)
        out.push_back(AnchorAt{x.state != CRDT_HIP_ANCHOR_UNKNOWN, (size_t)(bytes ? x.pos_bytes : x.pos)});
    return out;
}

// Rich text (crdt_hip.h, "formats"): attribute ranges between two anchors, last writer wins per key
// by op.  Formats travel beside the text, never in it: an adapter keeps its format ops by op, and
// sync_formats_from is the union of two such maps.
using Format = crdt_hip_format;
enum : unsigned { EXPAND_START = 1, EXPAND_END = 2 };  // text typed at that edge joins the range
// A maximal run of visible text with one attribute set (pos, len in codepoints;
// HipDownstreamBytes: bytes), its attributes ascending by key.
struct Span {
    size_t pos, len;
    std::vector<std::pair<uint32_t, uint64_t>> attrs;
};
struct Spans {
    std::vector<Span> spans;
    size_t pending;  // formats whose anchors name an item that has not arrived: ask again after a sync
};
struct FormatSet {
    std::map<uint64_t, Format> ops;  // by op
    uint64_t clock = 0;              // of this peer's last format
    uint16_t agent = 0;              // the low 16 bits of its ops
    // The next op: the clock passes the largest lamport of the text's state vector and the last format.
    uint64_t next_op(const std::vector<crdt_hip_sv_entry>& sv) {
        for (const crdt_hip_sv_entry& e : sv) clock = std::max<uint64_t>(clock, e.lamport);
        return (++clock << 16) | agent;
    }
    uint64_t add(const Anchor& start, const Anchor& end, uint32_t key, uint64_t value, uint32_t flags,
                 const std::vector<crdt_hip_sv_entry>& sv) {
        const uint64_t op = next_op(sv);
        ops[op] = Format{start, end, op, value, key, flags};
        return op;
    }
    size_t merge(const FormatSet& o) {
        const size_t before = ops.size();
        ops.insert(o.ops.begin(), o.ops.end());
        return ops.size() - before;
    }
    std::vector<Format> list() const {
        std::vector<Format> f;
        f.reserve(ops.size());
        for (const auto& kv : ops) f.push_back(kv.second);
        return f;
    }
};
// call(f, n, out, cap, out_n, attrs, attr_cap, out_attrs, pending) under the ESPACE convention.
template <class Call>
Spans spans_get(Call&& call, const FormatSet& set, crdt_hip_ctx* ctx, bool bytes) {
    const std::vector<Format> f = set.list();
    std::vector<crdt_hip_span> sp;
    std::vector<crdt_hip_span_attr> at;
    size_t n = 0, na = 0, pend = 0;
    int rc = call(f.data(), f.size(), sp.data(), sp.size(), &n, at.data(), at.size(), &na, &pend);
    if (rc == CRDT_HIP_ESPACE) {
        sp.resize(n);
        at.resize(na);
        rc = call(f.data(), f.size(), sp.data(), sp.size(), &n, at.data(), at.size(), &na, &pend);
    }
    check(rc, ctx, "spans");
    Spans out{{}, pend};
    for (size_t k = 0; k < n; ++k) {
        Span s{(size_t)(bytes ? sp[k].pos_bytes : sp[k].pos), (size_t)(bytes ? sp[k].len_bytes : sp[k].len), {}};
        for (uint32_t q = 0; q < sp[k].attr_n; ++q)
            s.attrs.push_back({at[sp[k].attr_off + q].key, at[sp[k].attr_off + q].value});
        out.spans.push_back(std::move(s));
    }
    return out;
}

class HipMerge {
public:
    static constexpr const char* NAME = "mi355x";
    static constexpr bool EDITS_USE_BYTE_OFFSETS = false;
    using Update = std::vector<uint8_t>;

    // Upstream::from_str (rope.rs:113-121: new op log, one insert of the start content);
    // `fugue`: a Fugue log (left/right anchors, in-order document, version-2 updates)
    static HipMerge from_str(std::string_view s, bool fugue = false) {
        HipMerge m;
        if (fugue) check(crdt_hip_oplog_set_fugue(m.log_.get(), 1), nullptr, "set_fugue");
        if (!s.empty()) m.insert(0, s);
        return m;
    }
    void insert(size_t at, std::string_view s) {
        check(crdt_hip_oplog_insert(log_.get(), at, s.data(), s.size()), nullptr, "insert");
    }
    void remove(size_t start, size_t end) {
        check(crdt_hip_oplog_remove(log_.get(), start, end), nullptr, "remove");
    }
    // Upstream::replace default (rope.rs:21-32)
    void replace(size_t start, size_t end, std::string_view s) {
        if (end > start) remove(start, end);
        if (!s.empty()) insert(start, s);
    }
    // Upstream::len: the merge (Dt: checkout_tip().len(), rope.rs:134-136).  Codepoints.
    size_t len() const {
        crdt_hip_oplog_view v;
        check(crdt_hip_oplog_get_view(log_.get(), &v), nullptr, "view");
        uint64_t cps = 0;
        check(crdt_hip_merge_len(dev_->ctx, &v, &cps, nullptr, nullptr), dev_->ctx,
              "crdt_hip_merge_len");
        return (size_t)cps;
    }
    std::string text() const {
        crdt_hip_oplog_view v;
        check(crdt_hip_oplog_get_view(log_.get(), &v), nullptr, "view");
        std::string out((size_t)v.n * 4 + 16, '\0');
        size_t n = 0;
        check(crdt_hip_merge(dev_->ctx, &v, reinterpret_cast<uint8_t*>(out.data()), out.size(), &n,
                             nullptr),
              dev_->ctx, "crdt_hip_merge");
        out.resize(n);
        return out;
    }
    uint64_t digest() const {
        crdt_hip_oplog_view v;
        check(crdt_hip_oplog_get_view(log_.get(), &v), nullptr, "view");
        size_t n = 0;
        uint64_t d = 0;
        check(crdt_hip_merge(dev_->ctx, &v, nullptr, 0, &n, &d), dev_->ctx, "crdt_hip_merge");
        return d;
    }
    // Borrowed SoA view of the host op log (valid until the next mutation).
    crdt_hip_oplog_view view() const {
        crdt_hip_oplog_view v;
        check(crdt_hip_oplog_get_view(log_.get(), &v), nullptr, "view");
        return v;
    }
    const std::shared_ptr<Device>& device() const { return dev_; }
    HipMerge clone() const {
        crdt_hip_oplog* c = nullptr;
        check(crdt_hip_oplog_clone(log_.get(), &c), nullptr, "clone");
        return HipMerge(c, dev_);
    }

    // Downstream::upstream_updates (rope.rs:196-220): replay on an upstream copy, encoding one
    // update per patch from the previous version.
    template <class PatchFn>
    static std::pair<HipMerge, std::vector<Update>> upstream_updates(std::string_view start,
                                                                      size_t npatches,
                                                                      PatchFn&& patch,
                                                                      bool fugue = false) {
        HipMerge up = from_str(start, fugue);
        std::vector<Update> updates;
        updates.reserve(npatches);
        for (size_t i = 0; i < npatches; ++i) {
            size_t pos, del;
            std::string_view ins;
            patch(i, pos, del, ins);
            uint64_t v = crdt_hip_oplog_version(up.log_.get());
            up.replace(pos, pos + del, ins);
            size_t need = 0;
            (void)crdt_hip_oplog_encode_from(up.log_.get(), v, nullptr, 0, &need);
            Update u(need);
            check(crdt_hip_oplog_encode_from(up.log_.get(), v, u.data(), u.size(), &need), nullptr,
                  "encode_from");
            updates.push_back(std::move(u));
        }
        return {from_str(start, fugue), std::move(updates)};
    }
    // Downstream::apply_update (rope.rs:222-224)
    void apply_update(const Update& u) {
        check(crdt_hip_oplog_apply_update(log_.get(), u.data(), u.size()), nullptr, "apply_update");
    }
    // Remember this version of the document; patches_since(mark) then gives what changed since,
    // ascending in pos: what an editor that keeps a text buffer beside this applies to it.
    Mark mark() const {
        crdt_hip_mark* m = nullptr;
        check(crdt_hip_oplog_mark(log_.get(), &m), nullptr, "oplog_mark");
        return Mark(m);
    }
    std::vector<Patch> patches_since(const Mark& m) const {
        return patches_get(
            [&](crdt_hip_patch* out, size_t cap, size_t* n, uint8_t* ins, size_t icap, size_t* nb) {
                return crdt_hip_oplog_patches_since(log_.get(), m.get(), out, cap, n, ins, icap, nb);
            },
            nullptr, 0, 0);
    }
    // Window [start, end) of the document now (what an editor paints), and the document as of a
    // mark, or a window of it: byte for byte what this log held when the mark was taken.
    std::string text_range(size_t start, size_t end = std::string::npos) const {
        return text_window(nullptr, start, end);
    }
    std::string text_at(const Mark& m, size_t start = 0, size_t end = std::string::npos) const {
        return text_window(m.get(), start, end);
    }
    // The line index (crdt_hip_lines.h) of the document now (m null) or as of a mark: where the
    // lines `lines` (0..L + 1, the last one the end) start, the line and column of gap positions,
    // and lines first .. first + count as text, clipped to the version (a viewport by lines).
    std::vector<LinePos> line_starts(const std::vector<uint64_t>& lines, const crdt_hip_mark* m = nullptr) const {
        return line_starts_of(lines, m, nullptr, nullptr);
    }
    std::vector<LinePos> lines_of(const std::vector<uint64_t>& pos, const crdt_hip_mark* m = nullptr) const {
        return lines_get(
            [&](const uint64_t* q, size_t n, LinePos* out, crdt_hip_line_info* info) {
                return crdt_hip_oplog_lines_of(log_.get(), m, q, n, 0, out, info);
            },
            nullptr, pos);
    }
    std::string text_lines(size_t first, size_t count, const crdt_hip_mark* m = nullptr) const {
        return text_lines_get(
            [&](const std::vector<uint64_t>& q, crdt_hip_line_info* info, bool* beyond) {
                return line_starts_of(q, m, info, beyond);
            },
            [&](size_t a, size_t b) { return text_window(m, a, b, true); }, first, count);
    }
    // UTF-16 positions (crdt_hip_utf16.h) for a caller that counts UTF-16 code units (a JavaScript
    // string, LSP's `character`): the gaps `pos`, given in `unit` (CRDT_HIP_UNIT_*), in all three
    // units, now (m null) or as of a mark; an edit and the patches since a mark in code units.
    std::vector<UnitPos> units_of(const std::vector<uint64_t>& pos, uint32_t unit, const crdt_hip_mark* m = nullptr,
                                  crdt_hip_unit_info* info = nullptr) const {
        return units_get(
            [&](const uint64_t* q, size_t n, UnitPos* out, crdt_hip_unit_info* i) {
                return crdt_hip_oplog_units_of(log_.get(), m, q, n, unit, out, i);
            },
            nullptr, pos, info);
    }
    void replace_utf16(size_t start, size_t end, std::string_view s) {
        check(crdt_hip_oplog_replace_utf16(log_.get(), start, end, s.data(), s.size()), nullptr,
              "oplog_replace_utf16");
    }
    std::vector<Patch> patches_since_utf16(const Mark& m) const {
        return patches_get(
            [&](crdt_hip_patch* out, size_t cap, size_t* n, uint8_t* ins, size_t icap, size_t* nb) {
                return crdt_hip_oplog_patches_since_utf16(log_.get(), m.get(), out, cap, n, ins, icap, nb);
            },
            nullptr, 0, 0);
    }
    // The anchor of gap `pos` (bias: CRDT_HIP_ANCHOR_AFTER sticks to the item before the gap,
    // BEFORE to the one after it), and where anchors made here or on any peer lie now.
    Anchor anchor_at(size_t pos, uint32_t bias = CRDT_HIP_ANCHOR_AFTER) const {
        const uint64_t p = pos;
        const uint8_t b = (uint8_t)bias;
        Anchor a;
        check(crdt_hip_oplog_anchors_at(log_.get(), &p, &b, 1, &a), nullptr, "oplog_anchors_at");
        return a;
    }
    std::vector<AnchorAt> resolve_many(const std::vector<Anchor>& a) const {
        std::vector<crdt_hip_anchor_pos> p(a.size());
        check(crdt_hip_oplog_anchors_resolve(log_.get(), a.data(), a.size(), p.data()), nullptr,
              "oplog_anchors_resolve");
        return anchors_known(p, false);
    }
    AnchorAt resolve(const Anchor& a) const { return resolve_many({a})[0]; }
    // Rich text: give the text between the gaps `start` and `end` the attribute (key, value), or
    // take `key` off it; returns the op.  The start anchor is AFTER if EXPAND_START is set, else
    // BEFORE; the end BEFORE if EXPAND_END is set, else AFTER.
    void set_agent(uint16_t agent) {
        check(crdt_hip_oplog_set_agent(log_.get(), agent), nullptr, "set_agent");
        formats_.agent = agent;
    }
    uint64_t format(size_t start, size_t end, uint32_t key, uint64_t value, unsigned expand = 0) {
        return format_op(start, end, key, value, 0, expand);
    }
    uint64_t unformat(size_t start, size_t end, uint32_t key, unsigned expand = 0) {
        return format_op(start, end, key, 0, CRDT_HIP_FORMAT_REMOVE, expand);
    }
    Spans spans() const {
        return spans_get(
            [&](const Format* f, size_t n, crdt_hip_span* out, size_t cap, size_t* on,
                crdt_hip_span_attr* at, size_t acap, size_t* oa, size_t* pend) {
                return crdt_hip_oplog_spans(log_.get(), f, n, out, cap, on, at, acap, oa, pend);
            },
            formats_, nullptr, false);
    }
    const FormatSet& formats() const { return formats_; }
    size_t sync_formats_from(const HipMerge& o) { return formats_.merge(o.formats_); }

private:
    uint64_t format_op(size_t start, size_t end, uint32_t key, uint64_t value, uint32_t flags,
                       unsigned expand) {
        std::vector<crdt_hip_sv_entry> sv(65536);
        size_t n = 0;
        check(crdt_hip_oplog_state_vector(log_.get(), sv.data(), sv.size(), &n), nullptr, "state_vector");
        sv.resize(n);
        return formats_.add(anchor_at(start, expand & EXPAND_START ? CRDT_HIP_ANCHOR_AFTER : CRDT_HIP_ANCHOR_BEFORE),
                            anchor_at(end, expand & EXPAND_END ? CRDT_HIP_ANCHOR_BEFORE : CRDT_HIP_ANCHOR_AFTER),
                            key, value, flags, sv);
    }
    std::string text_window(const crdt_hip_mark* m, size_t start, size_t end, bool bytes = false) const {
        return text_get(
            [&](uint64_t s, uint64_t e, uint32_t flags, uint8_t* out, size_t cap, size_t* n,
                crdt_hip_text_info* info) {
                return crdt_hip_oplog_text_at(log_.get(), m, s, e, flags, out, cap, n, info);
            },
            nullptr, start, end, bytes, 1 << 12);
    }
    std::vector<LinePos> line_starts_of(const std::vector<uint64_t>& lines, const crdt_hip_mark* m,
                                        crdt_hip_line_info* info, bool* beyond) const {
        return lines_get(
            [&](const uint64_t* q, size_t n, LinePos* out, crdt_hip_line_info* i) {
                return crdt_hip_oplog_line_starts(log_.get(), m, q, n, out, i);
            },
            nullptr, lines, info, beyond);
    }
    FormatSet formats_;
    struct Free {
        void operator()(crdt_hip_oplog* l) const { crdt_hip_oplog_free(l); }
    };
    std::unique_ptr<crdt_hip_oplog, Free> log_;
    std::shared_ptr<Device> dev_;

    HipMerge() : dev_(Device::shared()) {
        crdt_hip_oplog* l = nullptr;
        check(crdt_hip_oplog_new(&l), nullptr, "oplog_new");
        log_.reset(l);
    }
    HipMerge(crdt_hip_oplog* l, std::shared_ptr<Device> d) : log_(l), dev_(std::move(d)) {}
};

// Downstream with the replica resident on the device (crdt_hip_replica_*).  apply_update only
// queues the encoded update in a host buffer; len() decodes every queued update on the device in
// one batch (the decode_and_add of rope.rs:222-224 for all of them), merges the replica where it
// lies and returns its visible codepoints.  clone() copies the replica device to device.
class HipDownstream {
public:
    static constexpr const char* NAME = "mi355x-device";
    static constexpr bool EDITS_USE_BYTE_OFFSETS = false;
    using Update = HipMerge::Update;

    template <class PatchFn>
    static std::pair<HipDownstream, std::vector<Update>> upstream_updates(std::string_view start,
                                                                           size_t npatches,
                                                                           PatchFn&& patch,
                                                                           bool fugue = false) {
        auto pr = HipMerge::upstream_updates(start, npatches, patch, fugue);
        crdt_hip_oplog_view v = pr.first.view();
        HipDownstream d(pr.first.device());
        // (a Fugue log's view, empty or not, makes a Fugue replica)
        check(crdt_hip_replica_new(d.dev_->ctx, v.n || v.side ? &v : nullptr, &d.rep_), d.dev_->ctx,
              "replica_new");
        return {std::move(d), std::move(pr.second)};
    }
    HipDownstream(HipDownstream&& o) noexcept
        : formats_(std::move(o.formats_)), dev_(std::move(o.dev_)), rep_(o.rep_), buf_(std::move(o.buf_)),
          off_(std::move(o.off_)) {
        o.rep_ = nullptr;
    }
    HipDownstream(const HipDownstream&) = delete;
    ~HipDownstream() {
        if (rep_) crdt_hip_replica_free(rep_);
    }
    HipDownstream clone() const {  // main.rs:64
        HipDownstream c(dev_);
        check(crdt_hip_replica_clone(dev_->ctx, rep_, &c.rep_), dev_->ctx, "replica_clone");
        c.buf_ = buf_;
        c.off_ = off_;
        return c;
    }
    void apply_update(const Update& u) {  // rope.rs:222-224 (queued)
        buf_.insert(buf_.end(), u.begin(), u.end());
        off_.push_back(buf_.size());
    }
    // Upstream::len (codepoints) of the merged document: counted on the device from the merged
    // bytes, cross-checked against the decoder's counters.
    size_t len() const {
        flush();
        uint64_t mcps = 0, mbytes = 0, items = 0, cps = 0, bytes = 0;
        check(crdt_hip_replica_merge_len(dev_->ctx, rep_, &mcps, &mbytes, nullptr), dev_->ctx,
              "replica_merge_len");
        crdt_hip_replica_info(rep_, &items, &cps, &bytes);
        if (mcps != cps || mbytes != bytes) {
            std::fprintf(stderr, "replica: merged %llu codepoints / %llu bytes, decoder %llu / %llu\n",
                         (unsigned long long)mcps, (unsigned long long)mbytes,
                         (unsigned long long)cps, (unsigned long long)bytes);
            std::abort();
        }
        return (size_t)mcps;
    }
    std::string text() const {
        flush();
        uint64_t items = 0, cps = 0, bytes = 0;
        crdt_hip_replica_info(rep_, &items, &cps, &bytes);
        std::string out((size_t)bytes + 16, '\0');
        size_t n = 0;
        check(crdt_hip_replica_merge(dev_->ctx, rep_, reinterpret_cast<uint8_t*>(out.data()),
                                     out.size(), &n, nullptr),
              dev_->ctx, "replica_merge");
        out.resize(n);
        return out;
    }
    // HipMerge::mark / patches_since on the device (the queued updates are decoded first).
    Mark mark() const {
        flush();
        crdt_hip_mark* m = nullptr;
        check(crdt_hip_replica_mark(dev_->ctx, rep_, &m), dev_->ctx, "replica_mark");
        return Mark(m);
    }
    std::vector<Patch> patches_since(const Mark& m) const {
        flush();
        return patches_get(
            [&](crdt_hip_patch* out, size_t cap, size_t* n, uint8_t* ins, size_t icap, size_t* nb) {
                return crdt_hip_replica_patches_since(dev_->ctx, rep_, m.get(), out, cap, n, ins,
                                                      icap, nb);
            },
            dev_->ctx, 4096, 1 << 16);
    }
    // HipMerge::text_range / text_at on the device (the queued updates are decoded first): only the
    // window comes back, from kernels that write the tiles of the kept order it overlaps.
    std::string text_range(size_t start, size_t end = std::string::npos) const {
        return text_window(nullptr, start, end, false);
    }
    std::string text_at(const Mark& m, size_t start = 0, size_t end = std::string::npos) const {
        return text_window(m.get(), start, end, false);
    }
    // HipMerge::line_starts / lines_of / text_lines on the device (the queued updates are decoded
    // first): a wave per query over the replica's kept document order, and only the lines' text comes
    // back.  lines_of takes positions in the adapter's unit.
    std::vector<LinePos> line_starts(const std::vector<uint64_t>& lines, const crdt_hip_mark* m = nullptr) const {
        return line_starts_of(lines, m, nullptr, nullptr);
    }
    std::vector<LinePos> lines_of(const std::vector<uint64_t>& pos, const crdt_hip_mark* m = nullptr) const {
        return lines_at(pos, m, false);
    }
    std::string text_lines(size_t first, size_t count, const crdt_hip_mark* m = nullptr) const {
        return text_lines_get(
            [&](const std::vector<uint64_t>& q, crdt_hip_line_info* info, bool* beyond) {
                return line_starts_of(q, m, info, beyond);
            },
            [&](size_t a, size_t b) { return text_window(m, a, b, true); }, first, count);
    }
    // HipMerge::units_of / replace_utf16 / patches_since_utf16 on the device (the queued updates are
    // decoded first): a wave per position over the replica's kept document order; the edit and the
    // patches pay one such translation of their boundaries on top of the codepoint call.
    std::vector<UnitPos> units_of(const std::vector<uint64_t>& pos, uint32_t unit, const crdt_hip_mark* m = nullptr,
                                  crdt_hip_unit_info* info = nullptr) const {
        flush();
        return units_get(
            [&](const uint64_t* q, size_t n, UnitPos* out, crdt_hip_unit_info* i) {
                return crdt_hip_replica_units_of(dev_->ctx, rep_, m, q, n, unit, out, i);
            },
            dev_->ctx, pos, info);
    }
    void replace_utf16(size_t start, size_t end, std::string_view s) {
        flush();
        check(crdt_hip_replica_replace_utf16(dev_->ctx, rep_, start, end, s.data(), s.size()), dev_->ctx,
              "replica_replace_utf16");
    }
    std::vector<Patch> patches_since_utf16(const Mark& m) const {
        flush();
        return patches_get(
            [&](crdt_hip_patch* out, size_t cap, size_t* n, uint8_t* ins, size_t icap, size_t* nb) {
                return crdt_hip_replica_patches_since_utf16(dev_->ctx, rep_, m.get(), out, cap, n, ins,
                                                            icap, nb);
            },
            dev_->ctx, 4096, 1 << 16);
    }
    // HipMerge::anchor_at / resolve / resolve_many on the device (the queued updates are decoded
    // first): resolved in HIP kernels against the replica's kept document order.
    Anchor anchor_at(size_t pos, uint32_t bias = CRDT_HIP_ANCHOR_AFTER) const {
        return anchor_of(pos, bias, false);
    }
    std::vector<AnchorAt> resolve_many(const std::vector<Anchor>& a) const {
        return anchors_known(resolved(a), false);
    }
    AnchorAt resolve(const Anchor& a) const { return resolve_many({a})[0]; }
    // HipMerge::format / unformat / spans / sync_formats_from on the device (the queued updates are
    // decoded first): the spans come from HIP kernels over the replica's kept document order.
    void set_agent(uint16_t agent) {
        check(crdt_hip_replica_set_agent(rep_, agent), dev_->ctx, "replica_set_agent");
        formats_.agent = agent;
    }
    uint64_t format(size_t start, size_t end, uint32_t key, uint64_t value, unsigned expand = 0) {
        return format_op(start, end, key, value, 0, expand, false);
    }
    uint64_t unformat(size_t start, size_t end, uint32_t key, unsigned expand = 0) {
        return format_op(start, end, key, 0, CRDT_HIP_FORMAT_REMOVE, expand, false);
    }
    Spans spans() const { return spans_of(false); }
    const FormatSet& formats() const { return formats_; }
    size_t sync_formats_from(const HipDownstream& o) { return formats_.merge(o.formats_); }

protected:
    uint64_t format_op(size_t start, size_t end, uint32_t key, uint64_t value, uint32_t flags,
                       unsigned expand, bool bytes) {
        flush();
        std::vector<crdt_hip_sv_entry> sv(65536);
        size_t n = 0;
        check(crdt_hip_replica_state_vector(dev_->ctx, rep_, sv.data(), sv.size(), &n), dev_->ctx,
              "replica_state_vector");
        sv.resize(n);
        return formats_.add(
            anchor_of(start, expand & EXPAND_START ? CRDT_HIP_ANCHOR_AFTER : CRDT_HIP_ANCHOR_BEFORE, bytes),
            anchor_of(end, expand & EXPAND_END ? CRDT_HIP_ANCHOR_BEFORE : CRDT_HIP_ANCHOR_AFTER, bytes),
            key, value, flags, sv);
    }
    Spans spans_of(bool bytes) const {
        flush();
        return spans_get(
            [&](const Format* f, size_t n, crdt_hip_span* out, size_t cap, size_t* on,
                crdt_hip_span_attr* at, size_t acap, size_t* oa, size_t* pend) {
                return crdt_hip_replica_spans(dev_->ctx, rep_, f, n, out, cap, on, at, acap, oa, pend);
            },
            formats_, dev_->ctx, bytes);
    }
    FormatSet formats_;
    std::string text_window(const crdt_hip_mark* m, size_t start, size_t end, bool bytes) const {
        flush();
        return text_get(
            [&](uint64_t s, uint64_t e, uint32_t flags, uint8_t* out, size_t cap, size_t* n,
                crdt_hip_text_info* info) {
                return crdt_hip_replica_text_at(dev_->ctx, rep_, m, s, e, flags, out, cap, n, info);
            },
            dev_->ctx, start, end, bytes, 1 << 16);
    }
    std::vector<LinePos> line_starts_of(const std::vector<uint64_t>& lines, const crdt_hip_mark* m,
                                        crdt_hip_line_info* info, bool* beyond) const {
        flush();
        return lines_get(
            [&](const uint64_t* q, size_t n, LinePos* out, crdt_hip_line_info* i) {
                return crdt_hip_replica_line_starts(dev_->ctx, rep_, m, q, n, out, i);
            },
            dev_->ctx, lines, info, beyond);
    }
    std::vector<LinePos> lines_at(const std::vector<uint64_t>& pos, const crdt_hip_mark* m, bool bytes) const {
        flush();
        return lines_get(
            [&](const uint64_t* q, size_t n, LinePos* out, crdt_hip_line_info* info) {
                return crdt_hip_replica_lines_of(dev_->ctx, rep_, m, q, n, bytes ? (uint32_t)CRDT_HIP_TEXT_BYTES : 0u,
                                                 out, info);
            },
            dev_->ctx, pos);
    }
    Anchor anchor_of(size_t pos, uint32_t bias, bool bytes) const {
        flush();
        const uint64_t p = pos;
        const uint8_t b = (uint8_t)bias;
        Anchor a;
        check((bytes ? crdt_hip_replica_anchors_at_bytes
                     : crdt_hip_replica_anchors_at)(dev_->ctx, rep_, &p, &b, 1, &a),
              dev_->ctx, "replica_anchors_at");
        return a;
    }
    std::vector<crdt_hip_anchor_pos> resolved(const std::vector<Anchor>& a) const {
        flush();
        std::vector<crdt_hip_anchor_pos> p(a.size());
        check(crdt_hip_replica_anchors_resolve(dev_->ctx, rep_, a.data(), a.size(), p.data()),
              dev_->ctx, "replica_anchors_resolve");
        return p;
    }
    std::shared_ptr<Device> dev_;
    crdt_hip_replica* rep_ = nullptr;
    mutable std::vector<uint8_t> buf_;
    mutable std::vector<uint64_t> off_{0};

    explicit HipDownstream(std::shared_ptr<Device> d) : dev_(std::move(d)) {}
    void flush() const {
        if (off_.size() < 2) return;
        check(crdt_hip_replica_apply_updates(dev_->ctx, rep_, buf_.data(), buf_.size(), off_.data(),
                                             (uint32_t)(off_.size() - 1)),
              dev_->ctx, "replica_apply_updates");
        buf_.clear();
        off_.assign(1, 0);
    }
};

// HipDownstream for a caller that keeps its text as UTF-8 (EDITS_USE_BYTE_OFFSETS = true,
// rope.rs:8,16-19, as the cola and yrs adapters): an Upstream too, whose insert, remove and replace
// take byte offsets resolved on the device (crdt_hip_replica_replace_bytes); Patch::pos and
// Patch::del of patches_since are bytes, and len() is a byte length.  crdt_bench does not run it
// (its loop is the codepoint one); it is compiled with it.
class HipDownstreamBytes : public HipDownstream {
public:
    static constexpr const char* NAME = "mi355x-device-bytes";
    static constexpr bool EDITS_USE_BYTE_OFFSETS = true;

    explicit HipDownstreamBytes(HipDownstream&& d) : HipDownstream(std::move(d)) {}
    HipDownstreamBytes clone() const { return HipDownstreamBytes(HipDownstream::clone()); }
    // Upstream::replace (rope.rs:21-32) in byte offsets; a boundary inside a codepoint is an error
    void replace(size_t start, size_t end, std::string_view s) {
        flush();
        check(crdt_hip_replica_replace_bytes(dev_->ctx, rep_, start, end, s.data(), s.size()),
              dev_->ctx, "replica_replace_bytes");
    }
    void insert(size_t at, std::string_view s) { replace(at, at, s); }
    void remove(size_t start, size_t end) { replace(start, end, std::string_view()); }
    // Upstream::len in bytes: the merged document's UTF-8 length (HipDownstream::len checks it
    // against the decoder's counter).
    size_t len() const {
        (void)HipDownstream::len();
        uint64_t items = 0, cps = 0, bytes = 0;
        crdt_hip_replica_info(rep_, &items, &cps, &bytes);
        return (size_t)bytes;
    }
    std::vector<Patch> patches_since(const Mark& m) const {
        flush();
        return patches_get(
            [&](crdt_hip_patch* out, size_t cap, size_t* n, uint8_t* ins, size_t icap, size_t* nb) {
                return crdt_hip_replica_patches_since_bytes(dev_->ctx, rep_, m.get(), out, cap, n,
                                                            ins, icap, nb);
            },
            dev_->ctx, 4096, 1 << 16);
    }
    // Windows in byte offsets (a boundary inside a codepoint is an error).
    std::string text_range(size_t start, size_t end = std::string::npos) const {
        return text_window(nullptr, start, end, true);
    }
    std::string text_at(const Mark& m, size_t start = 0, size_t end = std::string::npos) const {
        return text_window(m.get(), start, end, true);
    }
    // Positions in byte offsets (one inside a codepoint is an error).
    std::vector<LinePos> lines_of(const std::vector<uint64_t>& pos, const crdt_hip_mark* m = nullptr) const {
        return lines_at(pos, m, true);
    }
    // Anchors taken at, and resolved to, byte offsets (one inside a codepoint is an error).
    Anchor anchor_at(size_t pos, uint32_t bias = CRDT_HIP_ANCHOR_AFTER) const {
        return anchor_of(pos, bias, true);
    }
    std::vector<AnchorAt> resolve_many(const std::vector<Anchor>& a) const {
        return anchors_known(resolved(a), true);
    }
    AnchorAt resolve(const Anchor& a) const { return resolve_many({a})[0]; }
    // Formats made at, and spans painted in, byte offsets.
    uint64_t format(size_t start, size_t end, uint32_t key, uint64_t value, unsigned expand = 0) {
        return format_op(start, end, key, value, 0, expand, true);
    }
    uint64_t unformat(size_t start, size_t end, uint32_t key, unsigned expand = 0) {
        return format_op(start, end, key, 0, CRDT_HIP_FORMAT_REMOVE, expand, true);
    }
    Spans spans() const { return spans_of(true); }
};

}  // namespace hipmerge
