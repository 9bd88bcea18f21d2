// capi.cpp — the extern "C" boundary declared in include/crdt_hip.h.  Nothing throws across it:
// every entry point catches, records the message and returns a CRDT_HIP_E* code.
//
// Each rule of the boundary is stated once, in the helpers of the first namespace below (DESIGN.md
// §2): the refusals (check_*), the two call shapes (host, device), the ESPACE copy-out (copy_out,
// copy_out2, text_out), handle creation (make_handle) and the optional outs (put).  An entry
// point names its own arguments and the OpLog / replica_* function; a `_bytes` twin forwards to
// the body it shares with its codepoint form.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "crdt_hip.h"
#include "crdt_hip_lines.h"
#include "crdt_hip_utf16.h"
#include "engine.hpp"
#include "oplog.hpp"
#include "replica.hpp"
#include "store.hpp"
#include "synth.hpp"
#include "trace.hpp"
#include "util.hpp"

struct crdt_hip_ctx {
    crdt::Engine eng;
    std::string last_err;
    crdt::DeviceLogs staging;
    ncclComm_t comm = nullptr;
    int nranks = 0, rank = 0;
    // replay sessions (crdt_hip_replica_replay): the work replica and learnt sizes per
    // (initial replica, update batch), most recent first
    std::vector<std::unique_ptr<crdt::ReplayState>> replays;
    crdt::JoinStats last_join;  // what the last crdt_hip_replica_join observed
    crdt::DeltaStats last_delta;  // what the last device encode_diff / apply_diff observed
    crdt::PatchStats last_patch;  // what the last device patches_since observed
    crdt::EditStats last_edit;    // what the last device apply_patches observed
    crdt::AnchorStats last_anchor;  // what the last device anchors_at / anchors_resolve observed
    crdt::FormatStats last_format;  // what the last device spans observed
    crdt::TextStats last_text;      // what the last device text_at observed
    crdt::LineStats last_line;      // what the last device line_starts / lines_of observed
    crdt::UnitStats last_unit;      // what the last device units_of observed, one inside a _utf16 call included
};
namespace {
// Names the owner of a mark: every log and replica handle gets its own, a clone included.
uint64_t next_uid() {
    static std::atomic<uint64_t> n{0};
    return ++n;
}
}  // namespace
struct crdt_hip_oplog {
    crdt::OpLog log;
    uint64_t uid = next_uid();
    crdt_hip_oplog() = default;
    crdt_hip_oplog(const crdt_hip_oplog& o) : log(o.log) {}
};
struct crdt_hip_mark {
    uint64_t owner = 0;           // uid of the log or replica the mark was taken from
    crdt_hip_ctx* ctx = nullptr;  // a replica's mark: its context (a host mark: null)
    crdt::LogMark host;
    crdt::DeviceMark dev;
};
struct crdt_hip_trace {
    crdt::Trace t;
};
struct crdt_hip_batch {
    crdt_hip_ctx* ctx = nullptr;
    crdt::DeviceLogs logs;
    uint64_t device_bytes = 0;
};
struct crdt_hip_replica {
    crdt_hip_ctx* ctx = nullptr;
    crdt::Replica r;
    uint64_t uid = next_uid();
};

struct crdt_hip_updates {
    crdt_hip_ctx* ctx = nullptr;
    crdt::UpdateBatch u;
};
struct crdt_hip_logfile {
    crdt::MappedLog m;
};

namespace {

// device bytes per op-log slot: parent (4) + key (lamport << 16 | agent, 8) + codepoint (3)
constexpr uint64_t kSlotBytes = 15;
thread_local std::string g_err;

// A refusal lands in the string of the context the call was made on; without one, the thread's.
int set_err(crdt_hip_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->last_err = msg;
    else g_err = msg;
    return code;
}
int from_engine(crdt_hip_ctx* ctx, int rc) {
    if (rc) ctx->last_err = ctx->eng.err;
    return rc;
}

template <class F>
int guard(crdt_hip_ctx* ctx, F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return set_err(ctx, CRDT_HIP_ENOMEM, "out of host memory");
    } catch (const std::exception& e) {
        return set_err(ctx, CRDT_HIP_EINVAL, e.what());
    } catch (...) {
        return set_err(ctx, CRDT_HIP_EINVAL, "unknown exception");
    }
}

// ---- refusals: a NULL argument first, then whose the handle is, then whose the mark is ---------
int null_arg(crdt_hip_ctx* ctx) { return set_err(ctx, CRDT_HIP_EINVAL, "null argument"); }
int null_ctx() { return set_err(nullptr, CRDT_HIP_EINVAL, "null context"); }

// `args_ok`: the call's other required pointers are there
int check_replica(crdt_hip_ctx* ctx, const crdt_hip_replica* r, bool args_ok = true) {
    if (!ctx || !r || !args_ok) return null_arg(ctx);
    if (r->ctx != ctx) return set_err(ctx, CRDT_HIP_EINVAL, "replica belongs to another context");
    return 0;
}
int check_replica_updates(crdt_hip_ctx* ctx, const crdt_hip_replica* r, const crdt_hip_updates* u) {
    if (!ctx || !r || !u) return null_arg(ctx);
    if (r->ctx != ctx || u->ctx != ctx)
        return set_err(ctx, CRDT_HIP_EINVAL, "replica or updates belong to another context");
    return 0;
}
int check_batch(crdt_hip_ctx* ctx, const crdt_hip_batch* b) {
    if (!ctx || !b) return null_arg(ctx);
    if (b->ctx != ctx) return set_err(ctx, CRDT_HIP_EINVAL, "batch belongs to another context");
    return 0;
}
// `optional`: m may be NULL (text_at: the version now)
int check_log_mark(const crdt_hip_oplog* log, const crdt_hip_mark* m, bool args_ok, bool optional = false) {
    if (!log || (!m && !optional) || !args_ok) return null_arg(nullptr);
    if (m && m->ctx) return set_err(nullptr, CRDT_HIP_EINVAL, "a replica's mark passed to a log");
    if (m && m->owner != log->uid) return set_err(nullptr, CRDT_HIP_EINVAL, "the mark belongs to another log");
    return 0;
}
int check_replica_mark(crdt_hip_ctx* ctx, const crdt_hip_replica* r, const crdt_hip_mark* m, bool args_ok,
                       bool optional = false) {
    if (int rc = check_replica(ctx, r, args_ok && (m || optional))) return rc;
    if (m && !m->ctx) return set_err(ctx, CRDT_HIP_EINVAL, "a log's mark passed to a replica");
    if (m && (m->ctx != ctx || m->owner != r->uid))
        return set_err(ctx, CRDT_HIP_EINVAL, "the mark belongs to another replica");
    return 0;
}

// ---- the two call shapes -----------------------------------------------------------------------
// A host call: fn(std::string& err) -> code, the message recorded for a code other than 0.
template <class F>
int host(F&& fn) {
    return guard(nullptr, [&] {
        std::string e;
        const int rc = fn(e);
        return rc ? set_err(nullptr, rc, e) : 0;
    });
}
// The OpLog and file calls that answer "" or a message: each has one fixed code.
template <class F>
int host_msg(int code, F&& fn) {
    return guard(nullptr, [&] {
        const std::string e = fn();
        return e.empty() ? 0 : set_err(nullptr, code, e);
    });
}
// A device call: `refused` is what the call's check_* answered (evaluated before anything runs);
// fn() -> the engine's code (its message is the engine's), then `then()` -> code for what the
// boundary itself does with the result.
struct Done {
    int operator()() const { return 0; }
};
template <class F, class Then = Done>
int device(crdt_hip_ctx* ctx, int refused, F&& fn, Then&& then = Then{}) {
    if (refused) return refused;
    return guard(ctx, [&] {
        const int rc = fn();
        return rc ? from_engine(ctx, rc) : then();
    });
}

// ---- outputs -----------------------------------------------------------------------------------
// Optional outs: put(p, v, q, w, ...) stores v through p and w through q where they are not NULL.
inline void put() {}
template <class T, class V, class... Rest>
void put(T* p, const V& v, const Rest&... rest) {
    if (p) *p = (T)v;
    put(rest...);
}

// One sized array under the ESPACE convention: the count is written first; a NULL or short buffer
// is CRDT_HIP_ESPACE and nothing is copied.  `empty_ok`: an empty result needs no buffer.
constexpr const char* kShort = "buffer too small";
template <class T, class O>
int copy_out(const std::vector<T>& v, O* out, size_t cap, size_t* out_n, bool empty_ok, std::string& err) {
    static_assert(sizeof(T) == sizeof(O), "copy_out: element layout");
    *out_n = v.size();
    if (v.empty() && empty_ok) return 0;
    if (!out || cap < v.size()) {
        err = kShort;
        return CRDT_HIP_ESPACE;
    }
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
    return 0;
}
// Two sized arrays: both counts are written first, either array short is ESPACE and neither is
// copied.  An array needs room if it holds something; `b_with_a`: b needs room (a non-NULL buffer,
// even for nothing) whenever a holds something (spans and their attributes).
template <class A, class OA, class B, class OB>
int copy_out2(const std::vector<A>& a, OA* out_a, size_t cap_a, size_t* n_a, const std::vector<B>& b,
              OB* out_b, size_t cap_b, size_t* n_b, bool b_with_a, std::string& err) {
    static_assert(sizeof(A) == sizeof(OA) && sizeof(B) == sizeof(OB), "copy_out2: element layout");
    *n_a = a.size();
    *n_b = b.size();
    const bool need_a = !a.empty(), need_b = b_with_a ? need_a : !b.empty();
    if ((need_a && (!out_a || cap_a < a.size())) || (need_b && (!out_b || cap_b < b.size()))) {
        err = kShort;
        return CRDT_HIP_ESPACE;
    }
    if (need_a) std::memcpy(out_a, a.data(), a.size() * sizeof(A));
    if (need_b && !b.empty()) std::memcpy(out_b, b.data(), b.size() * sizeof(B));
    return 0;
}
// The tail of the three merges: the text, if the caller gave a buffer (the counts are out already).
int text_out(crdt_hip_ctx* ctx, const std::vector<uint8_t>& text, uint64_t len, uint8_t* out, size_t cap) {
    if (!out) return 0;
    if (cap < len) return set_err(ctx, CRDT_HIP_ESPACE, "output buffer too small");
    if (len) std::memcpy(out, text.data(), (size_t)len);
    return 0;
}

// A new handle: fill(T&) -> code; a failed fill frees it and leaves *out alone.
template <class T, class F>
int make_handle(crdt_hip_ctx* ctx, T** out, F&& fill) {
    return guard(ctx, [&] {
        auto h = std::make_unique<T>();
        if (int rc = fill(*h)) return rc;
        *out = h.release();
        return 0;
    });
}

uint64_t visible_bytes(const crdt_hip_oplog_view& v) {
    // (branch-free, so that it vectorises: part of every crdt_hip_merge of a host view)
    uint64_t b = 0;
    for (uint32_t i = 0; i < v.n; ++i) {
        const uint32_t c = v.cp[i] & 0x1FFFFFu;
        const uint32_t len = 1u + (c >= 0x80u) + (c >= 0x800u) + (c >= 0x10000u);
        b += v.deleted[i] ? 0u : len;
    }
    return b;
}

int check_view(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* v) {
    if (!v) return set_err(ctx, CRDT_HIP_EINVAL, "null op log view");
    if (v->n && (!v->parent || !v->lamport || !v->agent || !v->deleted || !v->cp))
        return set_err(ctx, CRDT_HIP_EINVAL, "op log view has null arrays");
    if (v->n > 0x7FFFFF00u) return set_err(ctx, CRDT_HIP_ERANGE, "op log too large");
    return 0;
}

int stage_views(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* logs, uint32_t n) {
    std::vector<crdt::DocInfo> docs(n);
    for (uint32_t i = 0; i < n; ++i) {
        int rc = check_view(ctx, &logs[i]);
        if (rc) return rc;
        docs[i] = crdt::DocInfo{logs[i].n, visible_bytes(logs[i])};
    }
    int rc = ctx->eng.plan(ctx->staging, docs);
    if (rc) return from_engine(ctx, rc);
    return from_engine(ctx, ctx->eng.upload(ctx->staging, logs, n));
}
void view_of(const crdt::OpLog& L, crdt_hip_oplog_view* out) {
    out->n = L.size();
    out->parent = L.parent.data();
    out->origin_right = L.oright.data();
    out->lamport = L.lamport.data();
    out->agent = L.agent.data();
    out->deleted = L.deleted.data();
    out->cp = L.cp.data();
    // (non-NULL for an empty Fugue log too: a replica made from it is a Fugue replica)
    static const uint8_t kNoSide = 0;
    out->side = L.fugue ? (L.side.empty() ? &kNoSide : L.side.data()) : nullptr;
}
uint64_t batch_bytes(const crdt::DeviceLogs& logs) {
    return logs.total_slots * kSlotBytes + (logs.total_slots >> logs.log2m) * 4;
}
// Upstream::replace (rope.rs:21-32) as one patch; `what` applies it.  0 for the empty replace.
template <class Apply>
int replace_as_patch(crdt_hip_ctx* ctx, size_t start, size_t end, size_t nbytes, const char* too_long,
                     Apply&& what) {
    const size_t del = end > start ? end - start : 0;
    if (del == 0 && nbytes == 0) return 0;
    if (del > 0xFFFFFFFFull || nbytes > 0xFFFFFFFFull) return set_err(ctx, CRDT_HIP_ERANGE, too_long);
    const crdt_hip_patch one{(uint64_t)start, 0, (uint32_t)del, (uint32_t)nbytes};
    return what(&one);
}
constexpr const char* kReplaceBytes = "replace of 2^32 or more bytes";
constexpr const char* kReplaceCodepoints = "replace of 2^32 or more codepoints or bytes";

// The parameters of crdt_hip_set_param (all but "splitter_stride", which writes two knobs): the
// ABI name, the knob (engine.hpp Tunables, where each is described), the accepted values and the
// message for any other.  No message: a hook that takes any value, nonzero = on.
using crdt::Tunables;
template <uint64_t LO, uint64_t HI>
bool within(uint64_t v) { return v >= LO && v <= HI; }
bool runs_slots_ok(uint64_t v) { return v == 16 || v == 32 || v == 64; }
bool digit_bits_ok(uint64_t v) { return v == 0 || v == 8 || v == 10; }
struct Param {
    const char* name;
    uint64_t Tunables::*field;
    bool (*ok)(uint64_t);
    const char* msg;
};
const Param kParams[] = {
    {"max_wave_slots", &Tunables::max_wave_slots, within<4096, 1ull << 31>, "max_wave_slots out of range"},
    {"tail_wave_div", &Tunables::tail_wave_div, within<0, 64>, "tail_wave_div must be in [0, 64]"},
    {"lanes", &Tunables::lanes, within<1, 8>, "lanes must be in [1, 8]"},
    {"lane_gate", &Tunables::l0_gated, within<0, 1>, "lane_gate must be 0 or 1"},
    {"l1_split", &Tunables::l1_split, within<0, 1>, "l1_split must be 0 or 1"},
    {"plan_cache", &Tunables::plan_cache, within<0, 1>, "plan_cache must be 0 or 1"},
    {"fuse_text", &Tunables::fuse_text, nullptr, nullptr},
    {"doctree_lds_max", &Tunables::doctree_lds_max, nullptr, nullptr},
    {"xcd_order", &Tunables::xcd_order, within<0, 1>, "xcd_order must be 0 or 1"},
    {"group_docs", &Tunables::group_docs, within<0, 1>, "group_docs must be 0 or 1"},
    {"runs_slots", &Tunables::runs_slots, runs_slots_ok, "runs_slots must be 16, 32 or 64"},
    {"stile_text", &Tunables::stile_text, within<0, 2>, "stile_text must be 0, 1 or 2"},
    {"text_scatter", &Tunables::text_scatter, within<0, 1>, "text_scatter must be 0 or 1"},
    {"contraction", &Tunables::contraction, within<0, 2>, "contraction must be 0, 1 or 2"},
    {"l1_group", &Tunables::l1_group, within<0, 2>, "l1_group must be 0, 1 or 2"},
    {"rs_digit_bits", &Tunables::rs_digit_bits, digit_bits_ok, "rs_digit_bits must be 0, 8 or 10"},
    {"nsq_list", &Tunables::nsq_list, within<0, 2>, "nsq_list must be 0, 1 or 2"},
    {"static_jumps", &Tunables::static_jumps, within<0, 1>, "static_jumps must be 0 or 1"},
    {"dead_skip", &Tunables::dead_skip, within<0, 1>, "dead_skip must be 0 or 1"},
    {"plain_tiles", &Tunables::plain_tiles, within<0, 1>, "plain_tiles must be 0 or 1"},
    {"doctree_k32", &Tunables::doctree_k32, within<0, 1>, "doctree_k32 must be 0 or 1"},
    {"glds_late", &Tunables::glds_late, nullptr, nullptr},
    {"plan_shrink", &Tunables::plan_shrink, nullptr, nullptr},
    {"level1", &Tunables::level1_global, within<0, 1>, "level1 must be 0 (auto) or 1 (global)"},
};

// ---- codepoint and byte twins: one body, `bytes` picks the OpLog / replica_* function ------------
using crdt::OpLog;
using crdt::PatchRec;
const uint8_t* u8(const char* s) { return reinterpret_cast<const uint8_t*>(s); }

int oplog_apply_patches(crdt_hip_oplog* log, const crdt_hip_patch* p, size_t n, const uint8_t* ins,
                        size_t ins_len, uint32_t* added, uint32_t* tombstoned, bool bytes) {
    if (!log || (!p && n) || (!ins && ins_len)) return null_arg(nullptr);
    const auto apply = bytes ? &OpLog::apply_patches_bytes : &OpLog::apply_patches;
    return host([&](std::string& e) {
        return (log->log.*apply)(reinterpret_cast<const PatchRec*>(p), n, ins, ins_len, added, tombstoned, e);
    });
}
int replica_apply_patches(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_patch* p, size_t n,
                          const uint8_t* ins, size_t ins_len, uint32_t* added, uint32_t* tombstoned,
                          bool bytes) {
    const auto apply = bytes ? crdt::replica_apply_patches_bytes : crdt::replica_apply_patches;
    return device(ctx, check_replica(ctx, r, (p || !n) && (ins || !ins_len)), [&] {
        return apply(ctx->eng, r->r, reinterpret_cast<const PatchRec*>(p), n, ins, ins_len, added,
                     tombstoned, &ctx->last_edit);
    });
}
int replica_replace(crdt_hip_ctx* ctx, crdt_hip_replica* r, size_t start, size_t end, const char* utf8,
                    size_t nbytes, bool bytes) {
    if (int rc = check_replica(ctx, r, utf8 || !nbytes)) return rc;
    return replace_as_patch(ctx, start, end, nbytes, bytes ? kReplaceBytes : kReplaceCodepoints,
                            [&](const crdt_hip_patch* one) {
                                return replica_apply_patches(ctx, r, one, 1, u8(utf8), nbytes, nullptr,
                                                             nullptr, bytes);
                            });
}
int oplog_patches_since(crdt_hip_oplog* log, const crdt_hip_mark* m, crdt_hip_patch* out, size_t cap,
                        size_t* out_n, uint8_t* ins, size_t ins_cap, size_t* out_ins, bool bytes) {
    if (int rc = check_log_mark(log, m, out_n && out_ins)) return rc;
    const auto since = bytes ? &OpLog::patches_since_bytes : &OpLog::patches_since;
    return host([&](std::string& e) {
        std::vector<PatchRec> p;
        std::vector<uint8_t> text;
        if (int rc = (log->log.*since)(m->host, p, text, e)) return rc;
        return copy_out2(p, out, cap, out_n, text, ins, ins_cap, out_ins, false, e);
    });
}
int replica_patches_since(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                          crdt_hip_patch* out, size_t cap, size_t* out_n, uint8_t* ins, size_t ins_cap,
                          size_t* out_ins, bool bytes) {
    const auto since = bytes ? crdt::replica_patches_since_bytes : crdt::replica_patches_since;
    return device(ctx, check_replica_mark(ctx, r, m, out_n && out_ins), [&] {
        return since(ctx->eng, r->r, m->dev, reinterpret_cast<PatchRec*>(out), cap, out_n, ins, ins_cap,
                     out_ins, &ctx->last_patch);
    });
}
int oplog_anchors_at(crdt_hip_oplog* log, const uint64_t* pos, const uint8_t* bias, size_t n,
                     bool bytes, crdt_hip_anchor* out) {
    if (!log || ((!pos || !out) && n)) return null_arg(nullptr);
    return host([&](std::string& e) {
        return log->log.anchors_at(pos, bias, n, bytes, reinterpret_cast<crdt::AnchorRec*>(out), e);
    });
}
int replica_anchors_at(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint64_t* pos, const uint8_t* bias,
                       size_t n, bool bytes, crdt_hip_anchor* out) {
    return device(ctx, check_replica(ctx, r, (pos && out) || !n), [&] {
        return crdt::replica_anchors_at(ctx->eng, r->r, pos, bias, n, bytes,
                                        reinterpret_cast<crdt::AnchorRec*>(out), &ctx->last_anchor);
    });
}
int trace_resolve(const crdt_hip_trace* t, crdt_hip_oplog** out, bool fugue) {
    if (!t || !out) return null_arg(nullptr);
    if (t->t.byte_offsets)
        return set_err(nullptr, CRDT_HIP_EINVAL, "resolve needs codepoint offsets (EDITS_USE_BYTE_OFFSETS = false)");
    *out = nullptr;
    return make_handle(nullptr, out, [&](crdt_hip_oplog& L) {
        L.log.fugue = fugue;
        const crdt::Trace& T = t->t;
        std::string e;
        // (OpLog::replay sizes the columns to the patches' bounds itself)
        // from_str(start_content), then replace() every patch (main.rs:29-33, rope.rs:21-32)
        if (!T.start_content.empty())
            e = L.log.insert_utf8(0, T.start_content.data(), T.start_content.size());
        if (e.empty()) e = L.log.replay(T.patches.data(), T.patches.size(), T.ins.data(), T.ins.size());
        return e.empty() ? 0 : set_err(nullptr, CRDT_HIP_ERANGE, e);
    });
}
// A generated log into a handle (the generators answer a heap OpLog).
int synth_handle(crdt_hip_oplog** out, crdt::OpLog* made) {
    std::unique_ptr<crdt::OpLog> L(made);
    return make_handle(nullptr, out, [&](crdt_hip_oplog& o) {
        o.log = std::move(*L);
        return 0;
    });
}
void drop_replays(crdt_hip_ctx* ctx, const void* init, const void* ub) {
    if (!ctx) return;
    auto& v = ctx->replays;
    for (size_t i = v.size(); i-- > 0;)
        if (v[i]->init == init || v[i]->ub == ub) v.erase(v.begin() + (long)i);
}
}  // namespace

extern "C" {

int crdt_hip_abi_version(void) { return CRDT_HIP_ABI_VERSION; }

int crdt_hip_device_count(int* out) {
    if (!out) return set_err(nullptr, CRDT_HIP_EINVAL, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *out = e == hipSuccess ? n : 0;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(nullptr, CRDT_HIP_EDEVICE, hipGetErrorString(e));
    }
    return 0;
}

int crdt_hip_init(int device, crdt_hip_ctx** out) {
    if (!out) return set_err(nullptr, CRDT_HIP_EINVAL, "null out");
    *out = nullptr;
    return make_handle(nullptr, out, [&](crdt_hip_ctx& c) {
        const std::string e = c.eng.init(device);
        return e.empty() ? 0 : set_err(nullptr, CRDT_HIP_EDEVICE, e);
    });
}

int crdt_hip_destroy(crdt_hip_ctx* ctx) {
    if (!ctx) return 0;
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    delete ctx;
    return 0;
}

const char* crdt_hip_last_error(const crdt_hip_ctx* ctx) {
    return ctx ? ctx->last_err.c_str() : g_err.c_str();
}

int crdt_hip_set_param(crdt_hip_ctx* ctx, const char* key, uint64_t value) {
    if (!ctx || !key) return null_arg(ctx);
    std::string k = key;
    if (k == "splitter_stride") {
        if (value < 16 || value > 4096 || (value & (value - 1)))
            return set_err(ctx, CRDT_HIP_EINVAL, "splitter_stride must be a power of two in [16, 4096]");
        uint32_t l = 0;
        while ((1ull << l) < value) ++l;
        ctx->eng.log2m = l;
        ctx->eng.log2m_set = 1;
        return 0;
    }
    for (const Param& p : kParams) {
        if (k != p.name) continue;
        if (p.msg && !p.ok(value)) return set_err(ctx, CRDT_HIP_EINVAL, p.msg);
        ctx->eng.*p.field = p.msg ? value : (uint64_t)(value != 0);
        return CRDT_HIP_OK;
    }
    return set_err(ctx, CRDT_HIP_EINVAL, "unknown parameter " + k);
}

// ---- op log ----------------------------------------------------------------------------------
int crdt_hip_oplog_new(crdt_hip_oplog** out) {
    if (!out) return set_err(nullptr, CRDT_HIP_EINVAL, "null out");
    return guard(nullptr, [&] { *out = new crdt_hip_oplog(); return 0; });
}
int crdt_hip_oplog_set_fugue(crdt_hip_oplog* log, int on) {
    if (!log) return null_arg(nullptr);
    if (log->log.size()) return set_err(nullptr, CRDT_HIP_EINVAL, "set_fugue needs an empty log");
    log->log.fugue = on != 0;
    return 0;
}
int crdt_hip_oplog_set_agent(crdt_hip_oplog* log, uint16_t agent) {
    if (!log) return null_arg(nullptr);
    log->log.local_agent = agent;
    return 0;
}
int crdt_hip_oplog_clone(const crdt_hip_oplog* src, crdt_hip_oplog** out) {
    if (!src || !out) return null_arg(nullptr);
    return guard(nullptr, [&] { *out = new crdt_hip_oplog(*src); return 0; });
}
void crdt_hip_oplog_free(crdt_hip_oplog* log) { delete log; }

int crdt_hip_oplog_insert(crdt_hip_oplog* log, size_t pos, const char* utf8, size_t nbytes) {
    if (!log || (!utf8 && nbytes)) return null_arg(nullptr);
    return host_msg(CRDT_HIP_ERANGE, [&] { return log->log.insert_utf8(pos, utf8, nbytes); });
}
int crdt_hip_oplog_remove(crdt_hip_oplog* log, size_t start, size_t end) {
    if (!log) return null_arg(nullptr);
    return host_msg(CRDT_HIP_ERANGE, [&] { return log->log.remove(start, end); });
}
int crdt_hip_oplog_replace(crdt_hip_oplog* log, size_t start, size_t end, const char* utf8,
                           size_t nbytes) {
    if (end > start) {
        int rc = crdt_hip_oplog_remove(log, start, end);
        if (rc) return rc;
    }
    if (nbytes) return crdt_hip_oplog_insert(log, start, utf8, nbytes);
    return 0;
}
size_t crdt_hip_oplog_visible_len(const crdt_hip_oplog* log) { return log ? log->log.visible() : 0; }
int crdt_hip_oplog_visible_bytes(const crdt_hip_oplog* log, uint64_t* out) {
    if (!log || !out) return null_arg(nullptr);
    *out = log->log.visible_bytes();
    return 0;
}

int crdt_hip_oplog_get_view(const crdt_hip_oplog* log, crdt_hip_oplog_view* out) {
    if (!log || !out) return null_arg(nullptr);
    view_of(log->log, out);
    return 0;
}
uint64_t crdt_hip_oplog_version(const crdt_hip_oplog* log) { return log ? log->log.version() : 0; }

int crdt_hip_oplog_encode_from(const crdt_hip_oplog* log, uint64_t version, uint8_t* buf,
                               size_t cap, size_t* out_len) {
    if (!log || !out_len) return null_arg(nullptr);
    return host([&](std::string& e) {
        return copy_out(log->log.encode_from(version), buf, cap, out_len, false, e);
    });
}
int crdt_hip_oplog_apply_update(crdt_hip_oplog* log, const uint8_t* buf, size_t len) {
    if (!log || (!buf && len)) return null_arg(nullptr);
    return host_msg(CRDT_HIP_EINVAL, [&] { return log->log.apply_update(buf, len); });
}
int crdt_hip_oplog_join(crdt_hip_oplog* dst, const crdt_hip_oplog_view* src, uint32_t* added,
                        uint32_t* tombstoned) {
    if (!dst) return null_arg(nullptr);
    int rc = check_view(nullptr, src);
    if (rc) return rc;
    return host([&](std::string& e) {
        return dst->log.join(src->n, src->parent, src->origin_right, src->lamport, src->agent,
                             src->deleted, src->cp, src->side, added, tombstoned, e);
    });
}

// ---- traces ----------------------------------------------------------------------------------
int crdt_hip_trace_load(const char* path, crdt_hip_trace** out) {
    if (!path || !out) return null_arg(nullptr);
    *out = nullptr;
    return make_handle(nullptr, out, [&](crdt_hip_trace& t) {
        const std::string e = crdt::load_trace(path, t.t);
        return e.empty() ? 0 : set_err(nullptr, CRDT_HIP_EIO, e);
    });
}
void crdt_hip_trace_free(crdt_hip_trace* t) { delete t; }
size_t crdt_hip_trace_len(const crdt_hip_trace* t) { return t ? t->t.len() : 0; }
size_t crdt_hip_trace_txns(const crdt_hip_trace* t) { return t ? t->t.txn_end.size() : 0; }

int crdt_hip_trace_patch(const crdt_hip_trace* t, size_t i, size_t* pos, size_t* del,
                         const char** ins, size_t* ins_len) {
    if (!t || i >= t->t.patches.size()) return set_err(nullptr, CRDT_HIP_ERANGE, "patch index");
    const crdt::Patch& p = t->t.patches[i];
    put(pos, p.pos, del, p.del, ins, t->t.ins.data() + p.ins_off, ins_len, p.ins_len);
    return 0;
}
int crdt_hip_trace_start_content(const crdt_hip_trace* t, const char** s, size_t* len) {
    if (!t || !s || !len) return null_arg(nullptr);
    *s = t->t.start_content.data();
    *len = t->t.start_content.size();
    return 0;
}
int crdt_hip_trace_end_content(const crdt_hip_trace* t, const char** s, size_t* len) {
    if (!t || !s || !len) return null_arg(nullptr);
    *s = t->t.end_content.data();
    *len = t->t.end_content.size();
    return 0;
}
int crdt_hip_trace_chars_to_bytes(crdt_hip_trace* t) {
    if (!t) return null_arg(nullptr);
    return host_msg(CRDT_HIP_ERANGE, [&] { return crdt::chars_to_bytes(t->t); });
}
int crdt_hip_trace_resolve(const crdt_hip_trace* t, crdt_hip_oplog** out) {
    return trace_resolve(t, out, false);
}
int crdt_hip_trace_resolve_fugue(const crdt_hip_trace* t, crdt_hip_oplog** out) {
    return trace_resolve(t, out, true);
}

int crdt_hip_trace_resolve_many(const crdt_hip_trace* const* traces, uint32_t n, uint32_t threads,
                                crdt_hip_oplog** out) {
    if ((n && (!traces || !out))) return null_arg(nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        out[i] = nullptr;
        if (!traces[i]) return set_err(nullptr, CRDT_HIP_EINVAL, "null trace");
    }
    uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
    uint32_t k = threads ? threads : std::min(n, hw);
    k = std::max(1u, std::min(k, n ? n : 1u));
    std::vector<int> rc(n, 0);
    std::vector<std::string> msg(n);
    std::atomic<uint32_t> next{0};
    auto work = [&] {
        for (uint32_t i; (i = next.fetch_add(1)) < n;) {
            rc[i] = crdt_hip_trace_resolve(traces[i], &out[i]);
            if (rc[i]) msg[i] = crdt_hip_last_error(nullptr);  // (thread-local: read it here)
        }
    };
    std::vector<std::thread> pool;
    try {
        pool.reserve(k);
        for (uint32_t j = 1; j < k; ++j) pool.emplace_back(work);
    } catch (...) {
        // no more threads (std::system_error) or no memory: the threads already started and
        // the calling thread share the work; nothing may cross the C ABI
    }
    work();
    for (std::thread& th : pool) th.join();
    for (uint32_t i = 0; i < n; ++i)
        if (rc[i]) {
            for (uint32_t j = 0; j < n; ++j) {
                if (out[j]) crdt_hip_oplog_free(out[j]);
                out[j] = nullptr;
            }
            return set_err(nullptr, rc[i], "trace " + std::to_string(i) + ": " + msg[i]);
        }
    return 0;
}

// ---- binary files ----------------------------------------------------------------------------
int crdt_hip_trace_save(const crdt_hip_trace* t, const char* path) {
    if (!t || !path) return null_arg(nullptr);
    return host_msg(CRDT_HIP_EIO, [&] { return crdt::save_trace_bin(t->t, path); });
}
int crdt_hip_oplog_save(const crdt_hip_oplog* log, const char* path) {
    if (!log || !path) return null_arg(nullptr);
    return host_msg(CRDT_HIP_EIO, [&] { return crdt::save_oplog(log->log, path); });
}
int crdt_hip_oplog_load(const char* path, crdt_hip_oplog** out) {
    if (!path || !out) return null_arg(nullptr);
    *out = nullptr;
    return make_handle(nullptr, out, [&](crdt_hip_oplog& L) {
        const std::string e = crdt::load_oplog(path, L.log);
        return e.empty() ? 0 : set_err(nullptr, CRDT_HIP_EIO, e);
    });
}
int crdt_hip_logfile_open(const char* path, crdt_hip_logfile** out, crdt_hip_oplog_view* view) {
    if (!path || !out || !view) return null_arg(nullptr);
    *out = nullptr;
    return make_handle(nullptr, out, [&](crdt_hip_logfile& f) {
        const std::string e = crdt::map_oplog(path, f.m);
        if (!e.empty()) return set_err(nullptr, CRDT_HIP_EIO, e);
        view->n = f.m.n;
        view->parent = f.m.parent;
        view->origin_right = f.m.oright;
        view->lamport = f.m.lamport;
        view->agent = f.m.agent;
        view->deleted = f.m.deleted;
        view->cp = f.m.cp;
        static const uint8_t kNoSide = 0;  // (an empty Fugue file's view is still Fugue)
        view->side = f.m.fugue ? (f.m.n ? f.m.side : &kNoSide) : nullptr;
        return 0;
    });
}
int crdt_hip_logfile_close(crdt_hip_logfile* f) {
    delete f;
    return 0;
}

// ---- synthetic -------------------------------------------------------------------------------
int crdt_hip_synth_agents(uint32_t n_items, uint32_t agents, uint64_t seed, crdt_hip_oplog** out) {
    if (!out) return set_err(nullptr, CRDT_HIP_EINVAL, "null out");
    return guard(nullptr, [&] { return synth_handle(out, crdt::synth_agents(n_items, agents, seed)); });
}
int crdt_hip_synth_tree_visible(uint32_t n_items, uint32_t del_pct, uint64_t seed, uint64_t* out) {
    if (!out || del_pct > 100) return set_err(nullptr, CRDT_HIP_EINVAL, "bad arguments");
    return guard(nullptr, [&] { *out = crdt::synth_tree_visible(n_items, del_pct, seed); return 0; });
}
int crdt_hip_synth_tree(uint32_t n_items, uint32_t p_chain_pct, uint32_t del_pct, uint64_t seed,
                        crdt_hip_oplog** out) {
    if (!out) return set_err(nullptr, CRDT_HIP_EINVAL, "null out");
    if (p_chain_pct > 100 || del_pct > 100) return set_err(nullptr, CRDT_HIP_EINVAL, "percent > 100");
    return guard(nullptr, [&] {
        return synth_handle(out, crdt::synth_tree(n_items, p_chain_pct, del_pct, seed));
    });
}

// ---- merge -----------------------------------------------------------------------------------
int crdt_hip_merge(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* log, uint8_t* out, size_t cap,
                   size_t* out_len, uint64_t* digest) {
    if (!ctx) return null_ctx();
    return guard(ctx, [&] {
        int rc = stage_views(ctx, log, 1);
        if (rc) return rc;
        std::vector<uint8_t> text;
        uint64_t dig = 0, len = 0;
        rc = ctx->eng.merge(ctx->staging, crdt::Engine::TEXT, &dig, &len, nullptr,
                            out ? &text : nullptr, nullptr);
        if (rc) return from_engine(ctx, rc);
        put(out_len, len, digest, dig);
        return text_out(ctx, text, len, out, cap);
    });
}

int crdt_hip_merge_len(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* log, uint64_t* codepoints,
                       uint64_t* bytes, uint64_t* digest) {
    if (!ctx) return null_ctx();
    return guard(ctx, [&] {
        int rc = stage_views(ctx, log, 1);
        if (rc) return rc;
        uint64_t dig = 0, len = 0, cps = 0;
        rc = ctx->eng.merge(ctx->staging, crdt::Engine::TEXT, &dig, &len, nullptr, nullptr,
                            nullptr, &cps);
        if (rc) return from_engine(ctx, rc);
        put(codepoints, cps, bytes, len, digest, dig);
        return 0;
    });
}

int crdt_hip_merge_batch(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* logs, uint32_t n,
                         uint64_t* digests, uint64_t* lens, crdt_hip_stats* stats) {
    if (!ctx || (!logs && n)) return null_arg(ctx);
    return guard(ctx, [&] {
        if (n == 0) return 0;
        int rc = stage_views(ctx, logs, n);
        if (rc) return rc;
        return from_engine(ctx, ctx->eng.merge(ctx->staging, crdt::Engine::TEXT, digests, lens, stats));
    });
}

int crdt_hip_merge_order(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* log, uint32_t* order) {
    if (!ctx || !order) return null_arg(ctx);
    return guard(ctx, [&] {
        int rc = stage_views(ctx, log, 1);
        if (rc) return rc;
        std::vector<uint8_t> raw;
        rc = ctx->eng.merge(ctx->staging, crdt::Engine::ORDER, nullptr, nullptr, nullptr, &raw, nullptr);
        if (rc) return from_engine(ctx, rc);
        if (raw.size() != (size_t)log->n * 4)
            return set_err(ctx, CRDT_HIP_EBADLOG, "order output size mismatch");
        if (!raw.empty()) std::memcpy(order, raw.data(), raw.size());
        return 0;
    });
}

// ---- resident batches ------------------------------------------------------------------------
int crdt_hip_batch_create(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* bases, uint32_t nbases,
                          uint32_t replicas, uint32_t relabel, uint64_t seed,
                          crdt_hip_batch** out) {
    if (!ctx || !bases || !out || nbases == 0 || replicas == 0)
        return set_err(ctx, CRDT_HIP_EINVAL, "bad batch arguments");
    if (relabel > 2) return set_err(ctx, CRDT_HIP_EINVAL, "relabel must be 0, 1 or 2");
    *out = nullptr;
    return make_handle(ctx, out, [&](crdt_hip_batch& b) {
        int rc = stage_views(ctx, bases, nbases);
        if (rc) return rc;
        b.ctx = ctx;
        rc = from_engine(ctx, ctx->eng.replicate(ctx->staging, b.logs, replicas, relabel, seed));
        b.device_bytes = batch_bytes(b.logs);
        return rc;
    });
}
int crdt_hip_batch_synth_tree(crdt_hip_ctx* ctx, uint32_t n_items, uint32_t p_chain_pct,
                              uint32_t del_pct, uint64_t seed, crdt_hip_batch** out) {
    if (!ctx || !out || p_chain_pct > 100 || del_pct > 100)
        return set_err(ctx, CRDT_HIP_EINVAL, "bad synth arguments");
    *out = nullptr;
    return make_handle(ctx, out, [&](crdt_hip_batch& b) {
        b.ctx = ctx;
        const int rc = from_engine(ctx, ctx->eng.synth_tree(b.logs, n_items, p_chain_pct, del_pct, seed));
        b.device_bytes = batch_bytes(b.logs);
        return rc;
    });
}
int crdt_hip_batch_free(crdt_hip_batch* b) {
    delete b;
    return 0;
}
int crdt_hip_batch_info(const crdt_hip_batch* b, uint64_t* docs, uint64_t* items,
                        uint64_t* device_bytes) {
    if (!b) return set_err(nullptr, CRDT_HIP_EINVAL, "null batch");
    put(docs, b->logs.docs.size(), items, b->logs.items, device_bytes, b->device_bytes);
    return 0;
}
int crdt_hip_batch_merge(crdt_hip_ctx* ctx, crdt_hip_batch* b, uint64_t* digests, uint64_t* lens,
                         crdt_hip_stats* stats) {
    return device(ctx, check_batch(ctx, b),
                  [&] { return ctx->eng.merge(b->logs, crdt::Engine::TEXT, digests, lens, stats); });
}

int crdt_hip_batch_raw(crdt_hip_ctx* ctx, crdt_hip_batch* b, int on) {
    if (int rc = check_batch(ctx, b)) return rc;
    return guard(ctx, [&] {
        if (!on || b->logs.raw_lam) {
            b->logs.raw = on != 0;
            return 0;
        }
        return from_engine(ctx, ctx->eng.raw_keep(b->logs));
    });
}

// ---- device-resident replicas ----------------------------------------------------------------
int crdt_hip_replica_new(crdt_hip_ctx* ctx, const crdt_hip_oplog_view* init,
                         crdt_hip_replica** out) {
    if (!ctx || !out) return null_arg(ctx);
    *out = nullptr;
    if (init) {
        int rc = check_view(ctx, init);
        if (rc) return rc;
    }
    return make_handle(ctx, out, [&](crdt_hip_replica& r) {
        r.ctx = ctx;
        return from_engine(ctx, crdt::replica_upload(ctx->eng, r.r, init));
    });
}
int crdt_hip_replica_clone(crdt_hip_ctx* ctx, const crdt_hip_replica* src,
                           crdt_hip_replica** out) {
    if (int rc = check_replica(ctx, src, out)) return rc;
    *out = nullptr;
    return make_handle(ctx, out, [&](crdt_hip_replica& r) {
        r.ctx = ctx;
        return from_engine(ctx, crdt::replica_copy(ctx->eng, src->r, r.r));
    });
}

int crdt_hip_replica_free(crdt_hip_replica* r) {
    if (r) drop_replays(r->ctx, &r->r, nullptr);
    delete r;
    return 0;
}
int crdt_hip_replica_apply_updates(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint8_t* buf,
                                   size_t len, const uint64_t* offsets, uint32_t n) {
    return device(ctx, check_replica(ctx, r), [&] { return crdt::replica_apply(ctx->eng, r->r, buf, len, offsets, n); });
}
int crdt_hip_updates_upload(crdt_hip_ctx* ctx, const uint8_t* buf, size_t len,
                            const uint64_t* offsets, uint32_t n, crdt_hip_updates** out) {
    if (!ctx || !out) return null_arg(ctx);
    return make_handle(ctx, out, [&](crdt_hip_updates& u) {
        u.ctx = ctx;
        return from_engine(ctx, crdt::updates_upload(ctx->eng, u.u, buf, len, offsets, n));
    });
}
int crdt_hip_updates_free(crdt_hip_updates* u) {
    if (u) drop_replays(u->ctx, nullptr, &u->u);
    delete u;
    return 0;
}

int crdt_hip_replica_replay(crdt_hip_ctx* ctx, const crdt_hip_replica* init,
                            const crdt_hip_updates* u, uint64_t* codepoints, uint64_t* bytes,
                            uint64_t* digest) {
    if (int rc = check_replica_updates(ctx, init, u)) return rc;
    return guard(ctx, [&] {
        auto& v = ctx->replays;
        size_t i = 0;
        while (i < v.size() && !(v[i]->init == &init->r && v[i]->ub == &u->u)) ++i;
        if (i == v.size()) {
            if (v.size() >= 8) v.pop_back();
            v.insert(v.begin(), std::make_unique<crdt::ReplayState>());
            i = 0;
        }
        uint64_t c = 0, b = 0, d = 0;
        const int rc = crdt::replica_replay(ctx->eng, init->r, u->u, *v[i], &c, &b, &d);
        if (rc) return from_engine(ctx, rc);
        put(codepoints, c, bytes, b, digest, d);
        return 0;
    });
}
int crdt_hip_replica_apply_resident(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                    const crdt_hip_updates* u) {
    return device(ctx, check_replica_updates(ctx, r, u),
                  [&] { return crdt::replica_apply_resident(ctx->eng, r->r, u->u); });
}
int crdt_hip_replica_join(crdt_hip_ctx* ctx, crdt_hip_replica* dst, const crdt_hip_replica* src,
                          uint32_t* added, uint32_t* tombstoned) {
    if (int rc = check_replica(ctx, src, dst)) return rc;
    return device(ctx, check_replica(ctx, dst), [&] {
        return crdt::replica_join(ctx->eng, dst->r, src->r, added, tombstoned, &ctx->last_join);
    });
}
int crdt_hip_join_stats(const crdt_hip_ctx* ctx, uint64_t* prefix_slots, uint64_t* table_slots,
                        uint64_t* table_capacity, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::JoinStats& s = ctx->last_join;
    put(prefix_slots, s.prefix, table_slots, s.table_slots, table_capacity, s.table_cap, device_ns,
        s.device_ns);
    return 0;
}
// ---- state-vector delta sync ---------------------------------------------------------------------
int crdt_hip_oplog_state_vector(const crdt_hip_oplog* log, crdt_hip_sv_entry* out, size_t cap,
                                size_t* out_n) {
    if (!log || !out_n) return null_arg(nullptr);
    return host([&](std::string& e) { return copy_out(log->log.state_vector(), out, cap, out_n, true, e); });
}
int crdt_hip_oplog_encode_diff(const crdt_hip_oplog* log, const crdt_hip_sv_entry* sv, size_t nsv,
                               uint8_t* buf, size_t cap, size_t* out_len) {
    if (!log || !out_len || (!sv && nsv)) return null_arg(nullptr);
    return host([&](std::string& e) {
        std::vector<uint8_t> d;
        if (int rc = log->log.encode_diff(reinterpret_cast<const crdt::SvEntry*>(sv), nsv, d, e)) return rc;
        return copy_out(d, buf, cap, out_len, false, e);
    });
}
int crdt_hip_oplog_apply_diff(crdt_hip_oplog* log, const uint8_t* buf, size_t len, uint32_t* added,
                              uint32_t* tombstoned) {
    if (!log || (!buf && len)) return null_arg(nullptr);
    return host([&](std::string& e) { return log->log.apply_diff(buf, len, added, tombstoned, e); });
}
int crdt_hip_replica_state_vector(crdt_hip_ctx* ctx, const crdt_hip_replica* r,
                                  crdt_hip_sv_entry* out, size_t cap, size_t* out_n) {
    std::vector<crdt::SvEntry> sv;
    return device(
        ctx, check_replica(ctx, r, out_n), [&] { return crdt::replica_state_vector(ctx->eng, r->r, sv); },
        [&] {
            std::string e;
            const int rc = copy_out(sv, out, cap, out_n, true, e);
            return rc ? set_err(ctx, rc, e) : 0;
        });
}
int crdt_hip_replica_encode_diff(crdt_hip_ctx* ctx, const crdt_hip_replica* r,
                                 const crdt_hip_sv_entry* sv, size_t nsv, uint8_t* buf, size_t cap,
                                 size_t* out_len) {
    return device(ctx, check_replica(ctx, r, out_len && (sv || !nsv)), [&] {
        return crdt::replica_encode_diff(ctx->eng, r->r, reinterpret_cast<const crdt::SvEntry*>(sv), nsv,
                                         buf, cap, out_len, &ctx->last_delta);
    });
}
int crdt_hip_replica_apply_diff(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint8_t* buf,
                                size_t len, uint32_t* added, uint32_t* tombstoned) {
    return device(ctx, check_replica(ctx, r, buf || !len), [&] {
        return crdt::replica_apply_diff(ctx->eng, r->r, buf, len, added, tombstoned, &ctx->last_delta);
    });
}
int crdt_hip_delta_stats(const crdt_hip_ctx* ctx, uint64_t* items, uint64_t* ranges,
                         uint64_t* table_slots, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::DeltaStats& s = ctx->last_delta;
    put(items, s.items, ranges, s.ranges, table_slots, s.table_slots, device_ns, s.device_ns);
    return 0;
}
// ---- patches since a mark ------------------------------------------------------------------------
static_assert(sizeof(crdt_hip_patch) == sizeof(crdt::PatchRec) && sizeof(crdt_hip_patch) == 24,
              "patch layout");
int crdt_hip_oplog_mark(const crdt_hip_oplog* log, crdt_hip_mark** out) {
    if (!log || !out) return null_arg(nullptr);
    *out = nullptr;
    return make_handle(nullptr, out, [&](crdt_hip_mark& m) {
        m.owner = log->uid;
        m.host = log->log.mark();
        return 0;
    });
}
void crdt_hip_mark_free(crdt_hip_mark* m) { delete m; }
int crdt_hip_oplog_patches_since(crdt_hip_oplog* log, const crdt_hip_mark* m, crdt_hip_patch* out,
                                 size_t cap, size_t* out_n, uint8_t* ins, size_t ins_cap,
                                 size_t* out_ins) {
    return oplog_patches_since(log, m, out, cap, out_n, ins, ins_cap, out_ins, false);
}
int crdt_hip_replica_mark(crdt_hip_ctx* ctx, crdt_hip_replica* r, crdt_hip_mark** out) {
    if (!ctx || !r || !out) return null_arg(ctx);
    *out = nullptr;
    if (int rc = check_replica(ctx, r)) return rc;
    return make_handle(ctx, out, [&](crdt_hip_mark& m) {
        m.owner = r->uid;
        m.ctx = ctx;
        return from_engine(ctx, crdt::replica_mark(ctx->eng, r->r, m.dev));
    });
}
int crdt_hip_replica_patches_since(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                                   crdt_hip_patch* out, size_t cap, size_t* out_n, uint8_t* ins,
                                   size_t ins_cap, size_t* out_ins) {
    return replica_patches_since(ctx, r, m, out, cap, out_n, ins, ins_cap, out_ins, false);
}
int crdt_hip_patch_stats(const crdt_hip_ctx* ctx, uint64_t* patches, uint64_t* ins_bytes,
                         uint64_t* ranks, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::PatchStats& s = ctx->last_patch;
    put(patches, s.patches, ins_bytes, s.ins_bytes, ranks, s.ranks, device_ns, s.device_ns);
    return 0;
}
// ---- local edits: positional patches into a log or a replica ---------------------------------------
int crdt_hip_oplog_apply_patches(crdt_hip_oplog* log, const crdt_hip_patch* p, size_t n,
                                 const uint8_t* ins, size_t ins_len, uint32_t* added,
                                 uint32_t* tombstoned) {
    return oplog_apply_patches(log, p, n, ins, ins_len, added, tombstoned, false);
}
int crdt_hip_replica_set_agent(crdt_hip_replica* r, uint16_t agent) {
    if (!r) return set_err(nullptr, CRDT_HIP_EINVAL, "null replica");
    r->r.agent = agent;
    return 0;
}
int crdt_hip_replica_apply_patches(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_patch* p,
                                   size_t n, const uint8_t* ins, size_t ins_len, uint32_t* added,
                                   uint32_t* tombstoned) {
    return replica_apply_patches(ctx, r, p, n, ins, ins_len, added, tombstoned, false);
}
// Upstream::replace (rope.rs:21-32), as crdt_hip_oplog_replace: remove if end > start, insert if
// the text is non-empty, nothing otherwise
int crdt_hip_replica_replace(crdt_hip_ctx* ctx, crdt_hip_replica* r, size_t start, size_t end,
                             const char* utf8, size_t nbytes) {
    return replica_replace(ctx, r, start, end, utf8, nbytes, false);
}
int crdt_hip_edit_stats(const crdt_hip_ctx* ctx, uint64_t* patches, uint64_t* items,
                        uint64_t* tombstones, uint64_t* ranks, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::EditStats& s = ctx->last_edit;
    put(patches, s.patches, items, s.items, tombstones, s.tombstones, ranks, s.ranks, device_ns,
        s.device_ns);
    return 0;
}
// ---- byte offsets: the same patches with pos and del in UTF-8 bytes ---------------------------------
int crdt_hip_oplog_apply_patches_bytes(crdt_hip_oplog* log, const crdt_hip_patch* p, size_t n,
                                       const uint8_t* ins, size_t ins_len, uint32_t* added,
                                       uint32_t* tombstoned) {
    return oplog_apply_patches(log, p, n, ins, ins_len, added, tombstoned, true);
}
int crdt_hip_oplog_replace_bytes(crdt_hip_oplog* log, size_t start, size_t end, const char* utf8,
                                 size_t nbytes) {
    if (!log || (!utf8 && nbytes)) return null_arg(nullptr);
    return replace_as_patch(nullptr, start, end, nbytes, kReplaceBytes, [&](const crdt_hip_patch* one) {
        return oplog_apply_patches(log, one, 1, u8(utf8), nbytes, nullptr, nullptr, true);
    });
}
int crdt_hip_oplog_patches_since_bytes(crdt_hip_oplog* log, const crdt_hip_mark* m,
                                       crdt_hip_patch* out, size_t cap, size_t* out_n, uint8_t* ins,
                                       size_t ins_cap, size_t* out_ins) {
    return oplog_patches_since(log, m, out, cap, out_n, ins, ins_cap, out_ins, true);
}
int crdt_hip_replica_apply_patches_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_patch* p, size_t n, const uint8_t* ins,
                                         size_t ins_len, uint32_t* added, uint32_t* tombstoned) {
    return replica_apply_patches(ctx, r, p, n, ins, ins_len, added, tombstoned, true);
}
int crdt_hip_replica_replace_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r, size_t start, size_t end,
                                   const char* utf8, size_t nbytes) {
    return replica_replace(ctx, r, start, end, utf8, nbytes, true);
}
int crdt_hip_replica_patches_since_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_mark* m, crdt_hip_patch* out, size_t cap,
                                         size_t* out_n, uint8_t* ins, size_t ins_cap,
                                         size_t* out_ins) {
    return replica_patches_since(ctx, r, m, out, cap, out_n, ins, ins_cap, out_ins, true);
}
// ---- text windows: a range of the document, now or at a mark ---------------------------------------
static_assert(sizeof(crdt_hip_text_info) == sizeof(crdt::TextInfo) && sizeof(crdt_hip_text_info) == 48 &&
                  CRDT_HIP_TEXT_END == crdt::kTextEnd && CRDT_HIP_TEXT_BYTES == crdt::kTextBytes,
              "text info layout");
int crdt_hip_oplog_text_at(crdt_hip_oplog* log, const crdt_hip_mark* m, uint64_t start, uint64_t end,
                           uint32_t flags, uint8_t* out, size_t cap, size_t* out_len,
                           crdt_hip_text_info* info) {
    if (int rc = check_log_mark(log, m, true, true)) return rc;
    return host([&](std::string& e) {
        return log->log.text_at(m ? &m->host : nullptr, start, end, flags, out, cap, out_len,
                                reinterpret_cast<crdt::TextInfo*>(info), e);
    });
}
int crdt_hip_replica_text_at(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                             uint64_t start, uint64_t end, uint32_t flags, uint8_t* out, size_t cap,
                             size_t* out_len, crdt_hip_text_info* info) {
    return device(ctx, check_replica_mark(ctx, r, m, true, true), [&] {
        return crdt::replica_text_at(ctx->eng, r->r, m ? &m->dev : nullptr, start, end, flags, out, cap,
                                     out_len, reinterpret_cast<crdt::TextInfo*>(info), &ctx->last_text);
    });
}
int crdt_hip_text_stats(const crdt_hip_ctx* ctx, uint64_t* ranks, uint64_t* tiles_written,
                        uint64_t* bytes, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::TextStats& s = ctx->last_text;
    put(ranks, s.ranks, tiles_written, s.tiles_written, bytes, s.bytes, device_ns, s.device_ns);
    return 0;
}
// ---- the line index (crdt_hip_lines.h): line starts, and line / column of positions -----------------
static_assert(sizeof(crdt_hip_line_pos) == sizeof(crdt::LinePos) && sizeof(crdt_hip_line_pos) == 40 &&
                  sizeof(crdt_hip_line_info) == sizeof(crdt::LineInfo) && sizeof(crdt_hip_line_info) == 24,
              "line layouts");
int crdt_hip_oplog_line_starts(crdt_hip_oplog* log, const crdt_hip_mark* m, const uint64_t* lines,
                               size_t n, crdt_hip_line_pos* out, crdt_hip_line_info* info) {
    if (int rc = check_log_mark(log, m, true, true)) return rc;
    return host([&](std::string& e) {
        return log->log.line_starts(m ? &m->host : nullptr, lines, n, reinterpret_cast<crdt::LinePos*>(out),
                                    reinterpret_cast<crdt::LineInfo*>(info), e);
    });
}
int crdt_hip_oplog_lines_of(crdt_hip_oplog* log, const crdt_hip_mark* m, const uint64_t* pos, size_t n,
                            uint32_t flags, crdt_hip_line_pos* out, crdt_hip_line_info* info) {
    if (int rc = check_log_mark(log, m, true, true)) return rc;
    return host([&](std::string& e) {
        return log->log.lines_of(m ? &m->host : nullptr, pos, n, flags, reinterpret_cast<crdt::LinePos*>(out),
                                 reinterpret_cast<crdt::LineInfo*>(info), e);
    });
}
int crdt_hip_replica_line_starts(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                                 const uint64_t* lines, size_t n, crdt_hip_line_pos* out,
                                 crdt_hip_line_info* info) {
    return device(ctx, check_replica_mark(ctx, r, m, true, true), [&] {
        return crdt::replica_lines(ctx->eng, r->r, m ? &m->dev : nullptr, false, lines, n, 0,
                                   reinterpret_cast<crdt::LinePos*>(out),
                                   reinterpret_cast<crdt::LineInfo*>(info), &ctx->last_line);
    });
}
int crdt_hip_replica_lines_of(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                              const uint64_t* pos, size_t n, uint32_t flags, crdt_hip_line_pos* out,
                              crdt_hip_line_info* info) {
    return device(ctx, check_replica_mark(ctx, r, m, true, true), [&] {
        return crdt::replica_lines(ctx->eng, r->r, m ? &m->dev : nullptr, true, pos, n, flags,
                                   reinterpret_cast<crdt::LinePos*>(out),
                                   reinterpret_cast<crdt::LineInfo*>(info), &ctx->last_line);
    });
}
int crdt_hip_line_stats(const crdt_hip_ctx* ctx, uint64_t* queries, uint64_t* ranks, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::LineStats& s = ctx->last_line;
    put(queries, s.queries, ranks, s.ranks, device_ns, s.device_ns);
    return 0;
}
// ---- UTF-16 positions (crdt_hip_utf16.h): a gap in three units, edits and patches in UTF-16 --------
static_assert(sizeof(crdt_hip_unit_pos) == sizeof(crdt::UnitPos) && sizeof(crdt_hip_unit_pos) == 24 &&
                  sizeof(crdt_hip_unit_info) == sizeof(crdt::UnitInfo) && sizeof(crdt_hip_unit_info) == 24 &&
                  CRDT_HIP_UNIT_CODEPOINTS == crdt::kUnitCodepoints && CRDT_HIP_UNIT_BYTES == crdt::kUnitBytes &&
                  CRDT_HIP_UNIT_BYTES == CRDT_HIP_TEXT_BYTES && CRDT_HIP_UNIT_UTF16 == crdt::kUnitUtf16,
              "unit layouts");
int crdt_hip_oplog_units_of(crdt_hip_oplog* log, const crdt_hip_mark* m, const uint64_t* pos, size_t n,
                            uint32_t unit, crdt_hip_unit_pos* out, crdt_hip_unit_info* info) {
    if (int rc = check_log_mark(log, m, true, true)) return rc;
    return host([&](std::string& e) {
        return log->log.units_of(m ? &m->host : nullptr, pos, n, unit, reinterpret_cast<crdt::UnitPos*>(out),
                                 reinterpret_cast<crdt::UnitInfo*>(info), e);
    });
}
int crdt_hip_replica_units_of(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_mark* m,
                              const uint64_t* pos, size_t n, uint32_t unit, crdt_hip_unit_pos* out,
                              crdt_hip_unit_info* info) {
    return device(ctx, check_replica_mark(ctx, r, m, true, true), [&] {
        return crdt::replica_units(ctx->eng, r->r, m ? &m->dev : nullptr, unit, pos, n,
                                   reinterpret_cast<crdt::UnitPos*>(out),
                                   reinterpret_cast<crdt::UnitInfo*>(info), &ctx->last_unit);
    });
}
int crdt_hip_oplog_apply_patches_utf16(crdt_hip_oplog* log, const crdt_hip_patch* p, size_t n,
                                       const uint8_t* ins, size_t ins_len, uint32_t* added,
                                       uint32_t* tombstoned) {
    if (!log || (!p && n) || (!ins && ins_len)) return null_arg(nullptr);
    return host([&](std::string& e) {
        return log->log.apply_patches_utf16(reinterpret_cast<const PatchRec*>(p), n, ins, ins_len, added,
                                            tombstoned, e);
    });
}
constexpr const char* kReplaceUtf16 = "replace of 2^32 or more UTF-16 code units or bytes";
int crdt_hip_oplog_replace_utf16(crdt_hip_oplog* log, size_t start, size_t end, const char* utf8,
                                 size_t nbytes) {
    if (!log || (!utf8 && nbytes)) return null_arg(nullptr);
    return replace_as_patch(nullptr, start, end, nbytes, kReplaceUtf16, [&](const crdt_hip_patch* one) {
        return crdt_hip_oplog_apply_patches_utf16(log, one, 1, u8(utf8), nbytes, nullptr, nullptr);
    });
}
int crdt_hip_oplog_patches_since_utf16(crdt_hip_oplog* log, const crdt_hip_mark* m,
                                       crdt_hip_patch* out, size_t cap, size_t* out_n, uint8_t* ins,
                                       size_t ins_cap, size_t* out_ins) {
    if (int rc = check_log_mark(log, m, out_n && out_ins)) return rc;
    return host([&](std::string& e) {
        std::vector<PatchRec> p;
        std::vector<uint8_t> text;
        if (int rc = log->log.patches_since_utf16(m->host, p, text, e)) return rc;
        return copy_out2(p, out, cap, out_n, text, ins, ins_cap, out_ins, false, e);
    });
}
int crdt_hip_replica_apply_patches_utf16(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_patch* p, size_t n, const uint8_t* ins,
                                         size_t ins_len, uint32_t* added, uint32_t* tombstoned) {
    return device(ctx, check_replica(ctx, r, (p || !n) && (ins || !ins_len)), [&] {
        return crdt::replica_apply_patches_utf16(ctx->eng, r->r, reinterpret_cast<const PatchRec*>(p), n, ins,
                                                 ins_len, added, tombstoned, &ctx->last_edit,
                                                 &ctx->last_unit);
    });
}
int crdt_hip_replica_replace_utf16(crdt_hip_ctx* ctx, crdt_hip_replica* r, size_t start, size_t end,
                                   const char* utf8, size_t nbytes) {
    if (int rc = check_replica(ctx, r, utf8 || !nbytes)) return rc;
    return replace_as_patch(ctx, start, end, nbytes, kReplaceUtf16, [&](const crdt_hip_patch* one) {
        return crdt_hip_replica_apply_patches_utf16(ctx, r, one, 1, u8(utf8), nbytes, nullptr, nullptr);
    });
}
int crdt_hip_replica_patches_since_utf16(crdt_hip_ctx* ctx, crdt_hip_replica* r,
                                         const crdt_hip_mark* m, crdt_hip_patch* out, size_t cap,
                                         size_t* out_n, uint8_t* ins, size_t ins_cap,
                                         size_t* out_ins) {
    return device(ctx, check_replica_mark(ctx, r, m, out_n && out_ins), [&] {
        return crdt::replica_patches_since_utf16(ctx->eng, r->r, m->dev, reinterpret_cast<PatchRec*>(out), cap,
                                                 out_n, ins, ins_cap, out_ins, &ctx->last_patch,
                                                 &ctx->last_unit);
    });
}
int crdt_hip_unit_stats(const crdt_hip_ctx* ctx, uint64_t* queries, uint64_t* ranks, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::UnitStats& s = ctx->last_unit;
    put(queries, s.queries, ranks, s.ranks, device_ns, s.device_ns);
    return 0;
}
// ---- anchors: cursor and selection positions that survive sync --------------------------------------
static_assert(sizeof(crdt_hip_anchor) == sizeof(crdt::AnchorRec) && sizeof(crdt_hip_anchor) == 16 &&
                  sizeof(crdt_hip_anchor_pos) == sizeof(crdt::AnchorPosRec) &&
                  sizeof(crdt_hip_anchor_pos) == 24,
              "anchor layouts");
int crdt_hip_oplog_anchors_at(crdt_hip_oplog* log, const uint64_t* pos, const uint8_t* bias, size_t n,
                              crdt_hip_anchor* out) {
    return oplog_anchors_at(log, pos, bias, n, false, out);
}
int crdt_hip_oplog_anchors_at_bytes(crdt_hip_oplog* log, const uint64_t* pos, const uint8_t* bias,
                                    size_t n, crdt_hip_anchor* out) {
    return oplog_anchors_at(log, pos, bias, n, true, out);
}
int crdt_hip_oplog_anchors_resolve(crdt_hip_oplog* log, const crdt_hip_anchor* a, size_t n,
                                   crdt_hip_anchor_pos* out) {
    if (!log || ((!a || !out) && n)) return null_arg(nullptr);
    return host([&](std::string& e) {
        return log->log.anchors_resolve(reinterpret_cast<const crdt::AnchorRec*>(a), n,
                                        reinterpret_cast<crdt::AnchorPosRec*>(out), e);
    });
}
int crdt_hip_replica_anchors_at(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint64_t* pos,
                                const uint8_t* bias, size_t n, crdt_hip_anchor* out) {
    return replica_anchors_at(ctx, r, pos, bias, n, false, out);
}
int crdt_hip_replica_anchors_at_bytes(crdt_hip_ctx* ctx, crdt_hip_replica* r, const uint64_t* pos,
                                      const uint8_t* bias, size_t n, crdt_hip_anchor* out) {
    return replica_anchors_at(ctx, r, pos, bias, n, true, out);
}
int crdt_hip_replica_anchors_resolve(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_anchor* a,
                                     size_t n, crdt_hip_anchor_pos* out) {
    return device(ctx, check_replica(ctx, r, (a && out) || !n), [&] {
        return crdt::replica_anchors_resolve(ctx->eng, r->r, reinterpret_cast<const crdt::AnchorRec*>(a), n,
                                             reinterpret_cast<crdt::AnchorPosRec*>(out), &ctx->last_anchor);
    });
}
int crdt_hip_anchor_stats(const crdt_hip_ctx* ctx, uint64_t* anchors, uint64_t* unknown,
                          uint64_t* ranks, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::AnchorStats& s = ctx->last_anchor;
    put(anchors, s.anchors, unknown, s.unknown, ranks, s.ranks, device_ns, s.device_ns);
    return 0;
}
// ---- formats: rich-text attribute ranges on anchors, flattened into spans ---------------------------
static_assert(sizeof(crdt_hip_format) == sizeof(crdt::FormatRec) && sizeof(crdt_hip_format) == 56 &&
                  sizeof(crdt_hip_span) == sizeof(crdt::SpanRec) && sizeof(crdt_hip_span) == 40 &&
                  sizeof(crdt_hip_span_attr) == sizeof(crdt::SpanAttrRec) &&
                  sizeof(crdt_hip_span_attr) == 16,
              "format layouts");
int crdt_hip_oplog_spans(crdt_hip_oplog* log, const crdt_hip_format* f, size_t n, crdt_hip_span* out,
                         size_t cap, size_t* out_n, crdt_hip_span_attr* attrs, size_t attr_cap,
                         size_t* out_attrs, size_t* pending) {
    if (!log || (!f && n) || !out_n || !out_attrs || !pending) return null_arg(nullptr);
    return host([&](std::string& e) {
        std::vector<crdt::SpanRec> sp;
        std::vector<crdt::SpanAttrRec> at;
        uint64_t pend = 0;
        if (int rc = log->log.spans(reinterpret_cast<const crdt::FormatRec*>(f), n, sp, at, pend, e)) return rc;
        if (int rc = copy_out2(sp, out, cap, out_n, at, attrs, attr_cap, out_attrs, true, e)) return rc;
        *pending = (size_t)pend;
        return 0;
    });
}
int crdt_hip_replica_spans(crdt_hip_ctx* ctx, crdt_hip_replica* r, const crdt_hip_format* f, size_t n,
                           crdt_hip_span* out, size_t cap, size_t* out_n, crdt_hip_span_attr* attrs,
                           size_t attr_cap, size_t* out_attrs, size_t* pending) {
    return device(ctx, check_replica(ctx, r, (f || !n) && out_n && out_attrs && pending), [&] {
        return crdt::replica_spans(ctx->eng, r->r, reinterpret_cast<const crdt::FormatRec*>(f), n,
                                   reinterpret_cast<crdt::SpanRec*>(out), cap, out_n,
                                   reinterpret_cast<crdt::SpanAttrRec*>(attrs), attr_cap, out_attrs,
                                   pending, &ctx->last_format);
    });
}
int crdt_hip_format_stats(const crdt_hip_ctx* ctx, uint64_t* formats, uint64_t* pending,
                          uint64_t* segments, uint64_t* spans, uint64_t* ranks, uint64_t* device_ns) {
    if (!ctx) return null_ctx();
    const crdt::FormatStats& s = ctx->last_format;
    put(formats, s.formats, pending, s.pending, segments, s.segments, spans, s.spans, ranks, s.ranks,
        device_ns, s.device_ns);
    return 0;
}
int crdt_hip_replica_info(const crdt_hip_replica* r, uint64_t* items,
                          uint64_t* visible_codepoints, uint64_t* visible_bytes) {
    if (!r) return set_err(nullptr, CRDT_HIP_EINVAL, "null replica");
    put(items, r->r.n, visible_codepoints, r->r.vis_cp, visible_bytes, r->r.vis_bytes);
    return 0;
}
int crdt_hip_replica_merge(crdt_hip_ctx* ctx, crdt_hip_replica* r, uint8_t* out, size_t cap,
                           size_t* out_len, uint64_t* digest) {
    std::vector<uint8_t> text;
    uint64_t len = 0, dig = 0;
    return device(
        ctx, check_replica(ctx, r),
        [&] { return crdt::replica_merge(ctx->eng, r->r, out ? &text : nullptr, &len, &dig, nullptr); },
        [&] {
            put(out_len, len, digest, dig);
            return text_out(ctx, text, len, out, cap);
        });
}

int crdt_hip_replica_merge_len(crdt_hip_ctx* ctx, crdt_hip_replica* r, uint64_t* codepoints,
                               uint64_t* bytes, uint64_t* digest) {
    uint64_t len = 0, dig = 0, cps = 0;
    return device(
        ctx, check_replica(ctx, r),
        [&] { return crdt::replica_merge(ctx->eng, r->r, nullptr, &len, &dig, nullptr, &cps); },
        [&] {
            put(codepoints, cps, bytes, len, digest, dig);
            return 0;
        });
}

int crdt_hip_replica_merge_inc(crdt_hip_ctx* ctx, crdt_hip_replica* r, uint8_t* out, size_t cap,
                               size_t* out_len, uint64_t* codepoints, uint32_t* path) {
    std::vector<uint8_t> text;
    uint64_t len = 0, cps = 0;
    uint32_t p = 0;
    return device(
        ctx, check_replica(ctx, r),
        [&] { return crdt::replica_merge_inc(ctx->eng, r->r, out ? &text : nullptr, &len, &cps, &p); },
        [&] {
            put(out_len, len, codepoints, cps, path, p);
            return text_out(ctx, text, len, out, cap);
        });
}

// ---- RCCL ------------------------------------------------------------------------------------
int crdt_hip_comm_unique_id(uint8_t id[128]) {
    if (!id) return set_err(nullptr, CRDT_HIP_EINVAL, "null id");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return set_err(nullptr, CRDT_HIP_ECOMM, ncclGetErrorString(r));
    std::memcpy(id, &u, 128);
    return 0;
}
int crdt_hip_comm_init(crdt_hip_ctx* ctx, int nranks, int rank, const uint8_t id[128]) {
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks)
        return set_err(ctx, CRDT_HIP_EINVAL, "bad comm arguments");
    if (hipSetDevice(ctx->eng.device) != hipSuccess)
        return set_err(ctx, CRDT_HIP_EDEVICE, "hipSetDevice failed");
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
    ncclResult_t r = ncclCommInitRank(&ctx->comm, nranks, u, rank);
    if (r != ncclSuccess) return set_err(ctx, CRDT_HIP_ECOMM, ncclGetErrorString(r));
    ctx->nranks = nranks;
    ctx->rank = rank;
    return 0;
}
int crdt_hip_allgather_u64(crdt_hip_ctx* ctx, const uint64_t* send, size_t count, uint64_t* recv) {
    if (!ctx || !ctx->comm || (!send && count) || (!recv && count))
        return set_err(ctx, CRDT_HIP_EINVAL, "comm not initialised or null buffer");
    if (count == 0) return 0;
    uint64_t *ds = nullptr, *dr = nullptr;
    hipStream_t s = ctx->eng.stream;
    auto cleanup = [&] {
        if (ds) (void)hipFree(ds);
        if (dr) (void)hipFree(dr);
    };
    if (hipMalloc(&ds, count * 8) != hipSuccess ||
        hipMalloc(&dr, count * 8 * (size_t)ctx->nranks) != hipSuccess) {
        cleanup();
        return set_err(ctx, CRDT_HIP_ENOMEM, "device allocation for all-gather");
    }
    hipError_t e = hipMemcpyAsync(ds, send, count * 8, hipMemcpyHostToDevice, s);
    ncclResult_t r = ncclSuccess;
    if (e == hipSuccess) r = ncclAllGather(ds, dr, count, ncclUint64, ctx->comm, s);
    if (e == hipSuccess && r == ncclSuccess)
        e = hipMemcpyAsync(recv, dr, count * 8 * (size_t)ctx->nranks, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    cleanup();
    if (r != ncclSuccess) return set_err(ctx, CRDT_HIP_ECOMM, ncclGetErrorString(r));
    if (e != hipSuccess) return set_err(ctx, CRDT_HIP_EDEVICE, hipGetErrorString(e));
    return 0;
}
int crdt_hip_comm_destroy(crdt_hip_ctx* ctx) {
    if (!ctx) return 0;
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
    return 0;
}

// ---- helpers ---------------------------------------------------------------------------------
uint64_t crdt_hip_xxh64(const void* data, size_t len, uint64_t seed) { return crdt::xxh64(data, len, seed); }
uint64_t crdt_hip_tree_digest(const uint8_t* text, size_t len) { return crdt::tree_digest(text, len); }

}  // extern "C"
