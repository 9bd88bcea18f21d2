"""The C-ABI library loads and exports every symbol include/crdt_hip.h declares (CPU only)."""
import ctypes as C
import sys
import os
import re

import numpy as np
import pytest

import crdt_hip
from conftest import ROOT


def header_functions():
    with open(os.path.join(ROOT, "include", "crdt_hip.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(crdt_hip_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported():
    L = crdt_hip.lib()
    declared = header_functions()
    assert len(declared) >= 40
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(crdt_hip.EXPORTS) == declared


def test_abi_version():
    assert crdt_hip.lib().crdt_hip_abi_version() == 2


def test_library_is_native_gfx950():
    so = crdt_hip.LIB_PATH
    with open(so, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob, "libcrdt_hip.so carries no gfx950 code object"


def test_device_count_does_not_crash():
    n = crdt_hip.device_count()
    assert n >= 0


def test_errors_are_codes_not_crashes():
    L = crdt_hip.lib()
    h = C.c_void_p()
    rc = L.crdt_hip_trace_load(b"/nonexistent.json.gz", C.byref(h))
    assert rc == -7
    assert b"cannot open" in L.crdt_hip_last_error(None)
    log = crdt_hip.OpLog()
    try:
        log.insert(5, "x")
        raise AssertionError("expected ERANGE")
    except crdt_hip.CrdtHipError as e:
        assert e.code == -2
    assert L.crdt_hip_set_param(None, b"splitter_stride", 64) == -1


def test_host_digest_helpers_match_oracle(oracle):
    data = bytes(range(256)) * 50
    assert crdt_hip.xxh64(data, 7) == oracle.xxh64(data, 7)
    assert crdt_hip.tree_digest(data) == oracle.tree_digest(data)
    assert crdt_hip.tree_digest(b"") == oracle.tree_digest(b"")


def test_tree_digest_groups_above_16mib(oracle):
    """Documents of more than 4096 leaves hash their leaf digests in groups of 4096: the host
    library, the oracle and the pure-Python restatement (make_golden.py) agree."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import tree_digest as py_tree_digest
    rng = np.random.default_rng(3)
    for n in (4096 * 4096, 4096 * 4096 + 1, 20_000_003):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        d = crdt_hip.tree_digest(data)
        assert d == oracle.tree_digest(data) == py_tree_digest(data), n


# ---- the boundary's contract: which call refuses what, with which code and which text -----------
# Every refusal of a crdt_hip_oplog_*, crdt_hip_trace_* and crdt_hip_mark_* entry point that needs
# no device: the code and the exact crdt_hip_last_error(NULL) text, as include/crdt_hip.h states
# them.  (A replica's mark passed to a log needs a device: tests/test_gpu_abi_contract.py.)
EINVAL, ERANGE, ESPACE, EIO = -1, -2, -6, -7
NULLARG = "null argument"
SMALL = "buffer too small"
OTHER_LOG = "the mark belongs to another log"
SENTINEL = 0xA5


class _Doc:
    """A four-item log "abcd" marked, then edited into two patches ("Xbcd" + "YZ" at the end), a
    clone (another owner) with its own mark, an empty log, two formats, a trace."""

    def __init__(self):
        L = self.L = crdt_hip.lib()
        self.log = crdt_hip.OpLog()
        self.log.insert(0, "abcd")
        self.mark = self.log.mark()
        self.other = self.log.clone()
        self.other_mark = self.other.mark()
        self.log.replace(0, 1, "X")
        self.log.insert(4, "YZ")
        self.empty = crdt_hip.OpLog()
        a = self.log.anchors_at([0, 2, 2, 6], [crdt_hip.BEFORE, crdt_hip.AFTER] * 2)
        self.formats = crdt_hip._formats_pack([(a[0], a[1], 1, 7, 1 << 16, 0),
                                               (a[2], a[3], 2, 9, 2 << 16, 0)])
        self.trace = crdt_hip.Trace(os.path.join(ROOT, "traces", "sveltecomponent.json.gz"))
        self.btrace = crdt_hip.Trace(os.path.join(ROOT, "traces", "sveltecomponent.json.gz"))
        self.btrace.chars_to_bytes()
        self.h = C.c_void_p()
        self.n, self.n2, self.n3 = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.u32 = C.c_uint32()
        self.u64 = C.c_uint64()
        self.view = crdt_hip.View()
        self.bad_view = crdt_hip.View()
        self.bad_view.n = 1
        self.buf = C.create_string_buffer(256)
        self.p = C.c_void_p()


_DOC = None


def _doc() -> _Doc:
    global _DOC
    if _DOC is None:
        _DOC = _Doc()
    return _DOC


def _refusals():
    """(id, call(d) -> rc, code, text)."""
    R = C.byref
    log = lambda d: d.log._h
    buf = lambda d: C.cast(d.buf, C.c_void_p)
    T = []
    add = lambda *a: T.append(a)
    add("oplog_new/out", lambda d: d.L.crdt_hip_oplog_new(None), EINVAL, "null out")
    add("set_fugue/log", lambda d: d.L.crdt_hip_oplog_set_fugue(None, 1), EINVAL, NULLARG)
    add("set_fugue/nonempty", lambda d: d.L.crdt_hip_oplog_set_fugue(log(d), 1), EINVAL,
        "set_fugue needs an empty log")
    add("set_agent/log", lambda d: d.L.crdt_hip_oplog_set_agent(None, 1), EINVAL, NULLARG)
    add("clone/src", lambda d: d.L.crdt_hip_oplog_clone(None, R(d.h)), EINVAL, NULLARG)
    add("clone/out", lambda d: d.L.crdt_hip_oplog_clone(log(d), None), EINVAL, NULLARG)
    add("insert/log", lambda d: d.L.crdt_hip_oplog_insert(None, 0, b"x", 1), EINVAL, NULLARG)
    add("insert/utf8", lambda d: d.L.crdt_hip_oplog_insert(log(d), 0, None, 1), EINVAL, NULLARG)
    add("insert/range", lambda d: d.L.crdt_hip_oplog_insert(log(d), 99, b"x", 1), ERANGE,
        "insert position out of range")
    add("insert/log+range", lambda d: d.L.crdt_hip_oplog_insert(None, 99, b"x", 1), EINVAL, NULLARG)
    add("insert/utf8-invalid", lambda d: d.L.crdt_hip_oplog_insert(log(d), 0, b"\xff", 1), ERANGE,
        "invalid UTF-8")
    add("remove/log", lambda d: d.L.crdt_hip_oplog_remove(None, 0, 1), EINVAL, NULLARG)
    add("remove/range", lambda d: d.L.crdt_hip_oplog_remove(log(d), 2, 99), ERANGE,
        "remove range out of range")
    add("replace/log-remove", lambda d: d.L.crdt_hip_oplog_replace(None, 0, 1, b"x", 1), EINVAL, NULLARG)
    add("replace/log-insert", lambda d: d.L.crdt_hip_oplog_replace(None, 0, 0, b"x", 1), EINVAL, NULLARG)
    add("replace/utf8", lambda d: d.L.crdt_hip_oplog_replace(log(d), 0, 0, None, 1), EINVAL, NULLARG)
    add("replace/range", lambda d: d.L.crdt_hip_oplog_replace(log(d), 2, 99, b"x", 1), ERANGE,
        "remove range out of range")
    add("visible_bytes/log", lambda d: d.L.crdt_hip_oplog_visible_bytes(None, R(d.u64)), EINVAL, NULLARG)
    add("visible_bytes/out", lambda d: d.L.crdt_hip_oplog_visible_bytes(log(d), None), EINVAL, NULLARG)
    add("get_view/log", lambda d: d.L.crdt_hip_oplog_get_view(None, R(d.view)), EINVAL, NULLARG)
    add("get_view/out", lambda d: d.L.crdt_hip_oplog_get_view(log(d), None), EINVAL, NULLARG)
    add("encode_from/log", lambda d: d.L.crdt_hip_oplog_encode_from(None, 0, buf(d), 256, R(d.n)),
        EINVAL, NULLARG)
    add("encode_from/out_len", lambda d: d.L.crdt_hip_oplog_encode_from(log(d), 0, buf(d), 256, None),
        EINVAL, NULLARG)
    add("apply_update/log", lambda d: d.L.crdt_hip_oplog_apply_update(None, buf(d), 1), EINVAL, NULLARG)
    add("apply_update/buf", lambda d: d.L.crdt_hip_oplog_apply_update(log(d), None, 1), EINVAL, NULLARG)
    add("apply_update/garbage", lambda d: d.L.crdt_hip_oplog_apply_update(log(d), buf(d), 30), EINVAL,
        "not an update")
    add("join/dst", lambda d: d.L.crdt_hip_oplog_join(None, R(d.view), None, None), EINVAL, NULLARG)
    add("join/src", lambda d: d.L.crdt_hip_oplog_join(log(d), None, None, None), EINVAL,
        "null op log view")
    add("join/dst+src", lambda d: d.L.crdt_hip_oplog_join(None, None, None, None), EINVAL, NULLARG)
    add("join/arrays", lambda d: d.L.crdt_hip_oplog_join(log(d), R(d.bad_view), None, None), EINVAL,
        "op log view has null arrays")
    add("state_vector/log", lambda d: d.L.crdt_hip_oplog_state_vector(None, buf(d), 8, R(d.n)),
        EINVAL, NULLARG)
    add("state_vector/out_n", lambda d: d.L.crdt_hip_oplog_state_vector(log(d), buf(d), 8, None),
        EINVAL, NULLARG)
    add("encode_diff/log", lambda d: d.L.crdt_hip_oplog_encode_diff(None, None, 0, buf(d), 256, R(d.n)),
        EINVAL, NULLARG)
    add("encode_diff/out_len", lambda d: d.L.crdt_hip_oplog_encode_diff(log(d), None, 0, buf(d), 256, None),
        EINVAL, NULLARG)
    add("encode_diff/sv", lambda d: d.L.crdt_hip_oplog_encode_diff(log(d), None, 1, buf(d), 256, R(d.n)),
        EINVAL, NULLARG)
    add("apply_diff/log", lambda d: d.L.crdt_hip_oplog_apply_diff(None, buf(d), 1, None, None),
        EINVAL, NULLARG)
    add("apply_diff/buf", lambda d: d.L.crdt_hip_oplog_apply_diff(log(d), None, 1, None, None),
        EINVAL, NULLARG)
    add("apply_diff/garbage", lambda d: d.L.crdt_hip_oplog_apply_diff(log(d), buf(d), 30, None, None),
        EINVAL, "not a delta")
    add("mark/log", lambda d: d.L.crdt_hip_oplog_mark(None, R(d.h)), EINVAL, NULLARG)
    add("mark/out", lambda d: d.L.crdt_hip_oplog_mark(log(d), None), EINVAL, NULLARG)
    for sfx in ("", "_bytes"):
        ps = lambda d, sfx=sfx: getattr(d.L, "crdt_hip_oplog_patches_since" + sfx)
        ap = lambda d, sfx=sfx: getattr(d.L, "crdt_hip_oplog_apply_patches" + sfx)
        k = "patches_since" + sfx
        add(k + "/log", lambda d, ps=ps: ps(d)(None, d.mark._h, None, 0, R(d.n), None, 0, R(d.n2)),
            EINVAL, NULLARG)
        add(k + "/mark", lambda d, ps=ps: ps(d)(log(d), None, None, 0, R(d.n), None, 0, R(d.n2)),
            EINVAL, NULLARG)
        add(k + "/out_n", lambda d, ps=ps: ps(d)(log(d), d.mark._h, None, 0, None, None, 0, R(d.n2)),
            EINVAL, NULLARG)
        add(k + "/out_ins", lambda d, ps=ps: ps(d)(log(d), d.mark._h, None, 0, R(d.n), None, 0, None),
            EINVAL, NULLARG)
        add(k + "/other-log", lambda d, ps=ps: ps(d)(log(d), d.other_mark._h, None, 0, R(d.n), None, 0,
                                                     R(d.n2)), EINVAL, OTHER_LOG)
        add(k + "/out_n+other-log", lambda d, ps=ps: ps(d)(log(d), d.other_mark._h, None, 0, None, None,
                                                           0, R(d.n2)), EINVAL, NULLARG)
        k = "apply_patches" + sfx
        add(k + "/log", lambda d, ap=ap: ap(d)(None, None, 0, None, 0, None, None), EINVAL, NULLARG)
        add(k + "/p", lambda d, ap=ap: ap(d)(log(d), None, 1, buf(d), 1, None, None), EINVAL, NULLARG)
        add(k + "/ins", lambda d, ap=ap: ap(d)(log(d), buf(d), 1, None, 1, None, None), EINVAL, NULLARG)
        add(k + "/empty-patch", lambda d, ap=ap: ap(d)(
            log(d), np.zeros(1, crdt_hip.PATCH_DTYPE).ctypes.data, 1, None, 0, None, None), EINVAL,
            "empty patch")
    add("replace_bytes/log", lambda d: d.L.crdt_hip_oplog_replace_bytes(None, 0, 1, b"x", 1), EINVAL, NULLARG)
    add("replace_bytes/utf8", lambda d: d.L.crdt_hip_oplog_replace_bytes(log(d), 0, 1, None, 1), EINVAL, NULLARG)
    add("replace_bytes/2^32", lambda d: d.L.crdt_hip_oplog_replace_bytes(log(d), 0, 1 << 32, b"x", 1),
        ERANGE, "replace of 2^32 or more bytes")
    add("replace_bytes/log+2^32", lambda d: d.L.crdt_hip_oplog_replace_bytes(None, 0, 1 << 32, b"x", 1),
        EINVAL, NULLARG)
    add("replace_bytes/range", lambda d: d.L.crdt_hip_oplog_replace_bytes(log(d), 2, 99, b"x", 1),
        ERANGE, "patch range beyond the document")
    add("text_at/log", lambda d: d.L.crdt_hip_oplog_text_at(None, None, 0, 1, 0, buf(d), 256, R(d.n), None),
        EINVAL, NULLARG)
    add("text_at/other-log", lambda d: d.L.crdt_hip_oplog_text_at(
        log(d), d.other_mark._h, 0, 1, 0, buf(d), 256, R(d.n), None), EINVAL, OTHER_LOG)
    add("text_at/out_len", lambda d: d.L.crdt_hip_oplog_text_at(
        log(d), d.mark._h, 0, 1, 0, buf(d), 256, None, None), EINVAL, "null out_len")
    add("text_at/out_len+other-log", lambda d: d.L.crdt_hip_oplog_text_at(
        log(d), d.other_mark._h, 0, 1, 0, buf(d), 256, None, None), EINVAL, OTHER_LOG)
    add("text_at/flags+out_len", lambda d: d.L.crdt_hip_oplog_text_at(
        log(d), None, 0, 1, 2, buf(d), 256, None, None), EINVAL, "text flags are neither 0 nor BYTES")
    add("text_at/beyond", lambda d: d.L.crdt_hip_oplog_text_at(
        log(d), None, 0, 99, 0, buf(d), 256, R(d.n), None), ERANGE, "text window beyond the version")
    for name in ("anchors_at", "anchors_at_bytes"):
        at = lambda d, name=name: getattr(d.L, "crdt_hip_oplog_" + name)
        add(name + "/log", lambda d, at=at: at(d)(None, buf(d), None, 1, buf(d)), EINVAL, NULLARG)
        add(name + "/pos", lambda d, at=at: at(d)(log(d), None, None, 1, buf(d)), EINVAL, NULLARG)
        add(name + "/out", lambda d, at=at: at(d)(log(d), buf(d), None, 1, None), EINVAL, NULLARG)
        add(name + "/beyond", lambda d, at=at: at(d)(
            log(d), np.full(1, 99, np.uint64).ctypes.data, None, 1, buf(d)), ERANGE,
            "anchor position beyond the document")
    add("anchors_resolve/log", lambda d: d.L.crdt_hip_oplog_anchors_resolve(None, buf(d), 1, buf(d)),
        EINVAL, NULLARG)
    add("anchors_resolve/a", lambda d: d.L.crdt_hip_oplog_anchors_resolve(log(d), None, 1, buf(d)),
        EINVAL, NULLARG)
    add("anchors_resolve/out", lambda d: d.L.crdt_hip_oplog_anchors_resolve(log(d), buf(d), 1, None),
        EINVAL, NULLARG)
    sp = lambda d, h, f, n, a, b, c: d.L.crdt_hip_oplog_spans(h, f, n, None, 0, a, None, 0, b, c)
    add("spans/log", lambda d: sp(d, None, None, 0, R(d.n), R(d.n2), R(d.n3)), EINVAL, NULLARG)
    add("spans/f", lambda d: sp(d, log(d), None, 1, R(d.n), R(d.n2), R(d.n3)), EINVAL, NULLARG)
    add("spans/out_n", lambda d: sp(d, log(d), None, 0, None, R(d.n2), R(d.n3)), EINVAL, NULLARG)
    add("spans/out_attrs", lambda d: sp(d, log(d), None, 0, R(d.n), None, R(d.n3)), EINVAL, NULLARG)
    add("spans/pending", lambda d: sp(d, log(d), None, 0, R(d.n), R(d.n2), None), EINVAL, NULLARG)
    add("save/log", lambda d: d.L.crdt_hip_oplog_save(None, b"/nonexistent/x"), EINVAL, NULLARG)
    add("save/path", lambda d: d.L.crdt_hip_oplog_save(log(d), None), EINVAL, NULLARG)
    add("load/path", lambda d: d.L.crdt_hip_oplog_load(None, R(d.h)), EINVAL, NULLARG)
    add("load/out", lambda d: d.L.crdt_hip_oplog_load(b"/nonexistent/x", None), EINVAL, NULLARG)
    add("load/missing", lambda d: d.L.crdt_hip_oplog_load(b"/nonexistent/x", R(d.h)), EIO,
        "cannot open /nonexistent/x")
    tr = lambda d: d.trace._h
    add("trace_load/path", lambda d: d.L.crdt_hip_trace_load(None, R(d.h)), EINVAL, NULLARG)
    add("trace_load/out", lambda d: d.L.crdt_hip_trace_load(b"/nonexistent/x", None), EINVAL, NULLARG)
    add("trace_patch/t", lambda d: d.L.crdt_hip_trace_patch(None, 0, None, None, None, None), ERANGE,
        "patch index")
    add("trace_patch/index", lambda d: d.L.crdt_hip_trace_patch(tr(d), 1 << 40, None, None, None, None),
        ERANGE, "patch index")
    for name in ("start_content", "end_content"):
        fn = lambda d, name=name: getattr(d.L, "crdt_hip_trace_" + name)
        add(name + "/t", lambda d, fn=fn: fn(d)(None, R(d.p), R(d.n)), EINVAL, NULLARG)
        add(name + "/s", lambda d, fn=fn: fn(d)(tr(d), None, R(d.n)), EINVAL, NULLARG)
        add(name + "/len", lambda d, fn=fn: fn(d)(tr(d), R(d.p), None), EINVAL, NULLARG)
    add("chars_to_bytes/t", lambda d: d.L.crdt_hip_trace_chars_to_bytes(None), EINVAL, NULLARG)
    for name in ("resolve", "resolve_fugue"):
        fn = lambda d, name=name: getattr(d.L, "crdt_hip_trace_" + name)
        add(name + "/t", lambda d, fn=fn: fn(d)(None, R(d.h)), EINVAL, NULLARG)
        add(name + "/out", lambda d, fn=fn: fn(d)(tr(d), None), EINVAL, NULLARG)
        add(name + "/bytes", lambda d, fn=fn: fn(d)(d.btrace._h, R(d.h)), EINVAL,
            "resolve needs codepoint offsets (EDITS_USE_BYTE_OFFSETS = false)")
        add(name + "/out+bytes", lambda d, fn=fn: fn(d)(d.btrace._h, None), EINVAL, NULLARG)
    add("resolve_many/traces", lambda d: d.L.crdt_hip_trace_resolve_many(None, 1, 0, R(d.h)), EINVAL, NULLARG)
    add("resolve_many/out", lambda d: d.L.crdt_hip_trace_resolve_many(R(d.p), 1, 0, None), EINVAL, NULLARG)
    add("resolve_many/null-trace", lambda d: d.L.crdt_hip_trace_resolve_many(
        R(C.c_void_p()), 1, 0, R(d.h)), EINVAL, "null trace")
    add("resolve_many/bytes", lambda d: d.L.crdt_hip_trace_resolve_many(
        (C.c_void_p * 2)(tr(d), d.btrace._h), 2, 1, (C.c_void_p * 2)()), EINVAL,
        "trace 1: resolve needs codepoint offsets (EDITS_USE_BYTE_OFFSETS = false)")
    add("trace_save/t", lambda d: d.L.crdt_hip_trace_save(None, b"/nonexistent/x"), EINVAL, NULLARG)
    add("trace_save/path", lambda d: d.L.crdt_hip_trace_save(tr(d), None), EINVAL, NULLARG)
    return T


_REFUSALS = _refusals()


def _last_error(L, ctx=None) -> str:
    return L.crdt_hip_last_error(ctx).decode()


def _poison(L) -> None:
    """Leave a known other text in the thread's error string, so a stale one cannot pass."""
    assert L.crdt_hip_synth_tree_visible(0, 101, 0, None) == EINVAL
    assert _last_error(L) == "bad arguments"


@pytest.mark.parametrize("case", _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_refusal_code_and_text(case):
    _, call, code, text = case
    d = _doc()
    before = (d.log.version(), d.log.visible_len())
    _poison(d.L)
    rc = call(d)
    got = _last_error(d.L)
    print(case[0], rc, repr(got))
    assert (rc, got) == (code, text)
    assert (d.log.version(), d.log.visible_len()) == before, "a refused call changed the log"


def test_null_handles_that_are_not_refusals():
    """Calls that take a NULL handle without a code: they answer 0 and leave the error string."""
    L = crdt_hip.lib()
    _poison(L)
    assert L.crdt_hip_oplog_visible_len(None) == 0 and L.crdt_hip_oplog_version(None) == 0
    assert L.crdt_hip_trace_len(None) == 0 and L.crdt_hip_trace_txns(None) == 0
    L.crdt_hip_oplog_free(None), L.crdt_hip_trace_free(None), L.crdt_hip_mark_free(None)
    assert L.crdt_hip_logfile_close(None) == 0
    # the empty replace returns before any check, a NULL log included
    assert L.crdt_hip_oplog_replace(None, 0, 0, None, 0) == 0
    assert L.crdt_hip_oplog_replace_bytes(None, 0, 0, None, 0) == EINVAL
    assert _last_error(L) == NULLARG


def _sized(call, need, width):
    """One sized output under the ESPACE convention: call(buf, cap, count) -> rc, `need` items of
    `width` bytes.  NULL and short buffers give ESPACE with the count set to the need and the
    buffer untouched; an exact buffer succeeds with the count written."""
    L = crdt_hip.lib()
    n = C.c_size_t(12345)
    _poison(L)
    assert call(None, 0, C.byref(n)) == ESPACE and n.value == need and _last_error(L) == SMALL
    buf = np.full(need * width + 8, SENTINEL, np.uint8)
    n.value = 12345
    assert call(buf.ctypes.data, need - 1, C.byref(n)) == ESPACE and n.value == need
    assert (buf == SENTINEL).all(), "ESPACE wrote into the buffer"
    # a NULL buffer with room claimed is still short
    assert call(None, need, C.byref(n)) == ESPACE
    n.value = 12345
    assert call(buf.ctypes.data, need, C.byref(n)) == 0 and n.value == need
    assert not (buf[: need * width] == SENTINEL).all() and (buf[need * width:] == SENTINEL).all()
    return buf[: need * width]


def test_espace_state_vector():
    d = _doc()
    L = d.L
    _sized(lambda b, cap, n: L.crdt_hip_oplog_state_vector(d.log._h, b, cap, n), 1, 8)
    # an empty vector needs no buffer
    n = C.c_size_t(12345)
    assert L.crdt_hip_oplog_state_vector(d.empty._h, None, 0, C.byref(n)) == 0 and n.value == 0


def test_espace_encode_from_and_encode_diff():
    d = _doc()
    L = d.L
    full = d.log.encode_from(0)
    got = _sized(lambda b, cap, n: L.crdt_hip_oplog_encode_from(d.log._h, 0, b, cap, n), len(full), 1)
    assert got.tobytes() == full
    delta = d.log.encode_diff([])
    got = _sized(lambda b, cap, n: L.crdt_hip_oplog_encode_diff(d.log._h, None, 0, b, cap, n),
                 len(delta), 1)
    assert got.tobytes() == delta
    # neither is ever empty (a header), and a NULL buffer is ESPACE whatever the size
    n = C.c_size_t(12345)
    assert L.crdt_hip_oplog_encode_from(d.empty._h, 0, None, 0, C.byref(n)) == ESPACE and n.value > 0
    assert L.crdt_hip_oplog_encode_diff(d.empty._h, None, 0, None, 0, C.byref(n)) == ESPACE and n.value > 0


@pytest.mark.parametrize("sfx,patches", [("", [(0, 1, 0, 1), (4, 0, 1, 2)]),
                                         ("_bytes", [(0, 1, 0, 1), (4, 0, 1, 2)])])
def test_espace_patches_since(sfx, patches):
    """Both counts are written before the space check; either array short is ESPACE and neither is
    written; an array with nothing to hold may be NULL."""
    d = _doc()
    L = d.L
    fn = getattr(L, "crdt_hip_oplog_patches_since" + sfx)
    R = C.byref
    n, nb = C.c_size_t(12345), C.c_size_t(12345)
    out = np.full(3 * 24, SENTINEL, np.uint8)
    ins = np.full(8, SENTINEL, np.uint8)
    for cap, ins_cap, o, i in [(0, 0, None, None), (1, 8, out, ins), (3, 2, out, ins),
                               (3, 8, None, ins), (3, 8, out, None)]:
        n.value = nb.value = 12345
        _poison(L)
        rc = fn(d.log._h, d.mark._h, o.ctypes.data if o is not None else None, cap, R(n),
                i.ctypes.data if i is not None else None, ins_cap, R(nb))
        assert (rc, n.value, nb.value, _last_error(L)) == (ESPACE, 2, 3, SMALL), (cap, ins_cap)
        assert (out == SENTINEL).all() and (ins == SENTINEL).all(), "ESPACE wrote into a buffer"
    n.value = nb.value = 12345
    assert fn(d.log._h, d.mark._h, out.ctypes.data, 2, R(n), ins.ctypes.data, 3, R(nb)) == 0
    assert (n.value, nb.value) == (2, 3)
    got = out[:48].view(crdt_hip.PATCH_DTYPE)
    assert [(int(p["pos"]), int(p["del"]), int(p["ins_off"]), int(p["ins_len"])) for p in got] == patches
    assert ins[:3].tobytes() == b"XYZ" and (out[48:] == SENTINEL).all() and (ins[3:] == SENTINEL).all()
    # nothing changed since the mark: no buffers needed
    n.value = nb.value = 12345
    assert fn(d.other._h, d.other_mark._h, None, 0, R(n), None, 0, R(nb)) == 0
    assert (n.value, nb.value) == (0, 0)


def test_espace_spans():
    """The counts are written on ESPACE and on success, *pending on success only; both arrays are
    checked only when there is a span."""
    d = _doc()
    L = d.L
    R = C.byref
    f = d.formats
    n, na, pend = C.c_size_t(12345), C.c_size_t(12345), C.c_size_t(12345)
    sp = np.full(4 * 40, SENTINEL, np.uint8)
    at = np.full(4 * 16, SENTINEL, np.uint8)

    def call(o, cap, a, acap, log=d.log):
        n.value = na.value = pend.value = 12345
        _poison(L)
        return L.crdt_hip_oplog_spans(log._h, f.ctypes.data, f.size, o.ctypes.data if o is not None else None,
                                      cap, R(n), a.ctypes.data if a is not None else None, acap, R(na),
                                      R(pend))

    for o, cap, a, acap in [(None, 0, None, 0), (sp, 1, at, 4), (sp, 4, at, 1), (None, 4, at, 4),
                            (sp, 4, None, 4)]:
        assert call(o, cap, a, acap) == ESPACE and _last_error(L) == SMALL
        assert (n.value, na.value, pend.value) == (2, 2, 12345)
        assert (sp == SENTINEL).all() and (at == SENTINEL).all(), "ESPACE wrote into a buffer"
    assert call(sp, 2, at, 2) == 0 and (n.value, na.value, pend.value) == (2, 2, 0)
    got = sp[:80].view(crdt_hip.SPAN_DTYPE)
    assert [(int(x["pos"]), int(x["len"])) for x in got] == [(0, 2), (2, 4)]
    assert (sp[80:] == SENTINEL).all() and (at[32:] == SENTINEL).all()
    # no span (an empty document: both formats' anchors are unknown): no buffers needed
    assert call(None, 0, None, 0, d.empty) == 0 and (n.value, na.value, pend.value) == (0, 0, 2)


def test_espace_text_at():
    """*out_len and *info are written on ESPACE; an empty window needs no buffer."""
    d = _doc()
    L = d.L
    R = C.byref
    n, info = C.c_size_t(12345), crdt_hip.TextInfo()
    buf = np.full(16, SENTINEL, np.uint8)
    for m, want in [(None, b"XbcdYZ"), (d.mark, b"abcd")]:
        h = m._h if m else None
        for o, cap in [(None, 0), (buf, len(want) - 1), (None, 16)]:
            n.value, info.n = 12345, 12345
            _poison(L)
            rc = L.crdt_hip_oplog_text_at(d.log._h, h, 0, crdt_hip.TEXT_END, 0,
                                          o.ctypes.data if o is not None else None, cap, R(n), R(info))
            assert (rc, n.value, info.n, info.len, _last_error(L)) == (ESPACE, len(want), len(want),
                                                                       len(want), SMALL)
            assert (buf == SENTINEL).all(), "ESPACE wrote into the buffer"
        assert L.crdt_hip_oplog_text_at(d.log._h, h, 0, crdt_hip.TEXT_END, 0, buf.ctypes.data,
                                        len(want), R(n), None) == 0
        assert n.value == len(want) and buf[: n.value].tobytes() == want
        assert (buf[n.value:] == SENTINEL).all()
        buf[:] = SENTINEL
    n.value = 12345
    assert L.crdt_hip_oplog_text_at(d.log._h, None, 2, 2, 0, None, 0, R(n), R(info)) == 0
    assert (n.value, info.n, info.start, info.len) == (0, 0, 2, 6)
    # a refusal other than ESPACE leaves *out_len and *info as they were
    n.value, info.n = 12345, 12345
    assert L.crdt_hip_oplog_text_at(d.log._h, None, 0, 99, 0, None, 0, R(n), R(info)) == ERANGE
    assert (n.value, info.n) == (12345, 12345)
