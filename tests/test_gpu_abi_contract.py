"""The C ABI's contract for device handles: which crdt_hip_replica_*, crdt_hip_updates_*,
crdt_hip_batch_* and *_stats call refuses what, with which code, which exact text, and in which
error string (a NULL context: the thread's; otherwise the string of the context the call was made
on).  Two contexts on device 0 and three-item replicas; almost no kernel runs."""
import ctypes as C

import numpy as np
import pytest

import crdt_hip

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ESPACE = -1, -2, -6
NULLARG = "null argument"
OTHER_CTX = "replica belongs to another context"
OTHER_CTX2 = "replica or updates belong to another context"
OTHER_BATCH = "batch belongs to another context"
LOG_MARK = "a log's mark passed to a replica"
OTHER_REPLICA = "the mark belongs to another replica"
REPLICA_MARK = "a replica's mark passed to a log"
TL_POISON, CTX_POISON = "bad arguments", "unknown parameter nope"
TL, A, B = "thread", "A", "B"
PRESET = 0x1234


class _World:
    def __init__(self, ctx):
        L = self.L = crdt_hip.lib()
        self.A, self.B = ctx, crdt_hip.Context(ctx.device)
        self.log = crdt_hip.OpLog()
        self.log.insert(0, "abc")
        self.host_mark = self.log.mark()
        ahead = self.log.clone()
        v = ahead.version()
        ahead.insert(3, "d")
        upd = crdt_hip.pack_updates([ahead.encode_from(v)])
        self.rep, self.rep2 = crdt_hip.Replica(self.A, self.log), crdt_hip.Replica(self.A, self.log)
        self.repB = crdt_hip.Replica(self.B, self.log)
        self.mark, self.mark2, self.markB = self.rep.mark(), self.rep2.mark(), self.repB.mark()
        self.upd, self.updB = crdt_hip.UpdateBatch(self.A, *upd), crdt_hip.UpdateBatch(self.B, *upd)
        self.batch, self.batchB = self.A.batch([self.log], 1), self.B.batch([self.log], 1)
        self.view = self.log.view()
        self.bad_view = crdt_hip.View()
        self.bad_view.n = 1
        self.h = C.c_void_p()
        self.n, self.n2, self.n3 = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.buf = C.create_string_buffer(256)
        assert L.crdt_hip_abi_version() == 2

    def close(self):
        for x in (self.mark, self.mark2, self.markB, self.rep, self.rep2, self.repB, self.upd,
                  self.updB, self.batch, self.batchB, self.B):
            x.close()

    def poison(self):
        L = self.L
        assert L.crdt_hip_synth_tree_visible(0, 101, 0, None) == EINVAL
        for c in (self.A, self.B):
            assert L.crdt_hip_set_param(c._h, b"nope", 0) == EINVAL

    def errors(self) -> dict:
        e = self.L.crdt_hip_last_error
        return {TL: e(None).decode(), A: e(self.A._h).decode(), B: e(self.B._h).decode()}


@pytest.fixture(scope="module")
def w(ctx):
    world = _World(ctx)
    yield world
    world.close()


def _refusals():
    """(id, call(w) -> rc, code, text, the error string that receives it)."""
    R = C.byref
    T = []
    add = lambda *a: T.append(a)
    a, b = (lambda w: w.A._h), (lambda w: w.B._h)
    rep, buf = (lambda w: w.rep._h), (lambda w: C.cast(w.buf, C.c_void_p))

    def three(name, call):
        """NULL ctx, NULL replica, a replica of the other context, for call(w, ctx, replica)."""
        add(name + "/ctx", lambda w: call(w, None, rep(w)), EINVAL, NULLARG, TL)
        add(name + "/replica", lambda w: call(w, a(w), None), EINVAL, NULLARG, A)
        add(name + "/other-ctx", lambda w: call(w, b(w), rep(w)), EINVAL, OTHER_CTX, B)

    add("replica_new/ctx", lambda w: w.L.crdt_hip_replica_new(None, R(w.view), R(w.h)), EINVAL, NULLARG, TL)
    add("replica_new/out", lambda w: w.L.crdt_hip_replica_new(a(w), R(w.view), None), EINVAL, NULLARG, A)
    add("replica_new/arrays", lambda w: w.L.crdt_hip_replica_new(a(w), R(w.bad_view), R(w.h)), EINVAL,
        "op log view has null arrays", A)
    three("clone", lambda w, c, r: w.L.crdt_hip_replica_clone(c, r, R(w.h)))
    add("clone/out", lambda w: w.L.crdt_hip_replica_clone(a(w), rep(w), None), EINVAL, NULLARG, A)
    three("apply_updates", lambda w, c, r: w.L.crdt_hip_replica_apply_updates(c, r, None, 0, None, 0))
    add("updates_upload/ctx", lambda w: w.L.crdt_hip_updates_upload(None, None, 0, None, 0, R(w.h)),
        EINVAL, NULLARG, TL)
    add("updates_upload/out", lambda w: w.L.crdt_hip_updates_upload(a(w), None, 0, None, 0, None),
        EINVAL, NULLARG, A)
    for name in ("replay", "apply_resident"):
        def call(w, c, r, u, name=name):
            fn = getattr(w.L, "crdt_hip_replica_" + name)
            return fn(c, r, u, None, None, None) if name == "replay" else fn(c, r, u)
        add(name + "/ctx", lambda w, call=call: call(w, None, rep(w), w.upd._h), EINVAL, NULLARG, TL)
        add(name + "/replica", lambda w, call=call: call(w, a(w), None, w.upd._h), EINVAL, NULLARG, A)
        add(name + "/updates", lambda w, call=call: call(w, a(w), rep(w), None), EINVAL, NULLARG, A)
        add(name + "/other-ctx-replica", lambda w, call=call: call(w, a(w), w.repB._h, w.upd._h), EINVAL,
            OTHER_CTX2, A)
        add(name + "/other-ctx-updates", lambda w, call=call: call(w, a(w), rep(w), w.updB._h), EINVAL,
            OTHER_CTX2, A)
    join = lambda w, c, d, s: w.L.crdt_hip_replica_join(c, d, s, None, None)
    add("join/ctx", lambda w: join(w, None, rep(w), w.rep2._h), EINVAL, NULLARG, TL)
    add("join/dst", lambda w: join(w, a(w), None, w.rep2._h), EINVAL, NULLARG, A)
    add("join/src", lambda w: join(w, a(w), rep(w), None), EINVAL, NULLARG, A)
    add("join/other-ctx-dst", lambda w: join(w, a(w), w.repB._h, rep(w)), EINVAL, OTHER_CTX, A)
    add("join/other-ctx-src", lambda w: join(w, a(w), rep(w), w.repB._h), EINVAL, OTHER_CTX, A)
    three("state_vector", lambda w, c, r: w.L.crdt_hip_replica_state_vector(c, r, None, 0, R(w.n)))
    add("state_vector/out_n", lambda w: w.L.crdt_hip_replica_state_vector(a(w), rep(w), None, 0, None),
        EINVAL, NULLARG, A)
    add("state_vector/out_n+other-ctx", lambda w: w.L.crdt_hip_replica_state_vector(
        b(w), rep(w), None, 0, None), EINVAL, NULLARG, B)
    ed = lambda w, c, r, nsv, n: w.L.crdt_hip_replica_encode_diff(c, r, None, nsv, None, 0, n)
    three("encode_diff", lambda w, c, r: ed(w, c, r, 0, R(w.n)))
    add("encode_diff/out_len", lambda w: ed(w, a(w), rep(w), 0, None), EINVAL, NULLARG, A)
    add("encode_diff/sv", lambda w: ed(w, a(w), rep(w), 1, R(w.n)), EINVAL, NULLARG, A)
    three("apply_diff", lambda w, c, r: w.L.crdt_hip_replica_apply_diff(c, r, None, 0, None, None))
    add("apply_diff/buf", lambda w: w.L.crdt_hip_replica_apply_diff(a(w), rep(w), None, 1, None, None),
        EINVAL, NULLARG, A)
    three("mark", lambda w, c, r: w.L.crdt_hip_replica_mark(c, r, R(w.h)))
    add("mark/out", lambda w: w.L.crdt_hip_replica_mark(a(w), rep(w), None), EINVAL, NULLARG, A)
    for sfx in ("", "_bytes"):
        def ps(w, c, r, m, n, nb, sfx=sfx):
            return getattr(w.L, "crdt_hip_replica_patches_since" + sfx)(c, r, m, None, 0, n, None, 0, nb)
        k = "patches_since" + sfx
        three(k, lambda w, c, r, ps=ps: ps(w, c, r, w.mark._h, R(w.n), R(w.n2)))
        add(k + "/mark", lambda w, ps=ps: ps(w, a(w), rep(w), None, R(w.n), R(w.n2)), EINVAL, NULLARG, A)
        add(k + "/out_n", lambda w, ps=ps: ps(w, a(w), rep(w), w.mark._h, None, R(w.n2)), EINVAL, NULLARG, A)
        add(k + "/out_ins", lambda w, ps=ps: ps(w, a(w), rep(w), w.mark._h, R(w.n), None), EINVAL, NULLARG, A)
        add(k + "/log-mark", lambda w, ps=ps: ps(w, a(w), rep(w), w.host_mark._h, R(w.n), R(w.n2)),
            EINVAL, LOG_MARK, A)
        add(k + "/other-replica", lambda w, ps=ps: ps(w, a(w), rep(w), w.mark2._h, R(w.n), R(w.n2)),
            EINVAL, OTHER_REPLICA, A)
        add(k + "/other-ctx-mark", lambda w, ps=ps: ps(w, a(w), rep(w), w.markB._h, R(w.n), R(w.n2)),
            EINVAL, OTHER_REPLICA, A)
        add(k + "/out_n+log-mark", lambda w, ps=ps: ps(w, a(w), rep(w), w.host_mark._h, None, R(w.n2)),
            EINVAL, NULLARG, A)
        add(k + "/other-ctx+log-mark", lambda w, ps=ps: ps(w, b(w), rep(w), w.host_mark._h, R(w.n), R(w.n2)),
            EINVAL, OTHER_CTX, B)
        # the reverse: a replica's mark passed to the log's call (the thread's string)
        def lps(w, m, n, sfx=sfx):
            return getattr(w.L, "crdt_hip_oplog_patches_since" + sfx)(w.log._h, m, None, 0, n, None, 0,
                                                                      R(w.n2))
        add("oplog_" + k + "/replica-mark", lambda w, lps=lps: lps(w, w.mark._h, R(w.n)), EINVAL,
            REPLICA_MARK, TL)
        add("oplog_" + k + "/out_n+replica-mark", lambda w, lps=lps: lps(w, w.mark._h, None), EINVAL,
            NULLARG, TL)
        def ap(w, c, r, p, n, ins, ins_len, sfx=sfx):
            return getattr(w.L, "crdt_hip_replica_apply_patches" + sfx)(c, r, p, n, ins, ins_len, None, None)
        k = "apply_patches" + sfx
        three(k, lambda w, c, r, ap=ap: ap(w, c, r, None, 0, None, 0))
        add(k + "/p", lambda w, ap=ap: ap(w, a(w), rep(w), None, 1, buf(w), 1), EINVAL, NULLARG, A)
        add(k + "/ins", lambda w, ap=ap: ap(w, a(w), rep(w), buf(w), 1, None, 1), EINVAL, NULLARG, A)
        def rp(w, c, r, end, utf8, sfx=sfx):
            return getattr(w.L, "crdt_hip_replica_replace" + sfx)(c, r, 0, end, utf8, 1)
        k = "replace" + sfx
        three(k, lambda w, c, r, rp=rp: rp(w, c, r, 1, b"x"))
        add(k + "/utf8", lambda w, rp=rp: rp(w, a(w), rep(w), 1, None), EINVAL, NULLARG, A)
        add(k + "/2^32", lambda w, rp=rp: rp(w, a(w), rep(w), 1 << 32, b"x"), ERANGE,
            "replace of 2^32 or more bytes" if sfx else "replace of 2^32 or more codepoints or bytes", A)
        add(k + "/other-ctx+2^32", lambda w, rp=rp: rp(w, b(w), rep(w), 1 << 32, b"x"), EINVAL, OTHER_CTX, B)
    ta = lambda w, c, r, m, n: w.L.crdt_hip_replica_text_at(c, r, m, 0, 1, 0, buf(w), 256, n, None)
    three("text_at", lambda w, c, r: ta(w, c, r, None, R(w.n)))
    add("text_at/log-mark", lambda w: ta(w, a(w), rep(w), w.host_mark._h, R(w.n)), EINVAL, LOG_MARK, A)
    add("text_at/other-replica", lambda w: ta(w, a(w), rep(w), w.mark2._h, R(w.n)), EINVAL, OTHER_REPLICA, A)
    add("text_at/other-ctx-mark", lambda w: ta(w, a(w), rep(w), w.markB._h, R(w.n)), EINVAL, OTHER_REPLICA, A)
    add("text_at/out_len", lambda w: ta(w, a(w), rep(w), w.mark._h, None), EINVAL, "null out_len", A)
    add("text_at/out_len+log-mark", lambda w: ta(w, a(w), rep(w), w.host_mark._h, None), EINVAL, LOG_MARK, A)
    add("oplog_text_at/replica-mark", lambda w: w.L.crdt_hip_oplog_text_at(
        w.log._h, w.mark._h, 0, 1, 0, buf(w), 256, R(w.n), None), EINVAL, REPLICA_MARK, TL)
    add("oplog_text_at/out_len+replica-mark", lambda w: w.L.crdt_hip_oplog_text_at(
        w.log._h, w.mark._h, 0, 1, 0, buf(w), 256, None, None), EINVAL, REPLICA_MARK, TL)
    add("set_agent/replica", lambda w: w.L.crdt_hip_replica_set_agent(None, 1), EINVAL, "null replica", TL)
    for name in ("anchors_at", "anchors_at_bytes"):
        def at(w, c, r, pos, out, name=name):
            return getattr(w.L, "crdt_hip_replica_" + name)(c, r, pos, None, 1, out)
        three(name, lambda w, c, r, at=at: at(w, c, r, buf(w), buf(w)))
        add(name + "/pos", lambda w, at=at: at(w, a(w), rep(w), None, buf(w)), EINVAL, NULLARG, A)
        add(name + "/out", lambda w, at=at: at(w, a(w), rep(w), buf(w), None), EINVAL, NULLARG, A)
    ar = lambda w, c, r, x, out: w.L.crdt_hip_replica_anchors_resolve(c, r, x, 1, out)
    three("anchors_resolve", lambda w, c, r: ar(w, c, r, buf(w), buf(w)))
    add("anchors_resolve/a", lambda w: ar(w, a(w), rep(w), None, buf(w)), EINVAL, NULLARG, A)
    add("anchors_resolve/out", lambda w: ar(w, a(w), rep(w), buf(w), None), EINVAL, NULLARG, A)
    sp = lambda w, c, r, nf, n, na, pend: w.L.crdt_hip_replica_spans(c, r, None, nf, None, 0, n, None, 0,
                                                                     na, pend)
    three("spans", lambda w, c, r: sp(w, c, r, 0, R(w.n), R(w.n2), R(w.n3)))
    add("spans/f", lambda w: sp(w, a(w), rep(w), 1, R(w.n), R(w.n2), R(w.n3)), EINVAL, NULLARG, A)
    add("spans/out_n", lambda w: sp(w, a(w), rep(w), 0, None, R(w.n2), R(w.n3)), EINVAL, NULLARG, A)
    add("spans/out_attrs", lambda w: sp(w, a(w), rep(w), 0, R(w.n), None, R(w.n3)), EINVAL, NULLARG, A)
    add("spans/pending", lambda w: sp(w, a(w), rep(w), 0, R(w.n), R(w.n2), None), EINVAL, NULLARG, A)
    add("info/replica", lambda w: w.L.crdt_hip_replica_info(None, None, None, None), EINVAL, "null replica", TL)
    three("replica_merge", lambda w, c, r: w.L.crdt_hip_replica_merge(c, r, None, 0, None, None))
    three("replica_merge_len", lambda w, c, r: w.L.crdt_hip_replica_merge_len(c, r, None, None, None))
    three("replica_merge_inc", lambda w, c, r: w.L.crdt_hip_replica_merge_inc(c, r, None, 0, None, None, None))
    add("merge/ctx", lambda w: w.L.crdt_hip_merge(None, R(w.view), None, 0, None, None), EINVAL,
        "null context", TL)
    add("merge/view", lambda w: w.L.crdt_hip_merge(a(w), None, None, 0, None, None), EINVAL,
        "null op log view", A)
    add("merge_len/ctx", lambda w: w.L.crdt_hip_merge_len(None, R(w.view), None, None, None), EINVAL,
        "null context", TL)
    bc = lambda w, c, bases, nb, reps, relabel, out: w.L.crdt_hip_batch_create(c, bases, nb, reps, relabel, 0, out)
    add("batch_create/ctx", lambda w: bc(w, None, R(w.view), 1, 1, 0, R(w.h)), EINVAL, "bad batch arguments", TL)
    add("batch_create/bases", lambda w: bc(w, a(w), None, 1, 1, 0, R(w.h)), EINVAL, "bad batch arguments", A)
    add("batch_create/out", lambda w: bc(w, a(w), R(w.view), 1, 1, 0, None), EINVAL, "bad batch arguments", A)
    add("batch_create/nbases", lambda w: bc(w, a(w), R(w.view), 0, 1, 0, R(w.h)), EINVAL, "bad batch arguments", A)
    add("batch_create/replicas", lambda w: bc(w, a(w), R(w.view), 1, 0, 0, R(w.h)), EINVAL, "bad batch arguments", A)
    add("batch_create/relabel", lambda w: bc(w, a(w), R(w.view), 1, 1, 3, R(w.h)), EINVAL,
        "relabel must be 0, 1 or 2", A)
    add("batch_create/arrays", lambda w: bc(w, a(w), R(w.bad_view), 1, 1, 0, R(w.h)), EINVAL,
        "op log view has null arrays", A)
    st = lambda w, c, pct, out: w.L.crdt_hip_batch_synth_tree(c, 8, pct, 0, 0, out)
    add("batch_synth_tree/ctx", lambda w: st(w, None, 0, R(w.h)), EINVAL, "bad synth arguments", TL)
    add("batch_synth_tree/out", lambda w: st(w, a(w), 0, None), EINVAL, "bad synth arguments", A)
    add("batch_synth_tree/pct", lambda w: st(w, a(w), 101, R(w.h)), EINVAL, "bad synth arguments", A)
    add("batch_info/batch", lambda w: w.L.crdt_hip_batch_info(None, None, None, None), EINVAL, "null batch", TL)
    for name, tail in (("batch_merge", (None, None, None)), ("batch_raw", (1,))):
        fn = lambda w, name=name: getattr(w.L, "crdt_hip_" + name)
        add(name + "/ctx", lambda w, fn=fn, tail=tail: fn(w)(None, w.batch._h, *tail), EINVAL, NULLARG, TL)
        add(name + "/batch", lambda w, fn=fn, tail=tail: fn(w)(a(w), None, *tail), EINVAL, NULLARG, A)
        add(name + "/other-ctx", lambda w, fn=fn, tail=tail: fn(w)(b(w), w.batch._h, *tail), EINVAL,
            OTHER_BATCH, B)
    for name, outs in (("join", 4), ("delta", 4), ("patch", 4), ("edit", 5), ("anchor", 4), ("text", 4),
                       ("format", 6)):
        add(name + "_stats/ctx", lambda w, name=name, outs=outs: getattr(w.L, f"crdt_hip_{name}_stats")(
            None, *[None] * outs), EINVAL, "null context", TL)
    return T


_REFUSALS = _refusals()


@pytest.mark.parametrize("case", _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_refusal_code_text_and_string(w, case):
    _, call, code, text, where = case
    snap = (w.rep.info(), w.rep2.info(), w.repB.info())
    w.poison()
    rc = call(w)
    got = w.errors()
    print(case[0], rc, got)
    want = {TL: TL_POISON, A: CTX_POISON, B: CTX_POISON}
    want[where] = text
    assert (rc, got) == (code, want)
    assert (w.rep.info(), w.rep2.info(), w.repB.info()) == snap, "a refused call changed a replica"


def test_what_a_refusal_leaves_in_the_out_handle(w):
    """Which refusals null *out and which leave it as it was."""
    L, R = w.L, C.byref
    a, b, rep = w.A._h, w.B._h, w.rep._h
    cases = [
        ("replica_new/arrays", lambda h: L.crdt_hip_replica_new(a, R(w.bad_view), R(h)), None),
        ("clone/other-ctx", lambda h: L.crdt_hip_replica_clone(b, rep, R(h)), PRESET),
        ("mark/other-ctx", lambda h: L.crdt_hip_replica_mark(b, rep, R(h)), None),
        ("batch_create/relabel", lambda h: L.crdt_hip_batch_create(a, R(w.view), 1, 1, 3, 0, R(h)), PRESET),
        ("batch_create/arrays", lambda h: L.crdt_hip_batch_create(a, R(w.bad_view), 1, 1, 0, 0, R(h)), None),
        ("batch_synth_tree/pct", lambda h: L.crdt_hip_batch_synth_tree(a, 8, 101, 0, 0, R(h)), PRESET),
    ]
    for name, call, left in cases:
        h = C.c_void_p(PRESET)
        assert call(h) == EINVAL, name
        print(name, h.value)
        assert h.value == left, name


def test_null_handles_that_are_not_refusals(w):
    L = w.L
    w.poison()
    assert L.crdt_hip_replica_free(None) == 0 and L.crdt_hip_updates_free(None) == 0
    assert L.crdt_hip_batch_free(None) == 0 and L.crdt_hip_destroy(None) == 0
    for name, outs in (("join", 4), ("delta", 4), ("patch", 4), ("edit", 5), ("anchor", 4), ("text", 4),
                       ("format", 6)):
        assert getattr(L, f"crdt_hip_{name}_stats")(w.A._h, *[None] * outs) == 0
    assert L.crdt_hip_batch_info(w.batch._h, None, None, None) == 0
    assert L.crdt_hip_replica_info(w.rep._h, None, None, None) == 0
    # the empty replace returns 0 after the checks
    assert L.crdt_hip_replica_replace(w.A._h, w.rep._h, 0, 0, None, 0) == 0
    assert L.crdt_hip_replica_replace_bytes(w.A._h, w.rep._h, 0, 0, None, 0) == 0
    assert w.errors() == {TL: TL_POISON, A: CTX_POISON, B: CTX_POISON}


def test_espace_state_vector_and_merge_tails(w):
    """The sized outputs that capi.cpp itself copies out for a replica: the state vector (the count
    first, an empty vector needs no buffer) and the three merge tails (counts written before the
    space check, "output buffer too small", the buffer untouched)."""
    L, R = w.L, C.byref
    a, rep = w.A._h, w.rep._h
    n = C.c_size_t(12345)
    w.poison()
    assert L.crdt_hip_replica_state_vector(a, rep, None, 0, R(n)) == ESPACE and n.value == 1
    assert w.errors()[A] == "buffer too small"
    sv = np.full(24, 0xA5, np.uint8)
    assert L.crdt_hip_replica_state_vector(a, rep, sv.ctypes.data, 0, R(n)) == ESPACE
    assert (sv == 0xA5).all()
    n.value = 12345
    assert L.crdt_hip_replica_state_vector(a, rep, sv.ctypes.data, 1, R(n)) == 0 and n.value == 1
    assert sv[:8].view("<u4").tolist() == [0, 3] and (sv[8:] == 0xA5).all()
    empty = crdt_hip.Replica(w.A)
    n.value = 12345
    assert L.crdt_hip_replica_state_vector(a, empty._h, None, 0, R(n)) == 0 and n.value == 0
    empty.close()

    dig, cps, path = C.c_uint64(), C.c_uint64(), C.c_uint32(77)
    buf = np.full(8, 0xA5, np.uint8)
    calls = [
        lambda cap: L.crdt_hip_merge(a, R(w.view), buf.ctypes.data, cap, R(n), R(dig)),
        lambda cap: L.crdt_hip_replica_merge(a, rep, buf.ctypes.data, cap, R(n), R(dig)),
        lambda cap: L.crdt_hip_replica_merge_inc(a, rep, buf.ctypes.data, cap, R(n), R(cps), R(path)),
    ]
    for k, call in enumerate(calls):
        n.value, dig.value, cps.value = 12345, 0, 12345
        w.poison()
        assert call(2) == ESPACE and n.value == 3, k
        assert w.errors() == {TL: TL_POISON, A: "output buffer too small", B: CTX_POISON}
        assert (buf == 0xA5).all(), "ESPACE wrote into the buffer"
        assert dig.value == crdt_hip.tree_digest(b"abc") if k < 2 else cps.value == 3
        assert call(3) == 0 and n.value == 3 and buf[:3].tobytes() == b"abc" and (buf[3:] == 0xA5).all()
        buf[:] = 0xA5
    # no buffer: the length and the digest alone
    n.value = 12345
    assert L.crdt_hip_replica_merge(a, rep, None, 0, R(n), R(dig)) == 0 and n.value == 3
