"""Formats on a device replica (crdt_hip_replica_spans, format.hip).

Parity throughout: Replica.spans_raw equals OpLog.spans_raw byte for byte (spans, attrs, pending) on
a host log that holds the same items slot for slot, and both equal the plain Python restatement
over the CPU oracle's document order (format_util.FRef); exact integers, no tolerance.  The kernels
count and compact per tile of 4,096 ranks, give a boundary a wave that walks 64 ranks a step and a
segment a thread that walks the formats, so besides the ~300-item typed log the shapes are the
smallest that cross those: rank counts of 4095, 4096, 4097 and 8193 with a dead stretch over rank
4096, a wholly dead tile, boundaries at ranks 4094..4098, 1 and N, and format counts around 64 and
256 with key groups that straddle 64.
"""
import ctypes as C
import random

import numpy as np
import pytest

import crdt_hip
import format_util as fu
import patch_util as pu
from crdt_hip import AFTER, BEFORE, EDGE, REMOVE
from edit_util import KINDS, text_of
from format_util import EINVAL, ERANGE, ESPACE, fmt, op_of

pytestmark = pytest.mark.gpu

START, END_ = (EDGE, AFTER), (EDGE, BEFORE)


@pytest.fixture
def pair(ctx, oracle):
    made = []

    def make(log, fugue, agent=0):
        p = fu.Pair(ctx, oracle, log, fugue, agent)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("kind", KINDS)
def test_worked_example(pair, ctx, kind):
    fugue = kind == "fugue"
    log = pu.new_log(fugue)
    log.insert(0, "abcdef")
    t = pair(log, fugue)
    b, d, c0, c1 = t.host.anchors_at([1, 4, 2, 3], [BEFORE, AFTER, BEFORE, AFTER])
    formats = [fmt(b, d, 1, 1, op_of(10, 1)), fmt(c0, c1, 1, 0, op_of(11, 2), REMOVE),
               fmt(START, END_, 2, 0xFF0000, op_of(3, 1))]
    sp, at, pend = t.spans(t.ref(), formats)
    assert (len(sp), len(at), pend) == (5, 7, 0)
    s = ctx.format_stats()
    assert (s["formats"], s["pending"], s["segments"], s["spans"], s["ranks"]) == (3, 0, 5, 5, 6)
    assert s["device_ns"] > 0
    t.edit([(2, 1, "")])                                # "c" dies: b and d are neighbours
    assert t.rep.spans(formats) == t.host.spans(formats) == \
        ([(0, 1, 0, 1, {2: 0xFF0000}), (1, 2, 1, 2, {1: 1, 2: 0xFF0000}), (3, 2, 3, 2, {2: 0xFF0000})], 0)
    t.spans(t.ref(), formats)
    assert ctx.format_stats()["segments"] == 5 and ctx.format_stats()["spans"] == 3
    t.edit([(3, 0, "X")])                               # right after "d": outside F1
    assert t.spans(t.ref(), formats)[0]["len"].tolist() == [1, 2, 3]


@pytest.mark.parametrize("kind", KINDS)
def test_empty_replica_and_no_formats(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(pu.new_log(fugue), fugue)
    formats = [fmt(START, END_, 1, 1, 1), fmt((op_of(3, 1), AFTER), END_, 1, 1, 2)]
    assert t.spans(t.ref(), formats)[2] == 1            # nothing held: the identity is pending
    assert ctx.format_stats()["pending"] == 1 and ctx.format_stats()["ranks"] == 0
    t.edit([(0, 0, "€")])
    assert t.spans(t.ref(), formats)[0].tolist() == [(0, 0, 1, 3, 0, 1)]
    assert t.spans(t.ref(), [])[0].size == 0
    assert ctx.format_stats()["formats"] == 0
    t.edit([(0, 1, "")])                                # and that one item dead
    assert t.spans(t.ref(), formats)[0].size == 0


def tile_formats(ref: fu.FRef, rng: random.Random) -> list:
    """Formats whose ends sit on the items of ranks 4094..4098 and on ranks 1 and N, under both
    biases, over three keys, and the two EDGEs."""
    near = [k for k in (1, 2, 4094, 4095, 4096, 4097, 4098, ref.n - 1, ref.n) if 1 <= k <= ref.n]
    out, op = [fmt(START, END_, 7, 7, 1)], 2
    for a in near:
        for b in near:
            if a <= b:
                out.append(fmt((ref.ident_at_rank(a), rng.choice([AFTER, BEFORE])),
                               (ref.ident_at_rank(b), rng.choice([AFTER, BEFORE])),
                               rng.randrange(3), rng.choice([1, 2]), op_of(op, 0),
                               REMOVE if rng.random() < 0.2 else 0))
                op += 1
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ranks", [4095, 4096, 4097, 8193])
def test_tile_edges(pair, ctx, kind, ranks):
    fugue = kind == "fugue"
    n = ranks - 1
    # a dead stretch that spans rank 4096 where the log reaches it
    t = pair(fu.chain_log(fugue, n, [(min(4090, n - 3), min(4100, n - 1))], ranks), fugue)
    ref = t.ref()
    assert ref.order == list(range(1, n + 1))
    rng = random.Random(ranks)
    sp, _, _ = t.spans(ref, tile_formats(ref, rng))
    assert len(sp) >= 1 and ctx.format_stats()["ranks"] == n
    near = [k for k in range(1, n + 1) if min(k % 4096, 4096 - k % 4096) <= 70 or k in (1, n)]
    t.spans(ref, fu.random_formats(ref, rng, 257, 2, ranks=near))
    sp, _, _ = t.spans(ref, fu.random_formats(ref, rng, 65, 70))
    assert len(sp) > 20


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dead", [(1, 4100), (4090, 8191), (2, 8190)])
def test_dead_tiles(pair, kind, dead):
    """Tile 0 wholly dead, tile 1 wholly dead, and everything dead but the first and the last two
    items: segments with no visible item are dropped and do not break a run."""
    fugue = kind == "fugue"
    n = 8192
    alive = {1: (n - 1, n), 4090: (1, n), 2: (1, n - 1, n)}[dead[0]]   # visible 4-byte codepoints
    t = pair(fu.chain_log(fugue, n, [dead], 7, width4_at=alive), fugue)
    ref = t.ref()
    rng = random.Random(dead[0])
    t.spans(ref, tile_formats(ref, rng))
    ends = [1, 2, 3, 4089, 4090, 4095, 4096, 4097, 4100, 4101, 8189, 8190, 8191, 8192]
    sp, _, _ = t.spans(ref, fu.random_formats(ref, rng, 64, 1, ranks=ends))
    # X | all-dead Y | X across the dead stretch is one span
    lo, hi = dead
    if lo > 1:
        x = [fmt((ref.ident_at_rank(1), BEFORE), (ref.ident_at_rank(lo - 1), AFTER), 1, 1, 1),
             fmt((ref.ident_at_rank(lo), BEFORE), (ref.ident_at_rank(hi), AFTER), 2, 2, 2),
             fmt((ref.ident_at_rank(hi + 1), BEFORE), END_, 1, 1, 3)]
        sp, _, _ = t.spans(ref, x)
        assert len(sp) == 1 and int(sp[0]["len"]) == ref.len


@pytest.mark.parametrize("kind", KINDS)
def test_format_counts(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(pu.base_log(fugue), fugue)
    ref = t.ref()
    rng = random.Random(40)
    for count, keys in ((0, 1), (1, 1), (63, 2), (64, 1), (65, 70), (257, 2), (257, 70), (1000, 70),
                        (1000, 1)):
        formats = fu.random_formats(ref, rng, count, keys, absent=0.05 if count >= 257 else 0.0)
        sp, at, pend = t.spans(ref, formats)
        s = ctx.format_stats()
        assert (s["formats"], s["pending"], s["spans"]) == (count, pend, len(sp))
        assert s["ranks"] == (ref.n if count else 0)    # (no format: nothing is streamed)
        assert s["segments"] >= len(sp) and s["segments"] <= max(2 * count - 1, 0)
        if count >= 257:
            assert pend > 0 and (keys == 1 or len(sp) > 5)
    # one identity named by hundreds of formats
    x = ref.ident_at_rank(ref.n // 2)
    many = [fmt((x, rng.choice([AFTER, BEFORE])), END_, k % 3, k, op_of(k + 1, 0)) for k in range(300)] + \
           [fmt(START, (x, rng.choice([AFTER, BEFORE])), k % 3, k, op_of(k + 1, 1)) for k in range(300)]
    sp, _, _ = t.spans(ref, many)
    assert 1 <= len(sp) <= 3
    # a set that is nothing but pending
    gone = [fmt((op_of(k + 1, 0x7777), AFTER), END_, 1, 1, k) for k in range(100)]
    assert t.spans(ref, gone)[2] == 100
    s = ctx.format_stats()
    assert (s["pending"], s["segments"], s["spans"]) == (100, 0, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_after_each_way_the_order_changes(pair, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    fk = pu.jf.fork if fugue else pu.ju.fork
    t = pair(base, fugue, agent=1)
    rng = random.Random(11)
    kept = fu.random_formats(t.ref(), rng, 80, 3)
    t.rep.merge_inc()
    steps = [
        lambda: t.edit([(17, 0, "k")]),                                  # fast-path merge_inc
        lambda: t.join(fk(base, 2, 51, 60)),                             # full rebuild
        lambda: t.edit([(3, 1, "é")]),
        lambda: t.apply_diff(fk(base, 3, 52, 60)),                       # full rebuild
        lambda: t.edit([(40, 2, text_of(random.Random(3), 5000))]),      # more than a fast path takes
        lambda: t.edit([(2500, 0, "z")]),
    ]
    for i, step in enumerate(steps):
        step()
        ref = t.ref()
        sp, _, pend = t.spans(ref, kept)                # formats made before the change
        assert pend == 0 and len(sp) > 3
        kept = kept + fu.random_formats(ref, rng, 20, 3, op0=1000 * (i + 1))
        t.spans(ref, kept)
    if fugue:
        assert t.host.arrays().side.any()               # left children are among the items
    assert t.rep.merge_inc()[:2] == (ref.len, ref.nbytes)


@pytest.mark.parametrize("kind", KINDS)
def test_cross_peer_convergence(ctx, oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    fk = pu.jf.fork if fugue else pu.ju.fork
    a, b = crdt_hip.Replica(ctx, fk(base, 1, 61, 70)), crdt_hip.Replica(ctx, fk(base, 2, 62, 50))
    try:
        ra = fu.FRef(oracle, pu.replica_arrays(a, fugue))
        rb = fu.FRef(oracle, pu.replica_arrays(b, fugue))
        union = fu.random_formats(ra, random.Random(8), 90, 3, op0=1000) + \
            fu.random_formats(rb, random.Random(9), 90, 3, op0=2000)
        assert fu.check(b, rb, union)[2] > 0            # b lacks a's new items
        b.apply_diff(a.encode_diff(b.state_vector()))
        a.apply_diff(b.encode_diff(a.state_vector()))
        assert a.encode_diff([]) != b.encode_diff([])   # the same items, in different slots
        ga = fu.check(a, fu.FRef(oracle, pu.replica_arrays(a, fugue)), union)
        shuffled = list(union)
        random.Random(10).shuffle(shuffled)
        gb = fu.check(b, fu.FRef(oracle, pu.replica_arrays(b, fugue)), shuffled)
        assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()
        assert ga[2] == gb[2] == 0 and len(ga[0]) > 5
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_errors_on_the_device(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(fu.chain_log(fugue, 4200, [], 3, width4_at=(4095, 4096)), fugue)
    ref = t.ref()
    snap = (t.rep.encode_diff([]), t.rep.info())
    good = fmt((ref.ident_at_rank(4090), BEFORE), (ref.ident_at_rank(4100), AFTER), 1, 1, op_of(4, 1))
    for formats, code in fu.bad_formats(good):
        fu.fails(t.rep, formats, code)
        fu.fails(t.host, formats, code)                 # the host twin: the same code
        assert (t.rep.encode_diff([]), t.rep.info()) == snap
    many = np.zeros(65537, crdt_hip.FORMAT_DTYPE)
    many["start"]["id"], many["end"]["id"] = EDGE, EDGE
    many["op"] = np.arange(65537)
    fu.fails(t.rep, many, ERANGE)
    assert (t.rep.encode_diff([]), t.rep.info()) == snap
    # ESPACE sizes both outputs, and the second call succeeds
    formats = [good, fmt(START, END_, 2, 2, op_of(1, 1))]
    L, arr = crdt_hip.lib(), crdt_hip._formats_pack(formats)
    ns, na, pend = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
    sp, at = fu.outs(2, 3)
    was = (sp.tobytes(), at.tobytes())
    for out, cap, attrs, acap in ((None, 0, None, 0), (sp.ctypes.data, 2, at.ctypes.data, 3),
                                  (sp.ctypes.data, 3, None, 0)):
        assert L.crdt_hip_replica_spans(ctx._h, t.rep._h, arr.ctypes.data, 2, out, cap, C.byref(ns),
                                        attrs, acap, C.byref(na), C.byref(pend)) == ESPACE
        assert (ns.value, na.value, pend.value) == (3, 4, 77) and (sp.tobytes(), at.tobytes()) == was
    assert (t.rep.encode_diff([]), t.rep.info()) == snap
    t.spans(ref, formats)
    other = crdt_hip.Context(ctx.device)                # a replica of another context
    try:
        sp, at = fu.outs(3, 4)
        was = (sp.tobytes(), at.tobytes())
        assert L.crdt_hip_replica_spans(other._h, t.rep._h, arr.ctypes.data, 2, sp.ctypes.data, 3,
                                        C.byref(ns), at.ctypes.data, 4, C.byref(na),
                                        C.byref(pend)) == EINVAL
        assert (ns.value, na.value, pend.value) == (3, 4, 77) and (sp.tobytes(), at.tobytes()) == was
    finally:
        other.close()
    assert (t.rep.encode_diff([]), t.rep.info()) == snap


def test_adapters():
    text = "héllo wörld, €uro 😀 and more"
    for cls, unit in ((crdt_hip.HipMerge, len), (crdt_hip.HipDownstream, len),
                      (crdt_hip.HipDownstreamBytes, lambda s: len(s.encode("utf-8")))):
        a = cls.from_str(text)
        b = a.clone()
        a.set_agent(1)
        b.set_agent(2)
        try:
            u = lambda k: unit(text[:k])
            bold = a.format(u(0), u(5), 1, 1)                       # "héllo", concurrently with
            link = b.format(u(3), u(11), 2, 7, expand=b.START | b.END)   # "lo wörld"
            assert bold & 0xFFFF == 1 and link & 0xFFFF == 2
            b.insert(u(11), "ZZ")                                    # at the link's expanding end
            a.insert(u(5), "!")                                      # right after the bold range
            assert a.sync_formats_from(b) == 1 and b.sync_formats_from(a) == 1
            assert a.spans()[1] == 0 and b.spans()[1] == 0          # (all anchors name base items)
            a.sync_from(b)
            b.sync_from(a)
            now = a.text()
            assert now == b.text() == "héllo! wörldZZ, €uro 😀 and more"
            w = lambda s, e: (unit(now[:s]), unit(now[s:e]))
            assert a.spans() == b.spans() == ([w(0, 3) + ({1: 1},), w(3, 5) + ({1: 1, 2: 7},),
                                               w(5, 14) + ({2: 7},)], 0)
            off = b.unformat(u(0), u(2), 1)
            assert off >> 16 > bold >> 16
            assert a.sync_formats_from(b) == 1
            assert a.spans() == b.spans() and a.spans()[0][0] == w(2, 3) + ({1: 1},)
        finally:
            for x in (a, b):
                if hasattr(x, "replica"):
                    x.replica.close()
