"""Local edits on a device replica (crdt_hip_replica_apply_patches / crdt_hip_replica_replace,
edit.hip).

The parity check throughout is rep.encode_diff([]) == host.encode_diff([]): the host log got the
same patches one OpLog.replace at a time (the definition of the result), and by the delta contract
the bytes are equal exactly when the logs are, slot for slot.  It is backed by the merged text
against a plain Python string model.  The kernels stream the document order in tiles of 4,096
ranks, so besides the ~300-item typed log the shapes are the smallest that cross that tile: 9,000
items with dead stretches around rank 4,096, 3,000 patches over 6,001 ranks, a paste of 5,000
codepoints (more than a fast-path merge_inc takes).
"""
import random

import pytest

import crdt_hip
import edit_util as eu
import patch_util as pu
from conftest import trace_path
from edit_util import KINDS
from test_patches import TEXT, typed

pytestmark = pytest.mark.gpu


class Pair:
    """A replica and the host log that holds the same items, with the model of their text."""

    def __init__(self, ctx, log: crdt_hip.OpLog, fugue: bool, agent: int = 0):
        self.ctx, self.fugue = ctx, fugue
        self.host = log.clone()
        self.host.set_agent(agent)
        self.rep = crdt_hip.Replica(ctx, log if log.view().n or fugue else None)
        if agent:
            self.rep.set_agent(agent)
        self.made = [self.rep]
        self.text = self.rep.merge()[0].decode("utf-8")
        self.parity()

    def close(self):
        for r in self.made:
            r.close()

    def parity(self):
        assert self.rep.encode_diff([]) == self.host.encode_diff([])
        assert self.rep.info()[0] == self.host.arrays().n
        assert self.rep.info()[1] == self.host.visible_len() == len(self.text)

    def check_text(self):
        assert self.rep.merge()[0].decode("utf-8") == self.text
        assert self.rep.info()[2] == len(self.text.encode("utf-8"))

    def edit(self, plist, text: bool = True):
        eu.replace_loop(self.host, plist)
        got = self.rep.apply_patches(plist)
        assert got == (sum(len(i) for _, _, i in plist), sum(d for _, d, _ in plist))
        self.text = eu.model_apply(self.text, plist)
        self.parity()
        if text:
            self.check_text()

    def join(self, other: crdt_hip.OpLog):
        o = crdt_hip.Replica(self.ctx, other)
        self.made.append(o)
        assert self.rep.join(o) == self.host.join(other)
        self.text = self.ctx.merge(self.host)[0].decode("utf-8")

    def apply_diff(self, other: crdt_hip.OpLog):
        delta = other.encode_diff(self.host.state_vector())
        assert self.rep.apply_diff(delta) == self.host.apply_diff(delta)
        self.text = self.ctx.merge(self.host)[0].decode("utf-8")


@pytest.fixture
def pair(ctx):
    made = []

    def make(log, fugue, agent=0):
        p = Pair(ctx, log, fugue, agent)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("kind", KINDS)
def test_single_edits(pair, ctx, kind):
    fugue = kind == "fugue"
    n = len(TEXT)
    for p in [(0, 0, "é"), (n // 2, 0, "mid"), (n, 0, "end"), (0, 1, ""), (n - 1, 1, ""), (0, n, ""),
              (4, 2, "X€"), (n - 2, 2, "😀z")]:
        t = pair(typed(fugue), fugue)
        t.edit([p])
        assert ctx.edit_stats()["patches"] == 1 and ctx.edit_stats()["ranks"] == n
    t = pair(pu.new_log(fugue), fugue)                 # the empty replica
    t.edit([(0, 0, "héllo")])
    assert t.text == "héllo" and t.rep.apply_patches([]) == (0, 0)
    t.edit([(5, 0, "!")])
    # insert, remove and replace are one patch each
    t = pair(typed(fugue), fugue)
    t.rep.insert(3, "ab")
    t.rep.remove(0, 2)
    t.rep.replace(5, 7, "€")
    t.rep.replace(2, 2, "")                            # Upstream::replace of nothing: a no-op
    eu.replace_loop(t.host, [(3, 0, "ab"), (0, 2, ""), (5, 2, "€")])
    t.text = eu.model_apply(t.text, [(3, 0, "ab"), (0, 2, ""), (5, 2, "€")])
    t.parity()
    t.check_text()


@pytest.mark.parametrize("kind", KINDS)
def test_agent_of_the_new_identities(pair, kind):
    fugue = kind == "fugue"
    t = pair(typed(fugue), fugue)
    top = max(l for _, l in t.rep.state_vector())
    t.edit([(3, 0, "q")])                              # the default agent is 0
    assert t.rep.state_vector() == [(0, top + 1)]
    t.rep.set_agent(7)
    t.host.set_agent(7)
    t.edit([(1, 1, "rs")])
    assert t.rep.state_vector() == [(0, top + 1), (7, top + 3)]
    c = t.rep.clone()                                  # a clone keeps the agent
    t.made.append(c)
    c.insert(0, "x")
    assert c.state_vector() == [(0, top + 1), (7, top + 4)]


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_with_patches_since(pair, kind):
    fugue = kind == "fugue"
    hand = [(0, 2, "A€"), (9, 0, "😀"), (14, 3, ""), (20, 1, "xyz")]
    t = pair(typed(fugue), fugue)
    m = t.rep.mark()
    t.edit(hand)
    assert t.rep.patches_since(m) == hand
    # the patches a fork's join gives a host log, applied to a replica that holds the marked text
    base = pu.base_log(fugue)
    fork = (pu.jf if fugue else pu.ju).fork(base, 3, 77, 120)
    seen = base.clone()
    hm = seen.mark()
    seen.join(fork)
    plist = seen.patches_since(hm)
    assert len(plist) > 20
    t = pair(base, fugue, agent=4)
    m = t.rep.mark()
    t.edit(plist)
    assert t.rep.patches_since(m) == plist
    assert t.text == t.ctx.merge(fork)[0].decode("utf-8")


@pytest.mark.parametrize("kind", KINDS)
def test_257_tiles(ctx, kind):
    """Ranks 0..1,048,700 are 257 tiles: k_edit_top scans the tile counts in two rounds of 256, and
    the last patch lies in tile 256, the first of the second round, whose visible ranks need the
    carry of the first.  Device against the host twin slot for slot, and the round trip through
    patches_since byte for byte."""
    fugue = kind == "fugue"
    plist = [(5, 2, "Q"), (4095, 3, ""), (1_048_600, 0, "tail")]
    host = typed(fugue, (eu.ALPHABET * (1_048_700 // len(eu.ALPHABET) + 1))[:1_048_700])
    rep = crdt_hip.Replica(ctx, host)
    try:
        dm, hm = rep.mark(), host.mark()
        assert rep.apply_patches(plist) == host.apply_patches(plist) == (5, 5)
        s = ctx.edit_stats()
        assert (s["patches"], s["items"], s["tombstones"], s["ranks"]) == (3, 5, 5, 1_048_700)
        assert rep.encode_diff([]) == host.encode_diff([])
        raw = rep.patches_since_raw(dm)
        assert pu.same_raw(raw, host.patches_since_raw(hm))
        assert crdt_hip._patch_list(raw) == plist
    finally:
        rep.close()


def dead(log: crdt_hip.OpLog, first: int, last: int) -> None:
    """Tombstones the items of ranks first..last of a log typed in one piece and not edited since
    (rank k = item k), given that every rank below `first` is still visible."""
    log.remove(first - 1, last)


@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges(pair, kind):
    fugue = kind == "fugue"
    text = eu.text_of(random.Random(9), 9000)
    # a delete range from tile 0 into tile 1, with dead ranks on both sides of rank 4096
    log = typed(fugue, text)
    dead(log, 4094, 4098)
    t = pair(log, fugue)
    t.edit([(4090, 8, "")])                            # ranks 4091..4093 and 4099..4103
    # a left neighbour on rank 4095 and another on rank 4096; in a typed Fugue log every item has
    # a right child, so the first is anchored to its successor, the first rank of the next tile
    t = pair(typed(fugue, text), fugue)
    t.edit([(4095, 0, "L"), (4097, 0, "R")])
    if fugue:
        A = t.host.arrays()
        assert (A.parent[-2], A.side[-2]) == (4096, 1) and (A.parent[-1], A.side[-1]) == (4097, 1)
    # one delete over more than two whole tiles, between two inserts
    t = pair(typed(fugue, text), fugue)
    t.edit([(50, 0, "a"), (101, 8800, ""), (150, 0, "€b")])
    # a left neighbour followed by 9,000 dead ranks (Fugue: its successor is a tombstone)
    log = typed(fugue, text + "tail")
    dead(log, 3, 9002)
    t = pair(log, fugue)
    t.edit([(2, 0, "in"), (5, 1, "X")])
    if fugue:
        A = t.host.arrays()
        assert (A.parent[-3], A.side[-3], A.deleted[2]) == (3, 1, 1)
    # the last rank of the document as a left neighbour and as a deleted item
    t = pair(typed(fugue, text[:4096]), fugue)         # ranks 0..4096: two tiles, the second of one
    t.edit([(4095, 1, "")])
    t.edit([(4095, 0, "zz")])


@pytest.mark.parametrize("kind", KINDS)
def test_many_patches(pair, ctx, kind):
    fugue = kind == "fugue"
    text, plist = eu.interleaved(3000)                 # more patches than a workgroup has threads
    t = pair(typed(fugue, text), fugue)
    t.edit(plist)
    assert t.text == "aX" * 3000 + "a"
    s = ctx.edit_stats()
    assert (s["patches"], s["items"], s["tombstones"], s["ranks"]) == (3000, 3000, 3000, 6001)
    assert s["device_ns"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_large_paste_then_a_keystroke(pair, ctx, kind):
    fugue = kind == "fugue"
    paste = eu.text_of(random.Random(3), 5000)         # more than kIncMax items
    assert len({len(c.encode()) for c in paste}) == 4
    t = pair(typed(fugue), fugue)
    # a twin replica brought to the same state and given the same changes as wire updates
    w = crdt_hip.Replica(ctx, t.host)
    t.made.append(w)
    for plist in ([(10, 2, paste)], [(2500, 0, "k")]):
        v = t.host.version()
        w.merge_inc()                                  # (apply_patches brings the order up to date)
        t.edit(plist, text=False)
        w.apply_updates([t.host.encode_from(v)])
        cps, nbytes, path, data = t.rep.merge_inc(text=True)
        assert data.decode("utf-8") == t.text and cps == len(t.text)
        assert w.merge_inc(text=True) == (cps, nbytes, path, data)
    t.check_text()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["join", "apply_diff"])
@pytest.mark.parametrize("dead_successor", [False, True])
def test_edit_straight_after_a_sync(pair, kind, how, dead_successor):
    """No merge between the sync and the edit.  The other side typed after the last item, which
    therefore gained a right child through the sync: a Fugue insert after it becomes a left child
    of its successor, the other side's first character (tombstoned or not)."""
    fugue = kind == "fugue"
    base = typed(fugue, "hello")
    other = base.clone()
    other.set_agent(2)
    other.insert(5, " world")
    if dead_successor:
        other.remove(5, 6)
    t = pair(base, fugue, agent=1)
    getattr(t, how)(other)
    t.edit([(5, 0, "XY"), (9, 1, "")])
    A = t.host.arrays()
    assert t.text == ("helloXYwold" if dead_successor else "helloXY wrld")
    if fugue:
        assert (A.parent[-2], A.side[-2], A.deleted[5]) == (6, 1, int(dead_successor))
    else:
        assert A.parent[-2] == 5


@pytest.mark.parametrize("kind", KINDS)
def test_two_editing_replicas_converge(pair, ctx, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    rng = random.Random(12)
    a, b = pair(base, fugue, agent=1), pair(base, fugue, agent=2)
    for _ in range(2):
        a.edit(eu.random_patches(rng, len(a.text), 25), text=False)
        b.edit(eu.random_patches(rng, len(b.text), 25), text=False)
    da, db = crdt_hip.HipDownstream(a.rep), crdt_hip.HipDownstream(b.rep)
    b0 = b.host.clone()
    b.host.apply_diff(a.host.encode_diff(b.host.state_vector()))
    a.host.apply_diff(b0.encode_diff(a.host.state_vector()))
    rb = b.rep.clone()
    b.made.append(rb)
    db.sync_from(da)
    da.sync_from(crdt_hip.HipDownstream(rb))
    assert da.text() == db.text() == ctx.merge(a.host)[0].decode("utf-8") == \
        ctx.merge(b.host)[0].decode("utf-8")
    assert a.rep.encode_diff([]) == a.host.encode_diff([])
    assert b.rep.encode_diff([]) == b.host.encode_diff([])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_patch_sets_between_joins(pair, kind, seed):
    fugue = kind == "fugue"
    rng = random.Random(70 + seed)
    log = eu.two_agent_log(fugue, rng.randint(2000, 9000), seed)
    t = pair(log, fugue, agent=5)
    other = log.clone()
    other.set_agent(6)
    for step in range(3):
        t.edit(eu.random_patches(rng, len(t.text), rng.choice([1, 30, 300])), text=step == 2)
        eu.replace_loop(other, eu.random_patches(rng, other.visible_len(), 10))
        (t.join if step % 2 == 0 else t.apply_diff)(other)
        t.parity()
        t.edit(eu.random_patches(rng, len(t.text), 5), text=False)
    t.check_text()


@pytest.mark.parametrize("kind", KINDS)
def test_growth_keeps_marks_and_clones(pair, kind):
    fugue = kind == "fugue"
    t = pair(typed(fugue), fugue)
    m = t.rep.mark()
    c = t.rep.clone()
    t.made.append(c)
    before = c.encode_diff([])
    paste = eu.text_of(random.Random(5), 6000)         # a fresh replica holds 4,096 slots
    t.edit([(3, 0, "ab"), (20, 4, paste)])
    assert t.rep.patches_since(m) == [(3, 0, "ab"), (20, 4, paste)]
    assert c.encode_diff([]) == before and c.merge()[0].decode("utf-8") == TEXT


@pytest.mark.parametrize("kind", KINDS)
def test_rejected_calls_change_nothing(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(typed(fugue), fugue)
    n = len(TEXT)
    before = (t.rep.encode_diff([]), t.rep.info())
    for name, rows, ins, code in eu.rejections(n):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            t.rep.apply_patches(*eu.raw(rows, ins))
        assert e.value.code == code, name
        assert (t.rep.encode_diff([]), t.rep.info()) == before, name
        with pytest.raises(crdt_hip.CrdtHipError) as e:  # the host twin: the same code
            t.host.apply_patches(*eu.raw(rows, ins))
        assert e.value.code == code, name
    other = crdt_hip.Context(ctx.device)               # a replica of another context
    try:
        for call in (lambda: crdt_hip.lib().crdt_hip_replica_replace(other._h, t.rep._h, 0, 0, b"x", 1),
                     lambda: crdt_hip.lib().crdt_hip_replica_apply_patches(
                         other._h, t.rep._h, None, 0, None, 0, None, None)):
            assert call() == -1
            assert (t.rep.encode_diff([]), t.rep.info()) == before
    finally:
        other.close()
    # the lamport bound is found on the device, before anything is written
    arrs = crdt_hip.LogArrays([0], [0xFFFFFFF0], [1], [0], [ord("a")], side=[0] if fugue else None)
    big = crdt_hip.Replica(ctx, arrs)
    t.made.append(big)
    snap = (big.encode_diff([]), big.info())
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        big.apply_patches([(1, 0, "x" * 15)])
    assert e.value.code == -2 and (big.encode_diff([]), big.info()) == snap
    assert big.apply_patches([(1, 0, "x" * 14)]) == (14, 0)
    t.edit([(1, 1, "still fine")])


def test_hip_downstream_is_an_upstream():
    """The first 200 patches of automerge-paper through HipDownstream.replace, one call each."""
    tr = crdt_hip.Trace(trace_path("automerge-paper"))
    dev = crdt_hip.HipDownstream.from_str(tr.start_content)
    ref = crdt_hip.HipMerge.from_str(tr.start_content)
    try:
        for i in range(200):
            pos, dele, ins = tr.patch(i)
            dev.replace(pos, pos + dele, ins)
            ref.replace(pos, pos + dele, ins)
            if i % 40 == 39:
                assert dev.len() == ref.len()
        dev.insert(0, "é")
        ref.insert(0, "é")
        dev.remove(1, 3)
        ref.remove(1, 3)
        assert dev.len() == ref.len() and dev.text() == ref.text()
        assert dev.replica.encode_diff([]) == ref.log.encode_diff([])
    finally:
        dev.replica.close()
