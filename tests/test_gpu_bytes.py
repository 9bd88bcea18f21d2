"""Byte-offset edits and patches on a device replica (crdt_hip_replica_apply_patches_bytes /
_replace_bytes / _patches_since_bytes; bytes.hip, the BYTES instantiation of patch.hip).

The parity check is rep.encode_diff([]) == host.encode_diff([]) after the host log got the same
patches in codepoints, one OpLog.replace each (the definition of the result), backed by the merged
text against a plain Python string model.  The byte patch lists come from that model
(bytes_util.to_bytes) and differ from the codepoint lists throughout.  The kernels stream the
document order in tiles of 4,096 ranks, so besides the ~300-item typed log the shapes are the
smallest that cross that tile: 9,000 items of mixed-width text with dead stretches around rank
4,096, and 3,000 patches over 6,001 ranks.
"""
import random

import pytest

import bytes_util as bu
import crdt_hip
import edit_util as eu
import patch_util as pu
from conftest import trace_path
from edit_util import KINDS
from test_gpu_edit import Pair, dead
from test_patches import TEXT, typed

pytestmark = pytest.mark.gpu


class BPair(Pair):
    """test_gpu_edit.Pair whose replica is edited in byte offsets."""

    def edit(self, plist, text: bool = True, differ: bool = True):
        plist_b = bu.to_bytes(self.text, plist)
        assert plist_b != plist or not differ or not plist
        eu.replace_loop(self.host, plist)
        assert self.rep.apply_patches_bytes(plist_b) == bu.counts(plist)
        self.text = eu.model_apply(self.text, plist)
        self.parity()
        if text:
            self.check_text()
        return plist_b

    def state(self):
        return self.rep.encode_diff([]), self.rep.info()


@pytest.fixture
def pair(ctx):
    made = []

    def make(log, fugue, agent=0):
        p = BPair(ctx, log, fugue, agent)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


def mixed(n: int, seed: int = 9) -> str:
    """`n` characters of 1 to 4 bytes, the first a 2-byte one."""
    return "é" + eu.text_of(random.Random(seed), n - 1)


@pytest.mark.parametrize("kind", KINDS)
def test_single_edits(pair, ctx, kind):
    fugue = kind == "fugue"
    n = len(TEXT)
    i2, i3, i4 = TEXT.index("é"), TEXT.index("€"), TEXT.index("😀")
    for p in [(n, 0, "end"), (n - 5, 5, ""), (i2 + 1, 1, "X"), (i2, 1, "x"), (i3 + 1, 2, "Y"),
              (i3 - 1, 2, ""), (i4 + 1, 1, "z"), (i4, 1, "€"), (i4 - 1, 3, "😀é")]:
        t = pair(typed(fugue), fugue)
        t.edit([p])
        s = ctx.edit_stats()
        assert (s["patches"], s["ranks"]) == (1, n) and s["device_ns"] > 0
    for p in [(0, 0, "é"), (0, 1, "")]:                # position 0: the same in bytes
        pair(typed(fugue), fugue).edit([p], differ=False)
    t = pair(pu.new_log(fugue), fugue)                 # the empty replica
    t.edit([(0, 0, "héllo")], differ=False)
    assert t.text == "héllo" and t.rep.apply_patches_bytes([]) == (0, 0)
    assert t.edit([(5, 0, "!")]) == [(6, 0, "!")]
    # insert, remove and replace are one patch each
    t = pair(typed(fugue), fugue)
    b = lambda k: bu.blen(TEXT[:k])                    # noqa: E731
    t.rep.insert_bytes(b(3), "aé")
    t.rep.remove_bytes(0, b(2))
    t.rep.replace_bytes(b(5), b(7), "€")               # ("laélo" is as long as "héllo")
    t.rep.replace_bytes(4, 4, "")                      # Upstream::replace of nothing: a no-op
    plist = [(3, 0, "aé"), (0, 2, ""), (5, 2, "€")]
    eu.replace_loop(t.host, plist)
    t.text = eu.model_apply(t.text, plist)
    t.parity()
    t.check_text()


def tile_text() -> str:
    """9,000 characters of mixed width with a 😀 on rank 4,095, the last of tile 0, and another on
    rank 4,096, the first of tile 1 (rank k holds character k - 1 of a log typed in one piece)."""
    text = mixed(9000)
    return text[:4094] + "😀😀" + text[4096:]


@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges(pair, kind):
    fugue = kind == "fugue"
    text = tile_text()
    # a delete range from tile 0 into tile 1, with dead ranks on both sides of rank 4096
    log = typed(fugue, text)
    dead(log, 4094, 4098)
    t = pair(log, fugue)
    t.edit([(4090, 8, "")])                            # ranks 4091..4093 and 4099..4103
    # a delete that ends exactly on the tile edge (rank 4095), then one that starts on it
    t = pair(typed(fugue, text), fugue)
    t.edit([(4090, 5, "ß")])
    t.edit([(4091, 3, "")])
    # a left neighbour on rank 4095 and another on rank 4096
    t = pair(typed(fugue, text), fugue)
    t.edit([(4095, 0, "L"), (4097, 0, "R")])
    # one delete over more than two whole tiles, between two inserts
    t = pair(typed(fugue, text), fugue)
    t.edit([(50, 0, "a"), (101, 8800, ""), (150, 0, "€b")])
    # a left neighbour followed by 9,000 dead ranks
    log = typed(fugue, text + "tail")
    dead(log, 3, 9002)
    t = pair(log, fugue)
    t.edit([(2, 0, "in"), (5, 1, "X")])


@pytest.mark.parametrize("kind", KINDS)
def test_boundaries_inside_a_codepoint_at_the_tile_edge(pair, kind):
    fugue = kind == "fugue"
    text = tile_text()
    t = pair(typed(fugue, text), fugue)
    before = t.state()
    for idx in (4094, 4095):                           # the 😀 of rank 4095 and that of rank 4096
        start = bu.blen(text[:idx])
        prev = bu.blen(text[:idx - 1])
        rows = [[(start + k, 0, 0, 1)] for k in (1, 2, 3)]          # pos inside it
        rows += [[(prev, 0, start - prev + k, 0)] for k in (1, 2, 3)]   # a del ending inside it
        rows += [[(start + 1, 0, 3, 0)]]               # a del from inside it to its end
        for r in rows:
            with pytest.raises(crdt_hip.CrdtHipError) as e:
                t.rep.apply_patches_bytes(*bu.raw(r, b"x"))
            assert e.value.code == -1, r
            assert t.state() == before, r
    t.edit([(4094, 1, "a"), (4096, 1, "é")])           # a valid edit afterwards still matches
    t.edit([(4094, 2, "😀")])


@pytest.mark.parametrize("kind", KINDS)
def test_many_patches(pair, ctx, kind):
    fugue = kind == "fugue"
    text, plist = bu.aeu(3000)                         # more patches than a workgroup has threads
    t = pair(typed(fugue, text), fugue)
    m = t.rep.mark()
    plist_b = t.edit(plist)
    assert t.text == "a€" * 3000 + "a" and plist_b[-1] == (1 + 4 * 2999, 2, "€")
    s = ctx.edit_stats()
    assert (s["patches"], s["items"], s["tombstones"], s["ranks"]) == (3000, 3000, 3000, 6001)
    assert s["device_ns"] > 0
    assert t.rep.patches_since_bytes(m) == plist_b
    s = ctx.patch_stats()
    assert (s["patches"], s["ins_bytes"], s["ranks"]) == (3000, 9000, 9001) and s["device_ns"] > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["join", "apply_diff"])
def test_edit_straight_after_a_sync(pair, kind, how):
    """No merge between the sync and the edit: the call rebuilds the kept order first."""
    fugue = kind == "fugue"
    base = typed(fugue, "héllo")
    other = base.clone()
    other.set_agent(2)
    other.insert(5, " wörld")
    other.remove(5, 6)
    t = pair(base, fugue, agent=1)
    getattr(t, how)(other)
    assert t.edit([(5, 0, "X€"), (8, 1, "")]) == [(6, 0, "X€"), (11, 2, "")]
    assert t.text == "hélloX€wrld"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2])
def test_random_patch_sets_between_joins(pair, kind, seed):
    fugue = kind == "fugue"
    rng = random.Random(170 + seed)
    log = eu.two_agent_log(fugue, rng.randint(5000, 9000), seed)
    log.insert(0, "é")
    t = pair(log, fugue, agent=5)
    other = log.clone()
    other.set_agent(6)
    for step in range(2):
        t.edit(bu.shifted(eu.random_patches(rng, len(t.text) - 1, rng.choice([30, 300]))),
               text=False)
        eu.replace_loop(other, bu.shifted(eu.random_patches(rng, other.visible_len() - 1, 10)))
        (t.join if step == 0 else t.apply_diff)(other)
        t.parity()
        t.edit(bu.shifted(eu.random_patches(rng, len(t.text) - 1, 5)), text=False)
    t.check_text()
    assert t.rep.info()[0] > 5000


@pytest.mark.parametrize("kind", KINDS)
def test_growth_keeps_marks(pair, kind):
    fugue = kind == "fugue"
    t = pair(typed(fugue), fugue)
    m = t.rep.mark()
    paste = eu.text_of(random.Random(5), 6000)         # a fresh replica holds 4,096 slots
    plist = [(3, 0, "ab"), (20, 4, paste)]
    plist_b = t.edit(plist)
    assert t.rep.patches_since_bytes(m) == plist_b and t.rep.patches_since(m) == plist


@pytest.mark.parametrize("kind", KINDS)
def test_rejected_calls_change_nothing(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(typed(fugue), fugue)
    before = t.state()
    for name, rows, ins, code in bu.rejections(TEXT):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            t.rep.apply_patches_bytes(*bu.raw(rows, ins))
        assert e.value.code == code, name
        assert t.state() == before, name
    for k in (1, 2, 3):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            t.rep.replace_bytes(bu.inside(TEXT, "😀") + k, bu.inside(TEXT, "😀") + 4, "")
        assert e.value.code == -1 and t.state() == before
    other = crdt_hip.Context(ctx.device)               # a replica of another context
    try:
        L = crdt_hip.lib()
        assert L.crdt_hip_replica_replace_bytes(other._h, t.rep._h, 0, 0, b"x", 1) == -1
        assert L.crdt_hip_replica_apply_patches_bytes(other._h, t.rep._h, None, 0, None, 0,
                                                      None, None) == -1
        assert t.state() == before
    finally:
        other.close()
    # the lamport bound is found on the device, after the boundary check
    arrs = crdt_hip.LogArrays([0], [0xFFFFFFF0], [1], [0], [ord("é")], side=[0] if fugue else None)
    big = crdt_hip.Replica(ctx, arrs)
    t.made.append(big)
    snap = (big.encode_diff([]), big.info())
    for pos, code in ((1, -1), (2, -2)):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            big.apply_patches_bytes([(pos, 0, "x" * 15)])
        assert e.value.code == code and (big.encode_diff([]), big.info()) == snap
    assert big.apply_patches_bytes([(2, 0, "x" * 14)]) == (14, 0)
    t.edit([(2, 1, "still fine")])


@pytest.mark.parametrize("kind", KINDS)
def test_patches_since_bytes_equals_the_host(ctx, kind):
    """The same array and the same bytes as the host call after an update, a join and a delta, on
    the 9,000-item document, with a run of D and I items that straddles the tile edge."""
    fugue = kind == "fugue"
    host = typed(fugue, tile_text())
    host.set_agent(1)
    rep = crdt_hip.Replica(ctx, host)
    made = [rep]
    try:
        dm, hm = rep.mark(), host.mark()
        assert rep.patches_since_bytes(dm) == []
        fork = host.clone()
        fork.set_agent(2)
        rng = random.Random(21)

        def same(at_least: int):
            raw = rep.patches_since_bytes_raw(dm)
            want = host.patches_since_bytes_raw(hm)
            assert pu.same_raw(raw, want) and len(raw[0]) >= at_least
            pu.assert_raw(raw)
            assert not pu.same_raw(raw, host.patches_since_raw(hm))
            assert pu.same_raw(rep.patches_since_raw(dm), host.patches_since_raw(hm))
            return crdt_hip._patch_list(raw)
        # an update: ranks 4093..4098 replaced (D items on both sides of the edge, then I items)
        v = host.version()
        host.replace(4092, 4098, "straddle€")
        eu.replace_loop(host, bu.shifted(eu.random_patches(rng, 4000, 20, max_gap=100)))
        rep.apply_updates([host.encode_from(v)])
        got = same(2)
        assert [d for _, d, i in got if i == "straddle€"] == [bu.blen(tile_text()[4092:4098])]
        s = ctx.patch_stats()
        assert s["patches"] == len(got) and s["ranks"] == rep.info()[0] and s["device_ns"] > 0
        # a join
        for k in range(40):                            # edits of tile 1 and tile 2 on the fork
            fork.replace(5000 + 60 * k, 5000 + 60 * k + k % 3, "j€"[: 1 + k % 2])
        other = crdt_hip.Replica(ctx, fork)
        made.append(other)
        assert rep.join(other) == host.join(fork)
        same(2)
        # a delta
        fork.insert(4500, "delta😀")
        fork.remove(10, 14)
        delta = fork.encode_diff(host.state_vector())
        assert rep.apply_diff(delta) == host.apply_diff(delta)
        same(2)
        assert rep.encode_diff([]) == host.encode_diff([])
    finally:
        for r in made:
            r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_between_two_byte_editors(ctx, kind):
    """A edits in bytes; B follows with sync_patches and splices the returned byte patches into a
    bytes buffer kept beside it; then the other way round."""
    fugue = kind == "fugue"
    base = typed(fugue, mixed(5000, 4))
    ra, rb = crdt_hip.Replica(ctx, base), crdt_hip.Replica(ctx, base)
    ra.set_agent(1)
    rb.set_agent(2)
    a, b = crdt_hip.HipDownstreamBytes(ra), crdt_hip.HipDownstreamBytes(rb)
    assert a.EDITS_USE_BYTE_OFFSETS and not crdt_hip.HipDownstream.EDITS_USE_BYTE_OFFSETS
    try:
        bufs = {id(a): a.text().encode(), id(b): b.text().encode()}
        rng = random.Random(6)
        for rnd in range(4):
            src, dst = (a, b) if rnd % 2 == 0 else (b, a)
            text = bufs[id(src)].decode()
            plist = bu.shifted(eu.random_patches(rng, len(text) - 1, rng.choice([1, 40])))
            plist_b = bu.to_bytes(text, plist)
            assert plist_b != plist
            if len(plist_b) == 1:
                pos, dele, ins = plist_b[0]
                src.replace(pos, pos + dele, ins)
            else:
                src.flush()
                src.replica.apply_patches_bytes(plist_b)
            bufs[id(src)] = bu.apply_bytes(bufs[id(src)], plist_b)
            assert src.text().encode() == bufs[id(src)] and src.len() == len(bufs[id(src)])
            got = dst.sync_patches(src)
            assert got
            bufs[id(dst)] = bu.apply_bytes(bufs[id(dst)], got)
            assert dst.text().encode() == bufs[id(dst)] == bufs[id(src)]
            assert dst.len() == len(bufs[id(dst)])
    finally:
        ra.close()
        rb.close()


def test_hip_downstream_bytes_is_an_upstream(ctx):
    """The windows of rustcode in which bytes and codepoints differ, through
    HipDownstreamBytes.replace from a trace that went through chars_to_bytes, one call each."""
    cp_trace = crdt_hip.Trace(trace_path("rustcode"))
    b_trace = crdt_hip.Trace(trace_path("rustcode"))
    b_trace.chars_to_bytes()
    ref = crdt_hip.HipMerge.from_str(cp_trace.start_content)
    done = 0
    for first, last, differs in bu.RUSTCODE_WINDOWS:
        assert cp_trace.patch(differs) != b_trace.patch(differs)
        bu.replay(cp_trace, ref.log, done, first)
        dev = crdt_hip.HipDownstreamBytes(crdt_hip.Replica(ctx, ref.log))
        try:
            for i in range(first, last):
                bu.replay(cp_trace, ref.log, i, i + 1)
                pos, dele, ins = b_trace.patch(i)
                dev.replace(pos, pos + dele, ins)
                if i == differs - 1:                   # a multi-byte character is in the document
                    assert dev.len() == bu.blen(ref.text()) != ref.len()
            assert dev.replica.encode_diff([]) == ref.log.encode_diff([])
            assert dev.text() == ref.text()
            assert dev.len() == bu.blen(ref.text())
        finally:
            dev.replica.close()
        done = last
