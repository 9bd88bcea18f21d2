"""Anchors on the host (crdt_hip_oplog_anchors_at / _at_bytes / _resolve).

A cursor or a selection end is a place in the text, named by the identity of the item next to the
gap, that keeps its meaning while every peer edits around it.  Expected anchors and positions are
computed without the product (anchor_util.Ref over the CPU oracle's document order); every
comparison is of exact integers, the raw arrays byte for byte.  CPU only.
"""
import random

import numpy as np
import pytest

import anchor_util as au
import crdt_hip
import patch_util as pu
from anchor_util import EINVAL, ERANGE
from crdt_hip import AFTER, BEFORE, DEAD, EDGE, LIVE, UNKNOWN
from edit_util import KINDS, text_of


def ref_of(oracle, log) -> au.Ref:
    return au.Ref(oracle, log.arrays())


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_every_gap(oracle, kind):
    log = pu.base_log(kind == "fugue")                 # ~300 items, mixed width, tombstones
    ref = ref_of(oracle, log)
    assert ref.len < log.arrays().n and ref.nbytes > ref.len
    pos, bias = au.all_gaps(ref)
    back = au.check_resolve(log, ref, au.check_at(log, ref, pos, bias))
    assert back["pos"].tolist() == pos and set(back["state"].tolist()) == {LIVE}
    # in bytes: every codepoint boundary round-trips, every offset inside a codepoint is EINVAL
    bpos, bbias = au.all_gaps(ref, bytes=True)
    back = au.check_resolve(log, ref, au.check_at(log, ref, bpos, bbias, bytes=True))
    assert back["pos_bytes"].tolist() == bpos
    assert log.anchors_at_bytes_raw(bpos, bbias).tobytes() == log.anchors_at_raw(pos, bias).tobytes()
    inside = ref.insides()
    assert len(inside) > 100
    for p in inside:
        for b in (AFTER, BEFORE):
            out = au.raw_anchors([(7, 1), (9, 0)])
            au.fails(lambda o: log.anchors_at_bytes_raw([0, p], b, out=o), EINVAL, out)
    # the list forms and the default bias
    assert log.anchors_at([0, 3]) == [ref.at(0, AFTER), ref.at(3, AFTER)]
    assert log.anchors_at([3], BEFORE) == [ref.at(3, BEFORE)]
    assert log.resolve_anchors([ref.at(3, BEFORE)]) == [ref.resolve(ref.at(3, BEFORE))]
    assert log.anchors_at_bytes([ref.ends[5]], BEFORE) == [ref.at(5, BEFORE)]


@pytest.mark.parametrize("kind", KINDS)
def test_stickiness(oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    n = base.visible_len()
    for p in (0, 1, n // 2, n - 1, n):
        for ins in ("x", "é€😀k"):
            log = base.clone()
            after, before = log.anchors_at([p], AFTER)[0], log.anchors_at([p], BEFORE)[0]
            log.insert(p, ins)                          # at the very gap
            ref = ref_of(oracle, log)
            got = au.check_resolve(log, ref, [after, before])
            assert got["pos"].tolist() == [p, p + len(ins)]
            assert set(got["state"].tolist()) == {LIVE}
    for p in (1, n // 2, n):                            # delete the anchored item (the p-th)
        log = base.clone()
        ref0 = ref_of(oracle, log)
        a = log.anchors_at([p, p - 1], [AFTER, BEFORE])
        assert a[0][0] == a[1][0] != EDGE               # both name the p-th visible item
        assert [r[0] for r in log.resolve_anchors(a)] == [p, p - 1]
        log.remove(p - 1, p)
        ref = ref_of(oracle, log)
        got = au.check_resolve(log, ref, a)
        assert got["pos"].tolist() == [p - 1, p - 1] and got["state"].tolist() == [DEAD, DEAD]
        assert got["pos_bytes"].tolist() == [ref0.ends[p - 1]] * 2
    # an anchor on an item that was deleted before the call resolves the same under either bias
    log = base.clone()
    arrs = log.arrays()
    dead = [s for s in range(arrs.n) if arrs.deleted[s]]
    assert dead
    ref = ref_of(oracle, log)
    for s in dead:
        ident = (int(arrs.lamport[s]) << 16) | int(arrs.agent[s])
        got = au.check_resolve(log, ref, [(ident, AFTER), (ident, BEFORE)])
        assert got[0].tobytes()[:20] == got[1].tobytes()[:20] and got["state"].tolist() == [DEAD] * 2


@pytest.mark.parametrize("kind", KINDS)
def test_convergence(oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    f = pu.jf.fork if fugue else pu.ju.fork
    a, b = f(base, 1, 31, 80), f(base, 2, 32, 70)
    # both type at the same gap of the common text, then at gaps of their own
    a.insert(0, "Aé")
    b.insert(0, "B€")
    rng = random.Random(5)
    made = []
    for log in (a, b):
        n = log.visible_len()
        pos = [0, n] + [rng.randint(0, n) for _ in range(40)]
        bias = [rng.choice([AFTER, BEFORE]) for _ in pos]
        made.append(au.check_at(log, ref_of(oracle, log), pos, bias))
    anchors = np.concatenate(made)
    # the other side's own items are unknown before the sync
    own_b = [(((int(l) << 16) | 2), AFTER) for l, g in zip(b.arrays().lamport, b.arrays().agent) if g == 2]
    assert own_b and all(st == UNKNOWN for _, _, st in a.resolve_anchors(own_b))
    assert a.resolve_anchors(own_b) == [(0, 0, UNKNOWN)] * len(own_b)
    b0 = b.clone()
    b.join(a)                                           # a join one way
    a.apply_diff(b0.encode_diff(a.state_vector()))      # a delta the other
    ra, rb = ref_of(oracle, a), ref_of(oracle, b)
    ga, gb = au.check_resolve(a, ra, anchors), au.check_resolve(b, rb, anchors)
    assert ga.tobytes() == gb.tobytes()
    assert UNKNOWN not in ga["state"].tolist()
    assert all(st != UNKNOWN for _, _, st in a.resolve_anchors(own_b))
    live_b = [x for x in own_b if rb.resolve(x)[2] == LIVE]
    assert live_b and a.resolve_anchors(live_b) == b.resolve_anchors(live_b)


@pytest.mark.parametrize("kind", KINDS)
def test_argument_errors(oracle, kind):
    log = pu.base_log(kind == "fugue")
    n, nb = log.visible_len(), log.visible_bytes()
    out = au.raw_anchors([(1, 1)] * 3)
    au.fails(lambda o: log.anchors_at_raw([0, n + 1, 2], AFTER, out=o), ERANGE, out)
    au.fails(lambda o: log.anchors_at_raw([0, n, 2], [0, 2, 1], out=o), EINVAL, out)
    au.fails(lambda o: log.anchors_at_bytes_raw([0, nb + 1, 2], BEFORE, out=o), ERANGE, out)
    au.fails(lambda o: log.anchors_at_bytes_raw([0, nb, 2], [0, 1, 2], out=o), EINVAL, out)
    good = log.anchors_at_raw([0, n, 2], [0, 1, 1], out=out)
    assert good is out and out[1]["id"] == EDGE
    pout = au.raw_positions([(5, 5, 1)] * 3)
    for bad in ((1 << 48, AFTER, 0), (out[2]["id"], 2, 0), (out[2]["id"], BEFORE, 1),
                (EDGE - 1, AFTER, 0)):
        arr = out.copy()
        arr[1] = bad
        au.fails(lambda o: log.resolve_anchors_raw(arr, out=o), EINVAL, pout)
    assert log.resolve_anchors_raw(out, out=pout)["pos"].tolist() == [0, n, 2]
    # n == 0 is ok
    assert log.anchors_at([]) == [] and log.anchors_at_bytes([]) == [] and log.resolve_anchors([]) == []


@pytest.mark.parametrize("kind", KINDS)
def test_empty_log(oracle, kind):
    log = pu.new_log(kind == "fugue")
    assert log.anchors_at([0, 0], [AFTER, BEFORE]) == [(EDGE, AFTER), (EDGE, BEFORE)]
    assert log.anchors_at_bytes([0, 0], [AFTER, BEFORE]) == [(EDGE, AFTER), (EDGE, BEFORE)]
    assert log.resolve_anchors([(EDGE, AFTER), (EDGE, BEFORE), (5 << 16, AFTER)]) == \
        [(0, 0, LIVE), (0, 0, LIVE), (0, 0, UNKNOWN)]
    out = au.raw_anchors([(3, 1)])
    au.fails(lambda o: log.anchors_at_raw([1], AFTER, out=o), ERANGE, out)


@pytest.mark.parametrize("kind", KINDS)
def test_index_and_contents_are_untouched(oracle, kind):
    fugue = kind == "fugue"
    log = pu.base_log(fugue)
    twin = log.clone()
    before = (log.encode_diff([]), log.encode_from(0), log.version(), log.visible_len())
    ref = ref_of(oracle, log)
    pos, bias = au.all_gaps(ref)
    anchors = log.anchors_at_raw(pos, bias)
    log.anchors_at_bytes_raw(*au.all_gaps(ref, bytes=True))
    log.resolve_anchors_raw(anchors)
    assert (log.encode_diff([]), log.encode_from(0), log.version(), log.visible_len()) == before
    # the positional index still answers as the twin's, which no anchor call touched
    for l in (log, twin):
        l.insert(17, text_of(random.Random(2), 5))
        l.remove(3, 9)
    assert log.encode_diff([]) == twin.encode_diff([])
    # and after a join, which leaves the index stale, the calls do not rebuild or disturb it
    other = (pu.jf.fork if fugue else pu.ju.fork)(twin, 3, 9, 40)
    for l in (log, twin):
        l.join(other)
    log.resolve_anchors_raw(log.anchors_at_raw([0, 5, log.visible_len()], BEFORE))
    for l in (log, twin):
        l.insert(11, "zz")
    assert log.encode_diff([]) == twin.encode_diff([])


def test_two_slots_of_one_identity_the_lower_wins():
    """Of two slots of a malformed log that share an identity, an anchor names the lower one."""
    log = au.shared_identity_log()
    assert log.resolve_anchors([(au.SHARED, AFTER), (au.SHARED, BEFORE)]) == [(2, 2, LIVE), (1, 1, LIVE)]
    log.remove(1, 2)
    assert log.resolve_anchors([(au.SHARED, AFTER), (au.SHARED, BEFORE)]) == [(1, 1, DEAD)] * 2
    assert log.text_at() == b"acx"
