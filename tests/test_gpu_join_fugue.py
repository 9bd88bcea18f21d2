"""Device join of two Fugue replicas (crdt_hip_replica_join, join.hip).

dst <- dst U src by item identity (lamport, agent) = key & ~kLeftKey; the side bit of the key
(and of the codepoint word) is an attribute that comes along.  Expected results are computed
without the product: the union log is built in Python (join_fugue_util.union) from the forks'
arrays and merged by the CPU oracle's Fugue walk; the joined replica's text, digest and info()
must match it, and match a replica uploaded from the host join's log (OpLog.join), which the
device join must equal slot for slot.  Sizes are the smallest that reach each code path.
"""
import random

import numpy as np
import pytest

import crdt_hip
import join_util
from conftest import trace_path
from join_fugue_util import (assert_cases, assert_same_log, assert_unique_identities, crafted,
                             empty_arrays, expect, fork, merged, scripted_forks, union)
from join_util import random_edits

pytestmark = pytest.mark.gpu


def check(oracle, rep, arrs):
    text, dig, info = expect(oracle, arrs)
    got_text, got_dig = rep.merge()
    assert got_text == text
    assert got_dig == dig
    assert rep.info() == info


@pytest.fixture
def mk(ctx):
    """Replica factory (also takes a made replica or update batch) that closes what it made when
    the test ends: a replica must be freed before its context.  Without an argument: an empty
    Fugue replica."""
    made = []

    def make(init=None, context=None):
        if init is None:
            init = empty_arrays()
        r = (init if isinstance(init, (crdt_hip.Replica, crdt_hip.UpdateBatch))
             else crdt_hip.Replica(context or ctx, init))
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def host_join(dst, *srcs):
    out = dst.clone()
    for s in srcs:
        out.join(s)
    return out


@pytest.fixture(scope="module")
def forks():
    base, nb, a, b = scripted_forks(more=(150, 80))
    c = fork(base, 3, 33, 60)
    assert_unique_identities(a.arrays(), b.arrays(), c.arrays())
    return base, nb, a, b, c


@pytest.mark.parametrize("contraction", [1, 2])
def test_join_reaches_every_case(ctx, mk, oracle, forks, contraction):
    base, nb, a, b, _ = forks
    A, B = a.arrays(), b.arrays()
    want, added, tomb = union(A, B)
    assert_cases(base.arrays(), A, B, want)
    assert added == B.n - nb and tomb > 0
    ctx.set_param("contraction", contraction)
    try:
        dst, src = mk(a), mk(b)
        src_before = (src.merge(), src.info())
        assert dst.join(src) == (added, tomb)
        st = ctx.join_stats()
        assert st["prefix_slots"] == nb and st["table_slots"] == A.n - nb
        check(oracle, dst, want)
        assert (src.merge(), src.info()) == src_before
        # the host join gives the same log, and a replica uploaded from it the same result
        hj = host_join(a, b)
        assert_same_log(hj.arrays(), want)
        up = mk(hj)
        assert up.merge() == dst.merge() and up.info() == dst.info()
        # the document differs from both forks' (a previous-slot flag wrongly set on the left
        # child that follows its parent's slot would show in the text checked above)
        assert dst.merge()[0] not in (src_before[0][0], merged(oracle, A))
    finally:
        ctx.set_param("contraction", 0)


def test_forks_of_an_empty_replica(ctx, mk, oracle):
    """Concurrent right children of the document start: both forks typed into an empty log."""
    a, b = crdt_hip.OpLog(fugue=True, agent=1), crdt_hip.OpLog(fugue=True, agent=2)
    a.insert(0, "ab€")
    a.insert(0, "<")
    b.insert(0, "xy")
    b.insert(2, "😀")
    want, added, tomb = union(a.arrays(), b.arrays())
    assert ((want.parent == 0) & (want.side == 0)).sum() == 2
    dst = mk(a)
    assert dst.join(mk(b)) == (added, tomb) == (b.arrays().n, 0)
    check(oracle, dst, want)
    assert dst.merge()[0].decode() == "xy😀<ab€"
    assert_same_log(host_join(a, b).arrays(), want)
    other = mk(b)
    other.join(mk(a))
    assert other.merge() == dst.merge()


def test_shared_items_past_the_prefix_go_through_the_table(ctx, mk, oracle, forks):
    """C = A U B, then C U B' with B' = B + more edits: B's own items lie past the common prefix
    of C and B' (the base), at other slots in each, so the lookup finds them in the table by
    their masked keys (left children among them)."""
    _, nb, a, b, _ = forks
    b2 = b.clone()
    random_edits(b2, random.Random(77), 40)
    assert (b.arrays().side[nb:] == 1).any()
    ab, _, _ = union(a.arrays(), b.arrays())
    want, added, tomb = union(ab, b2.arrays())
    assert 0 < added == b2.arrays().n - b.arrays().n
    c, rb, rb2 = mk(a), mk(b), mk(b2)
    c.join(rb)
    assert c.join(rb2) == (added, tomb)
    st = ctx.join_stats()
    assert st["prefix_slots"] == nb and st["table_slots"] == ab.n - nb
    assert st["table_capacity"] >= 2 * st["table_slots"]
    check(oracle, c, want)
    hj = host_join(a, b, b2)
    assert_same_log(hj.arrays(), want)
    up = mk(hj)
    assert up.merge() == c.merge() and up.info() == c.info()


def test_prefix_keys_not_below_the_rest_take_the_full_table(ctx, mk, oracle, forks):
    """Y = A U B holds B's items (small lamports) behind A's (large ones); Z = A + local edits.
    The common prefix of Y and Z is the whole of A, and Y's items past it do not exceed its keys:
    the join runs again with every slot in the table.  Among Y's items past the prefix is a left
    child with a lamport below the prefix's largest: its raw key (bit 48) is above every prefix
    key, so only the masked comparison sees it."""
    _, nb, a, b, _ = forks
    z = a.clone()
    random_edits(z, random.Random(88), 30)
    y = host_join(a, b)
    Y, Z = y.arrays(), z.arrays()
    na = a.arrays().n
    tail_left = Y.side[na:] == 1
    assert (Y.lamport[na:][tail_left] < Y.lamport[:na].max()).any()
    want, added, tomb = union(Y, Z)
    ry, rz = mk(y), mk(z)
    assert ry.join(rz) == (added, tomb)
    assert ctx.join_stats()["prefix_slots"] == 0 and ctx.join_stats()["table_slots"] == Y.n
    check(oracle, ry, want)
    hj = host_join(y, z)
    assert_same_log(hj.arrays(), want)
    up = mk(hj)
    assert up.merge() == ry.merge() and up.info() == ry.info()


def test_duplicate_that_straddles_the_prefix_is_found(ctx, mk, forks):
    """src = dst + three new items whose keys exceed every key of dst + one more item, a left
    child that carries the identity of an item of the common prefix.  Every raw key past the
    prefix is above the prefix's largest identity (the left child's because of bit 48), so an
    unmasked disjointness test would skip the full-table run, never see the duplicate and append
    it.  The upload does not check identities, so such a replica can be made."""
    base = forks[0]
    D = base.arrays()
    n, top = D.n, int(D.lamport.max())
    k = 10                                              # the prefix item whose name is reused
    assert D.lamport[k - 1] < top
    S = crafted(
        D.parent.tolist() + [n, n + 1, 5, 12],
        D.lamport.tolist() + [top + 1, top + 2, top + 3, int(D.lamport[k - 1])],
        D.agent.tolist() + [7, 7, 7, int(D.agent[k - 1])],
        D.cp.tolist() + [120, 121, 122, int(D.cp[k - 1])],
        D.side.tolist() + [0, 0, 1, 1],
        D.deleted.tolist() + [0, 0, 0, 0])
    ident = lambda X: (X.lamport.astype(np.uint64) << np.uint64(16)) | X.agent  # noqa: E731
    raw = ident(S) | (S.side.astype(np.uint64) << np.uint64(48))
    assert raw[n:].min() > ident(D).max() and ident(S)[n:].min() <= ident(D).max()
    dst, src = mk(D), mk(S)
    before = (dst.merge(), dst.info())
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dst.join(src)
    assert e.value.code == -5 and "source" in str(e.value)
    assert (dst.merge(), dst.info()) == before
    # without the duplicate the same source joins, through the prefix
    good = crafted(*(getattr(S, f)[:-1] for f in ("parent", "lamport", "agent", "cp", "side",
                                                   "deleted")))
    assert dst.join(mk(good)) == (3, 0)
    assert ctx.join_stats()["prefix_slots"] == n


def test_prefix_across_blocks_and_tiles_and_a_regrow(ctx, mk, oracle):
    """sveltecomponent resolved with Fugue anchors as the base: the prefix pass spans hundreds of
    blocks, the new items and the new total cross a 64-slot padding boundary and a 4096-slot
    tile, and dst was uploaded tight, so the join's reserve regrows it."""
    base = crdt_hip.Trace(trace_path("sveltecomponent")).resolve(fugue=True)
    nb = base.arrays().n
    a, b = fork(base, 1, 101, 1000), fork(base, 2, 202, 1500)
    A, B = a.arrays(), b.arrays()
    assert_unique_identities(A, B)
    assert (A.side[nb:] == 1).any() and (B.side[nb:] == 1).any()
    want, added, tomb = union(A, B)
    assert A.n // 4096 != want.n // 4096 and (A.n + 1 + 63) // 64 != (want.n + 1 + 63) // 64
    assert added % 64 != 0 and added > 256
    dst, src = mk(a), mk(b)
    assert dst.join(src) == (added, tomb)
    assert ctx.join_stats()["prefix_slots"] == nb
    check(oracle, dst, want)
    hj = host_join(a, b)
    assert_same_log(hj.arrays(), want)
    up = mk(hj)
    assert up.merge() == dst.merge() and up.info() == dst.info()


def test_join_algebra_on_the_device(ctx, mk, oracle, forks):
    _, nb, a, b, c = forks
    A, B, C = a.arrays(), b.arrays(), c.arrays()

    def joined(first, *rest):
        r = mk(first)
        for s in rest:
            r.join(mk(s))
        return r

    ab, ba = joined(a, b), joined(b, a)
    t2 = expect(oracle, union(A, B)[0])
    assert ab.merge() == ba.merge() == t2[:2]                   # commutes, by text and digest
    left = joined(a, b, c)                                      # (A U B) U C
    right = joined(a, joined(b, c))                             # A U (B U C)
    t3 = expect(oracle, union(union(A, B)[0], C)[0])
    assert left.merge() == right.merge() == t3[:2]
    assert left.info() == right.info() == t3[2]
    before = (ab.merge(), ab.info())
    assert ab.join(mk(b)) == (0, 0)                             # idempotent
    assert ab.join(mk(a)) == (0, 0)                             # nothing new: (0, 0)
    assert ab.join(ab) == (0, 0)                                # self-join
    assert ab.join(mk()) == (0, 0)                              # empty Fugue src
    assert (ab.merge(), ab.info()) == before
    empty = mk(empty_arrays())
    assert empty.join(ba) == (ba.info()[0], 0)                  # into an empty Fugue replica: = src
    assert empty.merge() == ba.merge() and empty.info() == ba.info()
    assert_same_log(host_join(crdt_hip.OpLog(fugue=True), host_join(b, a)).arrays(), union(B, A)[0])
    # tombstones alone: src = dst with more deletes
    a2 = a.clone()
    a2.remove(3, 9)
    ra = mk(a)
    assert ra.join(mk(a2)) == (0, 6)
    check(oracle, ra, a2.arrays())


def test_after_the_join(ctx, mk, oracle, forks):
    """merge_inc merges in full once and incrementally again on a following local edit at the end
    of the document; a clone merges equal."""
    _, nb, a, b, _ = forks
    hj = host_join(a, b)
    dst, src = mk(a), mk(b)
    assert dst.merge_inc(text=True)[2:] == (0, merged(oracle, a.arrays()))
    dst.join(src)
    cps, nbytes, path, text = dst.merge_inc(text=True)
    t_j = expect(oracle, hj.arrays())
    assert (path, text, cps, nbytes) == (0, t_j[0], t_j[2][1], t_j[2][2])
    cl = mk(dst.clone())
    assert cl.merge() == t_j[:2] and cl.info() == t_j[2]
    # a local edit at the end of the joined document, shipped as a version-2 update: the
    # incremental path again
    v = hj.version()
    hj.set_agent(9)
    hj.insert(hj.visible_len(), "local édit")
    upd = hj.encode_from(v)
    assert upd[4:8] == b"\x02\0\0\0"
    dst.apply_updates([upd])
    cps, nbytes, path, text = dst.merge_inc(text=True)
    t_e = expect(oracle, hj.arrays())
    assert (path, text, cps, nbytes) == (1, t_e[0], t_e[2][1], t_e[2][2])
    # one in the middle: by text only (a left child under an item that already has one
    # legitimately merges in full)
    v = hj.version()
    hj.insert(hj.visible_len() // 2, "mid")
    dst.apply_updates([hj.encode_from(v)])
    cps, nbytes, path, text = dst.merge_inc(text=True)
    t_m = expect(oracle, hj.arrays())
    assert (text, cps, nbytes) == (t_m[0], t_m[2][1], t_m[2][2])
    assert dst.merge() == t_m[:2]


def test_rejected_joins_leave_dst_unchanged(ctx, mk, oracle, forks):
    #              parent      lamport     agent      cp                side       deleted
    good = crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 0x20AC], [0, 0, 1], [0, 1, 0])
    bad = {
        # item 3 found through the table (a new item precedes it in src), as a right child
        "side_past_prefix": crafted([0, 1, 1, 3], [1, 9, 2, 3], [1, 2, 1, 1],
                                    [97, 120, 98, 0x20AC], [0, 0, 0, 0], [0, 0, 1, 0]),
        # item 3 at its own slot as a right child: the key words differ there, the prefix ends
        "side_in_prefix": crafted([0, 1, 2, 3], [1, 2, 3, 8], [1, 1, 1, 2],
                                  [97, 98, 0x20AC, 120], [0, 0, 0, 0], [0, 1, 0, 0]),
        "dup_by_side": crafted([0, 1, 1], [1, 5, 5], [1, 2, 2], [97, 120, 121], [0, 0, 1]),
    }
    dst = mk(good)
    before = (dst.merge(), dst.info())
    assert before[1] == (3, 2, 4)
    for name, arrs in bad.items():
        src = mk(arrs)
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            dst.join(src)
        assert e.value.code == -5, name
        if name.startswith("side"):
            assert "side" in str(e.value), name
        assert (dst.merge(), dst.info()) == before, name
    # the same inside a prefix of many blocks: one left child of the base flipped in src
    base = forks[0].arrays()
    flipped = base.copy()
    k = int(np.flatnonzero(base.side == 1)[len(np.flatnonzero(base.side == 1)) // 2])
    assert k > 256
    flipped.side[k] = 0
    big = mk(base)
    big_before = (big.merge(), big.info())
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        big.join(mk(flipped))
    assert e.value.code == -5 and "side" in str(e.value)
    assert (big.merge(), big.info()) == big_before
    # two items of dst that differ only in side share an identity
    dup = mk(bad["dup_by_side"])
    dup_before = (dup.merge(), dup.info())
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dup.join(dst)
    assert e.value.code == -5 and "destination" in str(e.value)
    assert (dup.merge(), dup.info()) == dup_before
    # mixed kinds both ways (an empty replica of the other kind and a Fugue source without a left
    # child included), a replica of another context
    rga = mk(join_util.crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 0x20AC], [0, 1, 0]))
    rga_before = (rga.merge(), rga.info())
    rga_empty = mk(crdt_hip.Replica(ctx))
    zero_side = mk(crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 0x20AC], [0, 0, 0], [0, 1, 0]))
    for d, s in ((dst, rga), (rga, dst), (dst, rga_empty), (rga_empty, dst), (rga, zero_side),
                 (rga, mk()), (mk(), rga_empty)):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            d.join(s)
        assert e.value.code == -1
        assert "Fugue" in str(e.value) and "one kind" in str(e.value)
    assert (rga.merge(), rga.info()) == rga_before and rga_empty.info() == (0, 0, 0)
    other = crdt_hip.Context(0)
    foreign = crdt_hip.Replica(other, good)
    try:
        for d, s in ((dst, foreign), (foreign, dst)):
            with pytest.raises(crdt_hip.CrdtHipError) as e:
                d.join(s)
            assert e.value.code == -1
        assert (dst.merge(), dst.info()) == before
    finally:
        foreign.close()   # before its context
        other.close()
    # dst still joins: a second, newer left child of the tombstoned item 2
    ok = crafted([0, 1, 2, 2], [1, 2, 3, 9], [1, 1, 1, 2], [97, 98, 0x20AC, 122], [0, 0, 1, 1],
                 [0, 0, 0, 0])
    assert dst.join(mk(ok)) == (1, 0)
    want = union(good, ok)[0]
    check(oracle, dst, want)
    assert dst.merge()[0] == "az€".encode()
    assert big.join(mk(forks[3])) == (forks[3].arrays().n - base.n, union(base, forks[3].arrays())[2])


def test_hipdownstream_merge_from(oracle, forks):
    _, nb, a, b, _ = forks
    ctx = crdt_hip.HipMerge.context()
    x = crdt_hip.HipDownstream(crdt_hip.Replica(ctx, crdt_hip.OpLog(fugue=True)))
    y = crdt_hip.HipDownstream(crdt_hip.Replica(ctx, crdt_hip.OpLog(fugue=True)))
    try:
        x.apply_update(a.encode_from(0))
        y.apply_update(b.encode_from(0))
        want, added, tomb = union(a.arrays(), b.arrays())
        assert x.merge_from(y) == (added, tomb)
        assert x.text().encode() == merged(oracle, want)
        assert x.len() == join_util.visible(want)[0]
    finally:
        x.replica.close()
        y.replica.close()
