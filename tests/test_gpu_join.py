"""Device join (crdt_hip_replica_join, join.hip): state-based merge of two divergent replicas.

The reference's `Downstream for Automerge` merges a whole other replica
(rope.rs:234-236: apply_update(&mut self, other: &Self) = doc.merge(other)).
Replica.join does it in HBM: dst <- dst U src by item identity (lamport, agent).  Expected
results are computed without the product: the union log is built in Python (join_util.union) from
the forks' arrays and merged by the CPU oracle; the joined replica's text, digest and info() must
match it, and match a replica uploaded from the host join's log (OpLog.join), which the device
join must equal slot for slot.  Sizes are the smallest that reach each code path.
"""
import numpy as np
import pytest

import crdt_hip
from conftest import trace_path
from edit_util import ALPHABET
from join_util import (assert_same_log, assert_unique_identities, base_log, crafted, fork,
                       random_edits, to_anchor, union, visible)
import random

pytestmark = pytest.mark.gpu


def expect(oracle, arrs):
    """(text, digest, info) of a log, by the oracle."""
    text = oracle.merge(to_anchor(arrs))
    cps, nbytes = visible(arrs)
    assert nbytes == len(text) and cps == len(text.decode())
    return text, oracle.tree_digest(text), (arrs.n, cps, nbytes)


def check(oracle, rep, arrs):
    text, dig, info = expect(oracle, arrs)
    got_text, got_dig = rep.merge()
    assert got_text == text
    assert got_dig == dig
    assert rep.info() == info


@pytest.fixture
def mk(ctx):
    """Replica factory (also takes a made replica or update batch) that closes what it made when
    the test ends.  A replica must be freed
    before its context: one kept alive past the session context by a reference cycle (an excinfo
    holds the test's frame) would be freed by the garbage collector after crdt_hip_destroy."""
    made = []

    def make(init=None, context=None):
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


def scripted_forks():
    """Two forks whose union holds every case the join distinguishes (see the asserts of
    test_join_reaches_every_case)."""
    base = base_log(280)
    nb, n = base.arrays().n, base.visible_len()
    a, b = base.clone(), base.clone()
    a.set_agent(1)
    b.set_agent(2)
    # positions are the base's while the edits go from the end of the document to its start
    b.insert(n, "z")          # b's first item follows its parent's slot (the base's last item)
    a.remove(120, 121)        # a deletes the item ...
    b.insert(121, "q")        # ... that b anchors an insert to
    a.remove(100, 103)        # deleted by both
    b.remove(100, 103)
    a.insert(50, "aa")        # the same position edited by both: siblings ordered by key
    b.insert(50, "b€")
    a.insert(10, "XY😀")       # parent in the common prefix, then parents that are new
    a.insert(0, "A0")         # parent = the document start, in each fork
    b.insert(0, "é0")
    random_edits(a, random.Random(5), 150)
    random_edits(b, random.Random(6), 80)
    return base, nb, a, b


@pytest.fixture(scope="module")
def forks():
    base, nb, a, b = scripted_forks()
    c = fork(base, 3, 33, 60)
    assert_unique_identities(a.arrays(), b.arrays(), c.arrays())
    return base, nb, a, b, c


def test_more_than_262144_new_items(ctx, mk):
    """262,400 src slots past the prefix are 1,025 blocks of 256: k_join_top scans the block counts
    in two rounds of 1,024, the second with the carry of the first.  Device against the host join,
    slot for slot (the log read back as a delta against the empty vector)."""
    base = crdt_hip.OpLog()
    base.insert(0, (ALPHABET * 7)[:200])
    a, b = base.clone(), base.clone()
    a.set_agent(1)
    b.set_agent(2)
    a.insert(200, (ALPHABET * 2)[:50])
    b.insert(100, (ALPHABET * (262400 // len(ALPHABET) + 1))[:262400])
    for dst, src in ((a, b), (b, a)):
        want = dst.clone()
        added = want.join(src)
        assert added == (src.view().n - 200, 0)
        rd, rs = mk(dst), mk(src)
        assert rd.join(rs) == added
        assert ctx.join_stats()["prefix_slots"] == 200
        assert rd.encode_diff([]) == want.encode_diff([])
        assert rd.info()[0] == 200 + 50 + 262400


@pytest.mark.parametrize("contraction", [1, 2])
def test_join_reaches_every_case(ctx, mk, oracle, forks, contraction):
    base, nb, a, b, _ = forks
    A, B, base_arr = a.arrays(), b.arrays(), base.arrays()
    want, added, tomb = union(A, B)
    # the cases the union holds, read from the forks' arrays
    for f in (A, B):
        new_par = f.parent[nb:]
        assert ((new_par > 0) & (new_par <= nb)).any()      # new item, parent in the prefix
        assert (new_par > nb).any()                         # new item, parent new
        assert (new_par == 0).any()                         # new item, parent = document start
    both = (A.deleted[:nb] == 1) & (B.deleted[:nb] == 1) & (base_arr.deleted == 0)
    assert both.any()                                       # deleted by both forks
    only_a = np.flatnonzero((A.deleted[:nb] == 1) & (B.deleted[:nb] == 0)) + 1
    assert np.isin(B.parent[nb:], only_a).any()             # a's tombstone anchors b's insert
    assert B.parent[nb] == nb and want.parent[A.n] == nb and A.n > nb   # previous slot in src only
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
        # a wrong previous-slot flag would show: the document differs from both forks'
        assert dst.merge()[0] not in (src_before[0][0], oracle.merge(to_anchor(A)))
    finally:
        ctx.set_param("contraction", 0)


def test_previous_slot_flag_is_recomputed_both_ways(ctx, mk, oracle):
    """src = [base, X, S, Y] with Y typed after X: Y does not follow its parent's slot in src.
    dst = [base, S] holds S already, so X and Y become neighbours n + 1, n + 2: Y follows its
    parent's slot in dst.  The other way round for X: it follows the base's last slot in src only."""
    base = base_log(70, seed=3)
    n = base.visible_len()
    d, e = base.clone(), base.clone()
    d.set_agent(2)
    e.set_agent(3)
    d.insert(n, "X")
    e.insert(5, "S")
    src = host_join(d, e)
    src.set_agent(2)
    src.insert(n + 2, "Y")    # right after X (S sits at 5, before it)
    dst = host_join(base, e)
    S, D = src.arrays(), dst.arrays()
    nb = base.arrays().n
    assert S.parent[nb + 2] == nb + 1 and S.parent[nb] == nb            # Y -> X (not adjacent), X seq
    want, added, tomb = union(D, S)
    assert added == 2 and want.parent[D.n + 1] == D.n + 1 and want.parent[D.n] == nb
    rd, rs = mk(dst), mk(src)
    assert rd.join(rs) == (2, 0)
    check(oracle, rd, want)
    text = oracle.merge(to_anchor(want)).decode()
    assert text.endswith("XY") and oracle.merge_naive(to_anchor(want)).decode() == text
    assert_same_log(host_join(dst, src).arrays(), want)


def test_shared_items_past_the_prefix_go_through_the_table(ctx, mk, oracle, forks):
    """C = A U B, then C U B' with B' = B + more edits: B's own items lie past the common prefix
    of C and B' (the base), at other slots in each, so the lookup finds them in the table."""
    _, nb, a, b, _ = forks
    b2 = b.clone()
    random_edits(b2, random.Random(77), 40)
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
    assert_same_log(host_join(a, b, b2).arrays(), want)


def test_prefix_keys_not_below_the_rest_take_the_full_table(ctx, mk, oracle, forks):
    """Y = A U B holds B's items (small lamports) behind A's (large ones); Z = A + local edits.
    The common prefix of Y and Z is the whole of A, and Y's items past it do not exceed its keys:
    the prefix cannot be taken as disjoint from the rest, and the join runs with every slot in
    the table."""
    _, nb, a, b, _ = forks
    z = a.clone()
    random_edits(z, random.Random(88), 30)
    y = host_join(a, b)
    Y, Z = y.arrays(), z.arrays()
    assert Y.lamport[a.arrays().n:].min() < Y.lamport[: a.arrays().n].max()
    want, added, tomb = union(Y, Z)
    ry, rz = mk(y), mk(z)
    assert ry.join(rz) == (added, tomb)
    assert ctx.join_stats()["prefix_slots"] == 0 and ctx.join_stats()["table_slots"] == Y.n
    check(oracle, ry, want)
    assert_same_log(host_join(y, z).arrays(), want)


def test_prefix_across_blocks_and_tiles_and_a_regrow(ctx, mk, oracle):
    """sveltecomponent's resolved log as the base: the prefix pass spans hundreds of blocks, the
    new items and the new total cross a 64-slot padding boundary and a 4096-slot tile, and dst was
    uploaded tight, so the join's reserve regrows it."""
    base = crdt_hip.Trace(trace_path("sveltecomponent")).resolve()
    nb = base.arrays().n
    a, b = fork(base, 1, 101, 1000), fork(base, 2, 202, 1500)
    A, B = a.arrays(), b.arrays()
    assert_unique_identities(A, B)
    want, added, tomb = union(A, B)
    assert A.n // 4096 != want.n // 4096 and (A.n + 1 + 63) // 64 != (want.n + 1 + 63) // 64
    assert added % 64 != 0 and added > 256
    dst, src = mk(a), mk(b)
    assert dst.join(src) == (added, tomb)
    assert ctx.join_stats()["prefix_slots"] == nb
    check(oracle, dst, want)
    up = mk(host_join(a, b))
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
    assert ab.join(mk()) == (0, 0)                              # empty src
    assert (ab.merge(), ab.info()) == before
    empty = mk()
    assert empty.join(ba) == (ba.info()[0], 0)                  # into an empty replica: = src
    assert empty.merge() == ba.merge() and empty.info() == ba.info()
    # tombstones alone: src = dst with more deletes
    a2 = a.clone()
    a2.remove(3, 9)
    ra = mk(a)
    assert ra.join(mk(a2)) == (0, 6)
    check(oracle, ra, a2.arrays())


def test_after_the_join(ctx, mk, oracle, forks):
    """merge_inc merges in full once and incrementally again on a following local edit; a clone
    merges equal; a replay whose init was joined since its last call gives the new init's result."""
    _, nb, a, b, _ = forks
    hj = host_join(a, b)
    dst, src = mk(a), mk(b)
    text_a = oracle.merge(to_anchor(a.arrays()))
    assert dst.merge_inc(text=True)[2:] == (0, text_a)
    # a replay session of dst from before the join: deletes of three base items
    dels = a.clone()
    v = dels.version()
    dels.remove(0, 3)
    ub = mk(crdt_hip.UpdateBatch(ctx, *crdt_hip.pack_updates([dels.encode_from(v)])))
    t_dels = expect(oracle, dels.arrays())
    for _ in range(3):
        assert dst.replay(ub) == (t_dels[2][1], t_dels[2][2], t_dels[1])
    dst.join(src)
    cps, nbytes, path, text = dst.merge_inc(text=True)
    t_j = expect(oracle, hj.arrays())
    assert (path, text, cps, nbytes) == (0, t_j[0], t_j[2][1], t_j[2][2])
    cl = mk(dst.clone())
    assert cl.merge() == t_j[:2] and cl.info() == t_j[2]
    # the replay sees the joined init
    want = hj.arrays()
    newly = np.flatnonzero(dels.arrays().deleted != a.arrays().deleted)
    assert newly.size == 3
    want.deleted[newly] = 1      # a's ids are the joined log's ids
    t_jd = expect(oracle, want)
    for _ in range(2):
        assert dst.replay(ub) == (t_jd[2][1], t_jd[2][2], t_jd[1])
    assert dst.info() == t_j[2]
    # a local edit on the joined log, shipped as an update: the incremental path again
    v = hj.version()
    hj.set_agent(9)
    hj.insert(hj.visible_len() // 2, "local édit")
    dst.apply_updates([hj.encode_from(v)])
    cps, nbytes, path, text = dst.merge_inc(text=True)
    t_e = expect(oracle, hj.arrays())
    assert (path, text, cps, nbytes) == (1, t_e[0], t_e[2][1], t_e[2][2])


def test_rejected_joins_leave_dst_unchanged(ctx, mk, forks):
    #              parent      lamport     agent      cp             deleted
    good = crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 0x20AC], [0, 1, 0])
    bad = {
        "dup_src": crafted([0, 1, 1], [1, 5, 5], [1, 2, 2], [97, 120, 121]),
        "other_cp": crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 100]),
        "other_parent": crafted([0, 1, 1], [1, 2, 3], [1, 1, 1], [97, 98, 0x20AC]),
        # the same checks for items that lie at other slots in src (found through the table)
        "moved_cp": crafted([0, 1, 1], [1, 9, 2], [1, 2, 1], [97, 120, 66]),
        "moved_parent": crafted([0, 1, 2], [1, 9, 2], [1, 2, 1], [97, 120, 98]),
        "dup_src_far": crafted([0, 1, 2, 3, 1], [1, 2, 3, 7, 7], [1, 1, 1, 4, 4],
                               [97, 98, 0x20AC, 65, 66]),
    }
    dst = mk(good)
    before = (dst.merge(), dst.info())
    assert before[1] == (3, 2, 4)
    for name, arrs in bad.items():
        src = mk(arrs)
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            dst.join(src)
        assert e.value.code == -5, name
        assert (dst.merge(), dst.info()) == before, name
    # two items of dst share an identity
    dup = mk(bad["dup_src"])
    dup_before = (dup.merge(), dup.info())
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dup.join(dst)
    assert e.value.code == -5 and (dup.merge(), dup.info()) == dup_before
    # a replica of another context, a Fugue replica on either side
    other = crdt_hip.Context(0)
    foreign = crdt_hip.Replica(other, good)
    try:
        fug_log = crdt_hip.OpLog(fugue=True, agent=4)
        fug_log.insert(0, "abc")
        fug = mk(fug_log)
        for d, s in ((dst, foreign), (foreign, dst), (dst, fug), (fug, dst)):
            with pytest.raises(crdt_hip.CrdtHipError) as e:
                d.join(s)
            assert e.value.code == -1
        assert "Fugue" in str(e.value)
        assert (dst.merge(), dst.info()) == before
        assert fug.merge()[0] == b"abc"
    finally:
        foreign.close()   # before its context
        other.close()
    # dst still joins
    ok = crafted([0, 1, 0], [1, 2, 9], [1, 1, 2], [97, 98, 122])
    assert dst.join(mk(ok)) == (1, 0)
    assert dst.merge()[0] == "za€".encode()


def test_hipdownstream_merge_from(oracle, forks):
    _, nb, a, b, _ = forks
    ctx = crdt_hip.HipMerge.context()
    x = crdt_hip.HipDownstream(crdt_hip.Replica(ctx))
    y = crdt_hip.HipDownstream(crdt_hip.Replica(ctx))
    try:
        x.apply_update(a.encode_from(0))
        y.apply_update(b.encode_from(0))
        want, added, tomb = union(a.arrays(), b.arrays())
        assert x.merge_from(y) == (added, tomb)
        assert x.text().encode() == oracle.merge(to_anchor(want))
        assert x.len() == visible(want)[0]
    finally:
        x.replica.close()
        y.replica.close()
