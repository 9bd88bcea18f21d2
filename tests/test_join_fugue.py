"""Host join of two Fugue logs (crdt_hip_oplog_join with a side column on both sides; CPU only).

dst <- dst U src by item identity (lamport, agent); the side is an attribute of the item and comes
along.  The expected log is built in Python (join_fugue_util.union) and merged by the CPU oracle's
Fugue walk (oracle.merge_fugue); the smallest cases are also checked against a recursive in-order
walk written in the helper.  The kind of a log is the presence of its side column, never its
contents: Fugue joins Fugue, RGA joins RGA (test_join.py), a mixed pair is refused.
"""
import struct

import numpy as np
import pytest

import crdt_hip
import join_util
from join_fugue_util import (assert_cases, assert_same_log, assert_unique_identities, base_log,
                             crafted, empty_arrays, encode_update, fork, merged, scripted_forks,
                             union, walk_text)


@pytest.fixture(scope="module")
def forks():
    base = base_log()
    a, b, c = fork(base, 1, 11, 120), fork(base, 2, 22, 90), fork(base, 3, 33, 60)
    assert_unique_identities(a.arrays(), b.arrays(), c.arrays())
    return base, a, b, c


def joined(dst: crdt_hip.OpLog, *srcs) -> crdt_hip.OpLog:
    out = dst.clone()
    for s in srcs:
        out.join(s)
    return out


def test_host_join_equals_the_python_union(oracle):
    base, nb, a, b = scripted_forks()
    assert int(base.arrays().side.sum()) > 0       # the base has left children of its own
    A, B = a.arrays(), b.arrays()
    assert_unique_identities(A, B)
    want, added, tomb = union(A, B)
    assert_cases(base.arrays(), A, B, want)
    assert added == B.n - nb
    j = a.clone()
    assert j.join(b) == (added, tomb)
    assert_same_log(j.arrays(), want)
    text = merged(oracle, want)
    assert text == walk_text(want)
    # both forks' edits are in the document: it is neither fork's
    assert text != merged(oracle, A) and text != merged(oracle, B)
    # src is unchanged, and a LogArrays source joins like an OpLog
    assert_same_log(b.arrays(), B)
    j2 = a.clone()
    assert j2.join(B) == (added, tomb)
    assert_same_log(j2.arrays(), want)
    # the other way round: a's lone delete is a tombstone b takes
    want_ba, added_ba, tomb_ba = union(B, A)
    assert tomb_ba > 0
    k = b.clone()
    assert k.join(a) == (added_ba, tomb_ba)
    assert_same_log(k.arrays(), want_ba)
    assert merged(oracle, want_ba) == text


def test_small_join_matches_the_recursive_walk(oracle):
    base = base_log(40, seed=5, edits=6)
    a, b = fork(base, 1, 1, 25), fork(base, 2, 2, 25)
    A, B = a.arrays(), b.arrays()
    assert_unique_identities(A, B)
    assert (A.side[base.arrays().n:] == 1).any() and (B.side[base.arrays().n:] == 1).any()
    want, _, _ = union(A, B)
    walked = walk_text(want)
    ab, ba = joined(a, b), joined(b, a)
    assert_same_log(ab.arrays(), want)
    assert_same_log(ba.arrays(), union(B, A)[0])
    assert merged(oracle, ab.arrays()) == walked
    assert walk_text(ba.arrays()) == walked
    assert merged(oracle, ba.arrays()) == walked


def test_forks_of_an_empty_log_give_concurrent_children_of_the_document_start(oracle):
    a, b = crdt_hip.OpLog(fugue=True, agent=1), crdt_hip.OpLog(fugue=True, agent=2)
    a.insert(0, "ab€")
    a.insert(0, "<")
    b.insert(0, "xy")
    b.insert(2, "😀")
    A, B = a.arrays(), b.arrays()
    assert A.parent[0] == 0 and B.parent[0] == 0 and A.side[0] == 0 and B.side[0] == 0
    want, added, tomb = union(A, B)
    assert (added, tomb) == (B.n, 0)
    assert ((want.parent == 0) & (want.side == 0)).sum() == 2
    ab, ba = joined(a, b), joined(b, a)
    assert_same_log(ab.arrays(), want)
    text = walk_text(want)
    assert merged(oracle, ab.arrays()) == text == merged(oracle, ba.arrays())
    # each side by (lamport, agent) descending: b's first item (1, 2) goes before a's (1, 1)
    assert text.decode() == "xy😀<ab€"


def test_join_commutes_and_associates_by_text(oracle, forks):
    _, a, b, c = forks
    ab, ba = joined(a, b), joined(b, a)
    t = merged(oracle, ab.arrays())
    assert merged(oracle, ba.arrays()) == t
    left = joined(ab, c)                 # (A U B) U C
    right = joined(a, joined(b, c))      # A U (B U C)
    t3 = merged(oracle, left.arrays())
    assert merged(oracle, right.arrays()) == t3
    assert merged(oracle, joined(c, ba).arrays()) == t3
    assert left.arrays().n == right.arrays().n
    assert_same_log(left.arrays(), union(union(a.arrays(), b.arrays())[0], c.arrays())[0])


def test_join_is_idempotent_and_self_join_changes_nothing(forks):
    _, a, b, _ = forks
    j = joined(a, b)
    before = j.arrays()
    v = j.version()
    assert j.join(b) == (0, 0)
    assert j.join(a) == (0, 0)
    assert j.join(j) == (0, 0)
    assert j.join(j.arrays()) == (0, 0)
    assert j.join(crdt_hip.OpLog(fugue=True)) == (0, 0)      # an empty Fugue source
    assert j.join(empty_arrays()) == (0, 0)
    assert_same_log(j.arrays(), before)
    assert j.version() == v
    e = crdt_hip.OpLog(fugue=True)                            # an empty Fugue destination
    ve = e.version()
    assert e.join(crdt_hip.OpLog(fugue=True)) == (0, 0)
    assert e.join(e) == (0, 0)
    assert e.version() == ve and e.arrays().side is not None
    assert e.join(a) == (a.arrays().n, 0)
    assert_same_log(e.arrays(), a.arrays())


def test_positional_edits_after_a_join_see_the_joined_document(oracle, forks):
    _, a, b, _ = forks
    j = joined(a, b)
    text = merged(oracle, j.arrays()).decode()
    assert j.visible_len() == len(text)
    at = len(text) // 3
    j.set_agent(9)
    j.insert(at, "<<HERE>>")
    want = text[:at] + "<<HERE>>" + text[at:]
    assert merged(oracle, j.arrays()).decode() == want
    j.remove(at + 2, at + 6)
    assert merged(oracle, j.arrays()).decode() == want[: at + 2] + want[at + 6:]
    assert j.visible_len() == len(want) - 4


def test_insert_after_an_item_whose_right_child_came_from_the_other_fork(oracle):
    """`c` has no right child in dst; the other fork typed after it.  After the join an insert
    right after `c` must see that child (the rebuilt index recomputes which items have right
    children) and become a left child of c's successor, not a second right child of c."""
    base = crdt_hip.OpLog(fugue=True, agent=1)
    base.insert(0, "abc")
    d, s = base.clone(), base.clone()
    d.set_agent(2)
    s.set_agent(3)
    d.insert(0, "_")                     # dst edits elsewhere
    s.insert(3, "X")                     # src types after c
    S = s.arrays()
    assert S.parent[3] == 3 and S.side[3] == 0
    assert not ((d.arrays().parent == 3) & (d.arrays().side == 0)).any()
    assert d.join(s) == (1, 0)
    assert merged(oracle, d.arrays()).decode() == "_abcX"
    d.insert(4, "Y")                     # between c and X
    D = d.arrays()
    x = int(np.flatnonzero(D.cp == ord("X"))[0]) + 1
    assert D.cp[-1] == ord("Y") and D.side[-1] == 1 and D.parent[-1] == x
    assert ((D.parent == 3) & (D.side == 0)).sum() == 1
    assert merged(oracle, D) == walk_text(D) == b"_abcYX"


def test_joined_log_still_ships_updates_downstream(forks):
    """version() / encode_from keep their local meaning: a Fugue replica of the joined log that
    has everything up to a version takes the later ops (wire version 2), tombstones of the join
    included."""
    _, a, b, _ = forks
    down = crdt_hip.OpLog(fugue=True)
    down.apply_update(a.encode_from(0))
    j = a.clone()
    v = j.version()
    added, tomb = j.join(b)
    assert added > 0 and tomb > 0
    j.set_agent(7)
    j.insert(0, "tail")
    upd = j.encode_from(v)
    assert struct.unpack_from("<2I", upd) == (0x55445243, 2)
    down.apply_update(upd)
    assert_same_log(down.arrays(), j.arrays())


def test_hipmerge_merge_from_is_the_join(forks):
    _, a, b, _ = forks
    want, added, tomb = union(a.arrays(), b.arrays())
    m = crdt_hip.HipMerge(a.clone())
    assert m.merge_from(crdt_hip.HipMerge(b)) == (added, tomb)
    assert_same_log(m.log.arrays(), want)


#                       parent      lamport     agent      cp            side
DST = dict(parent=[0, 1, 2], lamport=[1, 2, 3], agent=[1, 1, 1], cp=[97, 98, 99], side=[0, 0, 1])
BAD = {
    # item 3 at its own slot, as a right child
    "side_mismatch": (crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 99], [0, 0, 0]), "side"),
    # the same item at another slot (a new item of another agent before it), as a right child
    "moved_side_mismatch": (crafted([0, 1, 1, 3], [1, 9, 2, 3], [1, 2, 1, 1], [97, 120, 98, 99],
                                    [0, 0, 0, 0]), "side"),
    # two source items that differ only in side share an identity
    "dup_by_side": (crafted([0, 1, 1], [1, 5, 5], [1, 2, 2], [97, 120, 121], [0, 0, 1]), "share"),
    "lamport_max": (crafted([0, 1], [1, 0xFFFFFFFF], [1, 2], [97, 120], [0, 0]), "0xFFFFFFFF"),
    "left_of_start": (crafted([0, 0], [1, 5], [1, 2], [97, 120], [0, 1]), "document start"),
}


def fugue_dst() -> crdt_hip.OpLog:
    dst = crdt_hip.OpLog(fugue=True)
    dst.apply_update(encode_update(crafted(**DST)))
    dst.remove(1, 2)
    return dst


@pytest.mark.parametrize("case", sorted(BAD))
def test_rejected_join_leaves_the_log_unchanged(case):
    dst = fugue_dst()
    before, v, vis = dst.arrays(), dst.version(), dst.visible_len()
    assert before.side.tolist() == DST["side"] and before.deleted.sum() == 1
    src, word = BAD[case]
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dst.join(src)
    assert e.value.code == -5 and word in str(e.value)
    assert_same_log(dst.arrays(), before)
    assert dst.version() == v and dst.visible_len() == vis
    # the log still joins a good source
    assert dst.join(crafted([0, 1, 2, 2], [1, 2, 3, 7], [1, 1, 1, 2], [97, 98, 99, 120],
                            [0, 0, 1, 1])) == (1, 0)
    assert dst.arrays().side.tolist() == [0, 0, 1, 1]


def test_duplicate_by_side_in_dst_is_rejected():
    dst = crdt_hip.OpLog(fugue=True)
    dst.apply_update(encode_update(BAD["dup_by_side"][0]))
    before = dst.arrays()
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dst.join(crafted([0], [1], [1], [97], [0]))
    assert e.value.code == -5 and "destination" in str(e.value)
    assert_same_log(dst.arrays(), before)


def test_mixed_kinds_are_refused_both_ways():
    """The kind is the presence of the side column, never its contents: a Fugue source without a
    single left child is still Fugue, and so is an empty Fugue log."""
    fug = fugue_dst()
    fug_before = fug.arrays()
    rga = crdt_hip.OpLog(agent=1)
    rga.insert(0, "abc")
    rga_before = rga.arrays()
    zero_side = crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 99], [0, 0, 0])
    no_side = join_util.crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 99])
    assert zero_side.side is not None and no_side.side is None
    pairs = [
        (rga, zero_side),                        # a Fugue source, all right children, into RGA
        (rga, fug),
        (rga, crdt_hip.OpLog(fugue=True)),       # an empty log of the other kind
        (rga, empty_arrays()),
        (crdt_hip.OpLog(), crdt_hip.OpLog(fugue=True)),
        (fug, no_side),                          # arrays without a side column into Fugue
        (fug, rga),
        (fug, crdt_hip.OpLog()),
        (crdt_hip.OpLog(fugue=True), crdt_hip.OpLog()),
        (crdt_hip.OpLog(fugue=True), rga),
    ]
    for dst, src in pairs:
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            dst.join(src)
        assert e.value.code == -1
        assert "Fugue" in str(e.value) and "one kind" in str(e.value)
    assert_same_log(fug.arrays(), fug_before)
    join_util.assert_same_log(rga.arrays(), rga_before)
    assert rga.arrays().side is None
