"""Host join (crdt_hip_oplog_join): state-based merge of two divergent op logs (CPU only).

The reference's `Downstream for Automerge` merges a whole other replica
(rope.rs:234-236: apply_update(&mut self, other: &Self) = doc.merge(other)).
OpLog.join is that operation for the anchor log: dst <- dst U src by item identity
(lamport, agent).  The expected log is built in Python (join_util.union, a dict keyed by the
identity) and merged by the CPU oracle; the smallest cases are also checked against the oracle's
naive O(n^2) integrator.
"""
import numpy as np
import pytest

import crdt_hip
from join_util import (assert_same_log, assert_unique_identities, base_log, crafted, encode_update,
                       fork, to_anchor, union)


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


def test_host_join_equals_the_python_union(oracle, forks):
    base, a, b, _ = forks
    want, added, tomb = union(a.arrays(), b.arrays())
    assert added > 0 and tomb > 0
    j = a.clone()
    assert j.join(b) == (added, tomb)
    assert_same_log(j.arrays(), want)
    text = oracle.merge(to_anchor(want))
    assert oracle.merge(to_anchor(j.arrays())) == text
    # both forks' edits are in the document: it is neither fork's
    assert text != oracle.merge(to_anchor(a.arrays())) and text != oracle.merge(to_anchor(b.arrays()))
    # src is unchanged, and a LogArrays source joins like an OpLog
    assert_same_log(b.arrays(), fork(base, 2, 22, 90).arrays())
    j2 = a.clone()
    assert j2.join(b.arrays()) == (added, tomb)
    assert_same_log(j2.arrays(), want)


def test_small_join_matches_the_naive_integrator(oracle):
    base = base_log(40, seed=5)
    a, b = fork(base, 1, 1, 25), fork(base, 2, 2, 25)
    assert_unique_identities(a.arrays(), b.arrays())
    want, _, _ = union(a.arrays(), b.arrays())
    j = joined(a, b)
    assert_same_log(j.arrays(), want)
    naive = oracle.merge_naive(to_anchor(want))
    assert oracle.merge(to_anchor(j.arrays())) == naive
    assert oracle.merge(to_anchor(joined(b, a).arrays())) == naive


def test_join_commutes_and_associates_by_text(oracle, forks):
    _, a, b, c = forks
    ab, ba = joined(a, b), joined(b, a)
    t = oracle.merge(to_anchor(ab.arrays()))
    assert oracle.merge(to_anchor(ba.arrays())) == t
    left = joined(ab, c)                 # (A U B) U C
    right = joined(a, joined(b, c))      # A U (B U C)
    t3 = oracle.merge(to_anchor(left.arrays()))
    assert oracle.merge(to_anchor(right.arrays())) == t3
    assert oracle.merge(to_anchor(joined(c, ba).arrays())) == t3
    assert left.arrays().n == right.arrays().n


def test_join_is_idempotent_and_self_join_changes_nothing(forks):
    _, a, b, _ = forks
    j = joined(a, b)
    before = j.arrays()
    v = j.version()
    assert j.join(b) == (0, 0)
    assert j.join(a) == (0, 0)
    assert j.join(j) == (0, 0)
    assert j.join(j.arrays()) == (0, 0)
    assert_same_log(j.arrays(), before)
    assert j.version() == v
    e = crdt_hip.OpLog()
    assert e.join(crdt_hip.OpLog()) == (0, 0)
    assert e.join(a) == (a.arrays().n, 0)
    assert_same_log(e.arrays(), a.arrays())
    assert a.clone().join(crdt_hip.OpLog()) == (0, 0)


def test_positional_edits_after_a_join_see_the_joined_document(oracle, forks):
    _, a, b, _ = forks
    j = joined(a, b)
    text = oracle.merge(to_anchor(j.arrays())).decode()
    assert j.visible_len() == len(text)
    at = len(text) // 3
    j.set_agent(9)
    j.insert(at, "<<HERE>>")
    want = text[:at] + "<<HERE>>" + text[at:]
    assert oracle.merge(to_anchor(j.arrays())).decode() == want
    j.remove(at + 2, at + 6)
    assert oracle.merge(to_anchor(j.arrays())).decode() == want[: at + 2] + want[at + 6:]
    assert j.visible_len() == len(want) - 4


def test_joined_log_still_ships_updates_downstream(oracle, forks):
    """version() / encode_from keep their local meaning: a replica of the joined log that has
    everything up to a version takes the later ops, tombstones of the join included."""
    _, a, b, _ = forks
    down = crdt_hip.OpLog()
    down.apply_update(a.encode_from(0))
    j = a.clone()
    v = j.version()
    j.join(b)
    j.set_agent(7)
    j.insert(0, "tail")
    down.apply_update(j.encode_from(v))
    got, want = down.arrays(), j.arrays()
    assert_same_log(got, want)


def _bad_cases():
    #            parent      lamport     agent      cp
    dst = crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 99])
    dup_src = crafted([0, 1, 1], [1, 5, 5], [1, 2, 2], [97, 120, 121])
    other_cp = crafted([0, 1, 2], [1, 2, 3], [1, 1, 1], [97, 98, 100])
    other_parent = crafted([0, 1, 1], [1, 2, 3], [1, 1, 1], [97, 98, 99])
    # the same two checks for items that do not lie at the same slot in both logs
    moved_cp = crafted([0, 1, 1], [1, 9, 2], [1, 2, 1], [97, 120, 66])
    moved_parent = crafted([0, 1, 2], [1, 9, 2], [1, 2, 1], [97, 120, 98])
    return dst, {"dup_src": dup_src, "other_cp": other_cp, "other_parent": other_parent,
                 "moved_cp": moved_cp, "moved_parent": moved_parent}


@pytest.mark.parametrize("case", ["dup_src", "other_cp", "other_parent", "moved_cp", "moved_parent"])
def test_rejected_join_leaves_the_log_unchanged(case):
    arrs, bad = _bad_cases()
    dst = crdt_hip.OpLog()
    dst.apply_update(encode_update(arrs))
    dst.remove(1, 2)
    before, v, vis = dst.arrays(), dst.version(), dst.visible_len()
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dst.join(bad[case])
    assert e.value.code == -5
    assert_same_log(dst.arrays(), before)
    assert dst.version() == v and dst.visible_len() == vis


def test_duplicate_identity_in_dst_is_rejected():
    dup = crafted([0, 1, 1], [1, 5, 5], [1, 2, 2], [97, 120, 121])
    dst = crdt_hip.OpLog()
    dst.apply_update(encode_update(dup))
    before = dst.arrays()
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dst.join(crafted([0], [1], [1], [97]))
    assert e.value.code == -5
    assert_same_log(dst.arrays(), before)


def test_fugue_side_is_refused(forks):
    _, a, _, _ = forks
    fug = crdt_hip.OpLog(fugue=True, agent=4)
    fug.insert(0, "abc")
    before = a.arrays()
    for dst, src in ((a.clone(), fug), (fug, a), (a.clone(), fug.arrays())):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            dst.join(src)
        assert e.value.code == -1 and "Fugue" in str(e.value)
    assert_same_log(a.arrays(), before)
    assert np.array_equal(fug.arrays().cp, [97, 98, 99])


def test_hipmerge_merge_from_is_the_join(forks):
    _, a, b, _ = forks
    want, added, tomb = union(a.arrays(), b.arrays())
    m = crdt_hip.HipMerge(a.clone())
    assert m.merge_from(crdt_hip.HipMerge(b)) == (added, tomb)
    assert_same_log(m.log.arrays(), want)
