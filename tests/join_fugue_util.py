"""Shared helpers of test_join_fugue.py and test_gpu_join_fugue.py (test infrastructure only).

As join_util, for Fugue logs: forks are made with the product's editing API on OpLog(fugue=True)
under distinct agents; the expected join is computed here without the product.  The union log is
built in Python with a dict keyed by (lamport, agent), the side carried along as an attribute of
the item (and asserted equal for items both logs hold), and merged by the CPU oracle's Fugue
in-order walk (oracle.merge_fugue).  The smallest case is also checked against `walk_text`, a
recursive restatement of that walk written here.
"""
from __future__ import annotations

import random
import struct
import sys

import numpy as np

import crdt_hip
from join_util import identities, random_edits, random_text, visible
from oracle_bind import AnchorLog

NIL = 0xFFFFFFFF


def to_anchor(arrs: crdt_hip.LogArrays) -> AnchorLog:
    assert arrs.side is not None
    a = AnchorLog(arrs.n)
    for f in ("parent", "lamport", "agent", "deleted", "cp", "side"):
        getattr(a, f)[: arrs.n] = getattr(arrs, f)
    return a


def merged(oracle, arrs: crdt_hip.LogArrays) -> bytes:
    return oracle.merge_fugue(to_anchor(arrs))


def expect(oracle, arrs: crdt_hip.LogArrays) -> tuple:
    """(text, digest, info) of a Fugue log, by the oracle."""
    text = merged(oracle, arrs)
    cps, nbytes = visible(arrs)
    assert nbytes == len(text) and cps == len(text.decode())
    return text, oracle.tree_digest(text), (arrs.n, cps, nbytes)


def walk_text(arrs: crdt_hip.LogArrays) -> bytes:
    """The Fugue document by a recursive in-order walk: left children, the item, right children,
    each side by (lamport, agent) descending."""
    kids: dict = {}
    for i in range(1, arrs.n + 1):
        kids.setdefault((int(arrs.parent[i - 1]), int(arrs.side[i - 1])), []).append(i)

    def key(i):
        return int(arrs.lamport[i - 1]), int(arrs.agent[i - 1])
    out = []

    def walk(v):
        for c in sorted(kids.get((v, 1), []), key=key, reverse=True):
            walk(c)
        if v and not arrs.deleted[v - 1]:
            out.append(chr(int(arrs.cp[v - 1])))
        for c in sorted(kids.get((v, 0), []), key=key, reverse=True):
            walk(c)
    assert not kids.get((0, 1)), "left child of the document start"
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * arrs.n + 1000))
    try:
        walk(0)
    finally:
        sys.setrecursionlimit(old)
    return "".join(out).encode()


def union(dst: crdt_hip.LogArrays, src: crdt_hip.LogArrays) -> tuple:
    """The join dst U src of two Fugue logs, computed without the product: (LogArrays, added,
    tombstoned).  An item is named by (lamport, agent); its side comes along."""
    assert dst.side is not None and src.side is not None
    ids = {k: i + 1 for i, k in enumerate(identities(dst))}
    assert len(ids) == dst.n
    parent, oright = dst.parent.tolist(), dst.origin_right.tolist()
    lamport, agent = dst.lamport.tolist(), dst.agent.tolist()
    deleted, cp, side = dst.deleted.tolist(), dst.cp.tolist(), dst.side.tolist()
    mp = [0] * (src.n + 1)
    added = tomb = 0
    sp, so = src.parent.tolist(), src.origin_right.tolist()
    sd, sc, ss = src.deleted.tolist(), src.cp.tolist(), src.side.tolist()
    for k, key in enumerate(identities(src)):
        d = ids.get(key)
        if d is not None and d <= dst.n:
            mp[k + 1] = d
            assert cp[d - 1] == sc[k]
            assert parent[d - 1] == mp[sp[k]]
            assert side[d - 1] == ss[k], "an item both hold has another side in each"
            if sd[k] and not deleted[d - 1]:
                deleted[d - 1] = 1
                tomb += 1
            continue
        assert d is None, "duplicate identity in src"
        assert sp[k] <= k, "src is not in causal order"
        new = len(parent) + 1
        ids[key] = new
        mp[k + 1] = new
        added += 1
        parent.append(mp[sp[k]])
        o = so[k]
        oright.append(mp[o] if 0 < o <= src.n else o)
        lamport.append(key[0])
        agent.append(key[1])
        deleted.append(sd[k])
        cp.append(sc[k])
        side.append(ss[k])
    return (crdt_hip.LogArrays(parent, lamport, agent, deleted, cp, oright, side), added, tomb)


def assert_same_log(got: crdt_hip.LogArrays, want: crdt_hip.LogArrays) -> None:
    """Array for array, side and origin_right included."""
    assert got.n == want.n
    assert got.side is not None and want.side is not None
    for f in ("parent", "lamport", "agent", "deleted", "cp", "origin_right", "side"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f


def assert_unique_identities(*logs) -> None:
    """(lamport, agent) names one item within each log, and across the logs an identity never
    names two different items (same codepoint, same side)."""
    seen = {}
    for arrs in logs:
        ids = identities(arrs)
        assert len(set(ids)) == len(ids)
        for k, c, s in zip(ids, arrs.cp.tolist(), arrs.side.tolist()):
            assert seen.setdefault(k, (c, s)) == (c, s)


def base_log(chars: int = 280, seed: int = 1, edits: int = 20, edit_seed: int = 14) -> crdt_hip.OpLog:
    """A Fugue base of about 300 items made through the API: a random multi-byte string, 8
    deletes, then random edits (which give it left children of its own).  The default seeds are
    ones at which `scripted_forks` holds every case of `assert_cases` (where an insert's Fugue
    anchor falls depends on which neighbours already have right children)."""
    rng = random.Random(seed)
    log = crdt_hip.OpLog(fugue=True)
    log.insert(0, random_text(rng, chars))
    for _ in range(8):
        a = rng.randint(0, log.visible_len() - 2)
        log.remove(a, a + 1)
    random_edits(log, random.Random(edit_seed), edits)
    return log


def fork(base: crdt_hip.OpLog, agent: int, seed: int, edits: int) -> crdt_hip.OpLog:
    f = base.clone()
    f.set_agent(agent)
    random_edits(f, random.Random(seed), edits)
    assert f.arrays().side is not None
    return f


def scripted_forks(more: tuple = (0, 0)) -> tuple:
    """(base, items of the base, fork a, fork b): two forks whose union holds every case the Fugue
    join distinguishes (asserted from the arrays by `assert_cases`).  Positions are the base's
    while each fork's edits go from the end of the document to its start.  `more`: seeded random
    edits of a and b after the scripted ones (the cases stay)."""
    base = base_log()
    nb, n = base.arrays().n, base.visible_len()
    a, b = base.clone(), base.clone()
    a.set_agent(1)
    b.set_agent(2)
    b.insert(n, "z")          # a new right child of an old item (the document's last)
    b.insert(121, "q")        # anchored where a deletes
    b.remove(100, 103)        # deleted by both
    b.insert(50, "b€")        # the same position in both forks
    b.insert(30, "q")         # a left child ...
    b.insert(30, "r")         # ... and a left child of it, on the slot right after it
    b.insert(0, "é0")         # position 0 in both forks: left children of the first item
    a.remove(120, 121)
    a.remove(100, 103)
    a.insert(50, "aa")
    a.insert(10, "XY😀")
    a.insert(0, "A0")
    random_edits(a, random.Random(5), more[0])
    random_edits(b, random.Random(6), more[1])
    return base, nb, a, b


def assert_cases(base: crdt_hip.LogArrays, A: crdt_hip.LogArrays, B: crdt_hip.LogArrays,
                 want: crdt_hip.LogArrays) -> None:
    """The cases the scripted forks hold, read from their arrays (want = A U B)."""
    nb = base.n
    ids_b = np.arange(nb + 1, B.n + 1)
    new_left = B.side[nb:] == 1
    assert (new_left & (B.parent[nb:] <= nb)).any()          # new left child of an old item
    assert (new_left & (B.parent[nb:] > nb)).any()           # new left child of a new item
    assert (A.side[nb:] == 1).any()
    # a new left child on the slot right after its parent's, in src and in the union
    assert (new_left & (B.parent[nb:] == ids_b - 1)).any()
    ids_w = np.arange(A.n + 1, want.n + 1)
    assert ((want.side[A.n:] == 1) & (want.parent[A.n:] == ids_w - 1)).any()
    # a new right child of an old item: the insert at the end of the document
    assert B.side[nb] == 0 and 0 < B.parent[nb] <= nb
    # both forks give the same old item a child on the same side
    ka = set(zip(A.parent[nb:].tolist(), A.side[nb:].tolist()))
    kb = set(zip(B.parent[nb:].tolist(), B.side[nb:].tolist()))
    shared = {k for k in ka & kb if 0 < k[0] <= nb}
    assert {s for _, s in shared} >= {1}
    assert not (B.parent[nb:] == 0).any() and not (A.parent[nb:] == 0).any()
    # an item that one fork tombstones anchors the other fork's insert
    only_a = np.flatnonzero((A.deleted[:nb] == 1) & (B.deleted[:nb] == 0)) + 1
    assert np.isin(B.parent[nb:], only_a).any()
    # deleted by both forks
    assert ((A.deleted[:nb] == 1) & (B.deleted[:nb] == 1) & (base.deleted == 0)).any()


def crafted(parent, lamport, agent, cp, side, deleted=None) -> crdt_hip.LogArrays:
    n = len(parent)
    return crdt_hip.LogArrays(parent, lamport, agent, deleted if deleted is not None else [0] * n,
                              cp, side=side)


def empty_arrays() -> crdt_hip.LogArrays:
    """An empty Fugue log: the side column is there."""
    return crafted([], [], [], [], [])


def encode_update(arrs: crdt_hip.LogArrays) -> bytes:
    """The whole of a Fugue `arrs` (no tombstones) as one version-2 wire update (oplog.cpp: bit 31
    of each cp word = left child): builds host logs that the editing API cannot."""
    n = arrs.n
    assert not arrs.deleted.any()
    b = struct.pack("<6I", 0x55445243, 2, 1, n, 0, 0)
    cpw = arrs.cp.astype(np.uint32) | (arrs.side.astype(np.uint32) << 31)
    for col in (arrs.parent, arrs.origin_right, arrs.lamport, cpw):
        b += col.astype("<u4").tobytes()
    b += arrs.agent.astype("<u2").tobytes()
    b += b"\0" * (-len(b) % 4)
    return b
