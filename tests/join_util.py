"""Shared helpers of test_join.py and test_gpu_join.py (test infrastructure only).

Forks are made with the product's own editing API (a base log cloned per editor, a distinct agent
per editor, seeded random insert / remove / replace); the expected join is computed here without
the product: the union log is built in Python with a dict keyed by (lamport, agent) from the two
forks' arrays, and merged by the CPU oracle.
"""
from __future__ import annotations

import random
import struct

import numpy as np

import crdt_hip
from oracle_bind import AnchorLog

NIL = 0xFFFFFFFF
ALPHABET = "abcxyz é€😀\n"   # 1-, 2-, 3- and 4-byte codepoints


def to_anchor(arrs: crdt_hip.LogArrays) -> AnchorLog:
    a = AnchorLog(arrs.n)
    for f, g in (("parent", "parent"), ("lamport", "lamport"), ("agent", "agent"),
                 ("deleted", "deleted"), ("cp", "cp")):
        getattr(a, f)[: arrs.n] = getattr(arrs, g)
    return a


def identities(arrs: crdt_hip.LogArrays) -> list:
    return list(zip(arrs.lamport.tolist(), arrs.agent.tolist()))


def assert_unique_identities(*logs) -> None:
    """(lamport, agent) identifies an item within each log, and across the logs an identity never
    names two different items (same codepoint): the resolver gives each editor lamport = max + 1,
    so distinct agents give distinct identities."""
    seen = {}
    for arrs in logs:
        ids = identities(arrs)
        assert len(set(ids)) == len(ids)
        for k, c in zip(ids, arrs.cp.tolist()):
            assert seen.setdefault(k, c) == c


def union(dst: crdt_hip.LogArrays, src: crdt_hip.LogArrays) -> tuple:
    """The join dst U src, computed without the product: (LogArrays, added, tombstoned)."""
    ids = {k: i + 1 for i, k in enumerate(identities(dst))}
    assert len(ids) == dst.n
    parent, oright = dst.parent.tolist(), dst.origin_right.tolist()
    lamport, agent = dst.lamport.tolist(), dst.agent.tolist()
    deleted, cp = dst.deleted.tolist(), dst.cp.tolist()
    mp = [0] * (src.n + 1)
    added = tomb = 0
    sp, so = src.parent.tolist(), src.origin_right.tolist()
    sd, sc = src.deleted.tolist(), src.cp.tolist()
    for k, key in enumerate(identities(src)):
        d = ids.get(key)
        if d is not None and d <= dst.n:
            mp[k + 1] = d
            assert cp[d - 1] == sc[k]
            assert parent[d - 1] == mp[sp[k]]
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
    return (crdt_hip.LogArrays(parent, lamport, agent, deleted, cp, oright), added, tomb)


def seq_flags(arrs: crdt_hip.LogArrays) -> np.ndarray:
    """The previous-slot flag of every item (parent == own id - 1)."""
    return arrs.parent == np.arange(arrs.n, dtype=np.uint32)


def assert_same_log(got: crdt_hip.LogArrays, want: crdt_hip.LogArrays, oright: bool = True) -> None:
    assert got.n == want.n
    for f in ("parent", "lamport", "agent", "deleted", "cp") + (("origin_right",) if oright else ()):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f


def visible(arrs: crdt_hip.LogArrays) -> tuple:
    """(visible codepoints, visible UTF-8 bytes)."""
    live = arrs.cp[arrs.deleted == 0]
    nbytes = 1 + (live >= 0x80).astype(np.int64) + (live >= 0x800) + (live >= 0x10000)
    return int(live.size), int(nbytes.sum())


def random_text(rng: random.Random, k: int) -> str:
    return "".join(rng.choice(ALPHABET) for _ in range(k))


def random_edits(log: crdt_hip.OpLog, rng: random.Random, edits: int) -> None:
    """Seeded positional edits through the product's API: typing runs, deletes, replaces."""
    for _ in range(edits):
        n = log.visible_len()
        op = rng.random()
        if n == 0 or op < 0.55:
            log.insert(rng.randint(0, n), random_text(rng, rng.choice([1, 1, 2, 3, 8])))
        elif op < 0.8:
            a = rng.randint(0, n - 1)
            log.remove(a, min(n, a + rng.choice([1, 1, 2, 5])))
        else:
            a = rng.randint(0, n - 1)
            log.replace(a, min(n, a + rng.choice([1, 2])), random_text(rng, rng.choice([1, 2])))


def fork(base: crdt_hip.OpLog, agent: int, seed: int, edits: int) -> crdt_hip.OpLog:
    f = base.clone()
    f.set_agent(agent)
    random_edits(f, random.Random(seed), edits)
    return f


def base_log(chars: int = 280, seed: int = 1) -> crdt_hip.OpLog:
    """A base typed through the API with multi-byte characters (bytes != codepoints), a few
    deletes included."""
    rng = random.Random(seed)
    log = crdt_hip.OpLog()
    log.insert(0, random_text(rng, chars))
    for _ in range(8):
        a = rng.randint(0, log.visible_len() - 2)
        log.remove(a, a + 1)
    return log


def encode_update(arrs: crdt_hip.LogArrays) -> bytes:
    """The whole of `arrs` (no tombstones) as one wire update (oplog.cpp: magic, version,
    first id, items, first delete, deletes, parent[n], origin_right[n], lamport[n], cp[n], agent[n]
    u16 padded to 4): builds host logs that the editing API cannot, such as one with a duplicate
    identity."""
    n = arrs.n
    assert not arrs.deleted.any()
    b = struct.pack("<6I", 0x55445243, 1, 1, n, 0, 0)
    for col in (arrs.parent, arrs.origin_right, arrs.lamport, arrs.cp):
        b += col.astype("<u4").tobytes()
    b += arrs.agent.astype("<u2").tobytes()
    b += b"\0" * (-len(b) % 4)
    return b


def crafted(parent, lamport, agent, cp, deleted=None) -> crdt_hip.LogArrays:
    n = len(parent)
    return crdt_hip.LogArrays(parent, lamport, agent, deleted if deleted is not None else [0] * n, cp)
