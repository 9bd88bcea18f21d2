"""Shared helpers of test_delta.py and test_gpu_delta.py (test infrastructure only).

Plain Python restatements of the state-vector delta sync (include/crdt_hip.h, "delta sync"),
computed from LogArrays without the product: the state vector, the delta's wire bytes and their
decoding.  The expected log after an apply is join_util.union (join_fugue_util.union for Fugue
logs) of the two logs' arrays.
"""
from __future__ import annotations

import random
import struct

import numpy as np

import crdt_hip
import join_fugue_util
import join_util
from join_util import base_log, random_edits

MAGIC = 0x44445243
START = 0xFFFFFFFFFFFFFFFF
TOMB, SIDE = 1 << 30, 1 << 31
EINVAL, ERANGE, EBADLOG, ESPACE = -1, -2, -5, -6


def state_vector(arrs: crdt_hip.LogArrays) -> list:
    top: dict = {}
    for lam, ag in zip(arrs.lamport.tolist(), arrs.agent.tolist()):
        top[ag] = max(top.get(ag, -1), lam)
    return sorted(top.items())


def keys(arrs: crdt_hip.LogArrays) -> list:
    return [(lam << 16) | ag for lam, ag in zip(arrs.lamport.tolist(), arrs.agent.tolist())]


def pack(version: int, key, pkey, cpw, rkey, rcount) -> bytes:
    """The wire layout: header, key[n], pkey[n], rkey[r], cp[n], rcount[r]."""
    assert len(key) == len(pkey) == len(cpw) and len(rkey) == len(rcount)
    b = struct.pack("<4I", MAGIC, version, len(key), len(rkey))
    for col, dt in ((key, "<u8"), (pkey, "<u8"), (rkey, "<u8"), (cpw, "<u4"), (rcount, "<u4")):
        b += np.asarray(col, dtype=np.uint64).astype(dt).tobytes()
    assert len(b) == 16 + 20 * len(key) + 12 * len(rkey)
    return b


def encode_diff(arrs: crdt_hip.LogArrays, sv) -> bytes:
    bound = dict(sv)
    k = keys(arrs)
    lam, ag = arrs.lamport.tolist(), arrs.agent.tolist()
    par, dele, cp = arrs.parent.tolist(), arrs.deleted.tolist(), arrs.cp.tolist()
    side = arrs.side.tolist() if arrs.side is not None else None
    covered = [ag[i] in bound and lam[i] <= bound[ag[i]] for i in range(arrs.n)]
    key, pkey, cpw, rkey, rcount = [], [], [], [], []
    prev_in_range = False
    for i in range(arrs.n):
        in_range = covered[i] and bool(dele[i])
        if not covered[i]:
            key.append(k[i])
            pkey.append(k[par[i] - 1] if par[i] else START)
            cpw.append((cp[i] & 0x1FFFFF) | (TOMB if dele[i] else 0) | (SIDE if side and side[i] else 0))
        elif in_range:
            if prev_in_range and k[i] == k[i - 1] + (1 << 16):
                rcount[-1] += 1
            else:
                rkey.append(k[i])
                rcount.append(1)
        prev_in_range = in_range
    return pack(2 if side is not None else 1, key, pkey, cpw, rkey, rcount)


def decode_diff(data: bytes) -> dict:
    magic, version, n, r = struct.unpack_from("<4I", data)
    assert magic == MAGIC and len(data) == 16 + 20 * n + 12 * r
    o = 16
    out = {"version": version, "n": n, "r": r}
    for name, cnt, dt, w in (("key", n, "<u8", 8), ("pkey", n, "<u8", 8), ("rkey", r, "<u8", 8),
                             ("cp", n, "<u4", 4), ("rcount", r, "<u4", 4)):
        out[name] = np.frombuffer(data, dt, cnt, o).astype(np.uint64).tolist()
        o += cnt * w
    return out


def repack(d: dict) -> bytes:
    return pack(d["version"], d["key"], d["pkey"], d["cp"], d["rkey"], d["rcount"])


def ranges(data: bytes) -> list:
    d = decode_diff(data)
    return list(zip(d["rkey"], d["rcount"]))


def union(dst: crdt_hip.LogArrays, src: crdt_hip.LogArrays) -> tuple:
    """(LogArrays, added, tombstoned) of dst U src, origin_right of appended items absent (NIL)."""
    u = join_fugue_util.union if dst.side is not None else join_util.union
    want, added, tomb = u(dst, src)
    want.origin_right[dst.n:] = 0xFFFFFFFF
    return want, added, tomb


def host_log(arrs: crdt_hip.LogArrays) -> crdt_hip.OpLog:
    """A host log holding exactly `arrs` (tombstones included): joined into an empty log."""
    log = crdt_hip.OpLog(fugue=arrs.side is not None)
    log.join(arrs)
    return log


def scripted_forks(more: tuple = (150, 80)) -> tuple:
    """test_gpu_join.scripted_forks restated: (base, items of the base, fork a, fork b), whose
    union holds a deletion by both forks, one fork's tombstone anchoring the other's insert, a
    parent that is the document start and parents that are new (asserted by `assert_cases`)."""
    base = base_log(280)
    nb, n = base.arrays().n, base.visible_len()
    a, b = base.clone(), base.clone()
    a.set_agent(1)
    b.set_agent(2)
    b.insert(n, "z")
    a.remove(120, 121)
    b.insert(121, "q")
    a.remove(100, 103)
    b.remove(100, 103)
    a.insert(50, "aa")
    b.insert(50, "b€")
    a.insert(10, "XY😀")
    a.insert(0, "A0")
    b.insert(0, "é0")
    random_edits(a, random.Random(5), more[0])
    random_edits(b, random.Random(6), more[1])
    return base, nb, a, b


def assert_cases(base: crdt_hip.LogArrays, A: crdt_hip.LogArrays, B: crdt_hip.LogArrays) -> None:
    nb = base.n
    for f in (A, B):
        new_par = f.parent[nb:]
        assert ((new_par > 0) & (new_par <= nb)).any()
        assert (new_par > nb).any()                         # parents that are new
        assert (new_par == 0).any()                         # parent = the document start
    assert ((A.deleted[:nb] == 1) & (B.deleted[:nb] == 1) & (base.deleted == 0)).any()
    only_a = np.flatnonzero((A.deleted[:nb] == 1) & (B.deleted[:nb] == 0)) + 1
    assert np.isin(B.parent[nb:], only_a).any()             # a's tombstone anchors b's insert


def range_edges() -> crdt_hip.LogArrays:
    """A chain whose tombstoned stretch is broken in turn by a live item, an agent change, a
    lamport gap and (under `range_edges_sv`) an uncovered item.  Slots 1..16:
      1 live | 2-4 dead (agent 1, lamports 2-4) | 5 live | 6-7 dead | 8-9 dead, agent 2 |
      10-11 dead, agent 1 again after a lamport gap | 12 dead, agent 3 (uncovered) |
      13-14 dead, agent 1 | 15 dead, lamport gap | 16 live."""
    lam = [1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 21, 22, 23, 24, 30, 31]
    ag = [1, 1, 1, 1, 1, 1, 1, 2, 2, 1, 1, 3, 1, 1, 1, 1]
    dele = [0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    n = len(lam)
    return join_util.crafted(list(range(n)), lam, ag, [97 + i for i in range(n)], dele)


def range_edges_sv() -> list:
    return [(1, 31), (2, 9)]        # agent 3 is not covered


def range_edges_want() -> list:
    k = lambda lam, ag: (lam << 16) | ag
    return [(k(2, 1), 3), (k(6, 1), 2), (k(8, 2), 2), (k(20, 1), 2), (k(23, 1), 2), (k(30, 1), 1)]


def big_log(agent_a: int = 1, agent_b: int = 2) -> tuple:
    """(x, y): two forks of a ~1,700-item base, about 2,500 items each, so that every kernel runs
    several 256-thread blocks and the one-workgroup scans see several block counts.  y deletes a
    stretch of about 700 of the base's typed items (consecutive slots, one agent, consecutive
    lamports): against x's state vector that is one tombstone range across block boundaries."""
    base = crdt_hip.OpLog()
    rng = random.Random(9)
    base.insert(0, join_util.random_text(rng, 1700))
    x, y = base.clone(), base.clone()
    x.set_agent(agent_a)
    y.set_agent(agent_b)
    y.remove(300, 1000)
    random_edits(x, random.Random(10), 400)
    random_edits(y, random.Random(11), 380)
    return x, y
