"""Shared helpers of test_anchors.py and test_gpu_anchors.py (test infrastructure only).

A plain Python restatement of anchors (include/crdt_hip.h, "anchors"), computed without the
product: from LogArrays and the document order the CPU oracle gives for them.  Logs and forks come
from join_util, join_fugue_util and patch_util.
"""
from __future__ import annotations

import numpy as np

import crdt_hip
import patch_util as pu
from crdt_hip import AFTER, BEFORE, DEAD, EDGE, LIVE, UNKNOWN

EINVAL, ERANGE = -1, -2
SHARED = 2 << 16    # the identity two slots of shared_identity_log() hold


def shared_identity_log() -> crdt_hip.OpLog:
    """A malformed host log "abcx": "abc" typed, then an update whose one item (id 4, parent 3,
    origin_right NIL, lamport 2, agent 0, "x") takes the identity of slot 2."""
    import struct
    log = crdt_hip.OpLog()
    log.insert(0, "abc")
    #                 magic, version, first id, items, first del, dels | parent, oright, lamport, cp, agent
    log.apply_update(struct.pack("<10IHH", 0x55445243, 1, 4, 1, 0, 0, 3, 0xFFFFFFFF, 2, ord("x"), 0, 0))
    a = log.arrays()
    assert log.text_at() == b"abcx" and a.n == 4
    assert [(int(l) << 16) | int(g) for l, g in zip(a.lamport, a.agent)].count(SHARED) == 2
    return log


def utf8_len(cp: int) -> int:
    return 1 if cp < 0x80 else 2 if cp < 0x800 else 3 if cp < 0x10000 else 4


class Ref:
    """The definitions, over the oracle's document order of `arrs` (tombstones included)."""

    def __init__(self, oracle, arrs: crdt_hip.LogArrays):
        self.order = pu.oracle_merge(oracle, arrs)[1]
        self.ident = [(int(l) << 16) | int(a) for l, a in zip(arrs.lamport, arrs.agent)]
        self.live = [not d for d in arrs.deleted]
        self.width = [utf8_len(int(c)) for c in arrs.cp]
        self.slot = {k: s + 1 for s, k in enumerate(self.ident)}
        assert len(self.slot) == arrs.n
        self.vis = [s for s in self.order if self.live[s - 1]]     # the visible items, in order
        self.ends = [0]                                             # bytes of the first v of them
        for s in self.vis:
            self.ends.append(self.ends[-1] + self.width[s - 1])
        self.len, self.nbytes = len(self.vis), self.ends[-1]
        self.end_rank = {e: v for v, e in enumerate(self.ends)}
        # per slot: the visible items, and their bytes, at the ranks strictly before its own
        self.before = {}
        v = b = 0
        for s in self.order:
            self.before[s] = (v, b)
            if self.live[s - 1]:
                v += 1
                b += self.width[s - 1]

    def at(self, p: int, bias: int, bytes: bool = False) -> tuple:
        """The anchor of gap p; raises ValueError for a byte position inside a codepoint."""
        if bytes:
            if p not in self.end_rank:
                raise ValueError("inside a codepoint")
            p = self.end_rank[p]
        assert 0 <= p <= self.len
        if bias == AFTER:
            return (EDGE if p == 0 else self.ident[self.vis[p - 1] - 1], AFTER)
        return (EDGE if p == self.len else self.ident[self.vis[p] - 1], BEFORE)

    def resolve(self, anchor: tuple) -> tuple:
        ident, bias = anchor
        if ident == EDGE:
            return (0, 0, LIVE) if bias == AFTER else (self.len, self.nbytes, LIVE)
        s = self.slot.get(ident)
        if s is None:
            return (0, 0, UNKNOWN)
        v, b = self.before[s]
        if self.live[s - 1] and bias == AFTER:
            return (v + 1, b + self.width[s - 1], LIVE)
        return (v, b, LIVE if self.live[s - 1] else DEAD)

    def boundaries(self) -> list:
        """Every byte offset that is a codepoint boundary of the visible document."""
        return list(self.ends)

    def insides(self) -> list:
        return sorted(set(range(self.nbytes + 1)) - set(self.ends))


def raw_anchors(anchors) -> np.ndarray:
    arr = np.zeros(len(anchors), crdt_hip.ANCHOR_DTYPE)
    for k, (ident, bias) in enumerate(anchors):
        arr[k] = (ident, bias, 0)
    return arr


def raw_positions(rows) -> np.ndarray:
    arr = np.zeros(len(rows), crdt_hip.ANCHOR_POS_DTYPE)
    for k, (pos, nbytes, state) in enumerate(rows):
        arr[k] = (pos, nbytes, state, 0)
    return arr


def all_gaps(ref: Ref, bytes: bool = False) -> tuple:
    """(positions, biases): every gap under both biases."""
    gaps = ref.boundaries() if bytes else list(range(ref.len + 1))
    return gaps + gaps, [AFTER] * len(gaps) + [BEFORE] * len(gaps)


def check_at(obj, ref: Ref, positions, biases, bytes: bool = False) -> np.ndarray:
    """obj.anchors_at[_bytes]_raw against the restatement; returns the raw anchors."""
    call = obj.anchors_at_bytes_raw if bytes else obj.anchors_at_raw
    got = call(positions, biases)
    want = raw_anchors([ref.at(p, b, bytes) for p, b in zip(positions, biases)])
    assert got.tobytes() == want.tobytes()
    return got


def check_resolve(obj, ref: Ref, anchors) -> np.ndarray:
    """obj.resolve_anchors_raw against the restatement; returns the raw positions."""
    alist = crdt_hip._anchor_list(anchors) if isinstance(anchors, np.ndarray) else list(anchors)
    got = obj.resolve_anchors_raw(anchors)
    want = raw_positions([ref.resolve(a) for a in alist])
    assert got.tobytes() == want.tobytes()
    return got


def fails(call, code: int, out: np.ndarray) -> None:
    """`call(out)` raises `code` and leaves `out` as it was."""
    before = out.tobytes()
    try:
        call(out)
    except crdt_hip.CrdtHipError as e:
        assert e.code == code, e
    else:
        raise AssertionError(f"expected error {code}")
    assert out.tobytes() == before


class Pair:
    """A replica and the host log that holds the same items slot for slot, with the restatement of
    their document (rebuilt by ref() after every change)."""

    def __init__(self, ctx, oracle, log: crdt_hip.OpLog, fugue: bool, agent: int = 0):
        self.ctx, self.oracle, self.fugue = ctx, oracle, fugue
        self.host = log.clone()
        self.host.set_agent(agent)
        self.rep = crdt_hip.Replica(ctx, log if log.view().n or fugue else None)
        if agent:
            self.rep.set_agent(agent)
        self.made = [self.rep]

    def close(self):
        for r in self.made:
            r.close()

    def ref(self) -> Ref:
        assert self.rep.encode_diff([]) == self.host.encode_diff([])
        return Ref(self.oracle, self.host.arrays())

    def at(self, ref: Ref, positions, biases, bytes: bool = False) -> np.ndarray:
        """Host and device against the restatement, and therefore each other, byte for byte."""
        got = check_at(self.rep, ref, positions, biases, bytes)
        assert check_at(self.host, ref, positions, biases, bytes).tobytes() == got.tobytes()
        return got

    def resolve(self, ref: Ref, anchors) -> np.ndarray:
        got = check_resolve(self.rep, ref, anchors)
        assert check_resolve(self.host, ref, anchors).tobytes() == got.tobytes()
        return got

    def edit(self, plist) -> None:
        for pos, dele, ins in plist:
            self.host.replace(pos, pos + dele, ins)
        self.rep.apply_patches(plist)

    def join(self, other: crdt_hip.OpLog) -> None:
        o = crdt_hip.Replica(self.ctx, other)
        self.made.append(o)
        assert self.rep.join(o) == self.host.join(other)

    def apply_diff(self, other: crdt_hip.OpLog) -> None:
        delta = other.encode_diff(self.host.state_vector())
        assert self.rep.apply_diff(delta) == self.host.apply_diff(delta)
