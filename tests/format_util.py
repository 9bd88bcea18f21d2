"""Shared helpers of test_formats.py and test_gpu_formats.py (test infrastructure only).

A plain Python restatement of formats (include/crdt_hip.h, "formats"), computed without the
product: gaps, coverage and the winner per item by brute force from the definitions (a numpy
row of all ranks per format), over the document order the CPU oracle gives (anchor_util.Ref), then
the runs of equal attribute sets over the visible items.  Logs and forks come from patch_util.
"""
from __future__ import annotations

import random

import numpy as np

import anchor_util as au
import crdt_hip
import patch_util as pu
from crdt_hip import AFTER, BEFORE, EDGE, REMOVE
from edit_util import text_of

EINVAL, ERANGE, EBADLOG, ESPACE = -1, -2, -5, -6


def op_of(lamport: int, agent: int) -> int:
    return (lamport << 16) | agent


def fmt(start, end, key, value, op, flags=0) -> tuple:
    """A format as crdt_hip.OpLog.spans takes it; start and end are anchors (id, bias)."""
    return (start, end, key, value, op, flags)


class FRef(au.Ref):
    """The definitions, over the oracle's document order (tombstones included)."""

    def __init__(self, oracle, arrs: crdt_hip.LogArrays):
        super().__init__(oracle, arrs)
        self.rank = {s: k + 1 for k, s in enumerate(self.order)}
        self.n = len(self.order)

    def ident_at_rank(self, k: int) -> int:
        return self.ident[self.order[k - 1] - 1]

    def gap(self, anchor):
        """Gap 0..N of an anchor, or None when the log does not hold its item."""
        ident, bias = anchor
        if ident == EDGE:
            return 0 if bias == AFTER else self.n
        s = self.slot.get(ident)
        if s is None:
            return None
        return self.rank[s] if bias == AFTER else self.rank[s] - 1

    def spans(self, formats) -> tuple:
        """([(pos, pos_bytes, len, len_bytes, [(key, value)])], pending)."""
        formats = list(formats)
        keys = sorted({f[2] for f in formats})
        row = {k: i for i, k in enumerate(keys)}
        ranks = np.arange(1, self.n + 1, dtype=np.int64)
        best = np.full((len(keys), self.n), -1, np.int64)      # per key and rank: the winner's op
        val = np.zeros((len(keys), self.n), np.uint64)
        gone = np.zeros((len(keys), self.n), bool)
        pending = 0
        for start, end, key, value, op, flags in formats:
            gs, ge = self.gap(start), self.gap(end)
            if gs is None or ge is None:
                pending += 1
                continue
            i = row[key]
            m = (ranks > gs) & (ranks <= ge) & (best[i] < op)
            best[i][m] = op
            val[i][m] = value
            gone[i][m] = bool(flags & REMOVE)
        has = (best >= 0) & ~gone
        val = np.where(has, val, 0)
        live = np.array([self.live[s - 1] for s in self.order], bool)
        has, val = has[:, live], val[:, live]
        nv = int(live.sum())
        out = []
        if nv == 0 or not keys:
            return out, pending
        head = np.ones(nv, bool)                                # the item's set differs from its
        head[1:] = (has[:, 1:] != has[:, :-1]).any(0) | (val[:, 1:] != val[:, :-1]).any(0)
        starts = np.flatnonzero(head).tolist() + [nv]           # predecessor's: a run begins
        for a, b in zip(starts, starts[1:]):
            attrs = [(keys[i], int(val[i, a])) for i in range(len(keys)) if has[i, a]]
            if attrs:
                out.append((a, self.ends[a], b - a, self.ends[b] - self.ends[a], attrs))
        return out, pending


def raw_spans(want) -> tuple:
    """The restatement's spans as the (crdt_hip_span array, crdt_hip_span_attr array) the product
    returns."""
    sp = np.zeros(len(want), crdt_hip.SPAN_DTYPE)
    at = []
    for k, (pos, posb, ln, lnb, attrs) in enumerate(want):
        sp[k] = (pos, posb, ln, lnb, len(at), len(attrs))
        at += attrs
    arr = np.zeros(len(at), crdt_hip.SPAN_ATTR_DTYPE)
    for k, (key, value) in enumerate(at):
        arr[k] = (value, key, 0)
    return sp, arr


def assert_layout(sp: np.ndarray, at: np.ndarray) -> None:
    """Spans ascend and never overlap; the attr pieces are contiguous and ascend by key."""
    off = end = 0
    for x in sp:
        assert int(x["len"]) >= 1 and int(x["attr_n"]) >= 1 and int(x["len_bytes"]) >= int(x["len"])
        assert int(x["pos"]) >= end and int(x["attr_off"]) == off
        end = int(x["pos"]) + int(x["len"])
        keys = at["key"][off: off + int(x["attr_n"])].tolist()
        assert keys == sorted(set(keys))
        off += int(x["attr_n"])
    assert off == len(at) and not at["pad"].any()


def check(obj, ref: FRef, formats) -> tuple:
    """obj.spans_raw against the restatement, byte for byte; returns the raw result."""
    formats = list(formats)
    sp, at, pend = obj.spans_raw(formats)
    want, wpend = ref.spans(formats)
    wsp, wat = raw_spans(want)
    assert pend == wpend
    assert sp.tobytes() == wsp.tobytes(), (sp.tolist()[:8], wsp.tolist()[:8])
    assert at.tobytes() == wat.tobytes()
    assert_layout(sp, at)
    return sp, at, pend


def outs(n_spans: int = 4, n_attrs: int = 8) -> tuple:
    """Output arrays of a pattern a failed call must leave as it is."""
    sp = np.zeros(n_spans, crdt_hip.SPAN_DTYPE)
    at = np.zeros(n_attrs, crdt_hip.SPAN_ATTR_DTYPE)
    sp["pos"], at["value"] = 0x5A5A, 0xA5A5
    return sp, at


def fails(obj, formats, code: int, out=None) -> None:
    """obj.spans_raw(formats, out) raises `code` and leaves both output arrays as they were."""
    out = out or outs()
    before = (out[0].tobytes(), out[1].tobytes())
    try:
        obj.spans_raw(formats, out=out)
    except crdt_hip.CrdtHipError as e:
        assert e.code == code, e
    else:
        raise AssertionError(f"expected error {code}")
    assert (out[0].tobytes(), out[1].tobytes()) == before


def bad_formats(good: tuple) -> list:
    """[(formats, code)]: every malformed argument, each beside well-formed formats."""
    s, e, key, value, op, flags = good
    other = fmt(s, e, key + 1, value, op + 1)
    return [
        ([good, fmt((1 << 48, AFTER), e, key, value, op + 2)], EINVAL),     # start id
        ([good, fmt(s, (e[0], 2), key, value, op + 2)], EINVAL),            # end bias
        ([fmt(s, e, key, value, 1 << 48), good], EINVAL),                   # op
        ([good, other, fmt(s, e, key, value, op + 2, 2)], EINVAL),          # flags
        ([good, other, fmt(e, s, 9, 9, op)], EINVAL),                       # a duplicate op
    ]


def chain_log(fugue: bool, n: int, dead_ranges, seed: int, width4_at=()) -> crdt_hip.OpLog:
    """A log of n items typed in one piece (rank k = item k), cut to n through LogArrays, with
    about 20 % of its items tombstoned at random and every rank of `dead_ranges` (first, last)
    tombstoned; the ranks of `width4_at` hold a visible 4-byte codepoint."""
    rng = random.Random(seed)
    text = list(text_of(rng, n + 50))
    for k in width4_at:
        text[k - 1] = "😀"
    full = pu.new_log(fugue)
    full.insert(0, "".join(text))
    A = full.arrays()
    deleted = np.array([1 if rng.random() < 0.2 else 0 for _ in range(n)], np.uint8)
    for first, last in dead_ranges:
        deleted[first - 1: last] = 1
    for k in width4_at:
        deleted[k - 1] = 0
    cut = crdt_hip.LogArrays(A.parent[:n], A.lamport[:n], A.agent[:n], deleted, A.cp[:n],
                             side=A.side[:n] if fugue else None)
    log = pu.new_log(fugue)
    assert log.join(cut) == (n, 0)
    return log


def random_formats(ref: FRef, rng: random.Random, count: int, keys: int, op0: int = 1,
                   absent: float = 0.0, ranks=None) -> list:
    """`count` formats with distinct ops over `keys` distinct keys: ends on random items (or on the
    ranks of `ranks`) under either bias, a few EDGE ends, inverted and collapsed ranges, REMOVEs and
    equal values among them; with probability `absent` an end names an item nobody holds."""
    def end():
        r = rng.random()
        if r < absent:
            return (op_of(rng.randint(1, 50), 0x7777), rng.choice([AFTER, BEFORE]))
        if r < absent + 0.05 or ref.n == 0:
            return (EDGE, rng.choice([AFTER, BEFORE]))
        k = rng.choice(ranks) if ranks else rng.randint(1, ref.n)
        return (ref.ident_at_rank(k), rng.choice([AFTER, BEFORE]))

    out = []
    for i in range(count):
        a, b = end(), end()
        ga, gb = ref.gap(a), ref.gap(b)
        if ga is not None and gb is not None and ga > gb and rng.random() < 0.9:
            a, b = b, a                                         # (one in ten stays inverted)
        out.append(fmt(a, b, 100 + rng.randrange(keys), rng.choice([1, 2, 0xFF0000]),
                       op_of(op0 + i // 3, i % 3), REMOVE if rng.random() < 0.25 else 0))
    rng.shuffle(out)
    return out


class Pair(au.Pair):
    """anchor_util.Pair with the restatement of formats: a replica and the host log that holds the
    same items slot for slot."""

    def ref(self) -> FRef:
        assert self.rep.encode_diff([]) == self.host.encode_diff([])
        return FRef(self.oracle, self.host.arrays())

    def spans(self, ref: FRef, formats) -> tuple:
        """Host and device against the restatement, and therefore each other, byte for byte."""
        formats = list(formats)
        got = check(self.rep, ref, formats)
        host = check(self.host, ref, formats)
        assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes()
        assert got[2] == host[2]
        return got
