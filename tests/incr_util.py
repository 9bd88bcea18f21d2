"""Shared helpers of test_incr_edges.py and test_gpu_incr_edges.py (test infrastructure only).

The incremental merge (csrc/incr.hip: k_inc) keeps a replica's document order, tombstones
included.  Two things live here:

- Pair, the observer.  A replica and a host log fed the same update bytes, and check(), which
  compares what the public calls show of the kept order with a plain model built on the CPU
  oracle's order of the same log: the text, every anchor (which pins the rank of every slot, dead
  ones too), the text at every earlier mark (the relative order of items that have died since) and
  the patches since it.  Without a context the pair is the host log alone, so the model and the
  case builders are checked before a GPU sees them.
- The case builders.  Each returns a Case: steps of update bytes (the first is the base, merged in
  full), the path every step is expected to take, and what the case claims about its own batch
  (item count, roots, sibling groups, losing roots, run heads), which test_incr_edges.py reads
  back from the update bytes.

An update's wire layout (OpLog.encode_from): a 24-byte header (magic, version, first id, items,
first delete, deletes), then parent, origin-right, lamport and codepoint words, then u16 agents.
"""
from __future__ import annotations

import functools
import random
import struct
import types
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

import crdt_hip
import anchor_util as au
import patch_util as pu
from crdt_hip import AFTER, BEFORE, EDGE
from test_gpu_incr import _with_item_id

CH = "aé中😀"          # 1-, 2-, 3- and 4-byte codepoints
BIG = 20_000           # items above which a pair keeps only its first and its latest mark
SIDE_BIT = 1 << 31     # (Fugue updates) a left child


def chars(k: int, off: int = 0) -> str:
    return (CH * (k // 4 + 2))[off % 4: off % 4 + k]


@dataclass
class Step:
    updates: list               # update bytes, shipped together
    path: int = 1               # what merge_inc must report (None: not determined)
    pre: list = field(default_factory=list)   # calls that merge with no new item, made before the
    #                             step: None (one anchor resolved) or a deletes-only update
    claims: dict = field(default_factory=dict)
    wrong: tuple = ()           # the wrong orders this step tells from the right one
    sees: tuple = ("text",)     # ... and the comparisons that see the difference
    only: bool = False          # ... and no other comparison does


@dataclass
class Case:
    steps: list
    fugue: bool = False
    agent: int = 0              # the host log's agent (the closing keystroke)
    stride: int = 1             # resolve every stride-th identity (and all the step touches)


# ---- update bytes -----------------------------------------------------------------------------
def update_items(u: bytes) -> tuple:
    """(first id, parents, keys (lamport << 16 | agent), left-child bits) of an update's items."""
    first, n = struct.unpack_from("<II", u, 8)
    par = np.frombuffer(u, "<u4", n, 24).astype(np.int64)
    lam = np.frombuffer(u, "<u4", n, 24 + 8 * n).astype(np.int64)
    cpw = np.frombuffer(u, "<u4", n, 24 + 12 * n)
    agent = np.frombuffer(u, "<u2", n, 24 + 16 * n).astype(np.int64)
    return first, par, (lam << 16) | agent, (cpw & SIDE_BIT) != 0


def batch_facts(n0: int, maxkey: int, updates) -> dict:
    """What k_inc sees of a batch appended to a log of n0 items whose largest key is maxkey."""
    par, key, left = [], [], []
    for u in updates:
        first, p, k, l = update_items(u)
        assert len(p) == 0 or first == n0 + 1 + len(par)
        par += p.tolist()
        key += k.tolist()
        left += l.tolist()
    m = len(par)
    kids = Counter(par)
    roots = [i for i in range(m) if par[i] <= n0]
    new_groups = [c for p, c in kids.items() if p > n0]
    root_groups = [c for p, c in kids.items() if p <= n0]
    # a run: item i continues i - 1 when i - 1 is its parent and i that parent's only child
    heads = [i for i in range(m) if not (i > 0 and par[i] == n0 + i and kids[n0 + i] == 1)]
    return dict(m=m, roots=len(roots), new_group=max(new_groups, default=0),
                root_group=max(root_groups, default=0),
                losing=sum(1 for i in roots if key[i] <= maxkey), heads=heads,
                new_left=sum(1 for i in range(m) if left[i] and par[i] > n0),
                idents=key)


def _delta(log: crdt_hip.OpLog, fn) -> bytes:
    v = log.version()
    fn(log)
    return log.encode_from(v)


def _set_parent(u: bytes, k: int, parent: int) -> bytes:
    b = bytearray(u)
    struct.pack_into("<I", b, 24 + 4 * k, parent)
    return bytes(b)


def _root(a: crdt_hip.OpLog, text: str, parent: int = None, key: tuple = None, pos: int = 0) -> bytes:
    """One insert of `a` as an update of its own, its first item re-parented and re-keyed."""
    u = _delta(a, lambda l: l.insert(pos, text))
    if parent is not None:
        u = _set_parent(u, 0, parent)
    if key is not None:
        u = _with_item_id(u, 0, key[0], key[1])
    return u


@functools.lru_cache(maxsize=None)
def _paste(n: int, fugue: bool = False, agent: int = 0) -> bytes:
    log = crdt_hip.OpLog(fugue=fugue, agent=agent)
    log.insert(0, chars(n))
    return log.encode_from(0)


def _author(base, fugue: bool = False, agent: int = 0) -> crdt_hip.OpLog:
    a = crdt_hip.OpLog(fugue=fugue, agent=agent)
    for u in base:
        a.apply_update(u)
    return a


# ---- the observer -----------------------------------------------------------------------------
class Pair:
    """A replica (with a context) and a host log fed the same update bytes: no joins and no
    deltas, which would rebuild the kept order instead of splicing it."""

    def __init__(self, oracle, ctx=None, fugue: bool = False, agent: int = 0):
        self.oracle, self.fugue = oracle, fugue
        self.host = crdt_hip.OpLog(fugue=fugue, agent=agent)
        self.rep = None
        if ctx is not None:
            self.rep = crdt_hip.Replica(ctx, crdt_hip.OpLog(fugue=True) if fugue else None)
        self.docs = [self.host] + ([self.rep] if self.rep is not None else [])
        self.marks = []     # (text then, At, [a mark per document])

    def close(self) -> None:
        for _, _, ms in self.marks:
            for mk in ms:
                mk.close()
        self.marks = []
        if self.rep is not None:
            self.rep.close()

    def ship(self, updates) -> None:
        if self.rep is not None:
            self.rep.apply_updates(list(updates))
        for u in updates:
            self.host.apply_update(u)

    def idle(self, pre) -> None:
        """Calls that merge with no new item: one anchor resolved, or a deletes-only update."""
        for u in pre:
            if u is not None:
                assert struct.unpack_from("<I", u, 12)[0] == 0
                self.ship([u])
            if self.rep is not None:
                if u is None:
                    self.rep.resolve_anchors([(EDGE, AFTER)])
                else:
                    assert self.rep.merge_inc()[2] == 1

    def keystroke(self) -> None:
        u = _delta(self.host, lambda l: l.insert(l.visible_len() // 2, "k"))
        if self.rep is not None:
            self.rep.apply_updates([u])

    def snapshot(self) -> tuple:
        """(items, the largest key) the log holds."""
        a = self.host.arrays()
        keys = (a.lamport.astype(np.int64) << 16) | a.agent.astype(np.int64)
        return a.n, int(keys.max()) if a.n else 0

    def check(self, expect_path=None, stride: int = 1, touched=()) -> au.Ref:
        host, rep = self.host, self.rep
        # 1. the same log, slot for slot
        if rep is not None:
            assert rep.encode_diff([]) == host.encode_diff([])
        arrs = host.arrays()
        ref = au.Ref(self.oracle, arrs)
        text = "".join(chr(int(arrs.cp[s - 1])) for s in ref.vis)
        # 2. text and counters
        if rep is not None:
            cps, nb, path, got = rep.merge_inc(text=True)
            assert got == text.encode("utf-8")
            assert (cps, nb) == rep.info()[1:] == (ref.len, ref.nbytes)
            if expect_path is not None:
                assert path == expect_path, f"path {path}, expected {expect_path}"
        assert host.text_at() == text.encode("utf-8")
        # 3. the order, tombstones included: every identity under both biases, and the edges
        idents = ref.ident[::stride] + ([int(k) for k in touched] if stride > 1 else [])
        anchors = [(EDGE, AFTER), (EDGE, BEFORE)]
        anchors += [(k, BEFORE) for k in idents] + [(k, AFTER) for k in idents]
        raw = au.raw_anchors(anchors)
        for d in self.docs:
            au.check_resolve(d, ref, raw)
        # 4. marks: the text then (items alive then and dead now keep their order), the patches
        for then, at, ms in self.marks:
            want = pu.patches(at, arrs, ref.order)
            assert pu.apply_patches(then, want) == text
            for d, mk in zip(self.docs, ms):
                assert d.text_at(mk) == then.encode("utf-8")
                got = d.patches_since(mk)
                assert pu.apply_patches(then, got) == text
                assert got == want
        at = types.SimpleNamespace(n=arrs.n, deleted=arrs.deleted.copy(), text=text)
        if arrs.n > BIG and len(self.marks) > 1:
            for mk in self.marks.pop()[2]:
                mk.close()
        self.marks.append((text, at, [d.mark() for d in self.docs]))
        # 5. the state left behind
        if rep is not None:
            cps, nb, path, got = rep.merge_inc(text=True)
            assert path == 1 and got == text.encode("utf-8")
        return ref


def run_case(case: Case, oracle, ctx=None, hook=None) -> None:
    """Every step shipped and checked, then one keystroke more, which a state that the batch left
    corrupt does not survive.  hook(pair, step, (items, largest key) before it, ref after it)."""
    pair = Pair(oracle, ctx, case.fugue, case.agent)
    try:
        for i, st in enumerate(case.steps):
            pair.idle(st.pre)
            before = pair.snapshot()
            pair.ship(st.updates)
            touched = batch_facts(before[0], before[1], st.updates)["idents"] if case.stride > 1 else ()
            ref = pair.check(0 if i == 0 else st.path, case.stride, touched)
            if hook is not None:
                hook(pair, st, before, ref)
        pair.keystroke()
        pair.check(1, case.stride)
    finally:
        pair.close()


# ---- the orders a wrong kernel would give -------------------------------------------------------
def _blocks(arrs, order, n0: int) -> list:
    """The oracle's order as [old item | (root, its new subtree in order)]."""
    root_of = {}
    for s in range(n0 + 1, arrs.n + 1):
        p = int(arrs.parent[s - 1])
        root_of[s] = s if p <= n0 else root_of[p]
    out = []
    for s in order:
        if s <= n0:
            out.append(s)
        elif out and isinstance(out[-1], tuple) and out[-1][0] == root_of[s]:
            out[-1][1].append(s)
        else:
            out.append((root_of[s], [s]))
    roots = [b[0] for b in out if isinstance(b, tuple)]
    assert len(roots) == len(set(roots)), "a new subtree is not contiguous"
    return out


def _flat(blocks) -> list:
    out = []
    for b in blocks:
        out += b[1] if isinstance(b, tuple) else [b]
    return out


def naive_order(arrs, order, n0: int) -> list:
    """Every new root right after its old parent (a Fugue left child: right before it), ahead of
    whatever the parent's old subtree holds: the order without inc_search."""
    key = lambda s: (int(arrs.lamport[s - 1]) << 16) | int(arrs.agent[s - 1])
    after, before, head = {}, {}, []
    for b in _blocks(arrs, order, n0):
        if isinstance(b, tuple):
            p = int(arrs.parent[b[0] - 1])
            left = arrs.side is not None and arrs.side[b[0] - 1]
            (before if left else after).setdefault(p, []).append(b)
    out = []
    for p in [0] + [s for s in order if s <= n0]:
        for b in sorted(before.get(p, []), key=lambda b: -key(b[0])):
            out += b[1]
        if p:
            out.append(p)
        for b in sorted(after.get(p, []), key=lambda b: -key(b[0])):
            out += b[1]
    return out


def tie_reversed_order(arrs, order, n0: int) -> list:
    """root_before's tie rule reversed: among the roots that follow the same old rank, the root
    whose parent ranks earlier first (Fugue: the left child of the next item before the right
    child of this one)."""
    rank = {s: r for r, s in enumerate(x for x in [0] + list(order) if x <= n0)}

    def pr(b):
        if arrs.side is not None:
            return 0 if arrs.side[b[0] - 1] else 1
        return rank[int(arrs.parent[b[0] - 1])]
    out, gap = [], []
    for b in _blocks(arrs, order, n0) + [0]:
        if isinstance(b, tuple):
            gap.append(b)
            continue
        out += sorted(gap, key=pr)
        gap = []
        out.append(b)
    return _flat(out[:-1])


def shown(arrs, order, at) -> dict:
    """What the observer compares, under `order`: the text, every identity's position, the text at
    the mark `at` and the patches since it."""
    live = [not d for d in arrs.deleted]
    text = "".join(chr(int(arrs.cp[s - 1])) for s in order if live[s - 1])
    pos, v = {}, 0
    for s in order:
        pos[s] = v
        v += live[s - 1]
    then = "".join(chr(int(arrs.cp[s - 1])) for s in order if s <= at.n and not at.deleted[s - 1])
    return dict(text=text, anchors=[pos[s] for s in range(1, arrs.n + 1)], marks=then,
                patches=pu.patches(at, arrs, order))


# ---- A: batch sizes and the three forest instances -------------------------------------------
A_SIZES = [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
A_FUGUE_SIZES = [1024, 1025, 2048, 2049, 4096, 4097]
A_N0 = 8200
A_HEADS = sorted({0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049} |
                 {q * 64 + d for q in (1, 2, 4) for d in (-1, 0, 1)})


def case_a(m: int, shape: str) -> Case:
    base = [_paste(A_N0)]
    a = _author(base)
    path = 1 if m <= 4096 else 0
    if shape == "paste":        # one root, one run
        u = _delta(a, lambda l: l.insert(A_N0 // 3, chars(m)))
        claims = dict(m=m, roots=1, heads=[0], heads_exact=True)
    elif shape == "singles":    # m roots at descending old positions, no run
        def go(l):
            for k in range(m):
                l.insert(2 * (m - k) - (k % 2), CH[k % 4])
        u = _delta(a, go)
        claims = dict(m=m, roots=m, root_group=1, heads=list(range(m)), heads_exact=True)
    else:                       # chunks whose heads fall on A_HEADS, each split in its middle
        heads = [h for h in A_HEADS if h < m]
        plan = []
        for h, nxt in zip(heads, heads[1:] + [m]):
            g = nxt - h
            plan.append((g - 1, True) if g >= 3 else (g, False))

        def go(l):
            for j, (length, split) in enumerate(plan):
                pos = 8000 - 37 * j     # descending: every chunk hangs under an old item
                l.insert(pos, chars(length, j))
                if split:               # a second child for an interior item of the chunk
                    l.insert(pos + length // 2, CH[(j + 3) % 4])
        u = _delta(a, go)
        claims = dict(m=m, roots=len(plan), heads=heads)
    return Case([Step(base, 0), Step([u], path, claims=claims)])


def case_a_fugue(m: int) -> Case:
    """A batch typed on a Fugue upstream: pastes, repeated inserts at the front of the previous
    insert (a chain of new left children, each the last left child of its parent), typing."""
    n0 = 6000
    base = [_paste(n0, True)]
    a = _author(base, True)
    rounds = (m - 1) // 44

    def go(l):
        for r in range(rounds):
            p = 5900 - 60 * r
            l.insert(p, chars(30, r))
            for j in range(6):
                l.insert(p, CH[(r + j) % 4])
            for j in range(8):
                l.insert(p + 10 + j, CH[(r + j + 1) % 4])
        l.insert(10, chars(m - 44 * rounds))
    u = _delta(a, go)
    return Case([Step(base, 0), Step([u], 1 if m <= 4096 else 0,
                                     claims=dict(m=m, min_new_left=5 * rounds))], fugue=True)


# ---- B: sibling groups ------------------------------------------------------------------------
def case_b_roots(k: int, shared: bool) -> Case:
    base = [_paste(3000)]
    a = _author(base)

    def go(l):
        for j in range(k):
            l.insert(1500 if shared else 100 + 2 * (k - j), CH[j % 4])
    u = _delta(a, go)
    claims = dict(m=k, roots=k, root_group=k if shared else 1)
    return Case([Step(base, 0), Step([u], 1, claims=claims)])


def case_b_children(k: int) -> Case:
    """k new children of one new item: more than 1024 of them merge in full (F_GROUP)."""
    base = [_paste(3000)]
    a = _author(base)

    def go(l):
        l.insert(50, "A")
        for j in range(k):
            l.insert(51, CH[j % 4])
    u = _delta(a, go)
    return Case([Step(base, 0), Step([u], 1 if k <= 1024 else 0,
                                     claims=dict(m=k + 1, roots=1, new_group=k))])


# ---- C: tile seams of the splice ----------------------------------------------------------------
C_N0 = [4094, 4095, 4096, 8191, 8192]


def case_c(n0: int, tomb: bool) -> Case:
    """Old item r sits at rank r.  Roots (a single character and a 3-character chunk each) under
    the items at ranks 0, 1, 4094, 4095, 4096, n0 - 1 and n0; old items around rank 4096 removed
    in the same batch; ranks 4094..4097 dead already in the `tomb` variant."""
    a = _author([_paste(n0)])
    dead = [x for x in range(4094, 4098) if x <= n0] if tomb else []
    base = [_paste(n0)]
    if tomb:
        base = base + [_delta(_author(base), lambda l: l.remove(4093, 4093 + len(dead)))]
    ranks = sorted({r for r in (0, 1, 4094, 4095, 4096, n0 - 1, n0) if r <= n0}, reverse=True)
    rm = [x for x in (4099, 4098, 4097, 4096, 4095, 4093, 4092) if x <= n0 and x not in dead]

    def go(l):
        for j, r in enumerate(ranks):
            l.insert(r, "😀" if r in (4095, 4096) else CH[j % 4])   # a 4-byte one each side
            l.insert(r, chars(3, j))
        for x in rm:    # (descending) old item x, whatever was put after the items before it
            i = x - 1 + 4 * sum(1 for r in ranks if r < x)
            l.remove(i, i + 1)
    u = bytearray(_delta(a, go))
    struct.pack_into("<I", u, 16, len(dead))    # its deletes follow the base's
    claims = dict(m=4 * len(ranks), roots=2 * len(ranks), root_group=2)
    return Case([Step(base, 0), Step([bytes(u)], 1, claims=claims)])


def case_c_fugue(n0: int) -> Case:
    """A new left child of the item at the first rank of tile 1 (its anchor is the last rank of
    tile 0), with a new right child of the item before it at the same anchor, and a new left child
    of the item at rank 1."""
    base = [_paste(n0, True)]
    a = _author(base, True)
    ups, wrong = [], ()
    if n0 >= 4096:
        ups.append(_delta(a, lambda l: l.insert(4095, "😀é")))
        ups.append(_set_parent(_delta(a, lambda l: l.insert(l.visible_len(), "中")), 0, 4095))
        wrong = ("tie",)
    ups.append(_delta(a, lambda l: l.insert(0, "中a")))
    # (typed at the end: a right child of the last item, which is that re-parented one if any)
    ups.append(_delta(a, lambda l: l.insert(l.visible_len(), "é")))
    m = sum(struct.unpack_from("<I", u, 12)[0] for u in ups)
    roots = len(ups) - (1 if n0 >= 4096 else 0)
    return Case([Step(base, 0), Step(ups, 1, claims=dict(m=m, roots=roots), wrong=wrong)],
                fugue=True)


# ---- D: a full staging area -------------------------------------------------------------------
def case_d(shape: str) -> Case:
    """4096 new items anchored inside tile 0 of a two-tile document: with its 4096 old ranks the
    tile stages 8192 words and writes its text in two passes."""
    base = [_paste(8192)]
    a = _author(base)
    if shape == "paste":
        u = _delta(a, lambda l: l.insert(100, chars(4096)))
        claims = dict(m=4096, roots=1)
    else:
        def go(l):
            for k in range(4096):
                l.insert((4095 - k) * 3999 // 4095, CH[k % 4])
        u = _delta(a, go)
        claims = dict(m=4096, roots=4096)
    return Case([Step(base, 0), Step([u], 1, claims=claims)])


# ---- E: look-back past one window ---------------------------------------------------------------
def case_e() -> Case:
    n0 = 65 * 4096 + 10     # 66 tiles: the last tile's first window of 64 predecessors ends at 1
    base = [_paste(n0)]
    a = _author(base)

    def go(l):
        for t in (65, 64, 63, 1):
            l.insert(t * 4096 + 5, "😀" + chars(3, t))
            l.remove(t * 4096 + 9, t * 4096 + 11)
        l.insert(10, "😀😀é")
        l.remove(2, 4)
    u = _delta(a, go)
    return Case([Step(base, 0), Step([u], 1, claims=dict(m=19, roots=5))], stride=7)


# ---- F: searched roots (RGA) ------------------------------------------------------------------
def case_f_scan(n: int) -> Case:
    """One typing chain under its first item and a losing root under the document start: the
    search examines ranks 1 .. 65536 and stops at rank n + 1."""
    base = [_paste(n, agent=1)]
    a = _author(base, agent=1)
    u = _with_item_id(_delta(a, lambda l: l.insert(0, "😀é")), 0, 1, 0)   # (1, 0) < (1, 1)
    return Case([Step(base, 0), Step([u], 1 if n <= 65535 else 0, wrong=("naive",),
                                     claims=dict(m=2, roots=1, losing=1))], agent=1)


def case_f_stops(variant: str) -> Case:
    """p (the end of a chunk in the middle) has two old children, c_hi with a subtree and c_lo.
    A root keyed between them goes after c_hi's subtree, before c_lo (the search stops at a child
    of p with a smaller key); a root keyed below both goes after c_lo's subtree (it stops at the
    next item, whose parent ranks before p).  `hi_gone`: all of c_hi's subtree is dead and only
    the first root is shipped, so the search moves it across tombstones alone: the text is the same
    wherever it lands, and only the anchors of the dead items tell."""
    a = crdt_hip.OpLog(agent=1)
    a.insert(0, chars(3000))
    a.insert(1500, "PQR")               # items 3001..3003: p = 3003
    a.insert(1503, chars(6, 1))         # c_lo = 3004 and its chain
    a.insert(1503, chars(9, 2))         # c_hi = 3010 and its chain, ahead of c_lo
    if variant == "p_dead":
        a.remove(1502, 1503)
    if variant == "hi_dead":
        a.remove(1505, 1508)
    if variant == "hi_gone":
        a.remove(1503, 1512)
    base = [a.encode_from(0)]
    ups = [_root(a, "😀中", 3003, (3005, 7)), _root(a, "é😀", 3003, (3004, 0))]
    if variant == "hi_gone":
        return Case([Step(base, 0), Step(ups[:1], 1, wrong=("naive",), sees=("anchors",), only=True,
                                         claims=dict(m=2, roots=1, losing=1))], agent=1)
    return Case([Step(base, 0), Step(ups, 1, wrong=("naive",),
                                     claims=dict(m=4, roots=2, losing=2, root_group=2))], agent=1)


def case_f_many(k: int) -> Case:
    """k losing roots (lamport 1, an agent each) under old items spread over a document of nested
    chunks: kIncSearchers workgroups share them; more than kIncHard merge in full."""
    a = crdt_hip.OpLog(agent=1)
    a.insert(0, chars(2000))
    for j in range(40):
        a.insert(1950 - 45 * j, chars(5, j))
    base = [a.encode_from(0)]
    n0 = 2200
    ups = [_root(a, CH[j % 4], 2 + (j * 37) % (n0 - 2), (1, 100 + j)) for j in range(k)]
    return Case([Step(base, 0), Step(ups, 1 if k <= 256 else 0, wrong=("naive",),
                                     claims=dict(m=k, roots=k, losing=k))], agent=1)


def case_f_key_edge(d: int) -> Case:
    """(500, 5) is the largest key.  A sibling of that item keyed (500, 4) is searched and goes
    after it; one keyed (500, 6) is not and goes right after the parent."""
    base = [_paste(500, agent=5)]
    a = _author(base, agent=5)
    u = _root(a, "é", 499, (500, 5 + d))     # (item 500 is a 4-byte one)
    return Case([Step(base, 0), Step([u], 1, wrong=("naive",) if d < 0 else (),
                                     claims=dict(m=1, roots=1, losing=1 if d < 0 else 0))], agent=5)


def case_f_tie() -> Case:
    """An old chain p -> c1 -> .. -> c4 whose subtrees all end at rank(c4).  A local child of c4
    and losing roots under c2, c1 and p (three, by key) all follow that rank: the anchor item's
    own child first, then the losers of the deeper ancestors before the shallower."""
    a = crdt_hip.OpLog(agent=1)
    a.insert(0, chars(1000))
    a.insert(500, "pcdef")              # p = 1001, c1..c4 = 1002..1005
    base = [a.encode_from(0)]
    ups = [_root(a, "L", 1005), _root(a, "l", 1001),
           _root(a, "😀", 1001, (1, 50)), _root(a, "é", 1002, (1, 51)), _root(a, "中", 1003, (1, 52)),
           _root(a, "u", 1001, (1, 60)), _root(a, "v", 1001, (1, 61))]
    return Case([Step(base, 0), Step(ups, 1, wrong=("tie", "naive"),
                                     claims=dict(m=7, roots=7, losing=5, root_group=4))], agent=1)


def case_f_parity(k: int) -> Case:
    """A fast-path batch, k calls that merge with no new item, then a root that loses to an item
    of that batch: the largest key must have been carried over every one of those calls."""
    base = [_paste(300, agent=1)]
    a = _author(base, agent=1)
    b1 = _delta(a, lambda l: l.insert(100, "HELLO😀"))     # H: (301, 1) under item 100
    pre = [None if j != 1 else _delta(a, lambda l: l.remove(5, 6)) for j in range(k)]
    u = _root(a, "中", 100, (301, 0))
    return Case([Step(base, 0), Step([b1], 1, claims=dict(m=6, roots=1, losing=0)),
                 Step([u], 1, pre=pre, wrong=("naive",), claims=dict(m=1, roots=1, losing=1))],
                agent=1)


# ---- G: Fugue state -----------------------------------------------------------------------------
def case_g(variant: str) -> Case:
    if variant == "low_root":
        # a right child of item 50 keyed below the largest key: no search for Fugue roots
        base = [_paste(100, True)]
        a = _author(base, True)
        u = _root(a, "😀", 50, (1, 9), pos=100)
        return Case([Step(base, 0), Step([u], 0, claims=dict(m=1, roots=1, losing=1))], fugue=True)
    base = [_paste(100, True)]
    a = _author(base, True)
    steps = [Step(base, 0)]
    # item 51 receives its first left child on the fast path
    steps.append(Step([_delta(a, lambda l: l.insert(50, "x"))], 1, claims=dict(m=1, roots=1)))
    pre = []
    if variant == "grow":   # (the order arrays and the left-child bits grow at the 2nd and 4th)
        for j in range(4):
            steps.append(Step([_delta(a, lambda l: l.insert(l.visible_len(), chars(4096, j)))], 1,
                              claims=dict(m=4096, roots=1)))
    else:
        pre = [None, None, None]
    # a remote left child of item 51 (typed as a left child of x, re-parented): merged in full
    u = _set_parent(_delta(a, lambda l: l.insert(50, "😀")), 0, 51)
    steps.append(Step([u], 0, pre=pre, claims=dict(m=1, roots=1)))
    return Case(steps, fugue=True)


# ---- H: seeded differential ---------------------------------------------------------------------
def case_h(seed: int, fugue: bool) -> Case:
    rng = random.Random(0x1AC0 + seed)
    a = crdt_hip.OpLog(fugue=fugue, agent=1)
    state = dict(items=0, maxlam=0, ups=0)

    def edit(l, room):
        """One random edit that appends at most `room` items; returns how many it appended."""
        n = l.visible_len()
        if n > 4 and (room == 0 or rng.random() < 0.3):
            p = rng.randrange(n - 3)
            l.remove(p, p + rng.randint(1, 3))
            return 0
        k = min(room, rng.randint(1, 6))
        l.insert(rng.randint(0, n), chars(k, rng.randrange(4)))
        return k

    def update(room, rekey):
        got = [0]

        def go(l):
            for _ in range(rng.randint(1, 3)):
                got[0] += edit(l, room - got[0])
        u = _delta(a, go)
        n = got[0]
        state["ups"] += 1
        if rekey and n and state["maxlam"] > 2:
            lam = rng.randint(1, state["maxlam"] - 1)
            for k in range(n):
                u = _with_item_id(u, k, lam + k, 1000 + state["ups"])
        for k in range(n):
            state["maxlam"] = max(state["maxlam"], struct.unpack_from("<I", u, 24 + 8 * n + 4 * k)[0])
        state["items"] += n
        return u, n

    base = []
    while state["items"] < 600:
        base.append(update(50, False)[0])
    steps = [Step(base, 0)]
    for _ in range(8):
        want, ups, have = rng.randint(1, 200), [], 0
        while have < want:
            u, n = update(want - have, not fugue and rng.random() < 0.2)
            ups.append(u)
            have += n
        steps.append(Step(ups, 1, claims=dict(m=want)))
    return Case(steps, fugue=fugue, agent=1)


# ---- every case by name: (builder, arguments) ---------------------------------------------------
def all_cases() -> dict:
    c = {}
    for m in A_SIZES:
        for shape in ("paste", "singles", "chunks"):
            c[f"A-{shape}-{m}"] = (case_a, m, shape)
    for m in A_FUGUE_SIZES:
        c[f"A-fugue-{m}"] = (case_a_fugue, m)
    for k in (32, 33):
        for shared in (True, False):
            c[f"B-roots-{k}-{'shared' if shared else 'distinct'}"] = (case_b_roots, k, shared)
    for k in (1024, 1025, 1100):
        c[f"B-roots-{k}-shared"] = (case_b_roots, k, True)
    for k in (1024, 1025):
        c[f"B-children-{k}"] = (case_b_children, k)
    for n0 in C_N0:
        for tomb in (False, True):
            c[f"C-{n0}-{'tomb' if tomb else 'live'}"] = (case_c, n0, tomb)
        c[f"C-fugue-{n0}"] = (case_c_fugue, n0)
    for shape in ("paste", "singles"):
        c[f"D-{shape}"] = (case_d, shape)
    c["E-66-tiles"] = (case_e,)
    for n in (4095, 4096, 8191, 8192, 65535, 65536):
        c[f"F-scan-{n}"] = (case_f_scan, n)
    for v in ("live", "p_dead", "hi_dead", "hi_gone"):
        c[f"F-stops-{v}"] = (case_f_stops, v)
    for k in (15, 16, 17, 33, 256, 257):
        c[f"F-many-{k}"] = (case_f_many, k)
    for d in (-1, 1):
        c[f"F-key-{'below' if d < 0 else 'above'}"] = (case_f_key_edge, d)
    c["F-tie"] = (case_f_tie,)
    for k in range(4):
        c[f"F-parity-{k}"] = (case_f_parity, k)
    for v in ("grow", "idle", "low_root"):
        c[f"G-{v}"] = (case_g, v)
    for seed in range(20):
        c[f"H-{seed}-rga"] = (case_h, seed, False)
        c[f"H-{seed}-fugue"] = (case_h, seed, True)
    return c


def build(entry: tuple) -> Case:
    return entry[0](*entry[1:])
