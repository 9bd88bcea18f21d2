"""Shared helpers of test_many_tiles.py and test_gpu_many_tiles.py (test infrastructure only).

The 258-tile shape: N = 1,056,000 items typed in one run, so the document order is the slot order
(rank k is item k) and ranks 0..N fill 258 tiles of 4,096 ranks.  Every kernel that reads the kept
order scans its tile aggregates in rounds of 256 tiles, so tile 255 (ranks 1,044,480..1,048,575) is
the last of round 1, tile 256 (ranks 1,048,576..1,052,671) the first of round 2, whose prefix is
the carry alone, and tile 257 (ranks 1,052,672..N) needs the carry and tile 256's aggregate.  The
text mixes the four UTF-8 widths and about 20 % of the items are tombstones, so no tile's count is
4,096, no byte prefix equals its codepoint prefix and the three carries (codepoints, bytes, and for
patches the deleted ones) all differ.

The reference (NRef) restates text windows, anchors, formats and patches since a mark from the
definitions of include/crdt_hip.h over three numpy arrays, the codepoint, the tombstone and the
identity of every rank, and calls the product for nothing: because the log is one run, "the
visible items at the ranks before rank k" is a cumulative sum.  test_many_tiles.py ties it to the
host calls at N and to the oracle-based restatements (anchor_util.Ref, format_util.FRef) at 300.
"""
from __future__ import annotations

import numpy as np

import crdt_hip
import patch_util as pu
import text_util as tu
from crdt_hip import AFTER, BEFORE, DEAD, EDGE, LIVE, REMOVE, UNKNOWN

TILE = 4096
TOP = 256                                   # tiles a round of the one-workgroup scan takes
N = 1_056_000
WIDE4 = (1_048_575, 1_048_576, 1_052_671, 1_052_672)   # last of tile 255, first of 256, ... of 257
E = (1_048_575, 1_048_576, 1_048_577, 1_052_671, 1_052_672, 1_052_673, N)
DEAD_EDGE = (1_040_384, 1_048_574)          # tile 254 and all of tile 255 but its last rank
LAYOUTS = ["sprinkled", "dead_edge"]
KINDS = ["rga", "fugue"]
ALPHABET = np.array([ord(c) for c in "abcdefgh  \n" + tu.WIDE], np.uint32)   # text_util.mixed_text's


def codepoints(n: int, seed: int) -> np.ndarray:
    """n codepoints, a seeded mix of the four UTF-8 widths (mostly ASCII, as text is)."""
    return ALPHABET[np.random.default_rng(seed).integers(0, ALPHABET.size, n)]


def widths(cps: np.ndarray) -> np.ndarray:
    """UTF-8 bytes of every codepoint."""
    c = cps.astype(np.int64)
    return 1 + (c >= 0x80) + (c >= 0x800) + (c >= 0x10000)


def to_str(cps: np.ndarray) -> str:
    return np.ascontiguousarray(cps, dtype="<u4").tobytes().decode("utf-32-le")


def shape(layout: str, n: int = N, seed: int = 1) -> tuple:
    """(cps, dead) of ranks 1..n: about 20 % of the items dead at random; with n == N the ranks of
    WIDE4 hold a visible 4-byte codepoint, rank N is visible (what is typed at the end then lands
    at the end), and `dead_edge` has every rank of DEAD_EDGE dead."""
    assert layout in LAYOUTS
    cps = codepoints(n, seed)
    dead = np.random.default_rng(seed + 1).random(n) < 0.2
    if n == N:
        if layout == "dead_edge":
            dead[DEAD_EDGE[0] - 1: DEAD_EDGE[1]] = True
        for k in WIDE4:
            cps[k - 1] = ord("😀")
            dead[k - 1] = False
        dead[N - 1] = False
    elif layout == "dead_edge":
        dead[n // 3: n // 2] = True
    return cps, dead


def build_log(fugue: bool, cps: np.ndarray, dead: np.ndarray) -> tuple:
    """(log, ident): the text typed in one insert, its tombstones set through LogArrays and joined
    into an empty log; ident[k - 1] is the identity lamport << 16 | agent of the item of rank k."""
    n = cps.size
    full = pu.new_log(fugue)
    full.insert(0, to_str(cps))
    A = full.arrays()
    assert A.n == n and (A.cp == cps).all()
    cut = crdt_hip.LogArrays(A.parent, A.lamport, A.agent, dead.astype(np.uint8), A.cp,
                             side=A.side if fugue else None)
    log = pu.new_log(fugue)
    assert log.join(cut) == (n, 0)
    return log, (A.lamport.astype(np.uint64) << np.uint64(16)) | A.agent.astype(np.uint64)


class NRef:
    """The definitions over a document whose rank k is item k: cps, dead and ident hold rank k at
    index k - 1.  `was`: the items selected by a mark (None: no mark taken)."""

    def __init__(self, cps, dead, ident, was=None):
        self.cps = np.asarray(cps, np.uint32)
        self.live = ~np.asarray(dead, bool)
        self.ident = np.asarray(ident, np.uint64)
        self.was = was
        self.n = self.cps.size
        self._index()

    def _index(self):
        w = widths(self.cps)
        self.width = w
        # cv[k], cb[k]: the visible items, and their bytes, of ranks 1..k (cv[k - 1]: before rank k)
        self.cv = np.concatenate([[0], np.cumsum(self.live, dtype=np.int64)])
        self.cb = np.concatenate([[0], np.cumsum(w * self.live, dtype=np.int64)])
        self.vis = np.flatnonzero(self.live) + 1            # rank of the visible items, in order
        self.bd = np.concatenate([[0], self.cb[self.vis]])  # bytes of the first v visible items
        self.len, self.nbytes = int(self.cv[-1]), int(self.cb[-1])
        self._by_id = self._text = None                     # (made when first asked for)

    # ---- text ----
    def text(self) -> str:
        if self._text is None:
            self._text = to_str(self.cps[self.live])
        return self._text

    def marked_text(self) -> str:
        return to_str(self.cps[: self.was.size][self.was])

    def boundaries(self) -> "IntSeq":
        """Byte offset of every codepoint boundary of the visible text (text_util.boundaries)."""
        return IntSeq(self.bd)

    # ---- edits that keep rank k == item k ----
    def take_mark(self) -> None:
        self.was = self.live.copy()

    def remove(self, a: int, b: int) -> None:
        """Visible positions [a, b) die."""
        self.live[self.vis[a:b] - 1] = False
        self._index()

    def append(self, cps, ident) -> None:
        """Items typed at the end of a document whose last rank is visible."""
        assert self.live[-1]
        self.cps = np.concatenate([self.cps, np.asarray(cps, np.uint32)])
        self.live = np.concatenate([self.live, np.ones(len(cps), bool)])
        self.ident = np.concatenate([self.ident, np.asarray(ident, np.uint64)])
        self.n = self.cps.size
        self._index()

    # ---- anchors ----
    def rank_of(self, ident: int):
        """Rank of the item with that identity, or None when the document does not hold it."""
        if self._by_id is None:
            self._by_id = np.argsort(self.ident, kind="stable")
        i = int(np.searchsorted(self.ident, np.uint64(ident), sorter=self._by_id))
        if i < self.n and int(self.ident[self._by_id[i]]) == ident:
            return int(self._by_id[i]) + 1
        return None

    def gap_of_bytes(self, p: int) -> int:
        """The gap (visible items before it) at byte offset p; ValueError inside a codepoint."""
        v = int(np.searchsorted(self.bd, p))
        if v > self.len or int(self.bd[v]) != p:
            raise ValueError("inside a codepoint")
        return v

    def at(self, p: int, bias: int, bytes: bool = False) -> tuple:
        if bytes:
            p = self.gap_of_bytes(p)
        assert 0 <= p <= self.len
        if bias == AFTER:
            return (EDGE if p == 0 else int(self.ident[self.vis[p - 1] - 1]), AFTER)
        return (EDGE if p == self.len else int(self.ident[self.vis[p] - 1]), BEFORE)

    def resolve(self, anchor: tuple) -> tuple:
        ident, bias = anchor
        if ident == EDGE:
            return (0, 0, LIVE) if bias == AFTER else (self.len, self.nbytes, LIVE)
        k = self.rank_of(ident)
        if k is None:
            return (0, 0, UNKNOWN)
        if self.live[k - 1] and bias == AFTER:
            return (int(self.cv[k]), int(self.cb[k]), LIVE)
        return (int(self.cv[k - 1]), int(self.cb[k - 1]), LIVE if self.live[k - 1] else DEAD)

    def anchors_raw(self, positions, biases, bytes: bool = False) -> np.ndarray:
        arr = np.zeros(len(positions), crdt_hip.ANCHOR_DTYPE)
        for i, (p, b) in enumerate(zip(positions, biases)):
            arr[i] = (*self.at(int(p), int(b), bytes), 0)
        return arr

    def positions_raw(self, anchors) -> np.ndarray:
        arr = np.zeros(len(anchors), crdt_hip.ANCHOR_POS_DTYPE)
        for i, a in enumerate(anchors):
            arr[i] = (*self.resolve((int(a[0]), int(a[1]))), 0)
        return arr

    # ---- formats ----
    def gap(self, anchor):
        """Gap 0..n of an anchor (gap g lies right after rank g), None when its item is not held."""
        ident, bias = anchor
        if ident == EDGE:
            return 0 if bias == AFTER else self.n
        k = self.rank_of(ident)
        if k is None:
            return None
        return k if bias == AFTER else k - 1

    def spans(self, formats) -> tuple:
        """([(pos, pos_bytes, len, len_bytes, [(key, value)])], pending, segments): the spans, the
        formats with an end the document does not hold, and the stretches between two neighbouring
        distinct gaps named by the placed formats that cover something."""
        placed, pending, gaps = [], 0, set()
        for start, end, key, value, op, flags in formats:
            gs, ge = self.gap(start), self.gap(end)
            if gs is None or ge is None:
                pending += 1
                continue
            placed.append((key, op, gs, ge, value, flags))
            if gs < ge:
                gaps |= {gs, ge}
        keys = sorted({f[0] for f in placed})
        nv = self.len
        has = np.zeros((len(keys), nv), bool)
        val = np.zeros((len(keys), nv), np.uint64)
        # ascending by op, a later format overwrites the items it covers: the largest op wins
        for key, op, gs, ge, value, flags in sorted(placed, key=lambda f: f[1]):
            i = keys.index(key)
            a, b = int(self.cv[gs]), int(self.cv[max(ge, gs)])   # the visible items of ranks gs+1..ge
            has[i, a:b] = not flags & REMOVE
            val[i, a:b] = 0 if flags & REMOVE else value
        out = []
        if nv and keys:
            head = np.ones(nv, bool)
            head[1:] = (has[:, 1:] != has[:, :-1]).any(0) | (val[:, 1:] != val[:, :-1]).any(0)
            starts = np.flatnonzero(head).tolist() + [nv]
            for a, b in zip(starts, starts[1:]):
                attrs = [(keys[i], int(val[i, a])) for i in range(len(keys)) if has[i, a]]
                if attrs:
                    out.append((a, int(self.bd[a]), b - a, int(self.bd[b] - self.bd[a]), attrs))
        return out, pending, max(len(gaps) - 1, 0)

    # ---- patches since the mark ----
    def patches(self, bytes: bool = False) -> list:
        """[(pos, del, ins: str)] since take_mark(), in codepoints or in UTF-8 bytes."""
        was = np.zeros(self.n, bool)
        was[: self.was.size] = self.was
        now = self.live
        keep = np.flatnonzero(was | now)                    # neither: dropped
        was, now = was[keep], now[keep]
        wt = self.width[keep] if bytes else np.ones(keep.size, np.int64)
        before = np.concatenate([[0], np.cumsum(wt * now)])  # the `now` items before each
        gone = np.concatenate([[0], np.cumsum(wt * (was & ~now))])
        k = np.concatenate([[True], was & now, [True]])      # K, with a sentinel at both ends
        first = np.flatnonzero(k[:-1] & ~k[1:])              # runs of non-K: [first, last)
        last = np.flatnonzero(~k[:-1] & k[1:])
        out = []
        for a, b in zip(first.tolist(), last.tolist()):
            ins = keep[a:b][now[a:b]]
            out.append((int(before[a]), int(gone[b] - gone[a]), to_str(self.cps[ins])))
        return out


def splice(text: str, plist) -> str:
    """patch_util.apply_patches by slices of the string (a few patches of a long text)."""
    for pos, dele, ins in plist:
        assert pos + dele <= len(text)
        text = text[:pos] + ins + text[pos + dele:]
    return text


def raw_patches(plist) -> tuple:
    """[(pos, del, ins)] as the (crdt_hip_patch array, ins bytes) the product returns."""
    arr, ins = crdt_hip._patches_pack(plist)
    return arr, ins


def raw_spans(want) -> tuple:
    sp = np.zeros(len(want), crdt_hip.SPAN_DTYPE)
    at = []
    for k, (pos, posb, ln, lnb, attrs) in enumerate(want):
        sp[k] = (pos, posb, ln, lnb, len(at), len(attrs))
        at += attrs
    arr = np.zeros(len(at), crdt_hip.SPAN_ATTR_DTYPE)
    for k, (key, value) in enumerate(at):
        arr[k] = (value, key, 0)
    return sp, arr


def near_visible(ref: NRef, k: int) -> list:
    """Rank k where it is visible, else the nearest visible rank on each side of it."""
    if ref.live[k - 1]:
        return [k]
    v = int(ref.cv[k])                                      # visible items of ranks 1..k
    return [int(ref.vis[i]) for i in (v - 1, v) if 0 <= i < ref.len]


def named_gaps(ref: NRef, ranks=E) -> list:
    """The gaps (visible positions) before and behind every rank of `ranks`, with the nearest
    visible rank on each side where one is dead, and 0, 1 and the end."""
    gaps = {0, 1, ref.len}
    for r in ranks:
        for k in [r] + near_visible(ref, r):
            gaps |= {int(ref.cv[k - 1]), int(ref.cv[k])}
    return sorted(gaps)


class IntSeq:
    """A numpy array read as a sequence of Python ints (what text_util.check_window indexes)."""

    def __init__(self, arr):
        self.arr = arr

    def __len__(self) -> int:
        return len(self.arr)

    def __getitem__(self, i) -> int:
        return int(self.arr[i])


# ---- the cases of test_many_tiles.py (host against NRef) and test_gpu_many_tiles.py (device
# against both): built from the reference's arrays alone ----
def window_pairs(ref: NRef) -> list:
    """Every ordered pair of the named gaps."""
    g = named_gaps(ref)
    return [(a, b) for i, a in enumerate(g) for b in g[i:]]


def tiles_of(ref: NRef, a: int, b: int) -> int:
    """The tiles from that of the first to that of the last item of the visible window [a, b)."""
    return int(ref.vis[b - 1]) // TILE - int(ref.vis[a]) // TILE + 1 if b > a else 0


def inside_wide4(ref: NRef) -> list:
    """The byte offsets 1, 2 and 3 bytes into each of the four named 4-byte codepoints."""
    assert all(ref.live[k - 1] and ref.width[k - 1] == 4 for k in WIDE4)
    return [int(ref.cb[k - 1]) + j for k in WIDE4 for j in (1, 2, 3)]


def anchor_gaps(ref: NRef, seed: int = 5) -> tuple:
    """(gaps, biases): the named gaps and 100 seeded random ones, each under both biases."""
    rnd = np.random.default_rng(seed).integers(0, ref.len + 1, 100).tolist()
    g = named_gaps(ref) + rnd
    return g + g, [AFTER] * len(g) + [BEFORE] * len(g)


def near_anchors(ref: NRef) -> list:
    """An anchor under each bias on every item within 70 ranks of the first rank of tiles 256 and
    257, the dead ones included."""
    ranks = [k for edge in (TOP * TILE, (TOP + 1) * TILE) for k in range(edge - 70, edge + 71)]
    return [(int(ref.ident[k - 1]), b) for k in ranks for b in (AFTER, BEFORE)]


def format_set(ref: NRef) -> list:
    """Thirteen formats over three keys whose ends are anchors on items of tiles 0, 100, 255, 256
    and 257: ten distinct gaps lie below tile 256's (among them 1,048,575, named once by an end
    AFTER rank 1,048,575 and once by a start BEFORE rank 1,048,576), four in tile 256 and eight in
    tile 257.  Format 8 is a REMOVE that wins over a part of format 5, 9 is pending (nobody holds
    its start), 10 ends at EDGE, 11 starts at EDGE, 12 loses to format 1 wherever both cover, and
    13 repeats format 6's value right behind it, so that two segments make one span."""
    def on(rank, bias):
        return (int(ref.ident[rank - 1]), bias)

    def op(lamport, agent=1):
        return (lamport << 16) | agent
    t100, t255, t256, t257 = 100 * TILE, 255 * TILE, 256 * TILE, 257 * TILE
    return [
        (on(100, BEFORE), on(t100 + 5, AFTER), 1, 1, op(20), 0),
        (on(3000, AFTER), on(t255 + 10, BEFORE), 2, 2, op(2), 0),
        (on(t100 + 2005, BEFORE), on(t256 - 1, AFTER), 1, 3, op(3), 0),
        (on(t256, BEFORE), on(t256 + 1000, AFTER), 3, 4, op(4), 0),
        (on(t256, AFTER), on(t257 - 1, AFTER), 2, 5, op(5), 0),
        (on(t257, BEFORE), on(t257 + 500, AFTER), 1, 6, op(6), 0),
        (on(t257, AFTER), on(N - 10, BEFORE), 3, 7, op(7), 0),
        (on(t256 + 424, BEFORE), on(t257 + 228, AFTER), 2, 0, op(8, 2), REMOVE),
        ((op(5, 0x7777), AFTER), (EDGE, BEFORE), 1, 9, op(9), 0),
        (on(t257 + 328, BEFORE), (EDGE, BEFORE), 2, 10, op(10), 0),
        ((EDGE, AFTER), on(50, AFTER), 3, 11, op(11), 0),
        (on(200, BEFORE), on(300_000, AFTER), 1, 12, op(1), 0),
        (on(t257 + 500, BEFORE), on(t257 + 900, AFTER), 1, 6, op(13), 0),
    ]


def mark_edit(ref: NRef, tail: np.ndarray):
    """The edit after the mark, on the reference and as a function of a log: a stretch inside tile
    257 dies, then the visible items of ranks 1,048,570..1,048,590, and `tail` is typed at the
    end.  The caller appends the tail's identities to the reference (NRef.append)."""
    cuts = [(int(ref.cv[257 * TILE + 300]), int(ref.cv[257 * TILE + 700])),
            (int(ref.cv[1_048_569]), int(ref.cv[1_048_590]))]
    for a, b in cuts:
        ref.remove(a, b)

    def fn(log):
        for a, b in cuts:
            log.remove(a, b)
        log.insert(log.visible_len(), to_str(tail))
    return fn


def byte_patches(ref: NRef) -> tuple:
    """(byte patch list, codepoint patch list) of four sequential patches: a replace in tile 0, a
    delete from the last visible ranks of tile 255 to inside tile 256, a replace inside tile 257
    and an insert at the end.  The boundaries come from the reference's byte prefixes."""
    ins = ["aé€😀", "", "x€", to_str(codepoints(20, 77))]
    spans = [(10, 13), (int(ref.cv[1_048_560]), int(ref.cv[1_048_580])),
             (int(ref.cv[257 * TILE + 28]), int(ref.cv[257 * TILE + 28]) + 2), (ref.len, ref.len)]
    assert int(ref.vis[spans[1][0]]) // TILE == 255 and int(ref.vis[spans[1][1] - 1]) // TILE == 256
    assert int(ref.vis[spans[2][0]]) // TILE == 257
    out_b, out_c, dc, db = [], [], 0, 0
    for (a, b), text in zip(spans, ins):
        out_c.append((a + dc, b - a, text))
        out_b.append((int(ref.bd[a]) + db, int(ref.bd[b] - ref.bd[a]), text))
        dc += len(text) - (b - a)
        db += len(text.encode()) - int(ref.bd[b] - ref.bd[a])
    return out_b, out_c


def codepoint_patches(ref: NRef) -> list:
    """test_gpu_edit.test_257_tiles' three patches, the last at an item of tile 256, and a fourth
    in tile 257 (sequential: each pos counts in the document as the earlier ones left it)."""
    p2, p3 = int(ref.cv[1_048_600]) - 4, int(ref.cv[257 * TILE + 128]) - 4 + 4
    return [(5, 2, "Q"), (4095, 3, ""), (p2, 0, "tail"), (p3, 1, "é")]


def read_window(obj, mark, start: int, end: int, in_bytes: bool, guess: int) -> tuple:
    """(bytes, info) of one text_at call of a log or a replica (`guess`: the buffer to try first)."""
    ctx = obj.ctx._h if isinstance(obj, crdt_hip.Replica) else None
    return crdt_hip._text_get(tu.call_of(obj), mark, start, end, in_bytes, ctx, guess=guess)


def want_window(text: str, bd, a: int, b: int) -> tuple:
    """(bytes, info) of the visible window [a, b) of `text` by the reference."""
    return text[a:b].encode("utf-8"), tu.want_info(text, a, b, bd)


class Doc:
    """A log of one kind and layout (the 258-tile shape unless n says otherwise) and its
    reference; after edit_after_mark also the mark, the reference at the mark and the two texts."""

    def __init__(self, kind: str, layout: str, n: int = N):
        self.fugue = kind == "fugue"
        cps, dead = shape(layout, n)
        self.host, ident = build_log(self.fugue, cps, dead)
        self.ref = NRef(cps, dead, ident)
        self.hmark = self.at_mark = None

    def clone(self) -> "Doc":
        """Another log with the same items and its own reference (for a test that edits)."""
        d = object.__new__(Doc)
        d.fugue, d.host = self.fugue, self.host.clone()
        d.ref = NRef(self.ref.cps, ~self.ref.live, self.ref.ident)
        d.hmark = d.at_mark = None
        return d

    def edit_after_mark(self, follow=None) -> None:
        """Takes a mark, then applies mark_edit with 5,000 mixed-width items typed at the end, as
        one wire update (made on a copy of the log, as a remote edit arrives); follow(update)
        feeds it to a replica."""
        n = self.ref.n
        self.at_mark = NRef(self.ref.cps, ~self.ref.live, self.ref.ident)
        self.ref.take_mark()
        self.hmark = self.host.mark()
        tail = codepoints(5000, 9)
        fn = mark_edit(self.ref, tail)
        src = self.host.clone()
        v = src.version()
        fn(src)
        upd = src.encode_from(v)
        self.host.apply_update(upd)
        if follow:
            follow(upd)
        A = self.host.arrays()
        assert A.n == n + tail.size and (A.cp[n:] == tail).all()
        self.ref.append(tail, (A.lamport[n:].astype(np.uint64) << np.uint64(16))
                        | A.agent[n:].astype(np.uint64))
