"""Shapes and edge arithmetic for the per-document LDS level 1 (k_doctree); no GPU needed.

Three things live here:

* generators of documents with an exact run count (`bush`, `ladder`, `comb64`), multi-agent keys
  and lamport ties, plus the text-heavy shapes of the text-size edges;
* `predicted_runs`: the run-head rule of k_heads / head_word (engine.hip) restated in numpy;
* `lds_bytes` / `plan`: doctree_lds_bytes and the predicates of Engine::plan_level1 transcribed,
  used only to compute where the edges are (tests/test_doctree_shapes.py pins the constants).
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import crdt_hip

# ---- constants of engine.hip the transcription depends on (pinned by test_doctree_shapes.py) ----
KDOC_LDS = 163840 - 1024   # kDocLds
KDOC_J = 17                # CRDT_DOC_J
KDOC_J_NARROW = 12         # kDocJNarrow
KDOC_LOG2S = 2             # CRDT_DOC_LOG2S
KDOC_TILES = 1024          # kDocTiles
KDOC_THREADS = 1024        # kDocThreads
SCAN_TILE = 4096           # kScanTile: no run crosses a tile
DOC_ALIGN = 64             # 1 << kDocAlignLog2: documents start on 64-slot boundaries
TEXT_LDS_LIMIT = 1 << 18   # plan_level1: max_doc_text < 2^18 on the LDS level 1

GROUP_SIZES = (1, 2, 3, 5, 8, 9, 17, 40, 64)
MAX_GROUP = 64


# ---- doctree_lds_bytes and its parts (engine.hip: doctree_ch_bytes .. doctree_lds_bytes) --------
def _ch_bytes(rcap: int) -> int:
    return (2 * rcap + 15) & ~15


def _defer_cap(rcap: int) -> int:
    return rcap // 2 + 8


def _gl_bytes(rcap: int, scap: int) -> int:
    return (max(2 * _defer_cap(rcap), 4 * scap) + 15) & ~15


def _key_off(rcap: int, scap: int, k32: bool) -> int:
    return ((2 if k32 else 4) * rcap + _ch_bytes(rcap) + 15) & ~15


def lds_bytes(rcap: int, scap: int, k32: bool) -> int:
    return _key_off(rcap, scap, k32) + (4 if k32 else 8) * rcap + _gl_bytes(rcap, scap)


def caps(rmax: int) -> tuple:
    """(rcap, scap) as Engine::plan_level1 rounds them."""
    rcap = (rmax + 2 + 7) & ~7
    scap = (((rmax + (1 << KDOC_LOG2S) - 1) >> KDOC_LOG2S) + 8) & ~7
    return rcap, scap


Plan = collections.namedtuple("Plan", "wide j lds1 fuse stile_text dyn_bytes unclamped")


def plan(rmax: int, max_doc_text: int, max_doc_slots: int, k32: bool = False,
         order: bool = False) -> Plan:
    """Engine::plan_level1 under default parameters (and doctree_k32 = k32): which instance a
    wave takes (wide, j = runs per thread), whether it takes the LDS level 1 (lds1), whether
    the text is fused (fuse) and staged from the tile segments (stile_text), the dynamic LDS
    of the launch, and `unclamped`: the launch got all the LDS the text formula asks for, so
    phase C cannot refuse a document (fused-and-fits)."""
    rcap, scap = caps(rmax)
    dbytes = lds_bytes(rcap, scap, False)
    wide = rmax > KDOC_J_NARROW * KDOC_THREADS or dbytes > KDOC_LDS or k32
    if wide:
        dbytes = lds_bytes(rcap, scap, True)
    lds1 = (rmax <= KDOC_J * KDOC_THREADS and dbytes <= KDOC_LDS
            and max_doc_text < TEXT_LDS_LIMIT)
    fuse = lds1 and not order and max_doc_text + 512 <= KDOC_LDS
    stile = fuse and max_doc_slots // SCAN_TILE + 2 <= KDOC_TILES
    want = (max_doc_text * 5 // 4 + 4 * rmax + 512
            + 44 * (max_doc_slots // SCAN_TILE + 3) + 15) & ~15
    dyn = min(KDOC_LDS, max(dbytes, want)) if fuse else dbytes
    j = KDOC_J if wide and rmax > KDOC_J_NARROW * KDOC_THREADS else KDOC_J_NARROW
    return Plan(wide, j, lds1, fuse, stile, dyn, fuse and want <= KDOC_LDS)


def doc_slots(n_items: int) -> int:
    """Slots of a document of n items: its start node and items, padded to 64 (Engine::plan)."""
    return (n_items + 1 + DOC_ALIGN - 1) // DOC_ALIGN * DOC_ALIGN


@functools.lru_cache(maxsize=None)
def narrow_max() -> int:
    """The largest rmax that stays on k_doctree (64-bit keys) under default parameters."""
    return max(r for r in range(1, KDOC_J * KDOC_THREADS + 2) if not plan(r, 0, 0).wide)


@functools.lru_cache(maxsize=None)
def lds_max(k32: bool = False) -> int:
    """The largest rmax that stays on the LDS level 1."""
    return max(r for r in range(1, KDOC_J * KDOC_THREADS + 4096) if plan(r, 0, 0, k32).lds1)


def fuse_max_text() -> int:
    """The largest document text that is fused (max_doc_text + 512 <= kDocLds)."""
    return KDOC_LDS - 512


def unclamped_max_text(rmax: int, max_doc_slots: int, k32: bool = False) -> int:
    """The largest document text on which the dyn_bytes clamp does not bite."""
    lo, hi = 0, KDOC_LDS
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if plan(rmax, mid, max_doc_slots, k32).unclamped:
            lo = mid
        else:
            hi = mid - 1
    return lo


# ---- the run-head rule --------------------------------------------------------------------------
def predicted_runs(parent, base_slot: int = 0) -> int:
    """Runs of an all-visible RGA document whose start node sits at wave slot `base_slot`
    (k_heads / head_word, engine.hip): the document start, plus every item g (slot g of the
    document) whose parent is not slot g - 1, or whose slot g - 1 has a child that is not
    slot g (its jump bit), or that is a tile's first slot."""
    parent = np.asarray(parent, dtype=np.int64)
    n = parent.size
    g = np.arange(1, n + 1, dtype=np.int64)
    nonnext = np.zeros(n + 1, bool)
    nonnext[parent[g != parent + 1]] = True
    head = (parent != g - 1) | nonnext[g - 1] | ((base_slot + g) % SCAN_TILE == 0)
    return 1 + int(head.sum())


def group_sizes(parent) -> np.ndarray:
    """Children per node (index 0: the document start)."""
    parent = np.asarray(parent, dtype=np.int64)
    return np.bincount(parent, minlength=parent.size + 1)


def tie_share(log) -> tuple:
    """(sibling groups of two or more, those of them in which two siblings share a lamport and
    differ only in the agent)."""
    par = log.parent.astype(np.int64)
    order = np.lexsort((log.agent, log.lamport, par))
    p, lam = par[order], log.lamport[order]
    tied = (p[1:] == p[:-1]) & (lam[1:] == lam[:-1])
    sizes = np.bincount(par)
    return int((sizes >= 2).sum()), int(np.unique(p[1:][tied]).size)


# ---- keys, text ---------------------------------------------------------------------------------
def _keys(parent: np.ndarray, rng, agents: int) -> tuple:
    """(lamport, agent) per item.  Sibling groups are taken in the order of their parents' ids
    (ids are causal: a parent comes before its children), each gets a fresh block of lamports
    dealt to its members in a seeded order, so a child's lamport exceeds its parent's and the
    sibling order is unrelated to the id order.  agent = f(item) % agents with f = a per-group
    base plus or minus the member's rank, so neighbours in a group differ in the agent whenever
    agents >= 2; in every third group of two or more, two such neighbours share a lamport."""
    n = parent.size
    par = parent.astype(np.int64)
    order = np.argsort(par, kind="stable")
    sp = par[order]
    first = np.r_[True, sp[1:] != sp[:-1]]
    start = np.flatnonzero(first)                       # group g: order[start[g] : start[g + 1]]
    gidx = np.cumsum(first) - 1
    size = np.diff(np.r_[start, n])
    rank = np.arange(n) - start[gidx]
    shuffled = np.lexsort((rng.random(n), gidx))        # a seeded order inside every group
    lam = np.zeros(n, np.int64)
    lam[order[shuffled]] = 1 + np.arange(n)             # block of group g: 1 + start[g] ..
    base = rng.integers(MAX_GROUP + 1, 1 << 16, start.size)
    sgn = np.where(rng.random(start.size) < 0.5, 1, -1)
    agent = np.zeros(n, np.int64)
    agent[order] = (base[gidx] + sgn[gidx] * rank) % agents
    if agents >= 2:
        multi = np.flatnonzero(size >= 2)
        tie = multi[::3]
        r = (rng.random(tie.size) * (size[tie] - 1)).astype(np.int64)
        u, v = order[start[tie] + r], order[start[tie] + r + 1]
        lam[v] = lam[u]
    return lam.astype(np.uint32), agent.astype(np.uint16)


_CP_BASE = (0x61, 0x3B1, 0x4E00, 0x1F600)  # a codepoint of each UTF-8 width (+ 0..23)


def _codepoints(widths: np.ndarray, rng) -> np.ndarray:
    return (np.asarray(_CP_BASE, np.uint32)[widths - 1]
            + rng.integers(0, 24, widths.size).astype(np.uint32))


def _sides(parent: np.ndarray, rng) -> np.ndarray:
    """Fugue variant: about a third of the items that do not continue a typed run (and do not
    hang off the document start) are left children."""
    g = np.arange(1, parent.size + 1)
    return ((parent > 0) & (parent != g - 1) & (rng.random(parent.size) < 0.35)).astype(np.uint8)


def _top_up(parent: list, need: int, rng) -> None:
    """`need` more runs: leaf items on items that already have a non-next child and fewer than
    64 children.  Each such leaf is a run head and changes no other item's head bit."""
    if need <= 0:
        return
    par = np.asarray(parent, dtype=np.int64)
    g = np.arange(1, par.size + 1)
    nkids = np.bincount(par, minlength=par.size + 1)
    nonnext = np.zeros(par.size + 1, bool)
    nonnext[par[g != par + 1]] = True
    cand = np.flatnonzero(nonnext & (nkids < MAX_GROUP))
    room = int((MAX_GROUP - nkids[cand]).sum())
    assert room >= need, "no item can take another leaf"
    cand = cand[rng.permutation(cand.size)]
    k = 0
    while need:
        p = int(cand[k % cand.size])
        k += 1
        if nkids[p] < MAX_GROUP:
            nkids[p] += 1
            parent.append(p)
            need -= 1


def _finish(parent: list, R: int, seed: int, agents: int, fugue: bool):
    rng = np.random.default_rng([seed, R, agents, 0xD0C])
    while predicted_runs(parent) > R:   # (a typed run cut by a tile: drop trailing leaves)
        parent.pop()
    _top_up(parent, R - predicted_runs(parent), rng)
    par = np.asarray(parent, np.uint32)
    assert predicted_runs(par) == R and group_sizes(par).max() <= MAX_GROUP
    lam, agent = _keys(par, rng, agents)
    widths = rng.choice(np.arange(1, 5), par.size, p=(0.4, 0.3, 0.2, 0.1))
    cp = _codepoints(widths, rng)
    assert int(widths.sum()) < 100_000  # these documents fuse
    return crdt_hip.LogArrays(par, lam, agent, np.zeros(par.size, np.uint8), cp,
                              side=_sides(par, rng) if fugue else None)


def _chain(R: int) -> list:
    """R = 2 exists only as a typed chain cut by a tile: with every item visible, a branch makes
    two heads at once, so the one head besides the document start is slot 4096."""
    assert R == 2
    return list(range(SCAN_TILE))


def _bush_parents(R: int, rng, mean_len: float) -> list:
    """Breadth-first: every run is a head and `len - 1` typed items in the slots after it, its
    children hang off its last item; group sizes drawn from GROUP_SIZES."""
    parent: list = []
    queue = collections.deque([0])   # last items of runs that may get children
    heads = R - 1
    while heads > 0 and queue:
        p = queue.popleft()
        if p and rng.random() < 0.35:   # a leaf run
            if not queue:
                queue.append(p)
            continue
        sizes = GROUP_SIZES[1:] if p == 0 else GROUP_SIZES
        k = min(int(rng.choice(sizes)), heads)
        heads -= k
        for _ in range(k):
            parent.append(p)
            extra = int(rng.integers(0, int(2 * (mean_len - 1)) + 1))
            for _ in range(extra):
                parent.append(len(parent))
            queue.append(len(parent))
    return parent


def bush(R: int, seed: int, agents: int, fugue: bool = False, mean_len: float = 2.0):
    """A tree of R runs whose sibling-group sizes are drawn from GROUP_SIZES (every sort path of
    the kernel, none above 64); runs are one to a few typed items long."""
    rng = np.random.default_rng([seed, R, 0xB05])
    parent = _chain(R) if R == 2 else _bush_parents(R, rng, mean_len)
    return _finish(parent, R, seed, agents, fugue)


def ladder(R: int, seed: int, agents: int, fugue: bool = False):
    """A spine: item 2k + 1 is a child of item 2k - 1 and item 2k a leaf child of item 2k - 1.
    No item contracts; the run tree is about R / 2 deep and every group has two members."""
    if R == 2:
        parent = _chain(R)
    else:
        n = R if R % 2 else R - 1
        parent = [0] + [2 * ((g - 2) // 2) + 1 for g in range(2, n + 1)]
    return _finish(parent, R, seed, agents, fugue)


def comb64(R: int, seed: int, agents: int, fugue: bool = False):
    """Every internal node has exactly 64 children (the last one takes what is left of R)."""
    if R == 2:
        parent = _chain(R)
    else:
        parent, node, left = [], 0, R - 1
        while left:
            k = min(MAX_GROUP, left)
            parent += [node] * k
            left -= k
            node += 1
    return _finish(parent, R, seed, agents, fugue)


SHAPES = {"bush": bush, "ladder": ladder, "comb64": comb64}


def to_anchor(arrs):
    from oracle_bind import AnchorLog
    a = AnchorLog(arrs.n)
    for f in ("parent", "lamport", "agent", "deleted", "cp"):
        getattr(a, f)[: arrs.n] = getattr(arrs, f)
    if arrs.side is not None:
        a.side[: arrs.n] = arrs.side
    return a


def fugue_order(arrs) -> np.ndarray:
    """Fugue in-order (left children descending, the item, right children descending) with an
    explicit stack: a plain restatement for trees too deep to recurse on."""
    n = arrs.n
    kids = [[[], []] for _ in range(n + 1)]
    key = list(zip(arrs.lamport.tolist(), arrs.agent.tolist()))
    for i, (p, s) in enumerate(zip(arrs.parent.tolist(), arrs.side.tolist()), 1):
        kids[p][s].append(i)
    out, stack = [], [(0, False)]
    while stack:
        v, emitted = stack.pop()
        if emitted:
            out.append(v)
            continue
        # popped in reverse: left children (greatest first), then v, then right children
        for c in sorted(kids[v][0], key=lambda i: key[i - 1]):
            stack.append((c, False))
        if v:
            stack.append((v, True))
        for c in sorted(kids[v][1], key=lambda i: key[i - 1]):
            stack.append((c, False))
    return np.asarray(out, np.uint32)


# ---- text-heavy shapes (text-size edges) --------------------------------------------------------
def _set_text(parent: np.ndarray, T: int, rng, del_frac: float):
    """(deleted, cp): about del_frac of the items tombstoned, never a run head or a tile's first
    slot (so no run is dead and predicted_runs holds), and the visible items' UTF-8 widths chosen
    so that the visible bytes are exactly T."""
    n = parent.size
    g = np.arange(1, n + 1)
    nonnext = np.zeros(n + 1, bool)
    nonnext[parent[g != parent.astype(np.int64) + 1]] = True
    head = (parent != g - 1) | nonnext[g - 1] | (g % SCAN_TILE == 0) | (g == 1)
    deleted = (~head) & (rng.random(n) < del_frac)
    vis = np.flatnonzero(~deleted)
    assert vis.size <= T <= 4 * vis.size, (vis.size, T)
    extra = T - vis.size
    w = np.full(vis.size, 1 + extra // vis.size, np.int64)
    w[rng.permutation(vis.size)[: extra % vis.size]] += 1
    widths = np.ones(n, np.int64)
    widths[vis] = w
    assert int(widths[vis].sum()) == T
    return deleted.astype(np.uint8), _codepoints(widths, rng)


TEXT_BUCKET = 16384


def _bucket(T: int) -> int:
    """The text-heavy shapes size their trees by T rounded up to 16 KiB, so that T and the next
    size up share one tree (run count, slots) and differ in one codepoint's width only."""
    return -(-T // TEXT_BUCKET) * TEXT_BUCKET


def typed_run(T: int, seed: int, del_frac: float = 0.2):
    """One typed run (cut only by the tiles) of mostly 4-byte codepoints: T visible bytes."""
    n = int(_bucket(T) / 3.9 / (1 - del_frac)) + 64
    parent = np.arange(n, dtype=np.uint32)
    deleted, cp = _set_text(parent, T, np.random.default_rng([seed, n, 0x7E]), del_frac)
    lam = np.arange(1, n + 1, dtype=np.uint32)
    return crdt_hip.LogArrays(parent, lam, np.zeros(n, np.uint16), deleted, cp)


def bush_text(T: int, seed: int, R: int = 8000, agents: int = 3, del_frac: float = 0.2):
    """A bush of R runs (before the tiles cut its typed runs) long enough to hold T visible
    bytes, its codepoints scaled so that the visible bytes are exactly T."""
    rng = np.random.default_rng([seed, _bucket(T), 0xB7])
    mean_len = max(2.0, _bucket(T) / 3.0 / (1 - del_frac) / R)
    par = np.asarray(_bush_parents(R, rng, mean_len), np.uint32)
    assert group_sizes(par).max() <= MAX_GROUP
    lam, agent = _keys(par, rng, agents)
    deleted, cp = _set_text(par, T, rng, del_frac)
    return crdt_hip.LogArrays(par, lam, agent, deleted, cp)


def tile_edge_doc(tiles: int, seed: int, visible: int = 50_000, branches: int = 300):
    """One typed chain with a few hundred seeded branches whose slots span `tiles` whole tiles
    (max_doc_slots / 4096 == tiles); `visible` two-byte characters, everything else tombstoned."""
    rng = np.random.default_rng([seed, tiles, 0x71E])
    n = tiles * SCAN_TILE + 100
    assert doc_slots(n) // SCAN_TILE == tiles
    parent = np.arange(n, dtype=np.uint32)
    b = rng.choice(np.arange(2, n), branches, replace=False)
    parent[b] = (rng.random(branches) * b).astype(np.uint32)
    deleted = np.ones(n, np.uint8)
    deleted[rng.choice(n, visible, replace=False)] = 0
    cp = _codepoints(np.full(n, 2, np.int64), rng)
    lam = np.arange(1, n + 1, dtype=np.uint32)
    return crdt_hip.LogArrays(parent, lam, (rng.integers(0, 3, n)).astype(np.uint16), deleted, cp)
