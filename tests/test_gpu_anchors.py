"""Anchors on a device replica (crdt_hip_replica_anchors_at / _at_bytes / _resolve, anchor.hip).

Parity throughout: Replica.*_raw equals OpLog.*_raw byte for byte on a host log that holds the same
items slot for slot, and both equal the plain Python restatement over the CPU oracle's document
order (anchor_util.Ref); exact integers, no tolerance.  The kernels count per tile of 4,096 ranks
and give each anchor a wave that walks 64 ranks a step, so besides the ~300-item typed log the
shapes are the smallest that cross those: rank counts of 4095, 4096, 4097, 8192 and 8193 with dead
stretches over the tile edge, whole dead tiles, and batches around 64 and 256 anchors.
"""
import random

import numpy as np
import pytest

import anchor_util as au
import crdt_hip
import patch_util as pu
from anchor_util import EINVAL, ERANGE
from crdt_hip import AFTER, BEFORE, DEAD, EDGE, LIVE, UNKNOWN
from edit_util import KINDS, text_of

pytestmark = pytest.mark.gpu

TILE = 4096


@pytest.fixture
def pair(ctx, oracle):
    made = []

    def make(log, fugue, agent=0):
        p = au.Pair(ctx, oracle, log, fugue, agent)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


def ident_of(arrs, slot: int) -> int:
    return (int(arrs.lamport[slot - 1]) << 16) | int(arrs.agent[slot - 1])


@pytest.mark.parametrize("kind", KINDS)
def test_typed_log_every_gap(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(pu.base_log(fugue), fugue)
    ref = t.ref()
    items = t.host.arrays().n
    for in_bytes in (False, True):
        pos, bias = au.all_gaps(ref, in_bytes)
        anchors = t.at(ref, pos, bias, in_bytes)
        s = ctx.anchor_stats()
        assert (s["anchors"], s["unknown"], s["ranks"]) == (len(pos), 0, items) and s["device_ns"] > 0
        back = t.resolve(ref, anchors)
        assert back["pos_bytes" if in_bytes else "pos"].tolist() == pos
        s = ctx.anchor_stats()
        assert (s["anchors"], s["unknown"], s["ranks"]) == (len(pos), 0, items)
    # every item held, tombstones included, under both biases
    arrs = t.host.arrays()
    every = [(ident_of(arrs, s), b) for s in range(1, items + 1) for b in (AFTER, BEFORE)]
    got = t.resolve(ref, every)
    assert DEAD in got["state"].tolist()
    assert t.rep.anchors_at([0, 3]) == t.host.anchors_at([0, 3])
    assert t.rep.resolve_anchors(every[:5]) == t.host.resolve_anchors(every[:5])
    assert t.rep.anchors_at_bytes([0], BEFORE) == t.host.anchors_at_bytes([0], BEFORE)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_and_one_item(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(pu.new_log(fugue), fugue)
    ref = t.ref()
    for in_bytes in (False, True):
        a = t.at(ref, [0, 0], [AFTER, BEFORE], in_bytes)
        assert a["id"].tolist() == [EDGE, EDGE]
    got = t.resolve(ref, [(EDGE, AFTER), (EDGE, BEFORE), (9 << 16, BEFORE)])
    assert got["state"].tolist() == [LIVE, LIVE, UNKNOWN]
    assert ctx.anchor_stats()["unknown"] == 1 and ctx.anchor_stats()["ranks"] == 0
    out = au.raw_anchors([(3, 1)])
    au.fails(lambda o: t.rep.anchors_at_raw([1], AFTER, out=o), ERANGE, out)
    t.edit([(0, 0, "€")])                               # one item, of three bytes
    ref = t.ref()
    a = t.at(ref, [0, 0, 1, 1], [AFTER, BEFORE, AFTER, BEFORE])
    assert t.at(ref, [0, 0, 3, 3], [AFTER, BEFORE, AFTER, BEFORE], True).tobytes() == a.tobytes()
    assert t.resolve(ref, a)["pos_bytes"].tolist() == [0, 0, 3, 3]
    for p in (1, 2):
        au.fails(lambda o: t.rep.anchors_at_bytes_raw([p], AFTER, out=o), EINVAL, out)
    t.edit([(0, 1, "")])                                # and that one item dead
    ref = t.ref()
    assert t.resolve(ref, a)["state"].tolist() == [LIVE, DEAD, DEAD, LIVE]


def chain_log(fugue: bool, n: int, dead_ranges, seed: int, width4_at=(), alive_at=()) -> crdt_hip.OpLog:
    """A log of n items typed in one piece (rank k = item k), cut to n through LogArrays, with
    about 20 % of its items tombstoned at random and every rank of `dead_ranges` (first, last)
    tombstoned; the ranks of `width4_at` hold a visible 4-byte codepoint, those of `alive_at` a
    visible item."""
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
    for k in (*width4_at, *alive_at):
        deleted[k - 1] = 0
    cut = crdt_hip.LogArrays(A.parent[:n], A.lamport[:n], A.agent[:n], deleted, A.cp[:n],
                             side=A.side[:n] if fugue else None)
    log = pu.new_log(fugue)
    assert log.join(cut) == (n, 0)
    return log


def edge_positions(ref: au.Ref, rng: random.Random) -> list:
    """Gaps next to the first and last visible item of every tile, the ends, and a random few."""
    pos = {0, 1, ref.len - 1, ref.len}
    rank_vis = {s: v + 1 for v, s in enumerate(ref.vis)}   # (rank k = item k) -> visible rank
    for edge in range(TILE, len(ref.order) + 1, TILE):
        below = [k for k in range(edge - 1, 0, -1) if k in rank_vis][:1]
        above = [k for k in range(edge, len(ref.order) + 1) if k in rank_vis][:1]
        for k in below + above:
            pos |= {rank_vis[k] - 1, rank_vis[k]}
    pos |= {rng.randint(0, ref.len) for _ in range(150)}
    return sorted(p for p in pos if 0 <= p <= ref.len)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ranks", [4095, 4096, 4097, 8192, 8193])
def test_tile_edges(pair, ctx, kind, ranks):
    fugue = kind == "fugue"
    n = ranks - 1
    # a dead stretch that spans rank 4096 where the log reaches it
    t = pair(chain_log(fugue, n, [(min(4090, n - 3), min(4100, n - 1))], ranks), fugue)
    ref = t.ref()
    assert ref.order == list(range(1, n + 1))
    rng = random.Random(ranks)
    gaps = edge_positions(ref, rng)
    arrs = t.host.arrays()
    for in_bytes in (False, True):
        pos = [ref.ends[p] for p in gaps] if in_bytes else gaps
        pos, bias = pos + pos, [AFTER] * len(pos) + [BEFORE] * len(pos)
        anchors = t.at(ref, pos, bias, in_bytes)
        back = t.resolve(ref, anchors)
        assert back["pos_bytes" if in_bytes else "pos"].tolist() == pos
    assert ctx.anchor_stats()["ranks"] == n
    # anchors on every item around the tile edges, the tombstones at ranks 4095 and 4096 included
    near = [s for s in range(1, n + 1) if min(s % TILE, TILE - s % TILE) <= 70]
    if n > 4100:
        assert arrs.deleted[4094] and arrs.deleted[4095]
    got = t.resolve(ref, [(ident_of(arrs, s), b) for s in near for b in (AFTER, BEFORE)])
    assert {LIVE, DEAD} <= set(got["state"].tolist())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ranks", [4097, 8193])
def test_chunk_edges(pair, kind, ranks):
    """A walk that loads a tile in chunks of 16 steps has an edge every 1,024 ranks inside a tile.
    k_anchor_create walks step by step today (the chunked view_seek is what text windows use): this
    guards its switch to view_seek.  Positions whose item lies one rank below, at and one rank above each such edge of tiles 0 and 1,
    under both biases, in codepoints and in bytes, round-tripped through resolve; ranks 1,024 and
    1,025 hold visible 4-byte codepoints, so the offsets one to three bytes inside them are EINVAL.
    A second replica has ranks 1,020..1,030 of each tile dead: the item a position there names is
    the first one past the edge."""
    fugue = kind == "fugue"
    n = ranks - 1
    named = [k for t in (0, 1) for c in (1024, 2048, 3072) for d in (-1, 0, 1)
             for k in [t * TILE + c + d] if k <= n]
    wide = [k for k in (1024, 1025, TILE + 1024, TILE + 1025) if k <= n]
    stretch = [(t * TILE + 1020, t * TILE + 1030) for t in (0, 1) if t * TILE + 1030 <= n]
    out = au.raw_anchors([(3, 1)])
    for dead, width4, alive in (([], wide, named), (stretch, (), ())):
        t = pair(chain_log(fugue, n, dead, ranks + 1, width4_at=width4, alive_at=alive), fugue)
        ref = t.ref()
        assert ref.order == list(range(1, n + 1))
        rank_vis = {s: v + 1 for v, s in enumerate(ref.vis)}   # (rank k = item k) -> visible rank
        assert all(k in rank_vis for k in alive) and not any(
            k in rank_vis for lo, hi in dead for k in range(lo, hi + 1))
        # the named ranks, or with a dead stretch over them the nearest visible item on either side
        items = {k for k in named if k in rank_vis}
        for lo, hi in dead:
            items |= {max(k for k in rank_vis if k < lo), min(k for k in rank_vis if k > hi)}
        gaps = sorted({g for k in items for g in (rank_vis[k] - 1, rank_vis[k])})
        for in_bytes in (False, True):
            pos = [ref.ends[p] for p in gaps] if in_bytes else gaps
            pos, bias = pos + pos, [AFTER] * len(pos) + [BEFORE] * len(pos)
            back = t.resolve(ref, t.at(ref, pos, bias, in_bytes))
            assert back["pos_bytes" if in_bytes else "pos"].tolist() == pos
        for k in width4:
            for inside in (1, 2, 3):
                p = ref.before[k][1] + inside
                for b in (AFTER, BEFORE):
                    for obj in (t.rep, t.host):
                        au.fails(lambda o: obj.anchors_at_bytes_raw([p], b, out=o), EINVAL, out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dead", [(1, 4100), (4090, 8191), (2, 8190)])
def test_dead_tiles(pair, kind, dead):
    """Targets in a tile with no visible item at all before them: tile 0 wholly dead, tile 1 wholly
    dead (the target then lies in tile 2, which holds one rank), and everything dead but the first
    and the last two items."""
    fugue = kind == "fugue"
    n = 8192
    alive = {1: (n - 1, n), 4090: (1, n), 2: (1, n - 1, n)}[dead[0]]   # visible 4-byte codepoints
    t = pair(chain_log(fugue, n, [dead], 7, width4_at=alive), fugue)
    ref = t.ref()
    gaps = sorted({0, 1, 2, ref.len // 2, ref.len - 2, ref.len - 1, ref.len} & set(range(ref.len + 1)))
    arrs = t.host.arrays()
    for in_bytes in (False, True):
        pos = [ref.ends[p] for p in gaps] if in_bytes else gaps
        pos, bias = pos + pos, [AFTER] * len(pos) + [BEFORE] * len(pos)
        back = t.resolve(ref, t.at(ref, pos, bias, in_bytes))
        assert back["pos_bytes" if in_bytes else "pos"].tolist() == pos
    t.resolve(ref, [(ident_of(arrs, s), b) for s in (1, 2, 4095, 4096, 4097, 8190, 8191, 8192)
                    for b in (AFTER, BEFORE)])
    out = au.raw_anchors([(3, 1)])
    au.fails(lambda o: t.rep.anchors_at_bytes_raw([ref.nbytes - 2], BEFORE, out=o), EINVAL, out)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_sizes(pair, ctx, kind):
    fugue = kind == "fugue"
    t = pair(pu.base_log(fugue), fugue)
    ref = t.ref()
    arrs = t.host.arrays()
    rng = random.Random(40)
    held = [ident_of(arrs, s) for s in range(1, arrs.n + 1)]
    dead = [ident_of(arrs, s) for s in range(1, arrs.n + 1) if arrs.deleted[s - 1]]
    absent = [(l << 16) | 77 for l in range(1, 40)]     # an agent the log has never seen
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 3000):
        pos = [rng.randint(0, ref.len) for _ in range(m)]   # unsorted, repeated
        bias = [rng.choice([AFTER, BEFORE]) for _ in range(m)]
        made = t.at(ref, pos, bias)
        assert t.resolve(ref, made)["pos"].tolist() == pos
        bpos = [ref.ends[p] for p in pos]
        assert t.at(ref, bpos, bias, True).tobytes() == made.tobytes()
        mixed = [(rng.choice(rng.choice([held, dead, absent, [EDGE]])), rng.choice([AFTER, BEFORE]))
                 for _ in range(m)]
        got = t.resolve(ref, mixed)
        unknown = sum(1 for i, _ in mixed if i in absent)
        assert got["state"].tolist().count(UNKNOWN) == unknown
        if m:
            s = ctx.anchor_stats()
            assert (s["anchors"], s["unknown"], s["ranks"]) == (m, unknown, arrs.n)
        if m >= 255:
            assert {LIVE, DEAD, UNKNOWN} == set(got["state"].tolist())
    # one identity many times over, and a batch that is nothing but unknown
    t.resolve(ref, [(held[5], AFTER)] * 300 + [(held[5], BEFORE)] * 300)
    t.resolve(ref, [(i, AFTER) for i in absent] * 4)
    assert ctx.anchor_stats()["unknown"] == 4 * len(absent)


@pytest.mark.parametrize("kind", KINDS)
def test_after_each_way_the_order_changes(pair, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    fk = pu.jf.fork if fugue else pu.ju.fork
    t = pair(base, fugue, agent=1)
    ref = t.ref()
    kept = t.at(ref, *au.all_gaps(ref))
    t.rep.merge_inc()
    steps = [
        lambda: t.edit([(17, 0, "k")]),                                  # fast-path merge_inc
        lambda: t.join(fk(base, 2, 51, 60)),                             # full rebuild
        lambda: t.edit([(3, 1, "é")]),
        lambda: t.apply_diff(fk(base, 3, 52, 60)),                       # full rebuild
        lambda: t.edit([(40, 2, text_of(random.Random(3), 5000))]),      # more than a fast path takes
        lambda: t.edit([(2500, 0, "z")]),
    ]
    for step in steps:
        step()
        ref = t.ref()
        got = t.resolve(ref, kept)                      # anchors made before the change
        assert UNKNOWN not in got["state"].tolist()
        pos = sorted({0, 1, 17, 18, ref.len // 2, ref.len - 1, ref.len})
        fresh = t.at(ref, pos + pos, [AFTER] * len(pos) + [BEFORE] * len(pos))
        assert t.resolve(ref, fresh)["pos"].tolist() == pos + pos
        kept = np.concatenate([kept, fresh])
    if fugue:
        assert t.host.arrays().side.any()               # left children are among the items
    assert t.rep.merge_inc()[:2] == (ref.len, ref.nbytes)


@pytest.mark.parametrize("kind", KINDS)
def test_cross_peer(ctx, oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    fk = pu.jf.fork if fugue else pu.ju.fork
    a, b = crdt_hip.Replica(ctx, fk(base, 1, 61, 70)), crdt_hip.Replica(ctx, fk(base, 2, 62, 50))
    try:
        ra = au.Ref(oracle, pu.replica_arrays(a, fugue))
        anchors = au.check_at(a, ra, *au.all_gaps(ra))
        before = au.check_resolve(b, au.Ref(oracle, pu.replica_arrays(b, fugue)), anchors)
        assert UNKNOWN in before["state"].tolist() and LIVE in before["state"].tolist()
        b.apply_diff(a.encode_diff(b.state_vector()))
        after = au.check_resolve(b, au.Ref(oracle, pu.replica_arrays(b, fugue)), anchors)
        assert UNKNOWN not in after["state"].tolist()
        # once both hold the same items, in different slots, they resolve alike
        a.apply_diff(b.encode_diff(a.state_vector()))
        assert a.encode_diff([]) != b.encode_diff([])
        mine = au.check_resolve(a, au.Ref(oracle, pu.replica_arrays(a, fugue)), anchors)
        assert mine.tobytes() == after.tobytes()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_errors_on_the_device(pair, ctx, kind):
    fugue = kind == "fugue"
    # ranks 4095 and 4096 hold visible 4-byte codepoints
    t = pair(chain_log(fugue, 4200, [], 3, width4_at=(4095, 4096)), fugue)
    ref = t.ref()
    n, nb = ref.len, ref.nbytes
    snap = (t.rep.encode_diff([]), t.rep.info())
    out = au.raw_anchors([(1, 1)] * 3)
    pout = au.raw_positions([(5, 5, 1)] * 3)
    good = t.host.anchors_at_raw([0, n, 2], [0, 1, 1])
    e4095 = ref.before[4095][1]                         # the bytes before the item of rank 4095
    cases = [
        (lambda o, r: o.anchors_at_raw([0, n + 1, 2], AFTER, out=r), ERANGE, out),
        (lambda o, r: o.anchors_at_raw([0, n, 2], [0, 2, 1], out=r), EINVAL, out),
        (lambda o, r: o.anchors_at_raw([n + 1, n, 2], [0, 2, 1], out=r), ERANGE, out),
        (lambda o, r: o.anchors_at_bytes_raw([0, nb + 1, 2], BEFORE, out=r), ERANGE, out),
        (lambda o, r: o.anchors_at_bytes_raw([0, nb, 2], [0, 1, 2], out=r), EINVAL, out),
    ]
    for inside in (e4095 + 1, e4095 + 3, e4095 + 5, e4095 + 7):   # in rank 4095's, in rank 4096's
        for b in (AFTER, BEFORE):
            cases.append((lambda o, r, p=inside, b=b: o.anchors_at_bytes_raw([0, p, nb], b, out=r),
                          EINVAL, out))
    for bad in ((1 << 48, AFTER, 0), (good[2]["id"], 2, 0), (good[2]["id"], BEFORE, 1)):
        arr = good.copy()
        arr[1] = bad
        cases.append((lambda o, r, arr=arr: o.resolve_anchors_raw(arr, out=r), EINVAL, pout))
    for call, code, res in cases:
        au.fails(lambda r: call(t.rep, r), code, res)
        au.fails(lambda r: call(t.host, r), code, res)  # the host twin: the same code
        assert (t.rep.encode_diff([]), t.rep.info()) == snap
    for p in (e4095, e4095 + 4, e4095 + 8):             # the boundaries around them are fine
        t.at(ref, [p, p], [AFTER, BEFORE], True)
    other = crdt_hip.Context(ctx.device)                # a replica of another context
    try:
        L = crdt_hip.lib()
        pos = np.zeros(1, np.uint64)
        for call in (lambda: L.crdt_hip_replica_anchors_at(other._h, t.rep._h, pos.ctypes.data, None,
                                                           1, out.ctypes.data),
                     lambda: L.crdt_hip_replica_anchors_at_bytes(other._h, t.rep._h, pos.ctypes.data,
                                                                 None, 1, out.ctypes.data),
                     lambda: L.crdt_hip_replica_anchors_resolve(other._h, t.rep._h, good.ctypes.data,
                                                                3, pout.ctypes.data)):
            before = (out.tobytes(), pout.tobytes())
            assert call() == EINVAL
            assert (out.tobytes(), pout.tobytes()) == before
    finally:
        other.close()
    assert (t.rep.encode_diff([]), t.rep.info()) == snap
    assert t.rep.anchors_at([]) == [] and t.rep.resolve_anchors([]) == []


def test_adapters():
    text = "héllo wörld, €uro 😀 and more"
    for cls, unit in ((crdt_hip.HipDownstream, len), (crdt_hip.HipDownstreamBytes,
                                                      lambda s: len(s.encode("utf-8")))):
        d = cls.from_str(text)
        try:
            for cut in (0, 1, 7, 19, len(text)):
                p = unit(text[:cut])
                for b in (AFTER, BEFORE):
                    assert d.resolve(d.anchor_at(p, b)) == p
            cur = d.anchor_at(unit(text[:7]), BEFORE)
            d.insert(0, "€€")                           # typing before the cursor moves it
            assert d.resolve(cur) == unit("€€" + text[:7])
            assert d.resolve_many([cur, (EDGE, AFTER), (5 << 16 | 9, AFTER)]) == \
                [unit("€€" + text[:7]), 0, None]
        finally:
            d.replica.close()
    # two peers keep each other's cursor through sync_from
    a = crdt_hip.HipDownstream.from_str(text)
    b = a.clone()
    a.replica.set_agent(1)
    b.replica.set_agent(2)
    try:
        a.insert(5, " big")
        b.insert(0, ">> ")
        ca, cb = a.anchor_at(9, AFTER), b.anchor_at(3, BEFORE)   # after "big", before "h"
        assert b.resolve(ca) is None and a.resolve(cb) == 0      # (b's cursor names a base item)
        a.sync_from(b)
        b.sync_from(a)
        assert a.text() == b.text() == ">> héllo big wörld, €uro 😀 and more"
        assert a.resolve_many([ca, cb]) == b.resolve_many([ca, cb]) == [12, 3]
    finally:
        a.replica.close()
        b.replica.close()
