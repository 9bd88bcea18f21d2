"""Level 0's plain-tile list (param plain_tiles, the default): a 4096-slot tile whose every slot is
an item of one document with the previous-slot flag and without a jump bit is the inside of one
typed run.  k_runs gives such a tile one thread (one run row: the forced head at its first slot)
and k_classify_plane leaves it after its first loads when it holds no visible item.  With
plain_tiles 0 every tile takes a workgroup of both kernels.

Every case merges three times per setting (the synchronous merge, the learnt plan, the plan
again), compares the digests and lengths with the oracle's bytes, and the two settings with each
other: equal digests, lengths and run counts.
"""
import numpy as np
import pytest

import crdt_hip
from test_gpu_merge import to_anchor

pytestmark = pytest.mark.gpu

REPLICAS = 8
TILE = 4096
N = 13000  # three whole tiles and a partial one; before a relabelling item k sits in slot k
UNIT = "aé中\U0001f600b߿ࠀ￿"  # 1, 2, 3, 4, 1, 2, 3, 3 bytes


def _typed(n: int, text=None) -> crdt_hip.OpLog:
    """n characters typed in one go: ids 1..n, id k at position k - 1."""
    lg = crdt_hip.OpLog()
    lg.insert(0, text if text is not None else "".join(chr(97 + i % 26) for i in range(n)))
    return lg


def _keep_only(lg: crdt_hip.OpLog, n: int, keep) -> None:
    """Remove ids 1..n of a log made by _typed except `keep`, from the highest gap down."""
    edges = sorted(set(keep)) + [n + 1]
    gaps = [(lo + 1, hi - 1) for lo, hi in zip([0] + edges[:-1], edges) if hi - lo > 1]
    for lo, hi in reversed(gaps):
        lg.remove(lo - 1, hi)
    assert lg.visible_len() == len(set(keep))


def _all_removed() -> crdt_hip.OpLog:
    """13,000 characters typed in one go and all removed: the inner tiles are plain and dead."""
    lg = _typed(N)
    lg.remove(0, N)
    assert lg.visible_len() == 0
    return lg


def _survivors() -> crdt_hip.OpLog:
    """The same log in the multi-byte alphabet with a few survivors inside the second tile (slots
    4096..8191 before a relabelling): a plain tile with visible text, its last slot a 3-byte
    character, its first slot and two others visible too; the third tile stays dead."""
    lg = _typed(N, UNIT * (N // len(UNIT)))
    assert len(UNIT[(2 * TILE - 2) % 8].encode()) == 3 and len(UNIT[(5004 - 1) % 8].encode()) == 4
    _keep_only(lg, N, [TILE, TILE + 100, 5004, 2 * TILE - 1])
    return lg


def _chain(n: int, extra=()) -> crdt_hip.LogArrays:
    """Items 1..n typed in one go by agent 1 (item k: parent k - 1, lamport k), all visible, then
    the items of `extra`, (parent, lamport, agent, codepoint) each."""
    parent = list(range(n)) + [e[0] for e in extra]
    lamport = list(range(1, n + 1)) + [e[1] for e in extra]
    agent = [1] * n + [e[2] for e in extra]
    cp = [97 + k % 26 for k in range(n)] + [e[3] for e in extra]
    return crdt_hip.LogArrays(parent, lamport, agent, [0] * len(parent), cp)


_LOGS = {
    "all_removed": lambda: [_all_removed().arrays()],
    "survivors": lambda: [_survivors().arrays()],
    # the slot before the plain second tile (item 4095) has a second child: typed later (it sorts
    # before the tile's first item), or concurrent with a smaller key (it sorts after the whole
    # chain, which only the tile-first head's own key can tell); and the mirror without one
    "sibling_later": lambda: [_chain(N, [(TILE - 1, N + 1, 1, ord("Z"))])],
    "sibling_smaller_key": lambda: [_chain(N, [(TILE - 1, TILE, 0, ord("Z"))])],
    "no_sibling": lambda: [_chain(N)],
    # not plain: a document start and padding inside a tile (documents of 4,000 + 1 slots, padded
    # to 4,032: every tile from the second on holds a start), two small documents in one tile,
    # and a wave's last, partial tile (13,000 items end in the fourth tile)
    "starts_in_tiles": lambda: [_chain(4000), _chain(4000), _chain(4000), _chain(4000)],
    "small_docs": lambda: [_chain(100), _chain(70), _all_removed().arrays()],
}
_CASES = {}


def _case(name, oracle):
    """The logs of a case and the oracle's digest and length of each, computed once."""
    if name not in _CASES:
        arrs = _LOGS[name]()
        refs = [oracle.merge(to_anchor(a)) for a in arrs]
        _CASES[name] = (arrs, [oracle.tree_digest(r) for r in refs], [len(r) for r in refs])
    return _CASES[name]


def _merge_both(c, b, want_d, want_l, merges=3):
    """The batch merged with plain_tiles 1 and 0, `merges` times each, every merge against the
    oracle; the two settings against each other; returns {setting: stats}."""
    nb = len(want_d)
    out = {}
    try:
        for pt in (1, 0):
            c.set_param("plain_tiles", pt)
            for _ in range(merges):
                d, l, st = b.merge()
                for r in range(b.docs):
                    assert int(d[r]) == want_d[r % nb] and int(l[r]) == want_l[r % nb], (pt, r)
            out[pt] = (list(map(int, d)), list(map(int, l)), st)
    finally:
        c.set_param("plain_tiles", 1)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2]["runs"] == out[1][2]["runs"]
    return {pt: out[pt][2] for pt in out}


@pytest.mark.parametrize("name", ["all_removed", "survivors"])
def test_plain_tiles_rotated_replicas(oracle, name):
    """8 rotated replicas: the tile boundaries fall on different items in each."""
    arrs, want_d, want_l = _case(name, oracle)
    c = crdt_hip.Context(0)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    st = _merge_both(c, b, want_d, want_l)
    # (no new launch: tile scan, k_runs, k_docmax)
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    assert st[0]["stage_launches"]["runs"] == 3 * st[0]["waves"]
    b.close()
    c.close()


@pytest.mark.parametrize("name", list(_LOGS))
def test_plain_tiles_known_boundaries(oracle, name):
    """relabel "none": item k of the first document sits in slot k, so its second and third tiles
    are the plain ones of the typed logs; the second replica starts at another offset in its
    tile.  The text itself against the oracle's for the first replica."""
    arrs, want_d, want_l = _case(name, oracle)
    c = crdt_hip.Context(0)
    b = c.batch(arrs, replicas=2, relabel="none")
    st = _merge_both(c, b, want_d, want_l)
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    b.close()
    want = oracle.merge(to_anchor(arrs[0]))
    try:
        for pt in (1, 0):
            c.set_param("plain_tiles", pt)
            text, dig = c.merge(arrs[0])
            assert text == want and dig == want_d[0], pt
    finally:
        c.set_param("plain_tiles", 1)
    c.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_plain_tiles_waves_and_lanes(oracle, lanes):
    """At least 3 waves, each with its own range of the list, on one lane and on two."""
    arrs, want_d, want_l = _case("survivors", oracle)
    c = crdt_hip.Context(0)
    c.set_param("lanes", lanes)
    c.set_param("max_wave_slots", 1 << 15)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    st = _merge_both(c, b, want_d, want_l)
    assert st[1]["waves"] >= 3 and st[0]["waves"] == st[1]["waves"]
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    b.close()
    c.close()


def test_plain_tiles_raw_soa(oracle):
    """Raw SoA mode rebuilds the list, the bits and the planes inside every merge, which ends the
    plain-tile list's validity: the batch's waves take a workgroup per tile from then on, also
    after raw mode is switched off again."""
    arrs, want_d, want_l = _case("survivors", oracle)
    c = crdt_hip.Context(0)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    d0, l0, st0 = b.merge()
    b.set_raw(True)
    st = _merge_both(c, b, want_d, want_l)
    assert st[1]["stage_launches"]["encode"] > 0
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    b.set_raw(False)
    d, l, st2 = b.merge()
    assert np.array_equal(d, d0) and np.array_equal(l, l0) and st2["runs"] == st0["runs"]
    b.close()
    c.close()


def test_plain_tile_that_stops_being_plain(oracle):
    """A replica that rebuilds its list and bits in every merge (nsq_list 2) keeps no plain-tile
    list, so nothing of one can go stale: after an update that inserts after an item inside a
    formerly plain tile (and one that tombstones most of another) the merge sees both."""
    host = _typed(N)
    c = crdt_hip.Context(0)
    try:
        c.set_param("nsq_list", 2)
        for pt in (1, 0):
            c.set_param("plain_tiles", pt)
            h = host.clone()
            r = crdt_hip.Replica(c)
            r.apply_updates([h.encode_from(0)])
            ref = oracle.merge(to_anchor(h.arrays()))
            for _ in range(2):
                text, dig = r.merge()
                assert text == ref and dig == oracle.tree_digest(ref), pt
            v = h.version()
            h.insert(6000, "Q")       # after id 6000, inside the second tile
            h.remove(8300, 12200)     # most of the third tile, tombstones only
            r.apply_updates([h.encode_from(v)])
            ref = oracle.merge(to_anchor(h.arrays()))
            assert len(ref) == N + 1 - 3900
            for _ in range(3):
                text, dig = r.merge()
                assert text == ref and dig == oracle.tree_digest(ref), pt
            v = h.version()
            h.remove(4000, 8200)      # the second tile dead too, but for the "Q"
            r.apply_updates([h.encode_from(v)])
            ref = oracle.merge(to_anchor(h.arrays()))
            for _ in range(2):
                text, dig = r.merge()
                assert text == ref and dig == oracle.tree_digest(ref), pt
            r.close()
    finally:
        c.set_param("plain_tiles", 1)
        c.set_param("nsq_list", 1)
    c.close()


def test_plain_tiles_malformed_parents():
    """An out-of-range parent and a self-parent still fail with EBADLOG under both settings, in a
    batch with plain tiles too (a bad parent may point into one)."""
    n = N
    ok = _chain(n)
    bad = _chain(n, [(n + 40000, n + 1, 1, 98)])
    selfp = _chain(n, [(n + 1, n + 1, 1, 98)])
    c = crdt_hip.Context(0)
    try:
        for b_ in (bad, selfp):
            b = c.batch([ok, b_, ok], replicas=2, relabel="none")
            for pt in (1, 0, 1):
                c.set_param("plain_tiles", pt)
                for _ in range(2):
                    with pytest.raises(crdt_hip.CrdtHipError) as e:
                        b.merge()
                    assert e.value.code == -5, pt
            b.close()
    finally:
        c.set_param("plain_tiles", 1)
    c.close()
