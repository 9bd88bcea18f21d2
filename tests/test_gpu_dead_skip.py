"""Level 0's plane path (param dead_skip, the default): RGA batches with a compact nsq list keep
their tombstone and previous-slot flags as two bit planes beside it, and on the static path of a
text merge k_classify_plane takes both from the planes and fetches the codepoint words only of
16-slot groups that hold a visible item.  With dead_skip 0 k_classify reads every slot's word.

Every case: 8 rotated replicas (group, word and tile boundaries fall on different items in each),
the digests and lengths against the oracle's bytes, and dead_skip 1 and 0 against each other: equal
digests, lengths and run counts; three merges per setting (the synchronous one, the learnt plan,
the plan again).
"""
import pytest

import crdt_hip
from test_gpu_merge import to_anchor
from test_gpu_static_jumps import _multibyte_log, _one_item_log

pytestmark = pytest.mark.gpu

REPLICAS = 8
TILE = 4096
UNIT = "aé中\U0001f600b߿ࠀ￿"  # (_multibyte_log's alphabet: 1, 2, 3, 4, 1, 2, 3, 3 bytes)


def _typed(n: int, text=None) -> crdt_hip.OpLog:
    """n characters typed in one go: ids 1..n, id k at position k - 1."""
    lg = crdt_hip.OpLog()
    lg.insert(0, text if text is not None else "".join(chr(97 + i % 26) for i in range(n)))
    return lg


def _keep_only(lg: crdt_hip.OpLog, n: int, keep) -> None:
    """Remove ids 1..n of a log made by _typed except `keep`, from the highest gap down, so
    that the positions of the ids below a gap are still id - 1 when it is removed."""
    edges = sorted(set(keep)) + [n + 1]
    gaps = [(lo + 1, hi - 1) for lo, hi in zip([0] + edges[:-1], edges) if hi - lo > 1]
    for lo, hi in reversed(gaps):
        lg.remove(lo - 1, hi)  # (ids lo..hi)
    assert lg.visible_len() == len(set(keep))


def _all_dead_logs():
    """9,000 characters typed and all removed (three tiles, none with a visible item), an empty
    log and a one-item log."""
    lg = _typed(9000)
    lg.remove(0, 9000)
    assert lg.visible_len() == 0
    return [lg, crdt_hip.OpLog(), _one_item_log()]


def _islands_log() -> crdt_hip.OpLog:
    """12,500 items (more than three tiles), deleted except single survivors around group, word
    and tile boundaries and the document's last item.  Before the rotation the third tile (slots
    8192..12287) holds the lone survivor 8192 and the fourth (12288..) the last item alone."""
    n = 12500
    lg = _typed(n)
    _keep_only(lg, n, [1, 15, 16, 63, 64, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n])
    return lg


def _jump_log() -> crdt_hip.OpLog:
    """A deleted stretch of 8,300 items (at least two whole tiles) whose last item has a child
    typed later, after an edit elsewhere: its run stays a head and weighs nothing.  Then a deleted
    stretch of 4,200 with no child: a dead run."""
    lg = _typed(100)                      # ids 1..100, kept
    lg.insert(50, "e" * 8300)             # ids 101..8400 at positions 50..8349
    lg.insert(5, "x")                     # an edit elsewhere: the child's id is not the next one
    lg.insert(8351, "C")                  # after the last 'e' (position 8350 since the 'x')
    lg.remove(51, 8351)                   # every 'e'
    assert lg.visible_len() == 102
    lg.insert(20, "d" * 4200)             # nothing is typed after these while they are visible
    lg.remove(20, 4220)
    assert lg.visible_len() == 102
    return lg


def _multibyte_islands_log() -> crdt_hip.OpLog:
    """9,600 items of the multi-byte alphabet, deleted except: id 100, a 4-byte character alone
    in its group; id 4095, a 3-byte character in a tile's last slot (before the rotation); and a
    visible ASCII character typed between two 4-byte ones that are then deleted."""
    n = 9600
    lg = _typed(n, UNIT * (n // len(UNIT)))
    assert UNIT[(100 - 1) % 8] == "\U0001f600" and len(UNIT[(TILE - 2) % 8].encode()) == 3
    _keep_only(lg, n, [100, TILE - 1])
    lg.insert(1, "\U0001f600z\U0001f600")
    lg.remove(3, 4)
    lg.remove(1, 2)
    assert lg.visible_len() == 3
    return lg


_LOGS = {
    "all_dead": _all_dead_logs,
    "islands": lambda: [_islands_log()],
    "jump": lambda: [_jump_log()],
    "multibyte_islands": lambda: [_multibyte_islands_log(), _multibyte_log()],
    "agents": lambda: [crdt_hip.OpLog.synth_agents(20000, 64, 0x5EED0012)],
}
_CASES = {}


def _case(name, oracle):
    """The logs of a case and the oracle's digest and length of each, computed once."""
    if name not in _CASES:
        arrs = [lg.arrays() for lg in _LOGS[name]()]
        refs = [oracle.merge(to_anchor(a)) for a in arrs]
        _CASES[name] = (arrs, [oracle.tree_digest(r) for r in refs], [len(r) for r in refs])
    return _CASES[name]


def _merge_both(c, b, want_d, want_l, merges=3):
    """The batch merged with dead_skip 1 and 0, `merges` times each, every merge against the
    oracle; the two settings against each other; returns {setting: stats}."""
    nb = len(want_d)
    out = {}
    try:
        for ds in (1, 0):
            c.set_param("dead_skip", ds)
            for _ in range(merges):
                d, l, st = b.merge()
                for r in range(b.docs):
                    assert int(d[r]) == want_d[r % nb] and int(l[r]) == want_l[r % nb], (ds, r)
            out[ds] = (list(map(int, d)), list(map(int, l)), st)
    finally:
        c.set_param("dead_skip", 1)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2]["runs"] == out[1][2]["runs"]
    return {ds: out[ds][2] for ds in out}


@pytest.mark.parametrize("name", list(_LOGS))
def test_dead_skip_matches_the_oracle_and_the_full_read(oracle, name):
    arrs, want_d, want_l = _case(name, oracle)
    c = crdt_hip.Context(0)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    st = _merge_both(c, b, want_d, want_l)
    # (both settings on level 0's static path: no k_heads launch)
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    assert st[0]["stage_launches"]["runs"] == 3 * st[0]["waves"]
    b.close()
    c.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_dead_skip_waves_and_lanes(oracle, lanes):
    """The islands batch in at least 3 waves (each reads its own range of the planes), on one
    lane and on two."""
    arrs, want_d, want_l = _case("islands", oracle)
    c = crdt_hip.Context(0)
    c.set_param("lanes", lanes)
    c.set_param("max_wave_slots", 1 << 15)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    st = _merge_both(c, b, want_d, want_l)
    assert st[1]["waves"] >= 3 and st[0]["waves"] == st[1]["waves"]
    b.close()
    c.close()


def test_dead_skip_raw_soa(oracle):
    """Raw SoA mode rebuilds the list, and the planes with it, inside every merge."""
    arrs, want_d, want_l = _case("multibyte_islands", oracle)
    c = crdt_hip.Context(0)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    b.set_raw(True)
    st = _merge_both(c, b, want_d, want_l)
    assert st[1]["stage_launches"]["encode"] > 0
    b.close()
    c.close()


def test_dead_skip_malformed_parents():
    """A resident batch with an out-of-range parent and one with a self-parent still fail with
    EBADLOG under dead_skip 1 (and 0)."""
    bad_parent = crdt_hip.LogArrays([0, 5], [1, 2], [0, 0], [0, 0], [97, 98])
    self_parent = crdt_hip.LogArrays([0, 2], [1, 2], [0, 0], [0, 0], [97, 98])
    ok = crdt_hip.LogArrays([0, 1], [1, 2], [0, 0], [0, 0], [97, 98])
    c = crdt_hip.Context(0)
    try:
        for bad in (bad_parent, self_parent):
            b = c.batch([ok, bad, ok], replicas=2, relabel="none")
            for ds in (1, 0, 1):
                c.set_param("dead_skip", ds)
                for _ in range(2):
                    with pytest.raises(crdt_hip.CrdtHipError) as e:
                        b.merge()
                    assert e.value.code == -5, ds
            b.close()
    finally:
        c.set_param("dead_skip", 1)
    c.close()


def test_dead_skip_list_rebuilding_replica(oracle):
    """A replica that rebuilds its list in every merge (nsq_list 2) rebuilds the planes with it:
    tombstones set through an update between two merges are seen by the second merge."""
    host = _typed(6000)
    c = crdt_hip.Context(0)
    try:
        c.set_param("nsq_list", 2)
        for ds in (1, 0):
            c.set_param("dead_skip", ds)
            h = host.clone()
            r = crdt_hip.Replica(c)
            r.apply_updates([h.encode_from(0)])
            text, dig = r.merge()
            ref = oracle.merge(to_anchor(h.arrays()))
            assert text == ref and dig == oracle.tree_digest(ref), ds
            v = h.version()
            h.remove(1000, 5500)  # more than a tile of tombstones
            h.remove(3, 40)
            r.apply_updates([h.encode_from(v)])
            ref = oracle.merge(to_anchor(h.arrays()))
            assert len(ref) == 6000 - 4500 - 37
            for _ in range(2):
                text, dig = r.merge()
                assert text == ref and dig == oracle.tree_digest(ref), ds
            r.close()
    finally:
        c.set_param("dead_skip", 1)
        c.set_param("nsq_list", 1)
    c.close()
