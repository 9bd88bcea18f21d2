"""Level 0's static path (param static_jumps, the default): RGA batches with a compact nsq list
keep their jump bits resident (built once with the list, from the parent column alone), and on
contracted waves k_classify reads them and computes the run heads of its tile itself; k_heads is
not launched.  With static_jumps 0 every merge rebuilds the bits in k_classify and runs k_heads.

Every case: 8 rotated replicas (word and tile boundaries fall on different items in each), the
digests and lengths against the oracle's bytes, and static_jumps 1 and 0 against each other:
equal digests, lengths and run counts (equal run counts = equal run heads).
"""
import numpy as np
import pytest

import crdt_hip
from conftest import trace_path
from test_gpu_merge import to_anchor

pytestmark = pytest.mark.gpu

REPLICAS = 8
TILE = 4096


def _boundary_log() -> crdt_hip.OpLog:
    """~9,000 items (three tiles).  Item k of a document sits in slot k before the relabelling, and
    a first insert of N characters gives ids 1..N at positions 0..N-1, so `insert(p, ..)` into it
    has the item with id p as its parent.  Later inserts go from high positions to low ones, so
    that the positions of the ids below them stay what they were."""
    lg = crdt_hip.OpLog()
    n0 = 8500
    lg.insert(0, "".join(chr(97 + i % 26) for i in range(n0)))  # ids 1..8500, one chain
    nid = n0  # ids used so far

    def ins(pos, text):
        nonlocal nid
        lg.insert(pos, text)
        nid += len(text)

    # parent in an earlier tile: these items land in the third tile (ids > 8192), their parents
    # in the second and the first
    ins(2 * TILE - 7, "P")  # parent id 8185: second tile
    # parents at the last slot of a tile / the first slot of the next (ids 4095, 4096), and the
    # same around 64-slot words (ids 4159 = 64 * 65 - 1, 4160; 63, 64)
    ins(4160, "Q")
    ins(4159, "R")
    ins(4096, "S")
    ins(4095, "T")
    ins(100, "U")   # parent id 100: first tile, from the third
    ins(64, "V")
    ins(63, "W")
    # a dead run across a word boundary without a child: 150 characters typed at position 30 and
    # all removed (nothing was inserted after them while they were visible)
    ins(30, "d" * 150)
    lg.remove(30, 180)
    # a deleted stretch whose last item has a child: 100 characters at position 20, something
    # typed elsewhere (so the child's id is not the next one), the child typed after the last of
    # them, then the 100 removed: the last one keeps its jump bit, so its run is not dead
    ins(20, "e" * 100)
    ins(5, "x")
    ins(121, "C")  # after the 100th 'e' (position 120 after the 'x' at 5)
    lg.remove(21, 121)
    # a deleted stretch that ends exactly at a word's last slot: a run of its own whose last id
    # is 63 mod 64 (pad the ids up to it with visible text typed at the document's end first)
    run = 70
    pad = (63 - (nid + run) % 64) % 64
    if pad:
        ins(lg.visible_len(), "p" * pad)
    ins(10, "f" * run)
    assert nid % 64 == 63
    lg.remove(10, 10 + run)
    return lg


def _chain_delete_log() -> crdt_hip.OpLog:
    """A chain of 300 whose ids 130..191 are deleted: the stretch ends at a word's last slot (191 =
    3 * 64 - 1) inside a run that goes on."""
    lg = crdt_hip.OpLog()
    lg.insert(0, "".join(chr(65 + i % 26) for i in range(300)))
    lg.remove(129, 191)
    return lg


def _one_item_log() -> crdt_hip.OpLog:
    lg = crdt_hip.OpLog()
    lg.insert(0, "z")
    return lg


def _multibyte_log() -> crdt_hip.OpLog:
    """A few tiles of mostly multi-byte text (2-, 3- and 4-byte UTF-8), with edits in the middle
    and a deleted stretch: the weight nibbles of the escape path."""
    lg = crdt_hip.OpLog()
    unit = "aé中\U0001f600b߿ࠀ￿"
    lg.insert(0, unit * 1200)  # 9,600 items
    lg.insert(5000, "中文")
    lg.insert(4096, "\U0001f600")
    lg.insert(63, "é")
    lg.remove(700, 900)
    return lg


_CASES = {}


def _case(name, oracle):
    """The logs of a case and the oracle's digest and length of each, computed once."""
    if name not in _CASES:
        if name == "boundary":
            logs = [_boundary_log(), _one_item_log(), crdt_hip.OpLog(), _chain_delete_log()]
        elif name == "agents":
            logs = [crdt_hip.OpLog.synth_agents(20000, 64, 0x5EED0011)]
        else:
            logs = [_multibyte_log()]
        arrs = [lg.arrays() for lg in logs]
        refs = [oracle.merge(to_anchor(a)) for a in arrs]
        _CASES[name] = (arrs, [oracle.tree_digest(r) for r in refs], [len(r) for r in refs])
    return _CASES[name]


def _merge_both(c, b, want_d, want_l, merges=2):
    """The batch merged with static_jumps 1 and 0 (`merges` times each: the synchronous merge,
    then the learnt-plan one), every merge against the oracle; returns {setting: stats}."""
    nb = len(want_d)
    out = {}
    try:
        for sj in (1, 0):
            c.set_param("static_jumps", sj)
            for _ in range(merges):
                d, l, st = b.merge()
                for r in range(b.docs):
                    assert int(d[r]) == want_d[r % nb] and int(l[r]) == want_l[r % nb], (sj, r)
            out[sj] = (list(map(int, d)), list(map(int, l)), st)
    finally:
        c.set_param("static_jumps", 1)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2]["runs"] == out[1][2]["runs"]
    return {sj: out[sj][2] for sj in out}


@pytest.mark.parametrize("name", ["boundary", "agents", "multibyte"])
def test_static_jumps_match_the_oracle_and_the_rebuilt_bits(oracle, name):
    """Cases 1-3: boundary placements, many nsq items per tile, the escape path."""
    arrs, want_d, want_l = _case(name, oracle)
    c = crdt_hip.Context(0)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    st = _merge_both(c, b, want_d, want_l)
    # (the static path ran: one launch fewer in the runs stage of every wave)
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    assert st[0]["stage_launches"]["runs"] == 4 * st[0]["waves"]
    b.close()
    c.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_static_jumps_waves_and_lanes(oracle, lanes):
    """Case 4: the boundary batch in at least 3 waves (each wave reads its own range of the
    resident bits), on one lane and on two."""
    arrs, want_d, want_l = _case("boundary", oracle)
    c = crdt_hip.Context(0)
    c.set_param("lanes", lanes)
    c.set_param("max_wave_slots", 1 << 15)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    st = _merge_both(c, b, want_d, want_l)
    assert st[1]["waves"] >= 3 and st[0]["waves"] == st[1]["waves"]
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    assert st[0]["stage_launches"]["runs"] == 4 * st[0]["waves"]
    b.close()
    c.close()


def test_static_jumps_malformed_parents(oracle):
    """Case 5: a resident batch with an out-of-range parent and one with a self-parent: the flag
    set when the bits were built makes every merge fail with EBADLOG, as the rebuilt bits'
    k_classify does; a well-formed batch on the same context is clean afterwards."""
    bad_parent = crdt_hip.LogArrays([0, 5], [1, 2], [0, 0], [0, 0], [97, 98])
    self_parent = crdt_hip.LogArrays([0, 2], [1, 2], [0, 0], [0, 0], [97, 98])
    ok = crdt_hip.LogArrays([0, 1], [1, 2], [0, 0], [0, 0], [97, 98])
    arrs, want_d, want_l = _case("multibyte", oracle)
    c = crdt_hip.Context(0)
    try:
        for bad in (bad_parent, self_parent):
            b = c.batch([ok, bad, ok], replicas=2, relabel="none")
            for sj in (1, 0, 1):
                c.set_param("static_jumps", sj)
                for _ in range(2):
                    with pytest.raises(crdt_hip.CrdtHipError) as e:
                        b.merge()
                    assert e.value.code == -5, sj
            b.close()
            good = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
            d, l, st = good.merge()
            assert all(int(x) == want_d[0] for x in d) and all(int(x) == want_l[0] for x in l)
            assert st["stage_launches"]["runs"] == 3 * st["waves"]
            good.close()
    finally:
        c.set_param("static_jumps", 1)
    c.close()


def test_static_jumps_raw_soa(oracle):
    """Case 6: raw SoA mode rebuilds the list, and the bits with it, inside every merge; the
    results equal the encoded batch's under both settings."""
    arrs, want_d, want_l = _case("boundary", oracle)
    c = crdt_hip.Context(0)
    b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
    d0, l0, st0 = b.merge()
    b.set_raw(True)
    st = _merge_both(c, b, want_d, want_l, merges=3)
    d, l, st1 = b.merge()
    assert np.array_equal(d, d0) and np.array_equal(l, l0) and st1["runs"] == st0["runs"]
    assert st[1]["stage_launches"]["encode"] > 0
    assert st[1]["stage_launches"]["runs"] == 3 * st[1]["waves"]
    assert st[0]["stage_launches"]["runs"] == 4 * st[0]["waves"]
    b.set_raw(False)
    d, l, st2 = b.merge()
    assert np.array_equal(d, d0) and np.array_equal(l, l0) and st2["runs"] == st0["runs"]
    b.close()
    c.close()


def test_static_jumps_launch_counts(oracle):
    """Case 7: the runs stage is 3 launches per wave on the static path (tile scan, k_runs,
    k_docmax) and 4 with static_jumps 0 (k_heads first); a batch encoded with static_jumps 0 has
    no resident bits and keeps 4 whatever the setting at merge time; Fugue batches keep theirs."""
    arrs, want_d, want_l = _case("agents", oracle)
    c = crdt_hip.Context(0)
    try:
        c.set_param("static_jumps", 0)
        b = c.batch(arrs, replicas=REPLICAS, relabel="rotate", seed=5)
        st = _merge_both(c, b, want_d, want_l)
        assert st[1]["stage_launches"]["runs"] == 4 * st[1]["waves"]
        assert st[0]["stage_launches"]["runs"] == 4 * st[0]["waves"]
        b.close()
        fg = crdt_hip.Trace(trace_path("sveltecomponent")).resolve(fugue=True).arrays()
        b = c.batch([fg], replicas=2, relabel="rotate", seed=1)
        res = {}
        for sj in (1, 0):
            c.set_param("static_jumps", sj)
            d, l, st = b.merge()
            res[sj] = (list(map(int, d)), list(map(int, l)), st["runs"])
            assert st["stage_launches"]["runs"] == 4 * st["waves"], sj
        assert res[0] == res[1]
        b.close()
    finally:
        c.set_param("static_jumps", 1)
    c.close()
