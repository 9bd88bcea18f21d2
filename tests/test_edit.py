"""Local edits as positional patches on the host (crdt_hip_oplog_apply_patches).

The result is defined as crdt_hip_oplog_replace called once per patch, in order: a clone that got
the patches that way must hold the same log slot for slot, every column and delete op included
(edit_util.same_logs), and the oracle's text of the log must be the plain string model's.  A
rejected call returns its code and leaves the log as it was.  CPU only.
"""
import random

import pytest

import crdt_hip
import edit_util as eu
import patch_util as pu
from conftest import TRACES, trace_path
from edit_util import KINDS
from test_patches import TEXT, typed


def both(oracle, log: crdt_hip.OpLog, text: str, plist) -> str:
    """apply_patches on `log`, the replace loop on a clone: same log, and the model's text."""
    ref = log.clone()
    eu.replace_loop(ref, plist)
    added, tomb = log.apply_patches(plist)
    assert added == sum(len(i) for _, _, i in plist) and tomb == sum(d for _, d, _ in plist)
    eu.same_logs(log, ref)
    want = eu.model_apply(text, plist)
    assert pu.oracle_merge(oracle, log.arrays())[0] == want
    assert log.visible_len() == len(want)
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_single_edits(oracle, kind):
    fugue = kind == "fugue"
    n = len(TEXT)
    for p in [(0, 0, "é"), (7, 0, "X€"), (n, 0, "end"), (0, 1, ""), (n - 1, 1, ""), (0, n, ""),
              (4, 2, "X€"), (n - 2, 2, "😀z")]:
        both(oracle, typed(fugue), TEXT, [p])
    log = pu.new_log(fugue)
    assert both(oracle, log, "", [(0, 0, "héllo")]) == "héllo"
    assert log.apply_patches([]) == (0, 0)
    # the new identities carry the log's agent
    log = typed(fugue)
    log.set_agent(7)
    log.apply_patches([(3, 0, "q")])
    A = log.arrays()
    assert A.agent[-1] == 7 and set(A.agent[:-1].tolist()) == {0}
    assert A.lamport[-1] == A.lamport[:-1].max() + 1


@pytest.mark.parametrize("kind", KINDS)
def test_many_patches(oracle, kind):
    text, plist = eu.interleaved(3000)
    log = typed(kind == "fugue", text)
    assert both(oracle, log, text, plist) == "aX" * 3000 + "a"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_patch_sets_between_joins(oracle, kind, seed):
    fugue = kind == "fugue"
    rng = random.Random(40 + seed)
    log = eu.two_agent_log(fugue, rng.randint(2000, 4000), seed)
    log.set_agent(5)
    other = log.clone()
    other.set_agent(6)
    text = pu.oracle_merge(oracle, log.arrays())[0]
    for step in range(3):
        plist = eu.random_patches(rng, len(text), rng.choice([1, 20, 200]))
        text = both(oracle, log, text, plist)
        # a join in between: the next call rebuilds the positional index first
        eu.replace_loop(other, eu.random_patches(rng, other.visible_len(), 10))
        log.join(other)
        text = pu.oracle_merge(oracle, log.arrays())[0]
    assert log.arrays().n > 2000


@pytest.mark.parametrize("kind", KINDS)
def test_rejected_calls_change_nothing(kind):
    log = typed(kind == "fugue")
    n = log.visible_len()
    before = (log.encode_diff([]), log.encode_from(0), log.version(), n)
    for name, rows, ins, code in eu.rejections(n):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            log.apply_patches(*eu.raw(rows, ins))
        assert e.value.code == code, name
        assert (log.encode_diff([]), log.encode_from(0), log.version(), log.visible_len()) == before, name
    # the limits that depend on the log: the lamports (ERANGE, nothing changed)
    big = pu.new_log(kind == "fugue")
    big.join(crdt_hip.LogArrays([0], [0xFFFFFFF0], [1], [0], [ord("a")],
                                side=[0] if kind == "fugue" else None))
    snap = big.encode_diff([])
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        big.apply_patches([(1, 0, "x" * 15)])
    assert e.value.code == -2 and big.encode_diff([]) == snap
    assert big.apply_patches([(1, 0, "x" * 14)]) == (14, 0)


@pytest.mark.parametrize("name", TRACES)
def test_traces_one_patch_per_call(name):
    """apply_patches equals the replace loop on the first 2,000 patches of every trace."""
    t = crdt_hip.Trace(trace_path(name))
    a, b = crdt_hip.OpLog(), crdt_hip.OpLog()
    if t.start_content:
        a.insert(0, t.start_content)
        b.insert(0, t.start_content)
    for i in range(min(2000, len(t))):
        pos, dele, ins = t.patch(i)
        if dele or ins:
            a.apply_patches([(pos, dele, ins)])
        b.replace(pos, pos + dele, ins)
    eu.same_logs(a, b)
