"""Patches since a mark on the host (crdt_hip_oplog_mark / crdt_hip_oplog_patches_since).

After an update, a join or a delta an editor needs what changed in its document as the
reference's positional edits, TestPatch(pos, del, ins) applied as Upstream::replace
(rope.rs:21-32).  Expected patches are computed without the product (patch_util.patches over the
CPU oracle's document order) and applied to the oracle's text at the mark.  CPU only.
"""
import ctypes as C
import random

import numpy as np
import pytest

import crdt_hip
import delta_util as du
import join_fugue_util as jf
import join_util as ju
import patch_util as pu

KINDS = ["rga", "fugue"]
TEXT = "héllo wörld, €uro 😀 and more text"


def typed(fugue: bool, text: str = TEXT) -> crdt_hip.OpLog:
    log = pu.new_log(fugue)
    log.insert(0, text)
    return log


def marked(oracle, log):
    return log.mark(), pu.At(oracle, log.arrays())


@pytest.mark.parametrize("kind", KINDS)
def test_single_edits_give_the_single_patch(oracle, kind):
    fugue = kind == "fugue"
    n = len(TEXT)
    cases = [
        (lambda l: l.insert(7, "X€"), [(7, 0, "X€")]),
        (lambda l: l.remove(3, 9), [(3, 6, "")]),
        (lambda l: l.replace(4, 6, "😀z"), [(4, 2, "😀z")]),
        (lambda l: l.insert(0, "é"), [(0, 0, "é")]),
        (lambda l: l.remove(n - 1, n), [(n - 1, 1, "")]),
        (lambda l: l.remove(0, n), [(0, n, "")]),
        (lambda l: None, []),
    ]
    for edit, want in cases:
        log = typed(fugue)
        m, at = marked(oracle, log)
        edit(log)
        assert log.patches_since(m) == want
        assert pu.check(oracle, log, m, at, log.arrays()) == want
    # a mark on the empty log: the whole text is one insert
    log = pu.new_log(fugue)
    m, at = marked(oracle, log)
    assert log.patches_since(m) == []
    log.insert(0, TEXT)
    assert pu.check(oracle, log, m, at, log.arrays()) == [(0, 0, TEXT)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("edits", [50, 400])
def test_random_edits_after_a_mark(oracle, kind, edits):
    log = pu.base_log(kind == "fugue")
    m, at = marked(oracle, log)
    ju.random_edits(log, random.Random(100 + edits), edits)
    got = pu.check(oracle, log, m, at, log.arrays())
    assert len(got) > 10
    assert any(len(i.encode()) > len(i) for _, _, i in got)      # multi-byte inserts


def forks_of(base, fugue):
    f = jf.fork if fugue else ju.fork
    return f(base, 1, 21, 60), f(base, 2, 22, 50)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["join", "apply_diff", "apply_update"])
def test_sync_after_a_mark(oracle, kind, how):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    a, b = forks_of(base, fugue)
    if how == "apply_update":
        # a downstream copy of the base receives a's ops as one wire update
        dst = base.clone()
        m, at = marked(oracle, dst)
        dst.apply_update(a.encode_from(base.version()))
        ju.assert_same_log(dst.arrays(), a.arrays(), oright=False)
        assert pu.check(oracle, dst, m, at, dst.arrays())
        return
    m, at = marked(oracle, a)
    if how == "join":
        a.join(b)
    else:
        a.apply_diff(b.encode_diff(a.state_vector()))
    arrs = a.arrays()
    got = pu.check(oracle, a, m, at, arrs)
    assert got and arrs.n > at.n


@pytest.mark.parametrize("kind", KINDS)
def test_concurrent_siblings_interleaved_runs_and_transient_items(oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    # two forks insert at the same position
    a, b = base.clone(), base.clone()
    a.set_agent(1)
    b.set_agent(2)
    a.insert(50, "aa")
    b.insert(50, "b€")
    dst = base.clone()
    m, at = marked(oracle, dst)
    dst.join(a)
    dst.join(b)
    got = pu.check(oracle, dst, m, at, dst.arrays())
    assert len(got) == 1 and got[0][:2] == (50, 0) and sorted(got[0][2]) == sorted("aab€")
    # a stretch deleted here, typed into there: one patch that deletes and inserts
    f = base.clone()
    f.set_agent(3)
    f.insert(105, "XY")
    dst = base.clone()
    m, at = marked(oracle, dst)
    dst.remove(100, 110)
    dst.join(f)
    assert pu.check(oracle, dst, m, at, dst.arrays()) == [(100, 10, "XY")]
    # an item a fork inserted and deleted again appears in no patch
    f = base.clone()
    f.set_agent(4)
    f.insert(50, "Q")
    f.remove(50, 51)
    dst = base.clone()
    m, at = marked(oracle, dst)
    assert dst.join(f)[0] == 1
    assert pu.check(oracle, dst, m, at, dst.arrays()) == []


@pytest.mark.parametrize("kind", KINDS)
def test_two_marks_alive_at_once(oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    a, b = forks_of(base, fugue)
    dst = base.clone()
    m1, at1 = marked(oracle, dst)
    dst.join(a)
    m2, at2 = marked(oracle, dst)
    dst.apply_diff(b.encode_diff(dst.state_vector()))
    dst.insert(3, "local")
    arrs = dst.arrays()
    p1 = pu.check(oracle, dst, m1, at1, arrs)
    p2 = pu.check(oracle, dst, m2, at2, arrs)
    assert p1 != p2 and at1.text != at2.text
    m1.close()
    assert pu.check(oracle, dst, m2, at2, arrs) == p2


def raw_call(log, mark, cap, ins_cap):
    out = np.zeros(max(cap, 1), crdt_hip.PATCH_DTYPE)
    ins = np.zeros(max(ins_cap, 1), np.uint8)
    n, nb = C.c_size_t(77), C.c_size_t(77)
    rc = crdt_hip.lib().crdt_hip_oplog_patches_since(
        log._h, mark._h, out.ctypes.data if cap else None, cap, C.byref(n),
        ins.ctypes.data if ins_cap else None, ins_cap, C.byref(nb))
    return rc, n.value, nb.value, out[:cap], ins[:ins_cap].tobytes()


def test_buffers_follow_the_espace_convention(oracle):
    log = pu.base_log(False)
    m, _ = marked(oracle, log)
    assert raw_call(log, m, 0, 0)[:3] == (0, 0, 0)               # nothing changed: nothing needed
    ju.random_edits(log, random.Random(3), 60)
    want, want_ins = log.patches_since_raw(m)
    np_, nb = len(want), len(want_ins)
    assert np_ > 3 and nb > 3
    assert raw_call(log, m, 0, 0)[:3] == (du.ESPACE, np_, nb)
    assert raw_call(log, m, np_ - 1, nb)[:3] == (du.ESPACE, np_, nb)
    assert raw_call(log, m, np_, nb - 1)[:3] == (du.ESPACE, np_, nb)
    rc, n, b, out, ins = raw_call(log, m, np_, nb)
    assert (rc, n, b) == (0, np_, nb)
    assert out.tobytes() == want.tobytes() and ins == want_ins


def test_marks_of_other_owners_are_refused(oracle):
    log, other = pu.base_log(False), pu.base_log(False)
    flog = pu.base_log(True)
    m = log.mark()
    for wrong in (other, log.clone(), flog):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            wrong.patches_since(m)
        assert e.value.code == du.EINVAL
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        log.patches_since(flog.mark())
    assert e.value.code == du.EINVAL
    n, nb = C.c_size_t(), C.c_size_t()
    L = crdt_hip.lib()
    assert L.crdt_hip_oplog_patches_since(log._h, None, None, 0, C.byref(n), None, 0, C.byref(nb)) == du.EINVAL
    assert L.crdt_hip_oplog_patches_since(log._h, m._h, None, 0, None, None, 0, C.byref(nb)) == du.EINVAL
    assert log.patches_since(m) == []                            # the mark itself still works


@pytest.mark.parametrize("kind", KINDS)
def test_a_call_leaves_the_resolver_index_alone(oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    a, _ = forks_of(base, fugue)
    logs = [base.clone(), base.clone()]           # the second is the twin that never asks
    marks = []
    for i, log in enumerate(logs):
        log.set_agent(7)
        m = log.mark()
        marks.append(m)
        rng = random.Random(9)
        ju.random_edits(log, rng, 20)
        if i == 0:
            assert log.patches_since(m)           # between two local edits: the index is live
        ju.random_edits(log, rng, 20)
        log.join(a)                               # the index goes stale
        if i == 0:
            assert log.patches_since(m)
        ju.random_edits(log, rng, 20)             # the next edit rebuilds it
        if i == 0:
            log.patches_since(m)
        log.insert(log.visible_len(), "end")
    x, y = logs[0].arrays(), logs[1].arrays()
    (jf.assert_same_log if fugue else ju.assert_same_log)(x, y)
    assert logs[0].visible_len() == logs[1].visible_len()
    assert logs[0].patches_since(marks[0]) == logs[1].patches_since(marks[1])
