"""UTF-16 positions on the host (crdt_hip_oplog_units_of and the *_utf16 edits and patches,
OpLog::units_of): the definition the device path is held to, against the plain Python model of
utf16_util over the oracle's text.  CPU only.
"""
import os
import random
import re

import numpy as np
import pytest

import crdt_hip
import crdt_hip_utf16 as cu
import patch_util as pu
import utf16_util as uu
from conftest import ROOT
from test_patches import KINDS, forks_of, typed

TINY = ["", "a", "😀", "a😀", "😀😀", "é€😀\n"]


def same_log(a, b) -> None:
    """Two logs hold the same items slot for slot."""
    A, B = a.arrays(), b.arrays()
    for col in ("parent", "lamport", "agent", "deleted", "cp"):
        assert (getattr(A, col) == getattr(B, col)).all(), col
    assert (A.side is None) == (B.side is None) and (A.side is None or (A.side == B.side).all())
    assert a.encode_diff([]) == b.encode_diff([])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("text", TINY, ids=[repr(t) for t in TINY])
def test_tiny_versions(oracle, kind, text):
    """Every gap in each of the three units, the info and the round trips."""
    fugue = kind == "fugue"
    log = typed(fugue, text) if text else pu.new_log(fugue)
    assert pu.oracle_merge(oracle, log.arrays())[0] == text
    m = uu.check_all(log, None, text)
    assert m.n16 == len(text) + text.count("😀")
    # the empty version of a mark taken before anything was typed
    empty = pu.new_log(fugue)
    mk = empty.mark()
    if text:
        empty.insert(0, text)
    uu.check_all(empty, mk, "")
    uu.check_all(empty, None, text)
    for unit in (uu.CP, uu.BYTES, uu.UTF16):
        uu.assert_refused(empty, [1], unit, uu.ERANGE, mark=mk)


def test_the_units_of_the_issue():
    """"a😀é" is 3 codepoints, 7 bytes and 4 code units; a surrogate's codepoint weighs 1 by value."""
    log = typed(False, "a😀é")
    rec, info = cu.units_of(log, [4, 0, 3, 1, 3], cu.UNIT_UTF16)
    assert info == {"len": 3, "len_bytes": 7, "len_utf16": 4}
    assert rec.tolist() == [(3, 7, 4), (0, 0, 0), (2, 5, 3), (1, 1, 1), (2, 5, 3)]
    uu.assert_refused(log, [2], uu.UTF16, uu.EINVAL)
    # a log built from raw arrays that holds U+D800 and U+DFFF: 3 bytes, 1 code unit each
    A = typed(False, "abc").arrays()
    A.cp[:] = [0xD800, 0x10000, 0xDFFF]
    raw = crdt_hip.OpLog()
    assert raw.join(A) == (3, 0)
    rec, info = cu.units_of(raw, [0, 1, 2, 3], cu.UNIT_CODEPOINTS)
    assert rec["utf16"].tolist() == [0, 1, 3, 4] and rec["bytes"].tolist() == [0, 3, 7, 10]


@pytest.mark.parametrize("kind", KINDS)
def test_trace_prefix_with_a_mark_part_way(oracle, kind):
    """The first 2,000 patches of sveltecomponent (the document order is not the slot order), an
    astral character typed before a mark taken after 1,200 of them and one typed after it, and after
    the rest the first one is deleted.  Now and at the mark."""
    fugue = kind == "fugue"
    t = crdt_hip.Trace(os.path.join(ROOT, "traces", "sveltecomponent.json.gz"))
    log = pu.new_log(fugue)
    if t.start_content:
        log.insert(0, t.start_content)
    mk = at = None
    for i in range(2000):
        if i == 1200:
            log.insert(40, "😀")
            mk, at = log.mark(), pu.At(oracle, log.arrays())
            log.insert(90, "𝄞x")
        pos, dele, ins = t.patch(i)
        log.replace(pos, pos + dele, ins)
    text, order = pu.oracle_merge(oracle, log.arrays())
    assert order != sorted(order) and at.text.count("😀") == 1 and text != at.text
    p = text.index("😀")
    assert "𝄞" in text
    log.remove(p, p + 1)
    text2 = pu.oracle_merge(oracle, log.arrays())[0]
    assert "😀" not in text2 and "𝄞" in text2
    m_now = uu.check_all(log, None, text2)
    m_at = uu.check_all(log, mk, at.text)
    assert m_now.n16 == m_now.len + 1 and m_at.n16 == m_at.len + 1
    assert m_now.ud.tolist() != m_at.ud.tolist()
    uu.check_since(log, mk, at.text, text2)
    for m, mark in ((m_now, None), (m_at, mk)):
        a, b = int(m.ud[m.len // 3]), int(m.ud[2 * m.len // 3])
        assert cu.text_range_utf16(log, a, b, mark).decode() == m.text[m.len // 3: 2 * m.len // 3]


SETS = [
    # an astral inserted by an earlier patch and one deleted: the running shift differs between units
    [(0, 0, "😀𝄞"), (5, 2, ""), (9, 1, "x😀"), (14, 3, "é")],
    [(1, 2, "")],
    [(0, 1, "😀"), (4, 3, "ab"), (8, 0, "𝄞")],
    [(13, 0, "end😀")],
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pset", SETS, ids=[str(i) for i in range(len(SETS))])
def test_apply_patches_utf16_is_apply_patches_of_the_translation(oracle, kind, pset):
    fugue = kind == "fugue"
    text = "a😀b😀cdé€😀z"                      # 10 codepoints, 13 code units
    log = typed(fugue, text)
    log.remove(4, 5)
    log.insert(4, "c")                           # (a tombstone in the middle)
    want = log.clone()
    cp_set = uu.to_cp_patches(text, pset)
    assert cp_set != pset
    got = cu.apply_patches_utf16(log, pset)
    assert got == want.apply_patches(cp_set)
    same_log(log, want)
    now = pu.oracle_merge(oracle, log.arrays())[0]
    assert now == uu.splice16(text, pset)
    uu.check_all(log, None, now)


@pytest.mark.parametrize("kind", KINDS)
def test_replace_insert_remove_utf16_follow_a_string_model(oracle, kind):
    """A seeded keystroke script in UTF-16 code units against a Python str held as UTF-16."""
    fugue = kind == "fugue"
    rng = random.Random(5)
    log, twin_log, text = pu.new_log(fugue), pu.new_log(fugue), ""
    for step in range(120):
        m = uu.Model(text)
        ga, gb = sorted(rng.randrange(m.len + 1) for _ in range(2))
        a, b = int(m.ud[ga]), int(m.ud[min(gb, ga + 5)])
        ins = "".join(rng.choice("ab é€😀𝄞\n") for _ in range(rng.randrange(4)))
        how = step % 3
        if how == 0:
            cu.replace_utf16(log, a, b, ins)
        elif how == 1:
            cu.insert_utf16(log, a, ins)
            b = a
        else:
            cu.remove_utf16(log, a, b)
            ins = ""
        ca, cb = m.ud.tolist().index(a), m.ud.tolist().index(b)
        twin_log.replace(ca, cb, ins)
        text = uu.splice16(text, [(a, b - a, ins)]) if (b > a or ins) else text
        assert cu.len_utf16(log) == uu.units16(text)
    same_log(log, twin_log)
    assert pu.oracle_merge(oracle, log.arrays())[0] == text
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        cu.remove_utf16(log, 3, 2)
    assert e.value.code == -2
    line, ch = cu.lines_of_utf16(log, uu.Model(text).ud)
    rows = text.split("\n")
    want = [(r, uu.units16(rows[r][:c])) for r in range(len(rows)) for c in range(len(rows[r]) + 1)]
    assert list(zip(line.tolist(), ch.tolist())) == want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["join", "apply_diff"])
def test_patches_since_utf16_after_a_sync(oracle, kind, how):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    base.insert(2, "😀x𝄞")
    base.insert(base.visible_len(), "😀")
    a, b = forks_of(base, fugue)
    a.insert(1, "𝄞")
    b.insert(0, "é😀")
    b.remove(3, 5)
    m, at = a.mark(), pu.At(oracle, a.arrays())
    if how == "join":
        a.join(b)
    else:
        a.apply_diff(b.encode_diff(a.state_vector()))
    now = pu.oracle_merge(oracle, a.arrays())[0]
    raw = uu.check_since(a, m, at.text, now)
    assert raw[0].size and raw[0].tobytes() != a.patches_since_raw(m)[0].tobytes()
    # the ESPACE convention of the bytes twin: the counts, and nothing copied
    L = cu.lib()
    import ctypes as C
    n, nb = C.c_size_t(0), C.c_size_t(0)
    assert L.crdt_hip_oplog_patches_since_utf16(a._h, m._h, None, 0, C.byref(n), None, 0, C.byref(nb)) == -6
    assert (n.value, nb.value) == (raw[0].size, len(raw[1]))
    assert L.crdt_hip_oplog_patches_since_utf16(a._h, m._h, None, 0, None, None, 0, C.byref(nb)) == -1
    assert L.crdt_hip_oplog_patches_since_utf16(a._h, b.mark()._h, None, 0, C.byref(n), None, 0, C.byref(nb)) == -1
    # nothing changed since a fresh mark
    assert cu.patches_since_utf16(a, a.mark()) == []


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_in_their_order(oracle, kind):
    fugue = kind == "fugue"
    text = "a😀b😀c\né€"
    log = typed(fugue, text)
    mk = log.mark()
    log.replace(6, 8, "Z😀\n")
    now = pu.oracle_merge(oracle, log.arrays())[0]
    clone = log.clone()
    foreign = [clone.mark()]
    before = log.encode_diff([])
    uu.refusals(log, None, uu.Model(now), foreign)
    uu.refusals(log, mk, uu.Model(text), foreign)
    assert log.encode_diff([]) == before, "a read changed the log"
    uu.patch_refusals(log, now)
    # an owner with fewer items than the mark, and NULL handles
    small = typed(fugue, "a")
    L = cu.lib()
    out = np.zeros(1, uu.DT)
    q = np.zeros(1, np.uint64)
    assert L.crdt_hip_oplog_units_of(small._h, log.mark()._h, q.ctypes.data, 1, 0, out.ctypes.data, None) == -1
    assert L.crdt_hip_oplog_units_of(None, None, q.ctypes.data, 1, 0, out.ctypes.data, None) == -1
    assert L.crdt_hip_oplog_apply_patches_utf16(None, None, 0, None, 0, None, None) == -1
    assert L.crdt_hip_oplog_replace_utf16(None, 0, 0, None, 0) == -1
    assert L.crdt_hip_unit_stats(None, None, None, None) == -1
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        cu.units_of(log, [99], cu.UNIT_UTF16)
    assert e.value.code == -2 and "beyond" in str(e.value)
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        cu.from_utf16(log, [2])
    assert e.value.code == -1 and "pair" in str(e.value)


def test_adapters_are_unwrapped_and_other_objects_refused():
    h = crdt_hip.HipMerge.from_str("a😀\nb𝄞c")
    assert cu.len_utf16(h) == 8 and cu.to_utf16(h, [2, 6]).tolist() == [3, 8]
    assert cu.text_range_utf16(h, 1, 5) == "😀\nb".encode()
    line, ch = cu.lines_of_utf16(h, [3, 4, 7])
    assert list(zip(line.tolist(), ch.tolist())) == [(0, 3), (1, 0), (1, 3)]
    cu.insert_utf16(h, 3, "é")
    assert h.log.visible_len() == 7
    with pytest.raises(TypeError):
        cu.len_utf16("a😀")


def _snapshot():
    return sorted(vars(crdt_hip)), list(crdt_hip.EXPORTS), {
        c.__name__: sorted(vars(c)) for c in (crdt_hip.OpLog, crdt_hip.Replica, crdt_hip.Context,
                                              crdt_hip.HipDownstream, crdt_hip._Adapter, crdt_hip._Document)}


def test_the_extension_touches_neither_surface():
    """import crdt_hip_utf16 adds nothing to the package, and crdt_hip_utf16.h declares exactly the
    nine functions the module binds, all exported and none of them in crdt_hip.h."""
    import importlib
    import sys
    before = _snapshot()
    kept = sys.modules.pop("crdt_hip_utf16", None)   # import it afresh, as a first import does
    try:
        mod = importlib.import_module("crdt_hip_utf16")
        mod.lib()
        assert mod.len_utf16(crdt_hip.OpLog()) == 0
    finally:
        if kept is not None:
            sys.modules["crdt_hip_utf16"] = kept
    assert _snapshot() == before
    assert "crdt_hip_utf16" not in vars(crdt_hip) and not hasattr(crdt_hip, "utf16")
    with open(os.path.join(ROOT, "include", "crdt_hip_utf16.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(crdt_hip_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(mod.EXPORTS) and len(declared) == 9
    assert all(hasattr(crdt_hip.lib(), s) for s in declared)
    assert not set(declared) & set(crdt_hip.EXPORTS)
    with open(os.path.join(ROOT, "include", "crdt_hip.h")) as f:
        base = f.read()
    assert "utf16" not in base.lower() and "crdt_hip_unit" not in base
