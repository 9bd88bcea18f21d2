"""The line index on the host (crdt_hip_oplog_line_starts / _lines_of, OpLog::line_starts and
OpLog::lines_of): the definition the device path is held to, against the plain Python model of
lines_util over the oracle's text.  CPU only.
"""
import os
import re

import numpy as np
import pytest

import crdt_hip
import crdt_hip_lines as cl
import lines_util as lu
import patch_util as pu
from conftest import ROOT
from test_patches import KINDS, typed

TINY = ["", "\n", "a", "a\n", "\n\n", "a\nb", "é\n😀€\n"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("text", TINY, ids=[repr(t) for t in TINY])
def test_tiny_versions(oracle, kind, text):
    """Every line number 0..L + 1, every gap in codepoints, every codepoint boundary in bytes."""
    fugue = kind == "fugue"
    log = typed(fugue, text) if text else pu.new_log(fugue)
    assert pu.oracle_merge(oracle, log.arrays())[0] == text
    m = lu.check_all(log, None, text)
    assert m.info["lines"] == text.count("\n") + 1
    lu.check_text_lines(log, None, m)
    # the empty version of a mark taken before anything was typed
    empty = pu.new_log(fugue)
    mk = empty.mark()
    if text:
        empty.insert(0, text)
    lu.check_all(empty, mk, "")
    lu.check_all(empty, None, text)


def test_the_lines_of_the_issue():
    """"a\\n" has two lines, the last one empty; the gap after a line break is column 0 of the next
    line, the gap before it belongs to the line it ends."""
    log = typed(False, "ab\ncd\n")
    st, info = cl.line_starts(log, [0, 1, 2, 3])
    assert info == {"lines": 3, "len": 6, "len_bytes": 6}
    assert st["start"].tolist() == [0, 3, 6, 6] and st["line"].tolist() == [0, 1, 2, 3]
    of = cl.lines_of(log, [2, 3, 5, 6])[0]
    assert list(zip(of["line"].tolist(), of["col"].tolist())) == [(0, 2), (1, 0), (1, 2), (2, 0)]
    # CR, U+2028 and the rest are ordinary characters
    assert cl.line_count(typed(False, "a\rb c\u0085d\x0b\x0c")) == 1
    # numbers in any order, repeated
    st = cl.line_starts(log, [2, 0, 2, 1, 1])[0]
    assert st["start"].tolist() == [6, 0, 6, 3, 3]


@pytest.mark.parametrize("kind", KINDS)
def test_trace_prefix_with_a_mark_part_way(oracle, kind):
    """The first 2,000 patches of sveltecomponent (the document order is not the slot order), a
    mark after 1,200 of them, and after the rest two more edits: a line break the mark saw is
    deleted and one is typed.  Now and at the mark."""
    fugue = kind == "fugue"
    t = crdt_hip.Trace(os.path.join(ROOT, "traces", "sveltecomponent.json.gz"))
    log = pu.new_log(fugue)
    if t.start_content:
        log.insert(0, t.start_content)
    mk = at = None
    for i in range(2000):
        if i == 1200:
            mk, at = log.mark(), pu.At(oracle, log.arrays())
        pos, dele, ins = t.patch(i)
        log.replace(pos, pos + dele, ins)
    arrs = log.arrays()
    text, order = pu.oracle_merge(oracle, arrs)
    assert order != sorted(order) and at.text.count("\n") > 5 and text != at.text
    # a line break that was there at the mark and still is: the first item of the order that is one
    # and selected both ways
    shared = next(s for s in order if arrs.cp[s - 1] == 10 and not arrs.deleted[s - 1]
                  and s <= at.n and not at.deleted[s - 1])
    pos = sum(1 for s in order[: order.index(shared)] if not arrs.deleted[s - 1])
    log.remove(pos, pos + 1)
    log.insert(7, "x\ny")
    text2 = pu.oracle_merge(oracle, log.arrays())[0]
    assert text2.count("\n") == text.count("\n")           # one deleted, one typed
    m_now = lu.check_all(log, None, text2)
    m_at = lu.check_all(log, mk, at.text)
    assert m_now.starts.tolist() != m_at.starts.tolist()
    lu.check_text_lines(log, None, m_now)
    lu.check_text_lines(log, mk, m_at, [(0, 3), (5, 2), (m_at.L - 1, 4)])


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_outputs_untouched(oracle, kind):
    fugue = kind == "fugue"
    text = "ab\n😀c\n\né€"
    log = typed(fugue, text)
    mk = log.mark()
    log.replace(1, 4, "Z\n\n😀")
    now = pu.oracle_merge(oracle, log.arrays())[0]
    clone = log.clone()
    foreign = [clone.mark()]
    before = log.encode_diff([])
    lu.refusals(log, None, lu.Model(now), foreign)
    lu.refusals(log, mk, lu.Model(text), foreign)
    # an owner with fewer items than the mark
    small = typed(fugue, "a")
    big_mark = log.mark()
    L = cl.lib()
    out = np.zeros(1, lu.DT)
    q = np.zeros(1, np.uint64)
    assert L.crdt_hip_oplog_line_starts(small._h, big_mark._h, q.ctypes.data, 1, out.ctypes.data, None) == -1
    assert L.crdt_hip_oplog_line_starts(None, None, q.ctypes.data, 1, out.ctypes.data, None) == -1
    assert L.crdt_hip_oplog_lines_of(None, None, q.ctypes.data, 1, 0, out.ctypes.data, None) == -1
    assert L.crdt_hip_line_stats(None, None, None, None) == -1
    assert log.encode_diff([]) == before, "a read changed the log"
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        cl.line_starts(log, [99])
    assert e.value.code == -2 and "beyond" in str(e.value)


def test_adapters_are_unwrapped_and_other_objects_refused():
    h = crdt_hip.HipMerge.from_str("one\ntwo\nthree")
    assert cl.line_count(h) == 3 and cl.text_lines(h, 1, 1) == b"two\n"
    assert cl.lines_of(h, [5])[0][["line", "col"]].tolist() == [(1, 1)]
    with pytest.raises(TypeError):
        cl.line_count("one\ntwo")
    with pytest.raises(ValueError):
        cl.text_lines(h, -1, 2)


def _snapshot():
    return sorted(vars(crdt_hip)), list(crdt_hip.EXPORTS), {
        c.__name__: sorted(vars(c)) for c in (crdt_hip.OpLog, crdt_hip.Replica, crdt_hip.Context)}


def test_the_extension_touches_neither_surface():
    """import crdt_hip_lines adds nothing to the package, and crdt_hip_lines.h declares exactly the
    five functions the module binds, all exported."""
    import importlib
    import sys
    before = _snapshot()
    kept = sys.modules.pop("crdt_hip_lines", None)   # import it afresh, as a first import does
    try:
        mod = importlib.import_module("crdt_hip_lines")
        mod.lib()
        assert mod.line_count(crdt_hip.OpLog()) == 1
    finally:
        if kept is not None:
            sys.modules["crdt_hip_lines"] = kept
    assert _snapshot() == before
    assert "crdt_hip_lines" not in vars(crdt_hip) and not hasattr(crdt_hip, "lines")
    with open(os.path.join(ROOT, "include", "crdt_hip_lines.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(crdt_hip_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(mod.EXPORTS) and len(declared) == 5
    assert all(hasattr(crdt_hip.lib(), s) for s in declared)
    assert not set(declared) & set(crdt_hip.EXPORTS)
    with open(os.path.join(ROOT, "include", "crdt_hip.h")) as f:
        assert "crdt_hip_line" not in f.read()
