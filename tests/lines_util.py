"""Shared helpers of test_lines.py and test_gpu_lines.py (test infrastructure only).

A plain Python restatement of the line index (include/crdt_hip_lines.h): the lines of a version are
`text.split("\\n")`, a line starts where the cumulative sum of the earlier lines' lengths (each
with its line break) ends, and a position's line is the last one that starts at or before it.  The
version's text itself comes from the CPU oracle (patch_util.oracle_merge) or from a recording made
when the mark was taken; nothing here calls the product.  `raw` is the C call with canary outputs,
for the refusals.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import crdt_hip
import crdt_hip_lines as cl
import tiles_util as tl

BYTES = crdt_hip.TEXT_BYTES
EINVAL, ERANGE = -1, -2
CANARY = 0xA5
DT = cl.LINE_POS_DTYPE


class Model:
    """The line index of the version whose text is `text`."""

    def __init__(self, text: str):
        self.text = text
        cps = np.frombuffer(text.encode("utf-32-le"), "<u4")
        # bd[v]: the UTF-8 bytes of the first v codepoints (text_util.boundaries)
        self.bd = np.concatenate([[0], np.cumsum(tl.widths(cps))]).astype(np.uint64)
        self.parts = text.split("\n")
        lens = np.array([len(p) for p in self.parts], np.int64)
        # starts[k]: where line k starts, k = 0..L; ends: the same with the version's end as L + 1
        self.starts = np.concatenate([[0], np.cumsum(lens[:-1] + 1)]).astype(np.uint64)
        self.L = len(self.parts) - 1
        self.ends = np.concatenate([self.starts, [len(text)]]).astype(np.uint64)
        self.len, self.nbytes = len(text), int(self.bd[-1])
        self.info = {"lines": self.L + 1, "len": self.len, "len_bytes": self.nbytes}

    def line_starts(self, lines) -> np.ndarray:
        k = np.asarray(lines, np.int64).reshape(-1)
        assert ((0 <= k) & (k <= self.L + 1)).all()
        out = np.zeros(k.size, DT)
        out["line"] = k
        out["start"] = self.ends[k]
        out["start_bytes"] = self.bd[self.ends[k].astype(np.int64)]
        return out

    def gaps_of_bytes(self, pos) -> np.ndarray:
        p = np.asarray(pos, np.uint64).reshape(-1)
        g = np.searchsorted(self.bd, p)
        assert (g <= self.len).all() and (self.bd[g] == p).all(), "inside a codepoint"
        return g

    def lines_of(self, positions, bytes: bool = False) -> np.ndarray:
        g = self.gaps_of_bytes(positions) if bytes else np.asarray(positions, np.int64).reshape(-1)
        assert ((0 <= g) & (g <= self.len)).all()
        line = np.searchsorted(self.starts, g.astype(np.uint64), side="right") - 1
        out = np.zeros(g.size, DT)
        out["line"] = line
        out["start"] = self.starts[line]
        out["start_bytes"] = self.bd[self.starts[line].astype(np.int64)]
        out["col"] = g.astype(np.uint64) - out["start"]
        out["col_bytes"] = self.bd[g] - out["start_bytes"]
        return out

    def text_lines(self, first: int, count: int) -> bytes:
        """Lines first .. first + count with their line breaks (the last line has none)."""
        with_breaks = [p + "\n" for p in self.parts[:-1]] + [self.parts[-1]]
        return "".join(with_breaks[first: first + count]).encode("utf-8")


def same(got: tuple, want: np.ndarray, info: dict) -> None:
    arr, inf = got
    assert arr.dtype == DT and arr.tobytes() == want.tobytes(), \
        [(g, w) for g, w in zip(arr.tolist(), want.tolist()) if g != w][:5]
    assert inf == info


def check_queries(obj, mark, m: Model, lines, gaps) -> None:
    """The line numbers `lines` and the gaps `gaps` (in codepoints, and the same gaps in bytes) of
    the version whose model is m, against the model."""
    same(cl.line_starts(obj, lines, mark), m.line_starts(lines), m.info)
    want = m.lines_of(gaps)
    same(cl.lines_of(obj, gaps, mark), want, m.info)
    same(cl.lines_of(obj, m.bd[np.asarray(gaps, np.int64)], mark, bytes=True), want, m.info)


def check_all(obj, mark, text: str) -> Model:
    """Every line number 0..L + 1, every gap in codepoints and every codepoint boundary in bytes,
    the identity lines_of(line_starts(k).start) == (k, col 0), and line_count."""
    m = Model(text)
    lines = np.arange(m.L + 2)
    check_queries(obj, mark, m, lines, np.arange(m.len + 1))
    st = cl.line_starts(obj, lines[:-1], mark)[0]
    back = cl.lines_of(obj, st["start"], mark)[0]
    assert (back["line"] == lines[:-1]).all() and not back["col"].any() and not back["col_bytes"].any()
    assert back["start"].tobytes() == st["start"].tobytes()
    assert cl.line_count(obj, mark) == m.L + 1
    return m


def check_text_lines(obj, mark, m: Model, cases=None) -> None:
    cases = cases or [(0, 0), (0, 1), (0, m.L + 1), (0, m.L + 5), (m.L, 1), (m.L + 1, 1), (m.L + 9, 2),
                      (m.L // 2, 3), (1, m.L)]
    for first, count in cases:
        assert cl.text_lines(obj, first, count, mark) == m.text_lines(first, count), (first, count)


# ---- the C calls with canaries, for the refusals ----
def raw(obj, name: str, queries, mark=None, flags: int = 0, n=None, null_in=False, null_out=False,
        info=True, ctx=None) -> tuple:
    """One C call of line_starts / lines_of with an output block of exactly n records filled with a
    canary and *info preset -> (rc, output bytes, info dict or None).  ctx: another context's
    handle for a replica call."""
    L = cl.lib()
    q = np.ascontiguousarray(queries, dtype=np.uint64).reshape(-1)
    n = q.size if n is None else n
    out = np.full(max(n, 1) * DT.itemsize, CANARY, np.uint8)
    inf = cl.LineInfo(0xDEAD, 0xDEAD, 0xDEAD)
    if isinstance(obj, crdt_hip.Replica):
        fn, lead = getattr(L, "crdt_hip_replica_" + name), (ctx if ctx is not None else obj.ctx._h, obj._h)
    else:
        fn, lead = getattr(L, "crdt_hip_oplog_" + name), (obj._h,)
    args = lead + (mark._h if mark is not None else None,
                   None if null_in or not q.size else q.ctypes.data, n)
    if name == "lines_of":
        args += (flags,)
    rc = fn(*args, None if null_out else out.ctypes.data, C.byref(inf) if info else None)
    return rc, out.tobytes(), inf.as_dict() if info else None


UNTOUCHED = {"lines": 0xDEAD, "len": 0xDEAD, "len_bytes": 0xDEAD}


def assert_refused(obj, name: str, queries, code: int, **kw) -> None:
    """The call returns `code` and leaves out and *info as they were."""
    rc, out, inf = raw(obj, name, queries, **kw)
    assert rc == code, (name, rc, code, list(queries)[:4])
    assert out == bytes([CANARY]) * len(out) and inf == UNTOUCHED


def refusals(obj, mark, m: Model, foreign_marks) -> None:
    """Every refusal of the check list on the version (mark, m), with canary outputs untouched.  m
    must hold a 4-byte codepoint.  foreign_marks: marks that are not `obj`'s."""
    wide = next(i for i, ch in enumerate(m.text) if len(ch.encode()) == 4)
    inside = [int(m.bd[wide]) + j for j in (1, 2, 3)]
    kw = {"mark": mark}
    assert_refused(obj, "line_starts", [0, m.L + 2], ERANGE, **kw)
    assert_refused(obj, "line_starts", [m.L + 2], ERANGE, **kw)
    assert_refused(obj, "line_starts", [1 << 63], ERANGE, **kw)
    assert_refused(obj, "lines_of", [0, m.len + 1], ERANGE, **kw)
    assert_refused(obj, "lines_of", [m.nbytes + 1, 0], ERANGE, flags=BYTES, **kw)
    for p in inside:
        assert_refused(obj, "lines_of", [0, p, m.nbytes], EINVAL, flags=BYTES, **kw)
        assert_refused(obj, "lines_of", [p, m.nbytes + 1], ERANGE, flags=BYTES, **kw)   # 3 before 4
    assert_refused(obj, "lines_of", [0], EINVAL, flags=2, **kw)
    assert_refused(obj, "lines_of", [0], EINVAL, flags=3, **kw)
    assert_refused(obj, "lines_of", [m.len + 1], EINVAL, flags=2, **kw)                 # 2 before 3
    for name in ("line_starts", "lines_of"):
        assert_refused(obj, name, [0], EINVAL, null_out=True, **kw)
        assert_refused(obj, name, [0], EINVAL, null_in=True, **kw)
        assert_refused(obj, name, [1 << 40], EINVAL, null_out=True, **kw)               # 2 before 3
        for fm in foreign_marks:
            assert_refused(obj, name, [0], EINVAL, mark=fm)
            assert_refused(obj, name, [1 << 40], EINVAL, mark=fm)                       # 1 before 3
    # n == 0 writes only info; info may be NULL
    for name in ("line_starts", "lines_of"):
        rc, out, inf = raw(obj, name, [], **kw)
        assert (rc, inf) == (0, m.info) and out == bytes([CANARY]) * len(out)
        rc, out, inf = raw(obj, name, [], null_out=True, null_in=True, **kw)
        assert (rc, inf) == (0, m.info)
        rc, out, inf = raw(obj, name, [0], info=False, **kw)
        assert rc == 0 and out == m.line_starts([0]).tobytes()
