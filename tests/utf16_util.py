"""Shared helpers of test_utf16.py and test_gpu_utf16.py (test infrastructure only).

A plain Python restatement of the UTF-16 positions (include/crdt_hip_utf16.h): a character weighs
`len(ch.encode("utf-16-le")) // 2` code units and `len(ch.encode("utf-8"))` bytes, and a gap is the
cumulative sum of the characters before it.  The version's text itself comes from the CPU oracle
(patch_util.oracle_merge) or from a recording made when the mark was taken; nothing here calls the
product.  `raw` is the C call with canary outputs, for the refusals.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import crdt_hip
import crdt_hip_utf16 as cu

CP, BYTES, UTF16 = cu.UNIT_CODEPOINTS, cu.UNIT_BYTES, cu.UNIT_UTF16
EINVAL, ERANGE = -1, -2
CANARY = 0xA5
DT = cu.UNIT_POS_DTYPE
FIELD = ("cp", "bytes", "utf16")


def units16(s: str) -> int:
    return len(s.encode("utf-16-le")) // 2


class Model:
    """The gaps of the version whose text is `text`, in the three units."""

    def __init__(self, text: str):
        self.text = text
        self.len = len(text)
        self.bd = np.concatenate([[0], np.cumsum([len(ch.encode("utf-8")) for ch in text])]).astype(np.uint64)
        self.ud = np.concatenate([[0], np.cumsum([units16(ch) for ch in text])]).astype(np.uint64)
        self.nbytes, self.n16 = int(self.bd[-1]), int(self.ud[-1])
        assert self.nbytes == len(text.encode("utf-8")) and self.n16 == units16(text)
        self.info = {"len": self.len, "len_bytes": self.nbytes, "len_utf16": self.n16}

    def records(self, gaps) -> np.ndarray:
        g = np.asarray(gaps, np.int64).reshape(-1)
        assert ((0 <= g) & (g <= self.len)).all()
        out = np.zeros(g.size, DT)
        out["cp"], out["bytes"], out["utf16"] = g, self.bd[g], self.ud[g]
        return out

    def total(self, unit: int) -> int:
        return (self.len, self.nbytes, self.n16)[unit]

    def inside(self, unit: int) -> list:
        """The positions of `unit` that name no gap."""
        ends = {BYTES: self.bd, UTF16: self.ud}.get(unit)
        if ends is None:
            return []
        return sorted(set(range(self.total(unit) + 1)) - set(ends.tolist()))


def same(got: tuple, want: np.ndarray, info: dict) -> None:
    arr, inf = got
    assert arr.dtype == DT and arr.tobytes() == want.tobytes(), \
        [(g, w) for g, w in zip(arr.tolist(), want.tolist()) if g != w][:5]
    assert inf == info


def check_gaps(obj, mark, m: Model, gaps) -> None:
    """The gaps `gaps` of the version whose model is m, asked in each of the three units."""
    want = m.records(gaps)
    for unit in (CP, BYTES, UTF16):
        same(cu.units_of(obj, want[FIELD[unit]], unit, mark), want, m.info)


def check_all(obj, mark, text: str) -> Model:
    """Every gap in each of the three units (in descending order too), the info, the round trips
    and the length."""
    m = Model(text)
    gaps = np.arange(m.len + 1)
    check_gaps(obj, mark, m, gaps)
    check_gaps(obj, mark, m, gaps[::-1].repeat(2))
    u = cu.to_utf16(obj, gaps, mark)
    assert u.tolist() == m.ud.tolist()
    assert cu.from_utf16(obj, u, mark).tolist() == gaps.tolist()
    assert cu.to_utf16(obj, m.bd, mark, bytes=True).tolist() == m.ud.tolist()
    assert cu.from_utf16(obj, u, mark, bytes=True).tolist() == m.bd.tolist()
    assert cu.len_utf16(obj, mark) == m.n16
    return m


# ---- patches in UTF-16 code units, by the definitions ----
def to_cp_patches(text: str, plist16) -> list:
    """[(pos, del, ins)] in UTF-16 code units -> the same patches in codepoints, each translated
    through the text as the earlier patches left it (which no boundary may split a pair of)."""
    out = []
    for pos, dele, ins in plist16:
        m = Model(text)
        a, b = (m.ud.tolist().index(x) for x in (pos, pos + dele))
        out.append((a, b - a, ins))
        text = text[:a] + ins + text[b:]
    return out


def patches16_at(m: Model, edits) -> list:
    """[(a, b, ins)], ascending ranges [a, b) in gaps (codepoints) of the document whose model is m
    -> the same edits as a patch set in UTF-16 code units: pos counted in the document as the
    earlier patches left it."""
    out, shift = [], 0
    for a, b, ins in edits:
        dele = int(m.ud[b] - m.ud[a])
        out.append((int(m.ud[a]) + shift, dele, ins))
        shift += units16(ins) - dele
    return out


def splice16(text: str, plist16) -> str:
    """The patches spliced in order into the UTF-16 of `text`."""
    u = text.encode("utf-16-le")
    for pos, dele, ins in plist16:
        assert 2 * (pos + dele) <= len(u)
        u = u[: 2 * pos] + ins.encode("utf-16-le") + u[2 * (pos + dele):]
    return u.decode("utf-16-le")


def check_since(obj, mark, at_text: str, now_text: str) -> tuple:
    """patches_since_utf16 of obj: the splice property, and the patch count and the `ins` of the
    codepoint call.  Returns the raw result."""
    raw = cu.patches_since_utf16_raw(obj, mark)
    cp_raw = obj.patches_since_raw(mark)
    assert raw[1] == cp_raw[1] and raw[0].size == cp_raw[0].size
    assert raw[0]["ins_off"].tobytes() == cp_raw[0]["ins_off"].tobytes()
    assert raw[0]["ins_len"].tobytes() == cp_raw[0]["ins_len"].tobytes()
    plist = crdt_hip._patch_list(raw)
    assert splice16(at_text, plist) == now_text
    assert plist == cu.patches_since_utf16(obj, mark)
    return raw


# ---- the C call with canaries, for the refusals ----
def raw(obj, positions, unit: int, mark=None, n=None, null_in=False, null_out=False, info=True,
        ctx=None) -> tuple:
    """One C call of units_of with an output block of exactly n records filled with a canary and
    *info preset -> (rc, output bytes, info dict or None).  ctx: another context's handle for a
    replica call."""
    L = cu.lib()
    q = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
    n = q.size if n is None else n
    out = np.full(max(n, 1) * DT.itemsize, CANARY, np.uint8)
    inf = cu.UnitInfo(0xDEAD, 0xDEAD, 0xDEAD)
    if isinstance(obj, crdt_hip.Replica):
        fn, lead = L.crdt_hip_replica_units_of, (ctx if ctx is not None else obj.ctx._h, obj._h)
    else:
        fn, lead = L.crdt_hip_oplog_units_of, (obj._h,)
    rc = fn(*lead, mark._h if mark is not None else None, None if null_in or not q.size else q.ctypes.data,
            n, unit, None if null_out else out.ctypes.data, C.byref(inf) if info else None)
    return rc, out.tobytes(), inf.as_dict() if info else None


UNTOUCHED = {"len": 0xDEAD, "len_bytes": 0xDEAD, "len_utf16": 0xDEAD}


def assert_refused(obj, positions, unit: int, code: int, **kw) -> None:
    """The call returns `code` and leaves out and *info as they were."""
    rc, out, inf = raw(obj, positions, unit, **kw)
    assert rc == code, (rc, code, unit, list(positions)[:4])
    assert out == bytes([CANARY]) * len(out) and inf == UNTOUCHED


def refusals(obj, mark, m: Model, foreign_marks) -> None:
    """Every refusal of the check list on the version (mark, m), in its stated order, with canary
    outputs untouched.  m must hold a character of two code units."""
    wide = next(i for i, ch in enumerate(m.text) if units16(ch) == 2)
    in16 = int(m.ud[wide]) + 1
    inb = [int(m.bd[wide]) + j for j in (1, 2, 3)]
    assert in16 in m.inside(UTF16) and set(inb) <= set(m.inside(BYTES))
    kw = {"mark": mark}
    for unit in (CP, BYTES, UTF16):
        assert_refused(obj, [0, m.total(unit) + 1], unit, ERANGE, **kw)            # len + 1
        assert_refused(obj, [m.total(unit) + 1], unit, ERANGE, **kw)
        assert_refused(obj, [1 << 63, 0], unit, ERANGE, **kw)
        assert_refused(obj, [0], unit, EINVAL, null_out=True, **kw)
        assert_refused(obj, [0], unit, EINVAL, null_in=True, **kw)
        assert_refused(obj, [1 << 40], unit, EINVAL, null_out=True, **kw)          # 2 before 3
        for fm in foreign_marks:
            assert_refused(obj, [0], unit, EINVAL, mark=fm)
            assert_refused(obj, [1 << 40], unit, EINVAL, mark=fm)                  # 1 before 3
    for bad in (3, 4, 1 << 31):
        assert_refused(obj, [0], bad, EINVAL, **kw)                                # unit 3
        assert_refused(obj, [1 << 40], bad, EINVAL, **kw)                          # 2 before 3
        assert_refused(obj, [0], bad, EINVAL, null_out=True, **kw)
    assert_refused(obj, [in16], UTF16, EINVAL, **kw)                               # inside a pair, alone
    assert_refused(obj, [0, in16, m.n16], UTF16, EINVAL, **kw)
    assert_refused(obj, [in16, m.n16 + 1], UTF16, ERANGE, **kw)                    # 3 before 4
    assert_refused(obj, [m.n16 + 1, in16], UTF16, ERANGE, **kw)
    for p in inb:
        assert_refused(obj, [0, p, m.nbytes], BYTES, EINVAL, **kw)
        assert_refused(obj, [p, m.nbytes + 1], BYTES, ERANGE, **kw)
    # n == 0 writes only info; info may be NULL
    for unit in (CP, BYTES, UTF16):
        rc, out, inf = raw(obj, [], unit, **kw)
        assert (rc, inf) == (0, m.info) and out == bytes([CANARY]) * len(out)
        rc, out, inf = raw(obj, [], unit, null_out=True, null_in=True, **kw)
        assert (rc, inf) == (0, m.info)
        rc, out, inf = raw(obj, [m.total(unit)], unit, info=False, **kw)
        assert rc == 0 and out == m.records([m.len]).tobytes()


def apply_refused(obj, plist16, code: int, ins=None) -> None:
    """apply_patches_utf16 raises `code`."""
    try:
        cu.apply_patches_utf16(obj, plist16, ins)
    except crdt_hip.CrdtHipError as e:
        assert e.code == code, (e.code, code, str(e))
    else:
        raise AssertionError(f"not refused: {plist16}")


def patch_refusals(obj, text: str) -> None:
    """The refusals of apply_patches_utf16 in their order on a document whose text is `text`, which
    must start with "a😀b😀" (positions 0 a 1 😀 3 b 4 😀 6).  Nothing changes."""
    assert text.startswith("a😀b😀")
    n16 = units16(text)
    before = obj.encode_diff([])
    apply_refused(obj, [(0, 0, "")], EINVAL)                          # empty
    apply_refused(obj, [(0, 1, "x"), (1, 1, "")], EINVAL)             # touching: 1 > 0 + 1 fails
    apply_refused(obj, [(0, 0, "😀"), (2, 1, "")], EINVAL)            # touching in UTF-16: 2 > 0 + 2 fails
    apply_refused(obj, [(4, 2, ""), (0, 1, "")], EINVAL)              # descending
    bad = np.zeros(1, crdt_hip.PATCH_DTYPE)
    bad[0] = (0, 0, 0, 2)
    apply_refused(obj, bad, EINVAL, ins=b"\xff\xfe")                  # not UTF-8
    bad[0] = (0, 1, 0, 2)
    apply_refused(obj, bad, EINVAL, ins=b"x")                         # a piece outside ins
    apply_refused(obj, [(n16, 1, "")], ERANGE)                        # beyond
    apply_refused(obj, [(n16 + 1, 0, "x")], ERANGE)
    apply_refused(obj, [(2, 1, "")], EINVAL)                          # pos inside a pair
    apply_refused(obj, [(0, 2, "")], EINVAL)                          # the end of a delete inside one
    apply_refused(obj, [(0, 1, "zz"), (6, 1, "")], EINVAL)            # ... of a later patch: 6 - 1 = 5
    apply_refused(obj, [(2, 0, "x"), (n16 + 2, 0, "y")], ERANGE)      # the range error wins
    apply_refused(obj, [(n16 + 1, 0, "y"), (0, 0, "")], ERANGE)       # array order: patch 0's range first
    apply_refused(obj, [(0, 0, ""), (n16 + 9, 0, "y")], EINVAL)       # ... and patch 0's emptiness first
    apply_refused(obj, [(2, 0, "x"), (3, 0, "")], EINVAL)             # an argument check before "inside"
    assert cu.apply_patches_utf16(obj, []) == (0, 0)
    assert obj.encode_diff([]) == before, "a refused call changed the log"
