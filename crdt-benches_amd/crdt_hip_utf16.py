"""UTF-16 positions for libcrdt_hip.so (include/crdt_hip_utf16.h): a gap position translated between
codepoints, UTF-8 bytes and UTF-16 code units, and edits and patches in UTF-16 code units, on an
OpLog (the definition) and on a device Replica (HIP kernels, csrc/utf16.hip), now or at a mark.

An extension beside the crdt_hip package, not a part of it: it takes the library handle from
crdt_hip.lib(), sets the argument types of its own nine functions and adds no name to the package
or to its classes.  `obj` is an OpLog or a Replica; a HipMerge, HipDownstream or HipDownstreamBytes
is unwrapped to the document it holds (queued updates decoded first).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import crdt_hip
import crdt_hip_lines
from crdt_hip_lines import _document

UNIT_CODEPOINTS, UNIT_BYTES, UNIT_UTF16 = 0, 1, 2
UNIT_POS_DTYPE = np.dtype([("cp", "<u8"), ("bytes", "<u8"), ("utf16", "<u8")])
_FIELD = ("cp", "bytes", "utf16")  # of a unit


class UnitInfo(C.Structure):
    """crdt_hip_unit_info: codepoints, UTF-8 bytes and UTF-16 code units of the whole version."""
    _fields_ = [("len", C.c_uint64), ("len_bytes", C.c_uint64), ("len_utf16", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert UNIT_POS_DTYPE.itemsize == 24 and C.sizeof(UnitInfo) == 24

_P, _U64, _U32, _SZ = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t
_APPLY = [_P, _SZ, C.c_char_p, _SZ, _U32, _U32]
_REPLACE = [_SZ, _SZ, C.c_char_p, _SZ]
_SINCE = [_P, _P, _SZ, C.POINTER(_SZ), _P, _SZ, C.POINTER(_SZ)]
_SIG = {
    "crdt_hip_oplog_units_of": (C.c_int, [_P, _P, _P, _SZ, C.c_uint32, _P, _P]),
    "crdt_hip_replica_units_of": (C.c_int, [_P, _P, _P, _P, _SZ, C.c_uint32, _P, _P]),
    "crdt_hip_oplog_apply_patches_utf16": (C.c_int, [_P] + _APPLY),
    "crdt_hip_replica_apply_patches_utf16": (C.c_int, [_P, _P] + _APPLY),
    "crdt_hip_oplog_replace_utf16": (C.c_int, [_P] + _REPLACE),
    "crdt_hip_replica_replace_utf16": (C.c_int, [_P, _P] + _REPLACE),
    "crdt_hip_oplog_patches_since_utf16": (C.c_int, [_P] + _SINCE),
    "crdt_hip_replica_patches_since_utf16": (C.c_int, [_P, _P] + _SINCE),
    "crdt_hip_unit_stats": (C.c_int, [_P, _U64, _U64, _U64]),
}
EXPORTS = list(_SIG)
_BOUND = False


def lib() -> C.CDLL:
    """crdt_hip.lib() with the signatures of the nine functions of crdt_hip_utf16.h set."""
    global _BOUND
    L = crdt_hip.lib()
    if not _BOUND:
        for name, (res, args) in _SIG.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _BOUND = True
    return L


def units_of(obj, positions, unit: int, mark=None, out=None) -> tuple:
    """The gap positions `positions` (in `unit`: UNIT_CODEPOINTS, UNIT_BYTES or UNIT_UTF16; any
    order, repeats allowed) of the version now (`mark` None) or at `mark`, each in all three units
    -> (array of UNIT_POS_DTYPE, {"len", "len_bytes", "len_utf16"}).  `out`: an array to write into
    (a failed call leaves it untouched)."""
    doc, prefix, lead, ectx = _document(obj)
    q = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
    if out is None:
        out = np.zeros(q.size, UNIT_POS_DTYPE)
    assert out.dtype == UNIT_POS_DTYPE and out.size == q.size
    info = UnitInfo()
    rc = getattr(lib(), prefix + "units_of")(*lead, mark._h if mark is not None else None,
                                             q.ctypes.data if q.size else None, q.size, unit,
                                             out.ctypes.data if out.size else None, C.byref(info))
    crdt_hip._check(rc, ectx)
    return out, info.as_dict()


def to_utf16(obj, positions, mark=None, bytes: bool = False) -> np.ndarray:
    """Positions in codepoints (with `bytes`: in UTF-8 bytes) -> the same gaps in UTF-16 code units."""
    return units_of(obj, positions, UNIT_BYTES if bytes else UNIT_CODEPOINTS, mark)[0]["utf16"].copy()


def from_utf16(obj, positions, mark=None, bytes: bool = False) -> np.ndarray:
    """Positions in UTF-16 code units -> the same gaps in codepoints (with `bytes`: in UTF-8 bytes).
    A position between the two code units of one character raises EINVAL."""
    return units_of(obj, positions, UNIT_UTF16, mark)[0]["bytes" if bytes else "cp"].copy()


def len_utf16(obj, mark=None) -> int:
    """UTF-16 code units of the version."""
    return units_of(obj, [], UNIT_UTF16, mark)[1]["len_utf16"]


def apply_patches_utf16(obj, patches, ins=None) -> tuple:
    """apply_patches with pos and del in UTF-16 code units (`ins` stays text): the log apply_patches
    gives for the patches translated through the text before the call.  A boundary inside a pair
    raises EINVAL.  Returns (items appended, items deleted); a rejected call changes nothing."""
    doc, prefix, lead, ectx = _document(obj)
    arr, text = crdt_hip._patches_pack(patches, ins)
    a, t = C.c_uint32(0), C.c_uint32(0)
    rc = getattr(lib(), prefix + "apply_patches_utf16")(*lead, arr.ctypes.data if arr.size else None,
                                                        arr.size, text, len(text), C.byref(a), C.byref(t))
    crdt_hip._check(rc, ectx)
    return int(a.value), int(t.value)


def replace_utf16(obj, start: int, end: int, text: str) -> None:
    """Upstream::replace in UTF-16 code units: one patch."""
    doc, prefix, lead, ectx = _document(obj)
    b = text.encode("utf-8")
    crdt_hip._check(getattr(lib(), prefix + "replace_utf16")(*lead, start, end, b, len(b)), ectx)


def insert_utf16(obj, pos: int, text: str) -> None:
    replace_utf16(obj, pos, pos, text)


def remove_utf16(obj, start: int, end: int) -> None:
    if end < start:
        raise crdt_hip.CrdtHipError(-2, "remove range out of range")
    replace_utf16(obj, start, end, "")


def patches_since_utf16_raw(obj, mark) -> tuple:
    """patches_since_utf16 as (crdt_hip_patch array as a structured numpy array, `ins` bytes)."""
    doc, prefix, lead, ectx = _document(obj)
    f = getattr(lib(), prefix + "patches_since_utf16")
    return crdt_hip._patches_get(lambda *a: f(*lead, mark._h, *a), ectx, doc._GUESS_PATCHES)


def patches_since_utf16(obj, mark) -> list:
    """patches_since with pos and del in UTF-16 code units, as [(pos, del, ins: str)]: spliced in
    order into the UTF-16 of the text at the mark they give the UTF-16 of the text now (what a
    JavaScript editor applies to its string)."""
    return crdt_hip._patch_list(patches_since_utf16_raw(obj, mark))


def text_range_utf16(obj, start: int, end: int, mark=None) -> bytes:
    """The UTF-8 of window [start, end) in UTF-16 code units of the version: units_of of the two
    ends, then text_at of that byte window (a replica gets only the window back)."""
    doc = _document(obj)[0]
    b = units_of(doc, [start, end], UNIT_UTF16, mark)[0]["bytes"]
    if b[1] < b[0]:
        raise crdt_hip.CrdtHipError(-1, "text window starts after its end")
    return doc.text_at(mark, int(b[0]), int(b[1]), bytes=True)


def lines_of_utf16(obj, positions, mark=None) -> tuple:
    """(line, character) of the positions `positions` in UTF-16 code units, as two arrays: the
    Language Server Protocol's pair under its default encoding.  Two translations and the line
    index between them: the positions to codepoints, lines_of, and the line starts to UTF-16."""
    doc = _document(obj)[0]
    q = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
    cps = units_of(doc, q, UNIT_UTF16, mark)[0]["cp"]
    lp = crdt_hip_lines.lines_of(doc, cps, mark)[0]
    starts = units_of(doc, lp["start"], UNIT_CODEPOINTS, mark)[0]["utf16"]
    return lp["line"].copy(), q - starts


def stats(ctx) -> dict:
    """What the context's last device translation observed (crdt_hip_unit_stats)."""
    v = [C.c_uint64() for _ in range(3)]
    crdt_hip._check(lib().crdt_hip_unit_stats(ctx._h, *map(C.byref, v)), ctx._h)
    return dict(zip(("queries", "ranks", "device_ns"), (int(x.value) for x in v)))


class HipDownstreamUtf16(crdt_hip.HipDownstream):
    """HipDownstream for a caller that counts UTF-16 code units (a JavaScript string, Monaco,
    CodeMirror, LSP's default `character`): every method that takes or returns a position does so
    in UTF-16 code units.  insert, remove, replace, patches_since and sync_patches are the *_utf16
    calls of the library (one translation inside the call).  The calls without a UTF-16 form in the
    library (len, text_range, text_at, anchor_at, resolve, resolve_many, format, unformat, spans,
    lines_of) translate through units_of: one more device call each, a pass over the kept order
    and a host wait."""

    NAME = "mi355x-device-utf16"

    def clone(self) -> "HipDownstreamUtf16":
        c = HipDownstreamUtf16(self.replica.clone())
        c.pending = list(self.pending)
        return c

    def insert(self, at: int, text: str) -> None:
        insert_utf16(self._rt_peer(), at, text)

    def remove(self, start: int, end: int) -> None:
        remove_utf16(self._rt_peer(), start, end)

    def replace(self, start: int, end: int, text: str) -> None:
        replace_utf16(self._rt_peer(), start, end, text)

    def len(self) -> int:
        """UTF-16 code units of the merged document (units_of's info: one device call)."""
        return len_utf16(self._rt_peer())

    def patches_since(self, mark) -> list:
        return patches_since_utf16(self._rt_peer(), mark)

    def text_at(self, mark, start: int = 0, end: int = None) -> str:
        """(one more device call: the translation of the two ends)"""
        doc = self._rt_peer()
        if end is None:
            end = len_utf16(doc, mark)
        return text_range_utf16(doc, start, end, mark).decode("utf-8")

    def _rt_anchors(self, positions, bias) -> list:
        """(one more device call: the translation of the positions)"""
        doc = self._rt_peer()
        return doc.anchors_at(from_utf16(doc, positions), bias)

    def resolve_many(self, anchors) -> list:
        """(one more device call: the translation of the resolved positions)"""
        doc = self._rt_peer()
        res = doc.resolve_anchors(anchors)
        known = [k for k, p in enumerate(res) if p[2] != crdt_hip.UNKNOWN]
        out = [None] * len(res)
        for k, u in zip(known, to_utf16(doc, [res[k][0] for k in known])):
            out[k] = int(u)
        return out

    def spans(self) -> tuple:
        """(one more device call: the translation of the spans' ends)"""
        doc = self._rt_peer()
        sp, pend = doc.spans([(f[0], f[1], f[2], f[3], op, f[4]) for op, f in sorted(self.formats.items())])
        ends = to_utf16(doc, [x[0] for x in sp] + [x[0] + x[1] for x in sp])
        n = len(sp)
        return [(int(ends[k]), int(ends[n + k] - ends[k]), sp[k][4]) for k in range(n)], pend

    def lines_of(self, positions) -> tuple:
        """(line, character) arrays of UTF-16 positions (lines_of_utf16: three device calls)."""
        return lines_of_utf16(self._rt_peer(), positions)
