"""The line index of libcrdt_hip.so (include/crdt_hip_lines.h): line numbers -> line starts, and
positions -> (line, column), on an OpLog (the definition) and on a device Replica (HIP kernels,
csrc/lines.hip), now or at a mark.

An extension beside the crdt_hip package, not a part of it: it takes the library handle from
crdt_hip.lib(), sets the argument types of its own five functions and adds no name to the package
or to its classes.  `obj` is an OpLog or a Replica; a HipMerge, HipDownstream or HipDownstreamBytes
is unwrapped to the document it holds (queued updates decoded first).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import crdt_hip

LINE_POS_DTYPE = np.dtype([("line", "<u8"), ("start", "<u8"), ("start_bytes", "<u8"), ("col", "<u8"),
                           ("col_bytes", "<u8")])


class LineInfo(C.Structure):
    """crdt_hip_line_info: lines, codepoints and UTF-8 bytes of the whole version."""
    _fields_ = [("lines", C.c_uint64), ("len", C.c_uint64), ("len_bytes", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert LINE_POS_DTYPE.itemsize == 40 and C.sizeof(LineInfo) == 24

_P, _U64 = C.c_void_p, C.POINTER(C.c_uint64)
_SIG = {
    "crdt_hip_oplog_line_starts": (C.c_int, [_P, _P, _P, C.c_size_t, _P, _P]),
    "crdt_hip_oplog_lines_of": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, _P, _P]),
    "crdt_hip_replica_line_starts": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, _P]),
    "crdt_hip_replica_lines_of": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, _P]),
    "crdt_hip_line_stats": (C.c_int, [_P, _U64, _U64, _U64]),
}
EXPORTS = list(_SIG)
_BOUND = False


def lib() -> C.CDLL:
    """crdt_hip.lib() with the signatures of the five functions of crdt_hip_lines.h set."""
    global _BOUND
    L = crdt_hip.lib()
    if not _BOUND:
        for name, (res, args) in _SIG.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _BOUND = True
    return L


def _document(obj):
    """(the OpLog or Replica behind obj, the handles its calls start with, its error context)."""
    if isinstance(obj, crdt_hip._Adapter):
        obj = obj._rt_peer()
    if isinstance(obj, crdt_hip.Replica):
        return obj, "crdt_hip_replica_", (obj.ctx._h, obj._h), obj.ctx._h
    if isinstance(obj, crdt_hip.OpLog):
        return obj, "crdt_hip_oplog_", (obj._h,), None
    raise TypeError(f"not an OpLog, a Replica or an adapter of one: {type(obj).__name__}")


def _call(obj, name: str, queries, mark, flags=None, out=None) -> tuple:
    doc, prefix, lead, ectx = _document(obj)
    q = np.ascontiguousarray(queries, dtype=np.uint64).reshape(-1)
    if out is None:
        out = np.zeros(q.size, LINE_POS_DTYPE)
    assert out.dtype == LINE_POS_DTYPE and out.size == q.size
    info = LineInfo()
    args = lead + (mark._h if mark is not None else None, q.ctypes.data if q.size else None, q.size)
    if flags is not None:
        args += (flags,)
    rc = getattr(lib(), prefix + name)(*args, out.ctypes.data if out.size else None, C.byref(info))
    crdt_hip._check(rc, ectx)
    return out, info.as_dict()


def line_starts(obj, lines, mark=None, out=None) -> tuple:
    """Where the lines `lines` (0-based, any order, repeats allowed, each in [0, L + 1]) of the
    version now (`mark` None) or at `mark` start -> (array of LINE_POS_DTYPE, {"lines", "len",
    "len_bytes"}).  Line L + 1 is the end of the version, so start(k) .. start(k + 1) is line k with
    its line break.  `out`: an array to write into (a failed call leaves it untouched)."""
    return _call(obj, "line_starts", lines, mark, out=out)


def lines_of(obj, positions, mark=None, bytes: bool = False, out=None) -> tuple:
    """Line, line start and column of the gap positions `positions`, in codepoints or, with
    `bytes`, in UTF-8 bytes -> (array of LINE_POS_DTYPE, info).  The gap right after a line break
    is column 0 of the next line."""
    return _call(obj, "lines_of", positions, mark, crdt_hip.TEXT_BYTES if bytes else 0, out=out)


def line_count(obj, mark=None) -> int:
    """Lines of the version: its line breaks + 1."""
    return line_starts(obj, [], mark)[1]["lines"]


def text_lines(obj, first: int, count: int, mark=None) -> bytes:
    """The UTF-8 of lines first .. first + count of the version, line breaks included, clipped to
    the version: line_starts of the two ends, then text_at of that byte window (a replica gets only
    the window back)."""
    if first < 0 or count < 0:
        raise ValueError("negative line number or count")
    doc = _document(obj)[0]
    try:
        s = line_starts(doc, [first, first + count], mark)[0]
    except crdt_hip.CrdtHipError as e:  # beyond the version: clip to its L + 1 lines
        if e.code != -2:
            raise
        end = line_count(doc, mark)
        s = line_starts(doc, [min(first, end), min(first + count, end)], mark)[0]
    return doc.text_at(mark, int(s["start_bytes"][0]), int(s["start_bytes"][1]), bytes=True)


def stats(ctx) -> dict:
    """What the context's last device line_starts / lines_of observed (crdt_hip_line_stats)."""
    v = [C.c_uint64() for _ in range(3)]
    crdt_hip._check(lib().crdt_hip_line_stats(ctx._h, *map(C.byref, v)), ctx._h)
    return dict(zip(("queries", "ranks", "device_ns"), (int(x.value) for x in v)))
