"""Shared helpers of test_text.py and test_gpu_text.py (test infrastructure only).

A plain Python restatement of "text windows" (include/crdt_hip.h): a window of a version is a slice
of the version's text, by codepoints or by UTF-8 bytes on codepoint boundaries, and its
crdt_hip_text_info follows from the slice.  The version's text itself comes from the CPU oracle
(patch_util.oracle_merge) or from a recording made when the mark was taken.  `raw` is the C call
with a canary buffer, for the refusals.
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np

import crdt_hip

END = crdt_hip.TEXT_END
BYTES = crdt_hip.TEXT_BYTES
EINVAL, ERANGE, ESPACE = -1, -2, -6
CANARY = 0xA5
WIDE = "aé€😀"          # 1, 2, 3 and 4 UTF-8 bytes


def mixed_text(n: int, seed: int) -> str:
    """n codepoints, a seeded mix of the four UTF-8 widths (mostly ASCII, as text is)."""
    rng = random.Random(seed)
    return "".join(rng.choice("abcdefgh  \n" + WIDE) for _ in range(n))


def boundaries(text: str) -> list:
    """Byte offset of every codepoint boundary of `text`: len(text) + 1 ascending values."""
    out, b = [0], 0
    for ch in text:
        b += len(ch.encode("utf-8"))
        out.append(b)
    return out


def want_info(text: str, a: int, b: int, bd=None) -> dict:
    """crdt_hip_text_info of the codepoint window [a, b) of `text` (bd: its boundaries, if the
    caller has them)."""
    bd = bd or boundaries(text)
    return {"len": len(text), "len_bytes": bd[-1], "start": a, "start_bytes": bd[a], "n": b - a,
            "n_bytes": bd[b] - bd[a]}


def call_of(obj):
    """The C entry point bound to a log or a replica: f(mark handle, start, end, flags, out, cap,
    out_len, info) -> rc."""
    L = crdt_hip.lib()
    if isinstance(obj, crdt_hip.Replica):
        return lambda *a: L.crdt_hip_replica_text_at(obj.ctx._h, obj._h, *a)
    return lambda *a: L.crdt_hip_oplog_text_at(obj._h, *a)


def raw(obj, mark, start, end, flags, cap, null_out=False, null_len=False, info=True) -> tuple:
    """One C call with a buffer of exactly `cap` bytes filled with a canary, *out_len and *info
    preset to canaries too -> (rc, buffer bytes, out_len, info dict or None)."""
    buf = np.full(cap, CANARY, np.uint8)
    n = C.c_size_t(0xDEAD)
    inf = crdt_hip.TextInfo(*([0xDEAD] * 6))
    rc = call_of(obj)(mark._h if mark is not None else None, start, end, flags,
                      None if null_out or cap == 0 else buf.ctypes.data, cap,
                      None if null_len else C.byref(n), C.byref(inf) if info else None)
    return rc, buf.tobytes(), int(n.value), inf.as_dict() if info else None


UNTOUCHED = {k: 0xDEAD for k in ("len", "len_bytes", "start", "start_bytes", "n", "n_bytes")}


def assert_refused(obj, mark, start, end, flags, code, cap=64, **kw) -> None:
    """The call returns `code` and leaves out, *out_len and *info as they were."""
    rc, buf, n, inf = raw(obj, mark, start, end, flags, cap, **kw)
    assert rc == code, (rc, code, start, end, flags)
    assert buf == bytes([CANARY]) * cap
    assert n == 0xDEAD and inf == UNTOUCHED


def check_window(obj, mark, text: str, a: int, b: int, bd=None) -> None:
    """Window [a, b) of the version whose text is `text`, asked in codepoints and in bytes: the
    slice and all six fields of the info, both ways, and text_info alone."""
    bd = bd or boundaries(text)
    want = text[a:b].encode("utf-8")
    info = want_info(text, a, b, bd)
    assert obj.text_at(mark, a, b) == want
    assert obj.text_info(mark, a, b) == info
    assert obj.text_at(mark, bd[a], bd[b], bytes=True) == want
    assert obj.text_info(mark, bd[a], bd[b], bytes=True) == info
