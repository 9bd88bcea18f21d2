"""Shared helpers of test_bytes.py and test_gpu_bytes.py (test infrastructure only).

Byte offsets (include/crdt_hip.h, "byte offsets"): the translation of a sequential codepoint patch
list into UTF-8 byte offsets through a plain Python string model, the byte splice model, and the
rejected calls both files check.  Texts, patch generators and logs come from edit_util and
patch_util.
"""
from __future__ import annotations

import numpy as np

import crdt_hip
import edit_util as eu

EINVAL, ERANGE = -1, -2


def blen(s: str) -> int:
    return len(s.encode("utf-8"))


def to_bytes(text: str, plist) -> list:
    """The byte patch list of a sequential codepoint patch list over `text`: pos and del of every
    patch measured in the UTF-8 of the document as the earlier patches left it."""
    cur, out = text, []
    for pos, dele, ins in plist:
        assert pos + dele <= len(cur)
        out.append((blen(cur[:pos]), blen(cur[pos: pos + dele]), ins))
        cur = cur[:pos] + ins + cur[pos + dele:]
    return out


def apply_bytes(buf: bytes, plist_b) -> bytes:
    """The byte splice model: replace(pos..pos + del, ins) on a bytes buffer, patch after patch."""
    for pos, dele, ins in plist_b:
        assert pos + dele <= len(buf)
        buf = buf[:pos] + ins.encode("utf-8") + buf[pos + dele:]
    return buf


def counts(plist) -> tuple:
    """(items appended, items deleted) of a codepoint patch list."""
    return sum(len(i) for _, _, i in plist), sum(d for _, d, _ in plist)


def shifted(plist, by: int = 1) -> list:
    """A patch list over text[by:] as one over text: nothing before `by` is touched, so a
    multi-byte character placed there makes every byte position differ from its codepoint one."""
    return [(pos + by, dele, ins) for pos, dele, ins in plist]


def aeu(n: int) -> tuple:
    """`n` patches over 2 n + 1 ranks: the text "aé" * n + "a" loses every é for a €."""
    return "aé" * n + "a", [(2 * k + 1, 1, "€") for k in range(n)]


def raw(rows, ins: bytes = b"") -> tuple:
    return eu.raw(rows, ins)


def inside(text: str, ch: str) -> int:
    """Byte offset of the first `ch` of `text`."""
    return blen(text[: text.index(ch)])


def rejections(text: str) -> list:
    """(name, patch rows (pos, ins_off, del, ins_len) in bytes, ins, code) for a document `text`
    of at least 20 bytes that holds an é, a € and a 😀, in that order and not at its start: the
    byte forms of edit_util.rejections (the argument checks run before any boundary is looked at,
    so the same rows read in bytes give the same codes), then the boundary check."""
    nb = blen(text)
    e2, e3, e4 = inside(text, "é"), inside(text, "€"), inside(text, "😀")
    assert 0 < e2 < e3 < e4 and nb >= 20
    out = list(eu.rejections(nb))
    out += [(f"pos {k} bytes into a 😀", [(e4 + k, 0, 0, 1)], b"x", EINVAL) for k in (1, 2, 3)]
    out += [
        ("del ends inside an é", [(0, 0, e2 + 1, 0)], b"", EINVAL),
        ("del ends inside a €", [(e2, 0, e3 - e2 + 2, 0)], b"", EINVAL),
        ("del ends inside a 😀", [(e3, 0, e4 - e3 + 3, 0)], b"", EINVAL),
        ("del starts inside a €", [(e3 + 1, 0, 2, 0)], b"", EINVAL),
        # nothing of a valid patch 0 may stick
        ("patch 1 inside a 😀", [(0, 0, 0, 1), (e4 + 1 + 2, 1, 1, 0)], b"xy", EINVAL),
        # an argument error in a later patch wins over a boundary error in an earlier one
        ("boundary, then del past the end", [(e2 + 1, 0, 0, 1), (nb, 0, 3, 0)], b"x", ERANGE),
        ("boundary, then empty patch", [(e4 + 2, 0, 1, 0), (nb - 1, 0, 0, 0)], b"", EINVAL),
    ]
    return out


def as_u8(buf: bytes) -> np.ndarray:
    return np.frombuffer(buf, np.uint8)


def replay(trace: crdt_hip.Trace, log: crdt_hip.OpLog, first: int, last: int) -> None:
    """Patches [first, last) of a codepoint trace, one OpLog.replace each."""
    for i in range(first, last):
        pos, dele, ins = trace.patch(i)
        log.replace(pos, pos + dele, ins)


# The two windows of rustcode in which byte and codepoint offsets differ: patch 4400 inserts a ÷,
# patch 4401 deletes 1 codepoint = 2 bytes, patch 6233 deletes 8 codepoints = 9 bytes.
RUSTCODE_WINDOWS = [(4390, 4410, 4401), (6225, 6240, 6233)]
