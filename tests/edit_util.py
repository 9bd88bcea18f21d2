"""Shared helpers of test_edit.py and test_gpu_edit.py (test infrastructure only).

Local edits as positional patches (include/crdt_hip.h, "local edits"): a plain Python string model
of a document, generators of non-touching patch sets, and the definition of the result, one
OpLog.replace per patch.  Logs and forks come from join_util, join_fugue_util and patch_util.
"""
from __future__ import annotations

import random

import numpy as np

import crdt_hip
import join_util as ju
import patch_util as pu

KINDS = ["rga", "fugue"]
ALPHABET = "abcdefghij klmnop\nqrstuvwxyzé€😀ßж"   # 1- to 4-byte characters


def text_of(rng: random.Random, k: int) -> str:
    return "".join(rng.choice(ALPHABET) for _ in range(k))


def replace_loop(log: crdt_hip.OpLog, plist) -> None:
    """The definition: crdt_hip_oplog_replace once per patch, in order."""
    for pos, dele, ins in plist:
        log.replace(pos, pos + dele, ins)


def model_apply(text: str, plist) -> str:
    return pu.apply_patches(text, plist)


def same_logs(a: crdt_hip.OpLog, b: crdt_hip.OpLog) -> None:
    """Two host logs hold the same log slot for slot, every column, and the same delete ops."""
    A, B = a.arrays(), b.arrays()
    assert A.n == B.n
    for f in ("parent", "lamport", "agent", "deleted", "cp", "origin_right"):
        assert np.array_equal(getattr(A, f), getattr(B, f)), f
    assert (A.side is None) == (B.side is None)
    if A.side is not None:
        assert np.array_equal(A.side, B.side)
    assert a.version() == b.version() and a.visible_len() == b.visible_len()
    assert a.encode_from(0) == b.encode_from(0)
    assert a.encode_diff([]) == b.encode_diff([])


def random_patches(rng: random.Random, length: int, count: int, max_gap: int = 40) -> list:
    """Up to `count` ascending, non-touching patches over a document of `length` codepoints, in the
    patches_since convention (pos counted in the document as the earlier patches left it): deletes,
    inserts of 1- to 4-byte text and replaces, the first sometimes at position 0 and the last
    sometimes reaching the end of the document."""
    out, old, shift = [], 0, 0
    for k in range(count):
        gap = rng.randint(0 if k == 0 else 1, max_gap)
        start = old + gap
        if start > length:
            break
        kind = rng.random()
        dele = 0 if kind < 0.4 else min(length - start, rng.choice([1, 1, 2, 3, 7, 30]))
        ins = "" if 0.4 <= kind < 0.7 and dele else text_of(rng, rng.choice([1, 1, 2, 5, 12]))
        if rng.random() < 0.1:
            dele = length - start                      # to the end of the document
        if not dele and not ins:
            ins = "z"
        out.append((start + shift, dele, ins))
        shift += len(ins) - dele
        old = start + dele
    pu.assert_never_touch(out)
    return out


def interleaved(n: int) -> tuple:
    """`n` patches over 2 n + 1 ranks: delete 1, insert 1, keep 1, repeated (the text "ab" * n +
    "a" loses every b for an X).  Returns (text, patches)."""
    return "ab" * n + "a", [(2 * k + 1, 1, "X") for k in range(n)]


def two_agent_log(fugue: bool, chars: int, seed: int, edits: int = 150) -> crdt_hip.OpLog:
    """A log of two agents' concurrent history with deletes: a typed base of `chars` characters,
    two forks that edit at random, joined."""
    rng = random.Random(seed)
    base = pu.new_log(fugue)
    base.insert(0, text_of(rng, chars))
    for _ in range(10):                                # dead stretches of the base
        a = rng.randint(0, base.visible_len() - 40)
        base.remove(a, a + rng.choice([1, 3, 30]))
    a, b = ju.fork(base, 1, seed + 1, edits), ju.fork(base, 2, seed + 2, edits)
    a.join(b)
    return a


# What every rejected call is checked with: (name, patches as (pos, ins_off, del, ins_len) rows,
# ins bytes, expected code), for a document of `n` visible codepoints (n >= 20).
def rejections(n: int) -> list:
    EINVAL, ERANGE = -1, -2
    return [
        ("touching", [(3, 0, 0, 2), (5, 2, 1, 0)], b"xy", EINVAL),         # pos[1] == pos[0] + 2
        ("touching deletes", [(3, 0, 2, 0), (3, 0, 1, 0)], b"", EINVAL),
        ("descending", [(9, 0, 1, 0), (4, 0, 1, 0)], b"", EINVAL),
        ("empty patch", [(2, 0, 1, 0), (6, 0, 0, 0)], b"", EINVAL),
        ("pos past the end", [(n + 1, 0, 0, 1)], b"x", ERANGE),
        ("del past the end", [(n - 2, 0, 3, 0)], b"", ERANGE),
        ("del past the end as left", [(0, 0, n, 0), (2, 0, 0, 1)], b"x", ERANGE),
        ("bad ins_off", [(1, 2, 0, 1)], b"xy", EINVAL),
        ("bad ins_off, far", [(1, 1 << 40, 0, 1)], b"xy", EINVAL),
        ("truncated UTF-8", [(1, 0, 0, 2)], "€".encode()[:2], EINVAL),
        ("truncated between pieces", [(1, 0, 0, 2), (9, 2, 0, 1)], "€".encode(), EINVAL),
        ("stray continuation byte", [(1, 0, 0, 1)], b"\x80", EINVAL),
        ("overlong form (5-byte lead)", [(1, 0, 0, 5)], b"\xf8\x88\x80\x80\x80", EINVAL),
    ]


def raw(rows, ins: bytes) -> tuple:
    arr = np.zeros(len(rows), crdt_hip.PATCH_DTYPE)
    for k, (pos, off, dele, ilen) in enumerate(rows):
        arr[k] = (pos, off, dele, ilen)
    return arr, ins
