"""Shared helpers of test_patches.py and test_gpu_patches.py (test infrastructure only).

A plain Python restatement of "patches since a mark" (include/crdt_hip.h), computed without the
product: from the arrays at the mark (item count, tombstones), the current LogArrays and the
document order the CPU oracle gives for them.  Forks and logs come from join_util,
join_fugue_util and delta_util.
"""
from __future__ import annotations

import itertools

import numpy as np

import crdt_hip
import delta_util as du
import join_fugue_util as jf
import join_util as ju


def anchor(arrs: crdt_hip.LogArrays):
    return jf.to_anchor(arrs) if arrs.side is not None else ju.to_anchor(arrs)


def oracle_merge(oracle, arrs: crdt_hip.LogArrays) -> tuple:
    """(text: str, document order: item ids, tombstones included) by the CPU oracle."""
    if arrs.n == 0:
        return "", []
    merge = oracle.merge_fugue if arrs.side is not None else oracle.merge
    text, order = merge(anchor(arrs), want_order=True)
    order = [int(x) for x in order]
    assert sorted(order) == list(range(1, arrs.n + 1))
    return text.decode("utf-8"), order


class At:
    """What a test remembers beside a mark: the item count, the tombstones and the oracle's text."""

    def __init__(self, oracle, arrs: crdt_hip.LogArrays):
        self.n = arrs.n
        self.deleted = arrs.deleted.copy()
        self.text = oracle_merge(oracle, arrs)[0]


def patches(at: At, arrs: crdt_hip.LogArrays, order) -> list:
    """[(pos, del, ins)] by the definition: over the document order, an item is K (visible at the
    mark and now), D (visible at the mark, not now) or I (not visible at the mark, now); the rest
    are dropped, and every maximal run of non-K items is one patch at the number of visible items
    before it."""
    assert arrs.n >= at.n
    kinds = []
    for s in order:
        was = s <= at.n and not at.deleted[s - 1]
        now = not arrs.deleted[s - 1]
        if was or now:
            kinds.append(("K" if was and now else "D" if was else "I", chr(int(arrs.cp[s - 1]))))
    out, pos = [], 0
    for kept, run in itertools.groupby(kinds, key=lambda kc: kc[0] == "K"):
        run = list(run)
        if kept:
            pos += len(run)
            continue
        ins = "".join(c for k, c in run if k == "I")
        out.append((pos, sum(1 for k, _ in run if k == "D"), ins))
        pos += len(ins)
    return out


def apply_patches(text: str, plist) -> str:
    """Upstream::replace (rope.rs:21-32) on codepoints, patch after patch."""
    cps = list(text)
    for pos, dele, ins in plist:
        assert pos + dele <= len(cps)
        cps[pos: pos + dele] = list(ins)
    return "".join(cps)


def assert_never_touch(plist) -> None:
    for (p0, _, i0), (p1, _, _) in zip(plist, plist[1:]):
        assert p1 > p0 + len(i0)
    for _, dele, ins in plist:
        assert dele or ins


def assert_raw(raw) -> None:
    """The crdt_hip_patch array: ins_off ascends and the pieces are contiguous."""
    arr, ins = raw
    off = 0
    for p in arr:
        assert int(p["ins_off"]) == off
        off += int(p["ins_len"])
    assert off == len(ins)


def same_raw(a, b) -> bool:
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


def check(oracle, obj, mark, at: At, arrs: crdt_hip.LogArrays) -> list:
    """obj.patches_since(mark) against the restatement, applied to the text at the mark, and the
    never-touch rule.  `arrs`: the arrays `obj` holds now.  Returns the patches."""
    text, order = oracle_merge(oracle, arrs)
    raw = obj.patches_since_raw(mark)
    assert_raw(raw)
    got = crdt_hip._patch_list(raw)
    assert got == patches(at, arrs, order)
    assert apply_patches(at.text, got) == text
    assert_never_touch(got)
    return got


def replica_arrays(rep: crdt_hip.Replica, fugue: bool) -> crdt_hip.LogArrays:
    """A replica's log read back through a delta against the empty vector (identity-anchored:
    every item, in slot order)."""
    d = du.decode_diff(rep.encode_diff([]))
    slot = {k: i + 1 for i, k in enumerate(d["key"])}
    parent = [0 if pk == du.START else slot[pk] for pk in d["pkey"]]
    cpw = np.asarray(d["cp"], dtype=np.uint64)
    return crdt_hip.LogArrays(
        parent, [k >> 16 for k in d["key"]], [k & 0xFFFF for k in d["key"]],
        ((cpw & du.TOMB) != 0).astype(np.uint8), (cpw & 0x1FFFFF).astype(np.uint32),
        side=((cpw & du.SIDE) != 0).astype(np.uint8) if fugue else None)


def new_log(fugue: bool, agent: int = 0) -> crdt_hip.OpLog:
    return crdt_hip.OpLog(fugue=fugue, agent=agent)


def base_log(fugue: bool) -> crdt_hip.OpLog:
    return jf.base_log() if fugue else ju.base_log()
