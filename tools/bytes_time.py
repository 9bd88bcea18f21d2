#!/usr/bin/env python3
"""Timing of the byte-offset calls on a device replica (crdt_hip_replica_apply_patches_bytes /
_replace_bytes / _patches_since_bytes) beside their codepoint twins, on the same build.

Setup as tools/edit_time.py and tools/patch_time.py: two forks of the automerge-paper log,
`--edits` seeded positional edits each (default 10,000), under distinct agents; the patch set is
what fork A's patches_since reports after it joined fork B (about 8,400 patches), with every
patch's text re-drawn, codepoint for codepoint, from an alphabet of 1- to 4-byte characters, so
that the byte offsets differ from the codepoint ones.  Timed, 1 warm-up and the median of `--reps`
(default 9, at least 7; min and max beside it), wall time of the one call through the binding, and
the summed device time of the call's kernels (HIP events, crdt_hip_edit_stats /
crdt_hip_patch_stats; the translation kernels of the byte edit are in it, the order update is not):
  keystroke      one é typed into a replica of fork A whose kept order is up to date:
                 Replica.replace beside Replica.replace_bytes
  patch_set      the patch set applied to a replica of fork A, one call:
                 Replica.apply_patches beside Replica.apply_patches_bytes
  patches_since  after fork A's replica, marked, applied the patch set (outside the timed region):
                 crdt_hip_replica_patches_since beside _patches_since_bytes, buffers of exact size
The byte edit's log is checked against the codepoint edit's through encode_diff([]), the byte
patches against the host's.  Reported, not gated: prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crdt-benches_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crdt_hip  # noqa: E402
from join_time import fork  # noqa: E402

AGENT = 1  # fork A's
ALPHABET = "abcdefghij klmnop\nqrstuvwxyzé€😀ßж"


def stat(xs, scale, digits):
    xs = [x * scale for x in xs[1:]]
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits)}


def ms(xs):
    return stat(xs, 1e3, 4)


def us(xs):
    return stat(xs, 1e-3, 2)


def redraw(plist, seed: int) -> list:
    rng = random.Random(seed)
    return [(p, d, "".join(rng.choice(ALPHABET) for _ in s)) for p, d, s in plist]


def to_bytes(text: str, plist) -> list:
    """The byte form of an ascending, non-touching codepoint patch list over `text` (pos counted
    as the earlier patches left the document), through the byte offsets of the old text."""
    w = np.frombuffer(text.encode("utf-32-le"), np.uint32)
    w = 1 + (w >= 0x80) + (w >= 0x800) + (w >= 0x10000)
    pre = np.concatenate(([0], np.cumsum(w, dtype=np.int64)))
    out, shift, shift_b = [], 0, 0
    for pos, dele, ins in plist:
        old = pos - shift
        nb = len(ins.encode("utf-8"))
        db = int(pre[old + dele] - pre[old])
        out.append((int(pre[old]) + shift_b, db, ins))
        shift += len(ins) - dele
        shift_b += nb - db
    return out


def keystroke(ctx, a, text, reps):
    cp, cp_ns, by, by_ns = [], [], [], []
    rc, rb = crdt_hip.Replica(ctx, a), crdt_hip.Replica(ctx, a)
    for r in (rc, rb):
        r.set_agent(AGENT)
        r.merge_inc()
    pos = a.visible_len() // 2
    pos_b = len(text[:pos].encode("utf-8"))
    for i in range(reps + 1):
        t0 = time.perf_counter()
        rc.replace(pos + i, pos + i, "é")
        cp.append(time.perf_counter() - t0)
        cp_ns.append(ctx.edit_stats()["device_ns"])
        t0 = time.perf_counter()
        rb.replace_bytes(pos_b + 2 * i, pos_b + 2 * i, "é")
        by.append(time.perf_counter() - t0)
        by_ns.append(ctx.edit_stats()["device_ns"])
    assert rc.encode_diff([]) == rb.encode_diff([]), "the byte edit differs from the codepoint edit"
    out = {"items": a.view().n, "codepoint_ms": ms(cp), "codepoint_kernels_us": us(cp_ns),
           "bytes_ms": ms(by), "bytes_kernels_us": us(by_ns)}
    rc.close()
    rb.close()
    return out


def patch_set(ctx, a, plist, plist_b, reps):
    arr, ins = crdt_hip._patches_pack(plist)
    arr_b, ins_b = crdt_hip._patches_pack(plist_b)
    assert ins == ins_b and arr.tobytes() != arr_b.tobytes()
    rd = crdt_hip.Replica(ctx, a)
    rd.set_agent(AGENT)
    rd.merge_inc()
    cp, cp_ns, by, by_ns = [], [], [], []
    for _ in range(reps + 1):
        r, rb = rd.clone(), rd.clone()
        r.merge_inc()
        rb.merge_inc()
        t0 = time.perf_counter()
        r.apply_patches(arr, ins)
        cp.append(time.perf_counter() - t0)
        cp_ns.append(ctx.edit_stats()["device_ns"])
        t0 = time.perf_counter()
        rb.apply_patches_bytes(arr_b, ins_b)
        by.append(time.perf_counter() - t0)
        st = ctx.edit_stats()
        by_ns.append(st["device_ns"])
        assert r.encode_diff([]) == rb.encode_diff([]), "the byte edit differs from the codepoint edit"
        r.close()
        rb.close()
    rd.close()
    return {"items": st["ranks"], "patches": st["patches"], "inserted": st["items"],
            "deleted": st["tombstones"], "codepoint_ms": ms(cp), "codepoint_kernels_us": us(cp_ns),
            "bytes_ms": ms(by), "bytes_kernels_us": us(by_ns)}


def dev_patches(fn, rep, mark, n, nb):
    out = np.zeros(max(n, 1), crdt_hip.PATCH_DTYPE)
    ins = np.zeros(max(nb, 1), np.uint8)
    gn, gb = C.c_size_t(), C.c_size_t()
    rc = fn(rep.ctx._h, rep._h, mark._h, out.ctypes.data, n, C.byref(gn), ins.ctypes.data, nb,
            C.byref(gb))
    assert rc == 0 and (gn.value, gb.value) == (n, nb), (rc, gn.value, gb.value)
    return out[:n], ins[:nb].tobytes()


def patches_since(ctx, a, plist, reps):
    host = a.clone()
    hm = host.mark()
    host.apply_patches(plist)
    want, want_ins = host.patches_since_raw(hm)
    want_b, want_b_ins = host.patches_since_bytes_raw(hm)
    assert want_ins == want_b_ins and want.tobytes() != want_b.tobytes()
    L = crdt_hip.lib()
    rd = crdt_hip.Replica(ctx, a)
    rd.set_agent(AGENT)
    cp, cp_ns, by, by_ns = [], [], [], []
    for _ in range(reps + 1):
        r = rd.clone()
        m = r.mark()
        r.apply_patches(plist)
        r.merge_inc()  # (the kept order up to date: the calls below time their own kernels)
        t0 = time.perf_counter()
        got, got_ins = dev_patches(L.crdt_hip_replica_patches_since, r, m, len(want), len(want_ins))
        cp.append(time.perf_counter() - t0)
        cp_ns.append(ctx.patch_stats()["device_ns"])
        t0 = time.perf_counter()
        got_b, got_b_ins = dev_patches(L.crdt_hip_replica_patches_since_bytes, r, m, len(want_b),
                                       len(want_b_ins))
        by.append(time.perf_counter() - t0)
        st = ctx.patch_stats()
        by_ns.append(st["device_ns"])
        assert got.tobytes() == want.tobytes() and got_ins == want_ins
        assert got_b.tobytes() == want_b.tobytes() and got_b_ins == want_b_ins, \
            "device byte patches differ from the host's"
        m.close()
        r.close()
    rd.close()
    hm.close()
    return {"items": st["ranks"], "patches": len(want_b), "ins_bytes": len(want_b_ins),
            "codepoint_ms": ms(cp), "codepoint_kernels_us": us(cp_ns),
            "bytes_ms": ms(by), "bytes_kernels_us": us(by_ns)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default="automerge-paper")
    ap.add_argument("--edits", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    args = ap.parse_args()
    reps = max(7, args.reps)
    base = crdt_hip.Trace(os.path.join(ROOT, "traces", f"{args.trace}.json.gz")).resolve()
    a, b = fork(base, AGENT, 1001, args.edits), fork(base, 2, 2002, args.edits)
    seen = a.clone()
    m = seen.mark()
    seen.join(b)
    plist = redraw(seen.patches_since(m), 7)
    m.close()
    ctx = crdt_hip.Context(0)
    text = ctx.merge(a)[0].decode("utf-8")
    plist_b = to_bytes(text, plist)
    out = {"trace": args.trace, "edits_per_fork": args.edits, "reps": reps,
           "base_items": base.view().n,
           "keystroke": keystroke(ctx, a, text, reps),
           "patch_set": patch_set(ctx, a, plist, plist_b, reps),
           "patches_since": patches_since(ctx, a, plist, reps)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
