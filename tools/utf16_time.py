#!/usr/bin/env python3
"""Timing of the UTF-16 positions on a device replica (crdt_hip_replica_units_of and the *_utf16
edits and patches, crdt_hip_utf16.h), beside what a caller without them does to turn UTF-16 code
units into the library's units: the replica's full copy-back (Replica.merge) followed by a numpy
decode of the UTF-8 lead bytes and a cumulative count.

Setup as tools/line_time.py: the automerge-paper log on a replica, a mark, then `--edits` seeded
positional edits (default 10,000) applied as one wire update, so the mark lies that many edits back;
a second fork of the base under another agent is what the replica joins.  Timed, 1 warm-up and the
median of `--reps` (default 9, at least 7): wall time of the call through the binding, and the
summed device time of the translation's own kernels (HIP events, crdt_hip_unit_stats; the order
update is not in it; for an edit or patches_since the kernels of the translation inside the call):
  units_of          1, 64 and 4,096 seeded UTF-16 positions, now
  keystroke         one replace of one character in the middle, in UTF-16, in codepoints, in bytes
  patch_set         8,396 seeded one-character patches as one call, in UTF-16, codepoints, bytes
  patches_since     the patches since the mark, in UTF-16, in codepoints, in bytes
each on a replica whose kept order is up to date (`up_to_date`); units_of also right after the
replica joined the other fork (`after_join`: the device call pays the full ORDER-mode merge that
rebuilds the kept order).  The baseline answers the same positions from the copied-back text:
widths from the lead bytes, two cumulative sums and a searchsorted.  Every device result is checked
against the host log's.  Reported, not gated: prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crdt-benches_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crdt_hip  # noqa: E402
import crdt_hip_utf16 as cu  # noqa: E402
from join_time import fork  # noqa: E402

COUNTS = (1, 64, 4096)
PATCHES = 8396


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def us(xs):
    return round(statistics.median(xs[1:]) / 1e3, 2)


def decode_count(data: bytes) -> tuple:
    """(code units before each codepoint gap, bytes before each gap) of UTF-8 text, by numpy."""
    arr = np.frombuffer(data, np.uint8)
    lead = arr[(arr & 0xC0) != 0x80]
    width = 1 + (lead >= 0xC0) + (lead >= 0xE0) + (lead >= 0xF0)
    u16 = np.concatenate([[0], np.cumsum(1 + (lead >= 0xF0))]).astype(np.uint64)
    return u16, np.concatenate([[0], np.cumsum(width)]).astype(np.uint64)


def copy_back_units(rep, q) -> np.ndarray:
    """The codepoint gap of each UTF-16 position, from the copied-back text."""
    u16, _ = decode_count(rep.merge()[0])
    return np.searchsorted(u16, q).astype(np.uint64)


def timed(reps, make, sync, call, check, baseline=None, stats=True):
    wall, dev, base = [], [], []
    for _ in range(reps + 1):
        rep, mark = make()
        sync(rep)
        t0 = time.perf_counter()
        got = call(rep, mark)
        wall.append(time.perf_counter() - t0)
        dev.append(cu.stats(rep.ctx)["device_ns"] if stats else 0)
        check(got, rep)
        rep.close()
        if baseline:
            rep, _ = make()
            sync(rep)
            t0 = time.perf_counter()
            check(baseline(rep), None)
            base.append(time.perf_counter() - t0)
            rep.close()
    row = {"device_ms_median": ms(wall)}
    if stats:
        row["unit_kernels_us_median"] = us(dev)
    if base:
        row["merge_and_count_ms_median"] = ms(base)
    return row


def units_cases(make, sync, host, reps) -> dict:
    out = {}
    rng = np.random.default_rng(7)
    info = cu.units_of(host, [], cu.UNIT_UTF16)[1]
    every = cu.to_utf16(host, np.arange(info["len"] + 1))
    for n in COUNTS:
        q = every[rng.integers(0, info["len"] + 1, n)]
        want = cu.units_of(host, q, cu.UNIT_UTF16)[0]["cp"]
        out[str(n)] = timed(
            reps, make, sync, lambda r, m: cu.units_of(r, q, cu.UNIT_UTF16)[0]["cp"],
            lambda got, r: np.array_equal(got, want) or sys.exit("units_of differ"),
            baseline=lambda r: copy_back_units(r, q))
    return out, info, every


def edit_cases(make, sync, host, hmark, info, every, reps) -> dict:
    """A keystroke, the patch set and patches_since, each in the three units."""
    out = {"keystroke": {}, "patch_set": {}, "patches_since": {}}
    mid = info["len"] // 2
    rec = cu.units_of(host, np.arange(info["len"] + 1), cu.UNIT_CODEPOINTS)[0]
    # one-character patches at ascending, non-touching gaps: delete one character, type "x"
    gaps = np.sort(np.random.default_rng(11).choice(info["len"] // 3, PATCHES, replace=False)) * 3
    units = {"utf16": ("utf16", cu.apply_patches_utf16, cu.patches_since_utf16_raw),
             "codepoints": ("cp", lambda r, p, i: r.apply_patches(p, i), lambda r, m: r.patches_since_raw(m)),
             "bytes": ("bytes", lambda r, p, i: r.apply_patches_bytes(p, i), lambda r, m: r.patches_since_bytes_raw(m))}
    for name, (field, apply, since) in units.items():
        pos = rec[field]
        one = np.zeros(1, crdt_hip.PATCH_DTYPE)
        one[0] = (pos[mid], 0, pos[mid + 1] - pos[mid], 1)
        arr = np.zeros(PATCHES, crdt_hip.PATCH_DTYPE)
        dele = pos[gaps + 1] - pos[gaps]
        shift = np.concatenate([[0], np.cumsum(1 - dele.astype(np.int64))[:-1]])
        arr["pos"], arr["ins_off"], arr["del"], arr["ins_len"] = pos[gaps].astype(np.int64) + shift, np.arange(PATCHES), dele, 1
        ins = b"x" * PATCHES
        ok = lambda got, r: got == (1, 1) or sys.exit("keystroke differs")  # noqa: E731
        out["keystroke"][name] = timed(reps, make, sync, lambda r, m: apply(r, one, b"x"), ok, stats=name == "utf16")
        okset = lambda got, r: got == (PATCHES, PATCHES) or sys.exit("patch set differs")  # noqa: E731
        out["patch_set"][name] = timed(reps, make, sync, lambda r, m: apply(r, arr, ins), okset, stats=name == "utf16")
        want = since(host, hmark)
        same = lambda got, r: (got[0].tobytes() == want[0].tobytes() and got[1] == want[1]) or sys.exit("patches differ")  # noqa: E731
        out["patches_since"][name] = dict(timed(reps, make, sync, lambda r, m: since(r, m), same, stats=name == "utf16"),
                                          patches=int(want[0].size))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default="automerge-paper")
    ap.add_argument("--edits", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    args = ap.parse_args()
    reps = max(7, args.reps)
    base = crdt_hip.Trace(os.path.join(ROOT, "traces", f"{args.trace}.json.gz")).resolve()
    a, b = fork(base, 1, 1001, args.edits), fork(base, 2, 2002, args.edits)
    update = a.encode_from(base.version())
    host = base.clone()
    hmark = host.mark()
    host.apply_update(update)
    ctx = crdt_hip.Context(0)
    r0, rb = crdt_hip.Replica(ctx, base), crdt_hip.Replica(ctx, b)

    def fresh():
        r = r0.clone()
        m = r.mark()
        r.apply_updates([update])
        r.merge_inc()  # (the kept order up to date, as in an editing session)
        return r, m

    def fresh_joined():
        r, m = fresh()
        r.join(rb)
        return r, m

    jhost = base.clone()
    jhost.apply_update(update)
    jhost.join(b)

    units, info, every = units_cases(fresh, lambda r: r.merge_inc(), host, reps)
    out = {"trace": args.trace, "edits_since_mark": args.edits, "reps": reps, "items": host.view().n,
           "items_after_join": jhost.view().n, **info,
           "up_to_date": dict(units_of=units, **edit_cases(fresh, lambda r: r.merge_inc(), host, hmark, info, every, reps)),
           "after_join": {"units_of": units_cases(fresh_joined, lambda r: r.merge_digest(), jhost, reps)[0]}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    r0.close()
    rb.close()
    ctx.close()


if __name__ == "__main__":
    main()
