#!/usr/bin/env python3
"""Timing of text windows on a device replica (crdt_hip_replica_text_at), beside the two paths a
caller without them takes to read the text now: the replica's full copy-back (Replica.merge) sliced
on the host, and the replica read back (encode_diff([])) into a host log whose text_at is called.

Setup as tools/anchor_time.py: the automerge-paper log on a replica, a mark, then `--edits` seeded
positional edits (default 10,000) applied as one wire update, so the mark lies that many edits
back; a second fork of the base under another agent is what the replica joins.  Timed, 1 warm-up
and the median of `--reps` (default 9, at least 7), for windows of 4,096 and 65,536 codepoints from
the middle of the version and for the whole version, now and at the mark: wall time of the one ABI
call through the binding, with a buffer of the exact size, and the summed device time of the call's own kernels (HIP events,
crdt_hip_text_stats; the order update is not in it):
  up_to_date    a replica whose kept order is up to date
  after_join    the same calls right after the replica joined the other fork: the device call pays
                the full ORDER-mode merge that rebuilds the kept order
A version at a mark has no baseline: without the call the caller must have saved the text when it
took the mark; the host twin's own text_at (a log kept beside the replica) is timed instead.  Every
device result is checked byte for byte against the host log's.  Reported, not gated: prints one
JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crdt-benches_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crdt_hip  # noqa: E402
from anchor_time import readback  # noqa: E402
from join_time import fork  # noqa: E402

WINDOWS = (4096, 65536, None)      # codepoints (None: the whole version)


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def us(xs):
    return round(statistics.median(xs[1:]) / 1e3, 2)


def exact(ctx, rep, mark, a, b, nbytes):
    """Replica.text_at with a buffer of the exact size: one ABI call, no sizing round."""
    call = lambda *x: crdt_hip.lib().crdt_hip_replica_text_at(ctx._h, rep._h, *x)  # noqa: E731
    return crdt_hip._text_get(call, mark, a, b, False, ctx._h, guess=nbytes)[0]


def measure(ctx, make, sync, host, hmark, reps):
    """make(): (a fresh replica in the state to measure, its mark or None).  sync(rep): waits for
    what made it.  host, hmark: the log that holds the same items, and its mark."""
    out = {}
    total = host.text_info(hmark)["len"]
    for w in WINDOWS:
        a = 0 if w is None else max(0, total // 2 - w // 2)
        b = None if w is None else min(total, a + w)
        want = host.text_at(hmark, a, b)
        info = host.text_info(hmark, a, b)
        wall, dev_ns, tiles, merge_slice, host_path, twin_call = [], [], [], [], [], []
        for _ in range(reps + 1):
            rep, mark = make()
            sync(rep)
            t0 = time.perf_counter()
            got = exact(ctx, rep, mark, a, b, info["n_bytes"])
            wall.append(time.perf_counter() - t0)
            s = ctx.text_stats()
            dev_ns.append(s["device_ns"])
            tiles.append(s["tiles_written"])
            assert got == want, "the device window differs from the host's"
            assert rep.text_info(mark, a, b) == info
            rep.close()
            t0 = time.perf_counter()
            assert host.text_at(hmark, a, b) == want
            twin_call.append(time.perf_counter() - t0)
            if hmark is not None:
                continue
            rep, _ = make()
            sync(rep)
            t0 = time.perf_counter()
            data = rep.merge()[0]
            sl = data[info["start_bytes"]: info["start_bytes"] + info["n_bytes"]]
            merge_slice.append(time.perf_counter() - t0)
            assert sl == want
            rep.close()
            rep, _ = make()
            sync(rep)
            t0 = time.perf_counter()
            ref = readback(rep).text_at(None, a, b)
            host_path.append(time.perf_counter() - t0)
            assert ref == want
            rep.close()
        row = {"codepoints": info["n"], "bytes": info["n_bytes"], "tiles_written": tiles[-1],
               "device_ms_median": ms(wall), "device_kernels_us_median": us(dev_ns),
               "host_twin_ms_median": ms(twin_call)}
        if hmark is None:
            row["merge_and_slice_ms_median"] = ms(merge_slice)
            row["readback_host_ms_median"] = ms(host_path)
        out["whole" if w is None else str(w)] = row
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

    # a mark belongs to the replica it was taken from, so every fresh replica is built the same way:
    # a clone of the base, its mark, then the edits as one wire update
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

    # (the host twin of the joined state: the same mark point, the base, then the join)
    jhost = base.clone()
    jhmark = jhost.mark()
    jhost.apply_update(update)
    jhost.join(b)

    out = {"trace": args.trace, "edits_since_mark": args.edits, "reps": reps,
           "items": host.view().n, "items_after_join": jhost.view().n,
           "up_to_date": {}, "after_join": {}}
    now = lambda f: (lambda: (f()[0], None))  # noqa: E731
    out["up_to_date"]["now"] = measure(ctx, now(fresh), lambda r: r.merge_inc(), host, None, reps)
    out["up_to_date"]["at_mark"] = measure(ctx, fresh, lambda r: r.merge_inc(), host, hmark, reps)
    out["after_join"]["now"] = measure(ctx, now(fresh_joined), lambda r: r.merge_digest(), jhost,
                                       None, reps)
    out["after_join"]["at_mark"] = measure(ctx, fresh_joined, lambda r: r.merge_digest(), jhost,
                                           jhmark, reps)
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
