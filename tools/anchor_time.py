#!/usr/bin/env python3
"""Timing of anchors on a device replica (crdt_hip_replica_anchors_at / _resolve), beside the path
a caller without them takes: read the replica back and resolve on a host log.

Setup as tools/edit_time.py: two forks of the automerge-paper log, `--edits` seeded positional
edits each (default 10,000), under distinct agents.  Timed, 1 warm-up and the median of `--reps`
(default 9, at least 7), at 1, 64 and 4,096 anchors, wall time of the calls named and, for the
device calls, the summed device time of the call's own kernels (HIP events, crdt_hip_anchor_stats;
the order update is not in it):
  up_to_date    a replica of fork A whose kept order is up to date
      resolve / create    Replica.resolve_anchors_raw / Replica.anchors_at_raw
      host path           the replica read back (encode_diff([])) into an empty host log
                          (apply_diff), then OpLog.resolve_anchors_raw on it
  after_join    the same calls right after the replica joined fork B: the device call pays the full
                ORDER-mode merge that rebuilds the kept order
The anchors are made at seeded random gaps of fork A (both biases).  Every device result is checked
byte for byte against the host log's.  Reported, not gated: prints one JSON line (and writes it to
--out).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crdt-benches_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crdt_hip  # noqa: E402
from join_time import fork  # noqa: E402

SIZES = (1, 64, 4096)


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def us(xs):
    return round(statistics.median(xs[1:]) / 1e3, 2)


def readback(rep, fugue=False):
    """What a caller has to do without the device calls: the whole log back to the host."""
    host = crdt_hip.OpLog(fugue=fugue)
    host.apply_diff(rep.encode_diff([]))
    return host


def measure(ctx, make, sync, host_log, m, reps, seed):
    """make(): a fresh replica in the state to measure.  sync(rep): waits for what made it."""
    rng = random.Random(seed)
    n = host_log.visible_len()
    pos = [rng.randint(0, n) for _ in range(m)]
    bias = [rng.choice([0, 1]) for _ in range(m)]
    anchors = host_log.anchors_at_raw(pos, bias)
    out = {}
    for what in ("resolve", "create"):
        wall, dev_ns, host = [], [], []
        for _ in range(reps + 1):
            rep = make()
            sync(rep)
            t0 = time.perf_counter()
            got = rep.resolve_anchors_raw(anchors) if what == "resolve" else rep.anchors_at_raw(pos, bias)
            wall.append(time.perf_counter() - t0)
            dev_ns.append(ctx.anchor_stats()["device_ns"])
            rep.close()
            rep = make()
            sync(rep)
            t0 = time.perf_counter()
            twin = readback(rep)
            ref = twin.resolve_anchors_raw(anchors) if what == "resolve" else twin.anchors_at_raw(pos, bias)
            host.append(time.perf_counter() - t0)
            rep.close()
            assert got.tobytes() == ref.tobytes(), "the device anchors differ from the host's"
        out[what] = {"device_ms_median": ms(wall), "device_kernels_us_median": us(dev_ns),
                     "host_path_ms_median": ms(host)}
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
    joined = a.clone()
    joined.join(b)
    ctx = crdt_hip.Context(0)
    ra, rb = crdt_hip.Replica(ctx, a), crdt_hip.Replica(ctx, b)
    ra.merge_inc()

    def fresh():
        r = ra.clone()
        r.merge_inc()  # (the kept order up to date, as in an editing session)
        return r

    def fresh_joined():
        r = fresh()
        r.join(rb)
        return r

    out = {"trace": args.trace, "edits_per_fork": args.edits, "reps": reps,
           "items": a.view().n, "items_after_join": joined.view().n,
           "up_to_date": {}, "after_join": {}}
    for m in SIZES:
        out["up_to_date"][str(m)] = measure(ctx, fresh, lambda r: r.merge_inc(), a, m, reps, 7 + m)
        out["after_join"][str(m)] = measure(ctx, fresh_joined, lambda r: r.merge_digest(), joined, m,
                                            reps, 9 + m)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ra.close()
    rb.close()
    ctx.close()


if __name__ == "__main__":
    main()
