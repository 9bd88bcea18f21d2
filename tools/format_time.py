#!/usr/bin/env python3
"""Timing of formats on a device replica (crdt_hip_replica_spans), beside the path a caller without
it takes: read the replica back and flatten on a host log.

Setup as tools/anchor_time.py: two forks of the automerge-paper log, `--edits` seeded positional
edits each (default 10,000), under distinct agents.  Timed, 1 warm-up and the median of `--reps`
(default 9, at least 7), at 16, 256 and 4,096 formats, wall time of the calls named and, for the
device call, the summed device time of the call's own kernels (HIP events, crdt_hip_format_stats;
the order update is not in it):
  up_to_date    a replica of fork A whose kept order is up to date (right after a merge_inc)
      device              Replica.spans_raw
      host path           the replica read back (encode_diff([])) into an empty host log
                          (apply_diff), then OpLog.spans_raw on it
  after_join    the same calls right after the replica joined fork B: the device call pays the full
                ORDER-mode merge that rebuilds the kept order
The formats are ranges between seeded random gaps of fork A (either bias at either end) over 8
keys, one in five a REMOVE.  `count_probe_us` is the kernel time of a call with as many formats
whose anchors name items nobody holds: the count, the table and the probe run in full and there is
no boundary, so it estimates the part of the kernel time that does not depend on the segments; the
rest of `device_kernels_us` is the boundary, attribute and span passes.  Every device result is
checked byte for byte against the host log's.  Reported, not gated: prints one JSON line (and
writes it to --out).
"""
import argparse
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

SIZES = (16, 256, 4096)


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def us(xs):
    return round(statistics.median(xs[1:]) / 1e3, 2)


def readback(rep, fugue=False):
    """What a caller has to do without the device call: the whole log back to the host."""
    host = crdt_hip.OpLog(fugue=fugue)
    host.apply_diff(rep.encode_diff([]))
    return host


def formats_of(host_log, m, seed):
    rng = random.Random(seed)
    n = host_log.visible_len()
    ends = [sorted((rng.randint(0, n), rng.randint(0, n))) for _ in range(m)]
    pos = [p for pair in ends for p in pair]
    anchors = host_log.anchors_at_raw(pos, [rng.choice([0, 1]) for _ in pos])
    f = np.zeros(m, crdt_hip.FORMAT_DTYPE)
    f["start"], f["end"] = anchors[0::2], anchors[1::2]
    f["op"] = [((k + 1) << 16) | (k % 3) for k in range(m)]
    f["key"] = [rng.randrange(8) for _ in range(m)]
    f["value"] = [rng.randrange(4) for _ in range(m)]
    f["flags"] = [crdt_hip.REMOVE if rng.random() < 0.2 else 0 for _ in range(m)]
    absent = f.copy()
    absent["start"]["id"] = [(k + 1) << 16 | 0x7777 for k in range(m)]
    return f, absent


def measure(ctx, make, sync, host_log, m, reps, seed):
    """make(): a fresh replica in the state to measure.  sync(rep): waits for what made it."""
    f, absent = formats_of(host_log, m, seed)
    wall, dev_ns, host, probe_ns = [], [], [], []
    stats = {}
    for _ in range(reps + 1):
        rep = make()
        sync(rep)
        t0 = time.perf_counter()
        got = rep.spans_raw(f)
        wall.append(time.perf_counter() - t0)
        stats = ctx.format_stats()
        dev_ns.append(stats["device_ns"])
        assert rep.spans_raw(absent)[2] == m
        probe_ns.append(ctx.format_stats()["device_ns"])
        rep.close()
        rep = make()
        sync(rep)
        t0 = time.perf_counter()
        ref = readback(rep).spans_raw(f)
        host.append(time.perf_counter() - t0)
        rep.close()
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and \
            got[2] == ref[2], "the device spans differ from the host's"
    return {"device_ms_median": ms(wall), "device_kernels_us_median": us(dev_ns),
            "count_probe_us_median": us(probe_ns), "host_path_ms_median": ms(host),
            "segments": stats["segments"], "spans": stats["spans"], "attrs": int(len(got[1]))}


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
