#!/usr/bin/env python3
"""Delta-sync timing (state_vector + encode_diff + apply_diff, on the host and on the device),
beside the whole-state join of the same pair.

Setup as tools/join_time.py: two forks of the automerge-paper log, `--edits` seeded positional
edits each (default 10,000), under distinct agents.  A third fork is the second plus `--more`
further edits (default 100).  Two cases:
  forks    dst = fork A, src = fork B: the peers diverged by 10,000 edits each
  plus100  dst already holds fork B, src = fork B + 100 edits: a small delta into a large log
Each repetition syncs src into a fresh clone of dst: wall time around the three ABI calls (the
clone is made, and on the device waited for, outside the timed region), 1 warm-up, median of
`--reps` (default 9, at least 7).  Per case: the delta's bytes, the host and device wall times, the
summed device time of the encode and apply kernels (HIP events, crdt_hip_delta_stats), the join's
wall time on the same pair, and the bytes a join moves (src's whole log in the delta's wire form:
a delta against the empty vector).  Every device result is checked against the host's.  Reported,
not gated: prints one JSON line (and writes it to --out).
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
from join_time import fork  # noqa: E402


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def case(ctx, dst, src, reps):
    out = {"dst_items": dst.view().n, "src_items": src.view().n}
    host, host_join = [], []
    for _ in range(reps + 1):
        d = dst.clone()
        t0 = time.perf_counter()
        delta = src.encode_diff(d.state_vector())
        got = d.apply_diff(delta)
        host.append(time.perf_counter() - t0)
        j = dst.clone()
        t0 = time.perf_counter()
        jgot = j.join(src)
        host_join.append(time.perf_counter() - t0)
        assert jgot == got and j.view().n == d.view().n
    whole = d.encode_diff([])
    assert whole == j.encode_diff([]), "host delta sync differs from the host join"
    rd, rs = crdt_hip.Replica(ctx, dst), crdt_hip.Replica(ctx, src)
    dev, dev_ns, dev_join, join_ns = [], [], [], []
    for _ in range(reps + 1):
        r = rd.clone()
        r.merge_digest()  # (waits for the clone)
        t0 = time.perf_counter()
        ddelta = rs.encode_diff(r.state_vector())
        enc_ns = ctx.delta_stats()["device_ns"]
        dgot = r.apply_diff(ddelta)
        dev.append(time.perf_counter() - t0)
        st = ctx.delta_stats()
        dev_ns.append(enc_ns + st["device_ns"])
        assert ddelta == delta and dgot == got
        assert r.encode_diff([]) == whole, "device delta sync differs from the host's"
        r.close()
        r = rd.clone()
        r.merge_digest()
        t0 = time.perf_counter()
        jgot = r.join(rs)
        dev_join.append(time.perf_counter() - t0)
        join_ns.append(ctx.join_stats()["device_ns"])
        assert jgot == got
        r.close()
    rd.close()
    rs.close()
    out.update({
        "added": got[0], "tombstoned": got[1],
        "delta_bytes": len(delta), "delta_items": st["items"], "delta_ranges": st["ranges"],
        "join_bytes": len(src.encode_diff([])),
        "host_delta_ms_median": ms(host), "host_join_ms_median": ms(host_join),
        "device_delta_ms_median": ms(dev), "device_join_ms_median": ms(dev_join),
        "device_delta_kernels_us_median": round(statistics.median(dev_ns[1:]) / 1e3, 2),
        "device_join_kernels_us_median": round(statistics.median(join_ns[1:]) / 1e3, 2),
        "apply_table_slots": st["table_slots"],
    })
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default="automerge-paper")
    ap.add_argument("--edits", type=int, default=10000)
    ap.add_argument("--more", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    args = ap.parse_args()
    reps = max(7, args.reps)
    base = crdt_hip.Trace(os.path.join(ROOT, "traces", f"{args.trace}.json.gz")).resolve()
    a, b = fork(base, 1, 1001, args.edits), fork(base, 2, 2002, args.edits)
    b3 = fork(b, 2, 3003, args.more)
    ctx = crdt_hip.Context(0)
    out = {"trace": args.trace, "edits_per_fork": args.edits, "more_edits": args.more, "reps": reps,
           "base_items": base.view().n,
           "forks": case(ctx, a, b, reps), "plus100": case(ctx, b, b3, reps)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
