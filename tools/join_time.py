#!/usr/bin/env python3
"""Join timing (crdt_hip_oplog_join on the host, crdt_hip_replica_join on the device).

Two forks of the automerge-paper log, `--edits` seeded positional edits each (default 10,000),
made with the editing API under distinct agents.  Each repetition joins fork B into a fresh clone
of fork A: wall time around the ABI call alone (the clone is made, and on the device waited for,
outside the timed region), 1 warm-up, median of `--reps` (default 9, at least 7).  For the device
join also the summed device time of its kernels (HIP events, crdt_hip_join_stats), the common
prefix it found and the identity table's occupancy.  `--order fugue` resolves
the trace with Fugue anchors (a Fugue base, Fugue forks, Fugue replicas); everything else is the
same.  Reported, not gated: prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crdt-benches_amd"))
import crdt_hip  # noqa: E402

ALPHABET = "abcdefgh \n"


def fork(base, agent, seed, edits):
    f = base.clone()
    f.set_agent(agent)
    rng = random.Random(seed)
    for _ in range(edits):
        n = f.visible_len()
        if n == 0 or rng.random() < 0.6:
            f.insert(rng.randint(0, n), "".join(rng.choice(ALPHABET) for _ in range(rng.choice([1, 2, 6]))))
        else:
            a = rng.randint(0, n - 1)
            f.remove(a, min(n, a + rng.choice([1, 2, 4])))
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default="automerge-paper")
    ap.add_argument("--edits", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--order", choices=["rga", "fugue"], default="rga")
    ap.add_argument("--out")
    args = ap.parse_args()
    reps = max(7, args.reps)
    L = crdt_hip.lib()
    base = crdt_hip.Trace(os.path.join(ROOT, "traces", f"{args.trace}.json.gz")).resolve(
        fugue=args.order == "fugue")
    a, b = fork(base, 1, 1001, args.edits), fork(base, 2, 2002, args.edits)
    na, nb, n0 = a.view().n, b.view().n, base.view().n
    added, tomb = C.c_uint32(), C.c_uint32()

    host = []
    vb = b.view()
    for _ in range(reps + 1):
        d = a.clone()
        t0 = time.perf_counter()
        rc = L.crdt_hip_oplog_join(d._h, C.byref(vb), C.byref(added), C.byref(tomb))
        host.append(time.perf_counter() - t0)
        assert rc == 0, rc
    host_result = (added.value, tomb.value, d.view().n)

    ctx = crdt_hip.Context(0)
    ra, rb = crdt_hip.Replica(ctx, a), crdt_hip.Replica(ctx, b)
    want = crdt_hip.Replica(ctx, d).merge_digest()
    dev, dev_ns = [], []
    for _ in range(reps + 1):
        r = ra.clone()
        r.merge_digest()  # (waits for the clone)
        t0 = time.perf_counter()
        rc = L.crdt_hip_replica_join(ctx._h, r._h, rb._h, C.byref(added), C.byref(tomb))
        dev.append(time.perf_counter() - t0)
        assert rc == 0, rc
        st = ctx.join_stats()
        dev_ns.append(st["device_ns"])
        assert (added.value, tomb.value, r.info()[0]) == host_result
        assert r.merge_digest() == want, "device join differs from the host join"
        r.close()
    out = {
        "trace": args.trace, "order": args.order, "edits_per_fork": args.edits, "reps": reps,
        "base_items": n0, "dst_items": na, "src_items": nb,
        "added": host_result[0], "tombstoned": host_result[1], "joined_items": host_result[2],
        "host_join_ms_median": round(statistics.median(host[1:]) * 1e3, 4),
        "host_join_ms_min": round(min(host[1:]) * 1e3, 4),
        "device_join_ms_median": round(statistics.median(dev[1:]) * 1e3, 4),
        "device_join_ms_min": round(min(dev[1:]) * 1e3, 4),
        "device_kernels_us_median": round(statistics.median(dev_ns[1:]) / 1e3, 2),
        "prefix_slots": st["prefix_slots"], "table_slots": st["table_slots"],
        "table_capacity": st["table_capacity"],
        "table_occupancy": round(st["table_slots"] / max(1, st["table_capacity"]), 4),
        "table_slots_over_dst_items": round(st["table_slots"] / max(1, na), 4),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
