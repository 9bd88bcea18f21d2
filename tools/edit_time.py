#!/usr/bin/env python3
"""Timing of local edits on a device replica (crdt_hip_replica_apply_patches / _replace), beside
the path a caller without them takes: resolve on a host twin, encode, ship the update back.

Setup as tools/patch_time.py: two forks of the automerge-paper log, `--edits` seeded positional
edits each (default 10,000), under distinct agents; the patch set is what fork A's patches_since
reports after it joined fork B (about 8,400 patches).  Timed, 1 warm-up and the median of `--reps`
(default 9, at least 7), wall time of the calls named, and for the device path the summed device
time of the call's kernels (HIP events, crdt_hip_edit_stats; the order update is not in it):
  keystroke         one character typed into a replica of fork A whose kept order is up to date
      device        Replica.replace
      host path     OpLog.replace on a host twin, encode_from, Replica.apply_updates
  patch_set         the patch set applied to a replica of fork A
      device        Replica.apply_patches, one call
      host path     OpLog.replace per patch on the twin (and, beside it, OpLog.apply_patches in one
                    call, which leaves out the per-call binding overhead), encode_from,
                    Replica.apply_updates
  keystroke_after_join   one character typed right after the replica joined fork B
      device        Replica.replace (pays the full ORDER-mode merge that rebuilds the kept order)
      host path     the replica read back (encode_diff([])) into the twin (apply_diff), OpLog.replace
                    (which rebuilds the twin's positional index), encode_from, apply_updates
Every device result is checked against the host twin's log through encode_diff([]).  Reported, not
gated: prints one JSON line (and writes it to --out).
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


AGENT = 1  # fork A's


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def us(xs):
    return round(statistics.median(xs[1:]) / 1e3, 2)


def ship(twin, rep, edit):
    """The host path: the edit on the twin, its ops encoded and applied to the replica."""
    v = twin.version()
    edit(twin)
    rep.apply_updates([twin.encode_from(v)])


def keystroke(ctx, a, reps):
    dev, dev_ns, host = [], [], []
    rep, twin = crdt_hip.Replica(ctx, a), a.clone()
    rep.set_agent(AGENT)  # (the twin, a clone of fork A, edits under fork A's agent)
    rep2 = crdt_hip.Replica(ctx, a)
    rep.merge_inc()
    pos = a.visible_len() // 2
    for i in range(reps + 1):
        t0 = time.perf_counter()
        rep.replace(pos + i, pos + i, "x")
        dev.append(time.perf_counter() - t0)
        dev_ns.append(ctx.edit_stats()["device_ns"])
        t0 = time.perf_counter()
        ship(twin, rep2, lambda l: l.replace(pos + i, pos + i, "x"))
        host.append(time.perf_counter() - t0)
    assert rep.encode_diff([]) == twin.encode_diff([]) == rep2.encode_diff([])
    out = {"items": a.view().n, "device_ms_median": ms(dev), "device_kernels_us_median": us(dev_ns),
           "host_path_ms_median": ms(host)}
    rep.close()
    rep2.close()
    return out


def patch_set(ctx, a, plist, reps):
    arr, ins = crdt_hip._patches_pack(plist)
    rd = crdt_hip.Replica(ctx, a)
    rd.set_agent(AGENT)  # (kept by the clones)
    rd.merge_inc()
    dev, dev_ns, host, host_one = [], [], [], []
    for _ in range(reps + 1):
        r = rd.clone()
        r.merge_inc()  # (the kept order up to date, as in an editing session)
        t0 = time.perf_counter()
        r.apply_patches(arr, ins)
        dev.append(time.perf_counter() - t0)
        st = ctx.edit_stats()
        dev_ns.append(st["device_ns"])
        r2, twin = rd.clone(), a.clone()
        t0 = time.perf_counter()
        ship(twin, r2, lambda l: [l.replace(p, p + d, s) for p, d, s in plist])
        host.append(time.perf_counter() - t0)
        r3, twin1 = rd.clone(), a.clone()
        t0 = time.perf_counter()
        ship(twin1, r3, lambda l: l.apply_patches(arr, ins))
        host_one.append(time.perf_counter() - t0)
        assert r.encode_diff([]) == twin.encode_diff([]) == r2.encode_diff([]), \
            "the device edit differs from the host's"
        for x in (r, r2, r3):
            x.close()
    rd.close()
    return {"items": st["ranks"], "patches": st["patches"], "inserted": st["items"],
            "deleted": st["tombstones"], "device_ms_median": ms(dev),
            "device_kernels_us_median": us(dev_ns), "host_path_ms_median": ms(host),
            "host_path_one_call_ms_median": ms(host_one)}


def after_join(ctx, a, b, reps):
    rd, rs = crdt_hip.Replica(ctx, a), crdt_hip.Replica(ctx, b)
    rd.set_agent(AGENT)
    rd.merge_inc()
    dev, dev_ns, host = [], [], []
    pos = a.visible_len() // 2
    for _ in range(reps + 1):
        r = rd.clone()
        r.merge_inc()
        r.join(rs)
        r.merge_digest()  # (waits for the join)
        t0 = time.perf_counter()
        r.replace(pos, pos, "x")
        dev.append(time.perf_counter() - t0)
        dev_ns.append(ctx.edit_stats()["device_ns"])
        r2, twin = rd.clone(), a.clone()
        r2.join(rs)
        r2.merge_digest()
        t0 = time.perf_counter()
        twin.apply_diff(r2.encode_diff(twin.state_vector()))  # the readback
        ship(twin, r2, lambda l: l.replace(pos, pos, "x"))
        host.append(time.perf_counter() - t0)
        assert r.encode_diff([]) == twin.encode_diff([]) == r2.encode_diff([]), \
            "the device edit differs from the host's"
        r.close()
        r2.close()
    items = rd.info()[0]
    rd.close()
    rs.close()
    return {"items_before_join": items, "device_ms_median": ms(dev),
            "device_kernels_us_median": us(dev_ns), "host_path_ms_median": ms(host)}


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
    plist = seen.patches_since(m)
    m.close()
    ctx = crdt_hip.Context(0)
    out = {"trace": args.trace, "edits_per_fork": args.edits, "reps": reps,
           "base_items": base.view().n,
           "keystroke": keystroke(ctx, a, reps),
           "patch_set": patch_set(ctx, a, plist, reps),
           "keystroke_after_join": after_join(ctx, a, b, reps)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
