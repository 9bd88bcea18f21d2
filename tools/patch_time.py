#!/usr/bin/env python3
"""Timing of patches_since (what a sync changed, as positional edits), on the host and on the
device, beside the text copy-back a caller without it needs before it can diff anything.

Setup as tools/delta_time.py: two forks of the automerge-paper log, `--edits` seeded positional
edits each (default 10,000), under distinct agents.  Fork A takes a mark and syncs fork B in, once
by a join and once by a delta (state_vector + encode_diff + apply_diff); the sync is outside the
timed region.  Timed, 1 warm-up and the median of `--reps` (default 9, at least 7):
  device   Replica.patches_since after the sync: wall time of the one ABI call with buffers of the
           exact size (so it includes the update of the kept document order, a full ORDER-mode
           merge after a join or a delta), and the summed device time of its own kernels (HIP
           events, crdt_hip_patch_stats)
  host     OpLog.patches_since of the host twin
  merge    Replica.merge() of the same replica: the merged text copied back to the host
Every device result is checked against the host's, byte for byte.  Reported, not gated: prints one
JSON line (and writes it to --out).
"""
import argparse
import ctypes as C
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
from join_time import fork  # noqa: E402


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def host_sync(d, src, how):
    if how == "join":
        d.join(src)
    else:
        d.apply_diff(src.encode_diff(d.state_vector()))


def dev_sync(r, rs, how):
    if how == "join":
        r.join(rs)
    else:
        r.apply_diff(rs.encode_diff(r.state_vector()))


def dev_patches(rep, mark, n, nb):
    """One crdt_hip_replica_patches_since with buffers of exactly the size needed."""
    out = np.zeros(max(n, 1), crdt_hip.PATCH_DTYPE)
    ins = np.zeros(max(nb, 1), np.uint8)
    gn, gb = C.c_size_t(), C.c_size_t()
    rc = crdt_hip.lib().crdt_hip_replica_patches_since(
        rep.ctx._h, rep._h, mark._h, out.ctypes.data, n, C.byref(gn), ins.ctypes.data, nb,
        C.byref(gb))
    assert rc == 0 and (gn.value, gb.value) == (n, nb), (rc, gn.value, gb.value)
    return out[:n], ins[:nb].tobytes()


def case(ctx, dst, src, reps, how):
    host = []
    for _ in range(reps + 1):
        d = dst.clone()
        m = d.mark()
        host_sync(d, src, how)
        t0 = time.perf_counter()
        want, want_ins = d.patches_since_raw(m)
        host.append(time.perf_counter() - t0)
        m.close()
    rd, rs = crdt_hip.Replica(ctx, dst), crdt_hip.Replica(ctx, src)
    dev, dev_ns, merge = [], [], []
    for _ in range(reps + 1):
        r = rd.clone()
        m = r.mark()
        dev_sync(r, rs, how)
        r.merge_digest()  # (waits for the sync)
        t0 = time.perf_counter()
        got, got_ins = dev_patches(r, m, len(want), len(want_ins))
        dev.append(time.perf_counter() - t0)
        st = ctx.patch_stats()
        dev_ns.append(st["device_ns"])
        assert got.tobytes() == want.tobytes() and got_ins == want_ins, "device patches differ from the host's"
        t0 = time.perf_counter()
        text, _ = r.merge()
        merge.append(time.perf_counter() - t0)
        m.close()
        r.close()
    rd.close()
    rs.close()
    return {
        "items": st["ranks"], "patches": len(want), "ins_bytes": len(want_ins),
        "text_bytes": len(text),
        "device_patches_ms_median": ms(dev),
        "device_patch_kernels_us_median": round(statistics.median(dev_ns[1:]) / 1e3, 2),
        "host_patches_ms_median": ms(host),
        "device_merge_copyback_ms_median": ms(merge),
    }


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
    ctx = crdt_hip.Context(0)
    out = {"trace": args.trace, "edits_per_fork": args.edits, "reps": reps,
           "base_items": base.view().n,
           "after_join": case(ctx, a, b, reps, "join"),
           "after_sync_from": case(ctx, a, b, reps, "delta")}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
