#!/usr/bin/env python3
"""Timing of the line index on a device replica (crdt_hip_replica_line_starts / _lines_of,
crdt_hip_lines.h), beside what a caller without it does to learn where the lines of the text now
lie: the replica's full copy-back (Replica.merge) followed by a host scan of the bytes for '\\n'.

Setup as tools/text_time.py: the automerge-paper log on a replica, a mark, then `--edits` seeded
positional edits (default 10,000) applied as one wire update, so the mark lies that many edits
back; a second fork of the base under another agent is what the replica joins.  Timed, 1 warm-up
and the median of `--reps` (default 9, at least 7): wall time of the call through the binding, and
the summed device time of the call's own kernels (HIP events, crdt_hip_line_stats; the order update
is not in it; for text_lines those of its line_starts call):
  line_starts   2, 64 and 4,096 seeded line numbers (repeats allowed), now
  lines_of      1, 64 and 4,096 seeded byte positions on codepoint boundaries, now
  text_lines    a 50-line viewport from the middle of the version, now and at the mark
each on a replica whose kept order is up to date (`up_to_date`) and right after the replica joined
the other fork (`after_join`: the device call pays the full ORDER-mode merge that rebuilds the kept
order).  The baseline answers the same queries in bytes from one numpy scan of the copied-back
text (numpy.flatnonzero(bytes == 10), then a gather or a searchsorted), which favours it: codepoint
starts and columns would need a decode as well.  A version at a mark has no such baseline; the host
twin's own call (a log kept beside the replica) is timed instead.  Every device result is checked
byte for byte against the host log's.  Reported, not gated: prints one JSON line (and writes it to
--out).
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
import crdt_hip_lines as cl  # noqa: E402
from join_time import fork  # noqa: E402

COUNTS_LINES = (2, 64, 4096)
COUNTS_POS = (1, 64, 4096)
VIEWPORT = 50


def ms(xs):
    return round(statistics.median(xs[1:]) * 1e3, 4)


def us(xs):
    return round(statistics.median(xs[1:]) / 1e3, 2)


def scan(data: bytes) -> tuple:
    """(the bytes as an array, the byte offset of every line start): the host scan for '\\n'."""
    arr = np.frombuffer(data, np.uint8)
    return arr, np.concatenate([[0], np.flatnonzero(arr == 10) + 1]).astype(np.uint64)


def timed(reps, make, sync, call, check, baseline=None, twin=None):
    """make(): (a fresh replica in the state to measure, its mark or None); call(rep, mark) is the
    device path, baseline(rep) the copy-back path on another fresh replica, twin() the host log's."""
    wall, dev, base, host = [], [], [], []
    for _ in range(reps + 1):
        rep, mark = make()
        sync(rep)
        t0 = time.perf_counter()
        got = call(rep, mark)
        wall.append(time.perf_counter() - t0)
        dev.append(cl.stats(rep.ctx)["device_ns"])
        check(got)
        rep.close()
        if twin:
            t0 = time.perf_counter()
            check(twin())
            host.append(time.perf_counter() - t0)
        if baseline:
            rep, _ = make()
            sync(rep)
            t0 = time.perf_counter()
            check(baseline(rep))
            base.append(time.perf_counter() - t0)
            rep.close()
    row = {"device_ms_median": ms(wall), "device_kernels_us_median": us(dev)}
    if host:
        row["host_twin_ms_median"] = ms(host)
    if base:
        row["merge_and_scan_ms_median"] = ms(base)
    return row


def measure(make, sync, host, hmark, reps):
    """The cases on the version now, and text_lines also at the mark."""
    out = {"line_starts": {}, "lines_of": {}, "text_lines": {}}
    rng = np.random.default_rng(7)
    lines = cl.line_count(host)
    info = host.text_info()
    text = host.text_at().decode("utf-8")
    bd = np.concatenate([[0], np.cumsum([len(c.encode("utf-8")) for c in text])]).astype(np.uint64)
    for n in COUNTS_LINES:
        q = rng.integers(0, lines + 1, n).astype(np.uint64)
        want = cl.line_starts(host, q)[0]
        out["line_starts"][str(n)] = timed(
            reps, make, sync, lambda r, m: cl.line_starts(r, q)[0]["start_bytes"],
            lambda got: np.array_equal(got, want["start_bytes"]) or sys.exit("line_starts differ"),
            baseline=lambda r: np.concatenate([scan(r.merge()[0])[1], [info["len_bytes"]]])[q.astype(np.int64)],
            twin=lambda: cl.line_starts(host, q)[0]["start_bytes"])
    for n in COUNTS_POS:
        q = bd[rng.integers(0, info["len"] + 1, n)]
        want = cl.lines_of(host, q, bytes=True)[0]
        out["lines_of"][str(n)] = timed(
            reps, make, sync, lambda r, m: cl.lines_of(r, q, bytes=True)[0]["line"],
            lambda got: np.array_equal(got, want["line"]) or sys.exit("lines_of differ"),
            baseline=lambda r: (np.searchsorted(scan(r.merge()[0])[1], q, side="right") - 1).astype(np.uint64),
            twin=lambda: cl.lines_of(host, q, bytes=True)[0]["line"])
    for name, hm in (("now", None), ("at_mark", hmark)):
        first = max(0, cl.line_count(host, hm) // 2 - VIEWPORT // 2)
        want = cl.text_lines(host, first, VIEWPORT, hm)

        def copy_back(r):
            data = r.merge()[0]
            st = np.concatenate([scan(data)[1], [len(data)]])
            return data[int(st[first]): int(st[min(first + VIEWPORT, st.size - 1)])]
        out["text_lines"][name] = dict(
            timed(reps, make, sync, lambda r, m: cl.text_lines(r, first, VIEWPORT, m if hm else None),
                  lambda got: got == want or sys.exit("text_lines differ"),
                  baseline=None if hm else copy_back,
                  twin=lambda: cl.text_lines(host, first, VIEWPORT, hm)),
            first_line=first, bytes=len(want))
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
           "lines": cl.line_count(host), "lines_at_mark": cl.line_count(host, hmark),
           "up_to_date": measure(fresh, lambda r: r.merge_inc(), host, hmark, reps),
           "after_join": measure(fresh_joined, lambda r: r.merge_digest(), jhost, jhmark, reps)}
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
