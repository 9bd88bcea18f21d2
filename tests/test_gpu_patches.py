"""Patches since a mark on the device (crdt_hip_replica_mark / crdt_hip_replica_patches_since,
patch.hip).

Every device result is compared with the host twin's crdt_hip_patch array and `ins` bytes, byte for
byte (a host log fed the same updates, joins and deltas holds the same log slot for slot), and with
the restatement of patch_util over the CPU oracle's document order; the replica's contents are read
back with encode_diff([]).  The kernels classify the document order in tiles of 4,096 consecutive
ranks, so besides the ~300-item logs of the CPU file the shapes here are the smallest that cross
that tile: 9,000 dead ranks between two changed items (more than two whole tiles that hold
nothing), runs of 9,000 items, and 3,000 patches over 6,001 ranks.
"""
import ctypes as C
import random

import numpy as np
import pytest

import crdt_hip
import delta_util as du
import join_fugue_util as jf
import join_util as ju
import patch_util as pu
from edit_util import ALPHABET
from test_gpu_replica import trace_updates
from test_patches import KINDS, TEXT, forks_of, typed

pytestmark = pytest.mark.gpu


class Twin:
    """A replica and the host log that holds the same items, each with its own marks."""

    def __init__(self, ctx, oracle, log: crdt_hip.OpLog, fugue: bool):
        self.oracle, self.fugue = oracle, fugue
        self.host = log.clone()
        self.rep = crdt_hip.Replica(ctx, log if log.view().n or fugue else None)
        self.made = [self.rep]

    def close(self):
        for r in self.made:
            r.close()

    def mark(self):
        arrs = self.arrays()
        return self.rep.mark(), self.host.mark(), pu.At(self.oracle, arrs)

    def arrays(self) -> crdt_hip.LogArrays:
        arrs = pu.replica_arrays(self.rep, self.fugue)
        (jf.assert_same_log if self.fugue else ju.assert_same_log)(
            arrs, self._nil(self.host.arrays()))
        return arrs

    @staticmethod
    def _nil(arrs):
        arrs.origin_right[:] = 0xFFFFFFFF          # (a delta carries no origin_right)
        return arrs

    def update(self, src: crdt_hip.OpLog, version: int):
        upd = src.encode_from(version)
        self.host.apply_update(upd)
        self.rep.apply_updates([upd])

    def edit(self, fn):
        """A local-style edit: made on a copy of the host log, shipped as one wire update."""
        src = self.host.clone()
        v = src.version()
        fn(src)
        self.update(src, v)

    def join(self, other: crdt_hip.OpLog):
        o = crdt_hip.Replica(self.rep.ctx, other)
        self.made.append(o)
        assert self.rep.join(o) == self.host.join(other)

    def apply_diff(self, other: crdt_hip.OpLog):
        delta = other.encode_diff(self.host.state_vector())
        assert self.rep.apply_diff(delta) == self.host.apply_diff(delta)

    def check(self, marks) -> list:
        dm, hm, at = marks
        dev = self.rep.patches_since_raw(dm)
        assert pu.same_raw(dev, self.host.patches_since_raw(hm))
        got = pu.check(self.oracle, self.rep, dm, at, self.arrays())
        assert got == crdt_hip._patch_list(dev)
        return got


@pytest.fixture
def twin(ctx, oracle):
    made = []

    def make(log, fugue):
        t = Twin(ctx, oracle, log, fugue)
        made.append(t)
        return t
    yield make
    for t in made:
        t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_257_tiles(ctx, kind):
    """Ranks 0..1,048,705 are 257 tiles: k_patch_top scans the tile aggregates in two rounds of
    256, and the last patch lies in tile 256, the first of the second round, whose position needs
    the carry of the first.  The edits arrive as one wire update; device against the host twin, the
    patch array and the bytes."""
    fugue = kind == "fugue"
    plist = [(5, 2, "Q"), (4095, 3, ""), (1_048_600, 0, "tail")]
    host = typed(fugue, (ALPHABET * (1_048_700 // len(ALPHABET) + 1))[:1_048_700])
    rep = crdt_hip.Replica(ctx, host)
    try:
        dm, hm = rep.mark(), host.mark()
        v = host.version()
        assert host.apply_patches(plist) == (5, 5)
        rep.apply_updates([host.encode_from(v)])
        raw = rep.patches_since_raw(dm)
        assert pu.same_raw(raw, host.patches_since_raw(hm))
        assert crdt_hip._patch_list(raw) == plist
        s = ctx.patch_stats()
        assert (s["patches"], s["ins_bytes"], s["ranks"]) == (3, 5, 1_048_705)
        assert rep.encode_diff([]) == host.encode_diff([])
    finally:
        rep.close()


@pytest.mark.parametrize("kind", KINDS)
def test_single_edits_give_the_single_patch(twin, kind):
    fugue = kind == "fugue"
    n = len(TEXT)
    cases = [
        (lambda l: l.insert(7, "X€"), [(7, 0, "X€")]),
        (lambda l: l.remove(3, 9), [(3, 6, "")]),
        (lambda l: l.replace(4, 6, "😀z"), [(4, 2, "😀z")]),
        (lambda l: l.insert(0, "é"), [(0, 0, "é")]),
        (lambda l: l.remove(n - 1, n), [(n - 1, 1, "")]),
        (lambda l: l.remove(0, n), [(0, n, "")]),
        (lambda l: None, []),
    ]
    for fn, want in cases:
        t = twin(typed(fugue), fugue)
        marks = t.mark()
        t.edit(fn)
        assert t.check(marks) == want
    t = twin(pu.new_log(fugue), fugue)            # a mark on the empty replica
    marks = t.mark()
    assert t.rep.patches_since(marks[0]) == []
    t.edit(lambda l: l.insert(0, TEXT))
    assert t.check(marks) == [(0, 0, TEXT)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("edits", [50, 400])
def test_random_edits_after_a_mark(twin, kind, edits):
    fugue = kind == "fugue"
    t = twin(pu.base_log(fugue), fugue)
    marks = t.mark()
    t.edit(lambda l: ju.random_edits(l, random.Random(100 + edits), edits))
    assert len(t.check(marks)) > 10


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["join", "apply_diff"])
def test_sync_after_a_mark(twin, kind, how):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    a, b = forks_of(base, fugue)
    t = twin(a, fugue)
    marks = t.mark()
    (t.join if how == "join" else t.apply_diff)(b)
    assert t.check(marks)
    # two marks alive at once: the second sync is seen from both
    marks2 = t.mark()
    c = (jf.fork if fugue else ju.fork)(base, 3, 23, 40)
    (t.apply_diff if how == "join" else t.join)(c)
    p1, p2 = t.check(marks), t.check(marks2)
    assert p1 != p2


@pytest.mark.parametrize("kind", KINDS)
def test_concurrent_siblings_interleaved_runs_and_transient_items(twin, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    a, b = base.clone(), base.clone()
    a.set_agent(1)
    b.set_agent(2)
    a.insert(50, "aa")
    b.insert(50, "b€")
    t = twin(base, fugue)
    marks = t.mark()
    t.join(a)
    t.join(b)
    got = t.check(marks)
    assert len(got) == 1 and got[0][:2] == (50, 0) and sorted(got[0][2]) == sorted("aab€")
    f = base.clone()
    f.set_agent(3)
    f.insert(105, "XY")
    t = twin(base, fugue)
    marks = t.mark()
    t.edit(lambda l: l.remove(100, 110))
    t.join(f)
    assert t.check(marks) == [(100, 10, "XY")]
    f = base.clone()
    f.set_agent(4)
    f.insert(50, "Q")
    f.remove(50, 51)
    t = twin(base, fugue)
    marks = t.mark()
    t.join(f)
    assert t.check(marks) == []


@pytest.fixture(scope="module")
def gap_logs():
    """Per kind: 12,000 characters typed in one insert, positions [1500, 10500) removed: 9,000
    consecutive ranks that are neither visible at the mark nor now."""
    out = {}
    for kind in KINDS:
        log = pu.new_log(kind == "fugue")
        log.insert(0, ju.random_text(random.Random(4), 12000))
        log.remove(1500, 10500)
        out[kind] = log
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["d_d", "k_d", "i_d"])
def test_classes_carry_across_tiles_that_hold_nothing(twin, gap_logs, kind, case):
    t = twin(gap_logs[kind], kind == "fugue")
    marks = t.mark()
    if case == "d_d":        # two D items joined across the empty tiles
        t.edit(lambda l: l.remove(1499, 1501))
        want = [(1499, 2, "")]
    elif case == "k_d":      # a K carried across the empty tiles to a head
        t.edit(lambda l: l.remove(1500, 1501))
        want = [(1500, 1, "")]
    else:                    # an I and a D joined across the empty tiles
        def fn(l):
            l.insert(1500, "Z")
            l.remove(1501, 1502)
        t.edit(fn)
        want = [(1500, 1, "Z")]
    assert t.rep.patches_since(marks[0]) == want
    assert t.check(marks) == want


@pytest.mark.parametrize("kind", KINDS)
def test_runs_longer_than_a_tile(twin, kind):
    fugue = kind == "fugue"
    rng = random.Random(8)
    long_text = ju.random_text(rng, 9000)
    assert len(long_text.encode()) > 9000 + 4096
    t = twin(typed(fugue), fugue)
    marks = t.mark()
    t.edit(lambda l: l.insert(5, long_text))
    assert t.check(marks) == [(5, 0, long_text)]
    marks = t.mark()
    t.edit(lambda l: l.remove(7, 9007))
    assert t.check(marks) == [(7, 9000, "")]


def test_heads_are_ranked_across_tiles(twin):
    log = pu.new_log(False)
    log.insert(0, "k" * 3001)
    t = twin(log, False)
    marks = t.mark()
    ins = ju.random_text(random.Random(12), 3000)

    def fn(l):
        for i, c in enumerate(ins):
            l.insert(2 * i + 1, c)
    t.edit(fn)
    got = t.check(marks)
    assert got == [(2 * i + 1, 0, c) for i, c in enumerate(ins)]


def test_order_from_the_incremental_path_and_from_a_rebuild(twin, oracle):
    base = ju.base_log()
    a, _ = forks_of(base, False)
    t = twin(base, False)
    t.rep.merge_inc()                              # the kept order is valid from here on
    marks = t.mark()
    t.edit(lambda l: l.insert(20, "0123456789"))   # 10 new items: the incremental path applies
    assert t.check(marks) == [(20, 0, "0123456789")]
    text = pu.oracle_merge(oracle, t.arrays())[0].encode()
    assert t.rep.merge_inc(text=True)[2:] == (1, text)
    assert t.rep.merge()[0] == text
    t.join(a)                                      # the kept order no longer covers the log
    assert t.check(marks)
    text = pu.oracle_merge(oracle, t.arrays())[0].encode()
    assert t.rep.merge()[0] == text
    assert t.rep.merge_inc(text=True)[3] == text
    t.edit(lambda l: l.insert(0, "again"))
    assert t.check(marks)
    assert t.rep.merge_inc(text=True)[3] == pu.oracle_merge(oracle, t.arrays())[0].encode()


def test_one_trace(ctx, py_trace):
    _, _, updates = trace_updates("sveltecomponent")
    rep = crdt_hip.Replica(ctx)
    try:
        half = len(updates) // 2
        rep.apply_updates(updates[:half])
        mark = rep.mark()
        before = rep.merge()[0].decode("utf-8")
        rep.apply_updates(updates[half:])
        got = rep.patches_since(mark)
        pu.assert_never_touch(got)
        assert pu.apply_patches(before, got) == py_trace("sveltecomponent").end_content
        st = ctx.patch_stats()
        assert st["patches"] == len(got) >= 1
        assert st["ins_bytes"] == sum(len(i.encode()) for _, _, i in got)
        assert st["ranks"] == rep.info()[0]
        mark.close()
    finally:
        rep.close()


def dev_call(rep, mark, cap, ins_cap):
    out = np.zeros(max(cap, 1), crdt_hip.PATCH_DTYPE)
    ins = np.zeros(max(ins_cap, 1), np.uint8)
    n, nb = C.c_size_t(77), C.c_size_t(77)
    rc = crdt_hip.lib().crdt_hip_replica_patches_since(
        rep.ctx._h, rep._h, mark._h, out.ctypes.data if cap else None, cap, C.byref(n),
        ins.ctypes.data if ins_cap else None, ins_cap, C.byref(nb))
    return rc, n.value, nb.value, out[:cap], ins[:ins_cap].tobytes()


def test_short_buffers_leave_the_replica_usable(twin):
    t = twin(ju.base_log(), False)
    marks = t.mark()
    assert dev_call(t.rep, marks[0], 0, 0)[:3] == (0, 0, 0)
    t.edit(lambda l: ju.random_edits(l, random.Random(3), 60))
    want, want_ins = t.host.patches_since_raw(marks[1])
    np_, nb = len(want), len(want_ins)
    assert np_ > 3 and nb > 3
    for cap, ins_cap in ((0, 0), (np_ - 1, nb), (np_, nb - 1)):
        assert dev_call(t.rep, marks[0], cap, ins_cap)[:3] == (du.ESPACE, np_, nb)
    rc, n, b, out, ins = dev_call(t.rep, marks[0], np_, nb)
    assert (rc, n, b) == (0, np_, nb)
    assert out.tobytes() == want.tobytes() and ins == want_ins
    t.check(marks)


def test_marks_of_other_owners_are_refused(twin):
    t = twin(ju.base_log(), False)
    u = twin(ju.base_log(), False)
    dm, hm, _ = t.mark()
    clone = t.rep.clone()
    t.made.append(clone)
    for call in (lambda: u.rep.patches_since(dm), lambda: clone.patches_since(dm),
                 lambda: t.rep.patches_since(hm), lambda: t.host.patches_since(dm)):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            call()
        assert e.value.code == du.EINVAL
    assert t.rep.patches_since(dm) == []
