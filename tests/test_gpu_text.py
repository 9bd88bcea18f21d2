"""Text windows on the device (crdt_hip_replica_text_at, text.hip).

Every device result is compared with the host twin's bytes and crdt_hip_text_info (a host log fed
the same updates, joins and deltas holds the same log slot for slot) and with the Python slice of
the version's text, which comes from the CPU oracle or from a recording made when the mark was
taken.  The kernels work in tiles of 4,096 ranks (rank 0 is the document start, so the item at
rank r is the r-th of the document order), words of 64 mark bits and wave steps of 64 ranks; the
shapes here are the smallest that cross those.
"""
import random

import pytest

import crdt_hip
import join_util as ju
import patch_util as pu
import text_util as tu
from test_gpu_patches import Twin
from test_patches import KINDS, forks_of, typed

pytestmark = pytest.mark.gpu

TILE = 4096


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


def both(t: Twin, marks, text: str, a: int, b: int, bd=None) -> None:
    """Window [a, b) of a version on the replica and on the host twin, in both units: the slice of
    `text` and the info.  marks: (device mark, host mark) or None for the version now."""
    dm, hm = marks if marks else (None, None)
    tu.check_window(t.rep, dm, text, a, b, bd)
    tu.check_window(t.host, hm, text, a, b, bd)


def sized_log(fugue: bool, n: int, seed: int) -> crdt_hip.OpLog:
    """n items of mixed widths, typed in pieces (the document order is not the slot order), with
    tombstones sprinkled in, the first and the last item among them."""
    rng = random.Random(seed)
    log = pu.new_log(fugue)
    log.insert(0, tu.mixed_text(n - 40, seed))
    for i in range(4):
        log.insert(rng.randint(0, log.visible_len()), tu.mixed_text(10, seed + 1 + i))
    for _ in range(n // 37):
        p = rng.randrange(log.visible_len())
        log.remove(p, p + 1)
    log.remove(0, 1)
    log.remove(log.visible_len() - 1, log.visible_len())
    assert log.arrays().n == n
    return log


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [4094, 4095, 4096, 4097, 8191, 8192, 8193])
def test_replica_sizes(twin, oracle, kind, n):
    fugue = kind == "fugue"
    t = twin(sized_log(fugue, n, n), fugue)
    arrs = t.arrays()
    text, order = pu.oracle_merge(oracle, arrs)
    assert t.host.text_at() == text.encode() == t.rep.text_at()
    # the visible items at the ranks before rank r: where a window edge falls on a tile edge
    before, v = [0], 0
    for s in order:
        before.append(v)
        v += 0 if arrs.deleted[s - 1] else 1
    before.append(v)
    ends = {0, 1, 63, 64, 65, len(text) - 1, len(text)}
    ends |= {before[min(r, n + 1)] for r in (4095, 4096, 4097, 8191, 8192, 8193)}
    ends = sorted(ends)
    bd = tu.boundaries(text)
    for i, a in enumerate(ends):
        for b in ends[i:]:
            both(t, None, text, a, b, bd)
    assert t.rep.ctx.text_stats()["ranks"] == n


@pytest.mark.parametrize("kind", KINDS)
def test_two_whole_tiles_select_nothing(ctx, twin, kind):
    """16,000 items typed in one run (rank r holds full[r - 1]); ranks 3,501..12,500 are then
    deleted, 9,000 dead ranks between two visible stretches of 3,500: tiles 1 and 2 (ranks
    4,096..12,287) select nothing now, between tile 0 and tile 3, which do.  Windows that end before
    the dead stretch, start after it and span it; the mark from before the delete reads all 16,000."""
    fugue = kind == "fugue"
    full = tu.mixed_text(16000, 5)
    t = twin(typed(fugue, full), fugue)
    dm, hm, _ = t.mark()
    t.edit(lambda l: l.remove(3500, 12500))
    text = full[:3500] + full[12500:]
    assert t.rep.text_at() == text.encode()
    assert ctx.text_stats()["tiles_written"] == 4           # tiles 0..3, the two in the middle empty
    # the shape: a window that ends with tile 0's last visible item is written from tile 0 alone, one
    # that starts with tile 3's first from tile 3 alone, and the two items span all four tiles
    for (a, b), tiles in (((3499, 3500), 1), ((3500, 3501), 1), ((3499, 3501), 4)):
        assert t.rep.text_at(None, a, b) == text[a:b].encode()
        assert ctx.text_stats()["tiles_written"] == tiles
    for a, b in ((0, 3500), (3400, 3500), (3499, 3500), (3500, 3500), (3500, 3501), (3500, 3600),
                 (3510, 7000), (3490, 3510), (0, 7000), (3499, 3501), (7000, 7000)):
        both(t, None, text, a, b)
    for a, b in ((0, 16000), (3400, 3600), (3499, 12501), (4000, 4200), (4095, 4097), (8191, 8193),
                 (12287, 12289), (12500, 16000)):
        both(t, (dm, hm), full, a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_wide_codepoints_on_tile_edges(twin, kind):
    """12,300 items typed in one run (rank r holds text[r - 1]): a 4-byte codepoint is the last rank
    of tiles 0 and 1 and another the first rank of tiles 1 and 2.  Byte windows that cut at each of
    those boundaries, and cuts one, two and three bytes inside, which are EINVAL."""
    fugue = kind == "fugue"
    cps = list(tu.mixed_text(12300, 9))
    wide = [TILE - 2, TILE - 1, 2 * TILE - 2, 2 * TILE - 1]      # ranks 4095, 4096, 8191, 8192
    for i in wide:
        cps[i] = "😀"
    full = "".join(cps)
    t = twin(typed(fugue, full), fugue)
    t.edit(lambda l: (l.remove(9000, 9050), l.remove(12000, 12001)))
    text = full[:9000] + full[9050:12050] + full[12051:]    # (the second remove counts after the first)
    bd = tu.boundaries(text)
    nb = bd[-1]
    for i in sorted({i for w in wide for i in (w, w + 1)}):
        for a, b in ((i - 50, i), (i, i + 50), (i, i), (0, i), (i, len(text)), (i, i + 1)):
            both(t, None, text, a, b, bd)
    for obj in (t.rep, t.host):
        for i in wide:
            for k in (1, 2, 3):
                tu.assert_refused(obj, None, bd[i] + k, tu.END, tu.BYTES, tu.EINVAL)
                tu.assert_refused(obj, None, 0, bd[i] + k, tu.BYTES, tu.EINVAL)
                tu.assert_refused(obj, None, bd[i] + k, nb + 1, tu.BYTES, tu.ERANGE)   # 4 before 5
            assert obj.text_at(None, bd[i], bd[i + 1], bytes=True) == "😀".encode()


@pytest.mark.parametrize("kind", KINDS)
def test_chunk_edges_of_a_boundary_walk(twin, kind):
    """8,300 items typed in one run (rank r holds full[r - 1]).  A boundary's walk loads its tile in
    chunks of 16 steps, an edge every 1,024 ranks inside a tile: windows that start and end with the
    item one rank below, at and one rank above each such edge of tiles 0 and 1, at the mark (which
    selects every rank) and now (ranks 501..510 and 1,020..1,030 of tile 1 dead, so every boundary
    has moved and three of them fall together behind a dead stretch over an edge).  Ranks 1,024 and
    1,025 hold 4-byte codepoints: a cut inside them is EINVAL."""
    fugue = kind == "fugue"
    cps = list(tu.mixed_text(8300, 17))
    cps[1023] = cps[1024] = "😀"
    full = "".join(cps)
    t = twin(typed(fugue, full), fugue)
    dm, hm, _ = t.mark()
    dead = [(TILE + 1020, TILE + 1030), (501, 510)]             # ranks, the later stretch first
    t.edit(lambda l: [l.remove(lo - 1, hi) for lo, hi in dead])
    alive = [True] * (len(full) + 1)
    for lo, hi in dead:
        alive[lo:hi + 1] = [False] * (hi + 1 - lo)
    now = "".join(full[k - 1] for k in range(1, len(full) + 1) if alive[k])
    assert t.rep.text_at() == now.encode() and t.rep.text_at(dm) == full.encode()
    named = [tile * TILE + c + d for tile in (0, 1) for c in (1024, 2048, 3072) for d in (-1, 0, 1)]
    # the boundary behind the item of rank k: the selected items of ranks 1..k
    for marks, text, ends in (((dm, hm), full, named),
                              (None, now, sorted({sum(alive[1:k + 1]) for k in named}))):
        bd = tu.boundaries(text)
        cuts = [0] + ends + [len(text)]
        for a, b in zip(cuts, cuts[1:]):
            both(t, marks, text, a, b, bd)
        both(t, marks, text, ends[0], ends[-1], bd)
    bd = tu.boundaries(full)
    for obj, mk in ((t.rep, dm), (t.host, hm)):
        for i in (1023, 1024):
            for k in (1, 2, 3):
                tu.assert_refused(obj, mk, bd[i] + k, tu.END, tu.BYTES, tu.EINVAL)
                tu.assert_refused(obj, mk, 0, bd[i] + k, tu.BYTES, tu.EINVAL)


@pytest.mark.parametrize("kind", KINDS)
def test_marks_far_below_the_replica(twin, kind):
    """Marks at 63, 64, 65 and 100 items, then 9,000 more items, some typed into the marked text:
    the replica holds slots far past each mark's bit plane.  Then everything the marks saw is
    deleted: the marked texts are unchanged and the text now has none of it."""
    fugue = kind == "fugue"
    base = tu.mixed_text(100, 3)
    t = twin(typed(fugue, base[:63]), fugue)
    marks = []

    def take():
        dm, hm, at = t.mark()
        marks.append(((dm, hm), at.text))
    take()
    for lo, hi in ((63, 64), (64, 65), (65, 100)):
        t.edit(lambda l: l.insert(lo, base[lo:hi]))
        take()
    assert [len(x) for _, x in marks] == [63, 64, 65, 100] and marks[-1][1] == base
    a, b, c = tu.mixed_text(1000, 11), tu.mixed_text(3000, 12), tu.mixed_text(5000, 13)
    t.edit(lambda l: (l.insert(30, b), l.insert(l.visible_len(), c), l.insert(10, a)))
    now = base[:10] + a + base[10:30] + b + base[30:] + c
    assert t.rep.text_at() == now.encode() == t.host.text_at()
    assert t.rep.info()[0] == 9100

    def check_marks():
        for mk, rec in marks:
            assert t.rep.text_at(mk[0]) == rec.encode() == t.host.text_at(mk[1])
            for x, y in ((0, len(rec)), (9, 31), (29, 63), (62, len(rec)), (len(rec), len(rec))):
                both(t, mk, rec, x, y)
            assert pu.apply_patches(rec, t.rep.patches_since(mk[0])) == t.rep.text_at().decode()
    check_marks()
    t.edit(lambda l: (l.remove(0, 10), l.remove(1000, 1020), l.remove(4000, 4070)))
    assert t.rep.text_at() == (a + b + c).encode() == t.host.text_at()
    check_marks()
    for x, y in ((0, 9000), (990, 1010), (4090, 4100), (8999, 9000)):
        both(t, None, a + b + c, x, y)


def test_order_from_the_incremental_path_and_from_rebuilds(twin, oracle):
    base = ju.base_log()
    fa, fb = forks_of(base, False)
    t = twin(base, False)

    def read_only_call(check):
        """`check` makes text_at calls; they leave the log as it was and the replica as a merge_inc
        would: the next merge_inc returns what it returns on an untouched clone."""
        clone = t.rep.clone()
        t.made.append(clone)
        before = t.rep.encode_diff([])
        check()
        assert t.rep.encode_diff([]) == before
        got, want = t.rep.merge_inc(text=True), clone.merge_inc(text=True)
        assert (got[0], got[1], got[3]) == (want[0], want[1], want[3])
        return got[3].decode()

    t.rep.merge_inc()                              # the kept order is valid from here on
    t.edit(lambda l: l.insert(20, "0123456789"))   # 10 new items: the incremental path applies
    assert t.rep.merge_inc()[2] == 1
    text = pu.oracle_merge(oracle, t.arrays())[0]
    assert read_only_call(lambda: both(t, None, text, 15, 40)) == text
    m = t.mark()
    for sync, fork in ((t.join, fa), (t.apply_diff, fb)):
        sync(fork)                                 # the kept order no longer covers the log
        now = pu.oracle_merge(oracle, t.arrays())[0]
        assert read_only_call(lambda: both(t, None, now, 15, len(now) - 3)) == now
        sync(fork)                                 # (nothing new: the order stays valid)
        assert read_only_call(lambda: both(t, m[:2], text, 0, len(text))) == now


@pytest.mark.parametrize("kind", KINDS)
def test_edge_cases(ctx, twin, kind):
    fugue = kind == "fugue"
    t = twin(pu.new_log(fugue), fugue)             # the empty replica
    for obj in (t.rep, t.host):
        assert tu.raw(obj, None, 0, tu.END, 0, 0)[::2] == (0, 0)
        assert tu.raw(obj, None, 0, 0, tu.BYTES, 8)[::2] == (0, 0)
        assert obj.text_info() == tu.want_info("", 0, 0)
        tu.assert_refused(obj, None, 1, tu.END, 0, tu.ERANGE)
        tu.assert_refused(obj, None, 0, 1, tu.BYTES, tu.ERANGE)
    dm0, hm0, _ = t.mark()
    text = tu.mixed_text(300, 21)
    t.edit(lambda l: l.insert(0, text))
    bd = tu.boundaries(text)
    nb, inside = bd[-1], next(x for x in range(bd[-1]) if x not in set(bd))
    other = twin(t.host.clone(), fugue)            # another replica with the same items
    clone = t.rep.clone()
    t.made.append(clone)
    foreign = (other.rep.mark(), clone.mark(), t.host.mark())   # ... a clone's, and a host mark
    for obj, mk in ((t.rep, dm0), (t.host, hm0)):
        assert obj.text_at(mk) == b"" and obj.text_info(mk)["len"] == 0   # an empty version
        tu.assert_refused(obj, mk, 0, 1, 0, tu.ERANGE)
        for start in (0, 150, 300):                # an empty window at 0, in the middle, at len
            assert tu.raw(obj, None, start, start, 0, 0)[::2] == (0, 0)
            assert obj.text_info(None, start, start) == tu.want_info(text, start, start)
        assert obj.text_at(None, 100, None) == text[100:].encode()          # TEXT_END
        assert obj.text_at(None, bd[100], None, bytes=True) == text[100:].encode()
        want = tu.want_info(text, 3, 290)
        for kw in ({"cap": want["n_bytes"] - 1}, {"cap": 64, "null_out": True}):
            rc, buf, n, inf = tu.raw(obj, None, 3, 290, 0, **kw)
            assert rc == tu.ESPACE and n == want["n_bytes"] and inf == want
            assert buf == bytes([tu.CANARY]) * kw["cap"]
        rc, buf, n, _ = tu.raw(obj, None, 3, 290, 0, want["n_bytes"], info=False)
        assert (rc, buf, n) == (0, text[3:290].encode(), want["n_bytes"])
        tu.assert_refused(obj, None, 0, 1, 2, tu.EINVAL)
        tu.assert_refused(obj, None, 0, 1, 0, tu.EINVAL, null_len=True)
        tu.assert_refused(obj, None, 5, 4, 0, tu.EINVAL)
        tu.assert_refused(obj, None, 301, tu.END, 0, tu.ERANGE)
        tu.assert_refused(obj, None, 0, nb + 1, tu.BYTES, tu.ERANGE)
        tu.assert_refused(obj, None, inside, tu.END, tu.BYTES, tu.EINVAL)
        tu.assert_refused(obj, None, 301, tu.END, 2, tu.EINVAL)               # 2 before 4
        tu.assert_refused(obj, None, 305, 302, 0, tu.EINVAL)                  # 3 before 4
        tu.assert_refused(obj, None, inside, nb + 1, tu.BYTES, tu.ERANGE)     # 4 before 5
        tu.assert_refused(obj, None, inside, tu.END, tu.BYTES, tu.EINVAL, cap=0)   # 5 before 7
    for mk in foreign:
        tu.assert_refused(t.rep, mk, 0, 1, 0, tu.EINVAL)
        tu.assert_refused(t.rep, mk, 301, tu.END, 0, tu.EINVAL)               # 1 before 4
    tu.assert_refused(t.host, dm0, 0, 1, 0, tu.EINVAL)                        # a device mark on a log
    ctx2 = crdt_hip.Context(0)                     # a replica of another context
    try:
        rc = crdt_hip.lib().crdt_hip_replica_text_at(ctx2._h, t.rep._h, None, 0, 1, 0, None, 0,
                                                     None, None)
        assert rc == tu.EINVAL
    finally:
        ctx2.close()
    assert t.rep.text_at() == text.encode() and t.rep.encode_diff([]) == t.host.encode_diff([])


def test_stats_of_a_window_inside_one_tile(ctx, twin):
    """A 100-codepoint window inside one tile of a three-tile replica: the write pass launches a
    workgroup for the tiles the window overlaps, not for all three."""
    n = 2 * TILE + 1000
    text = tu.mixed_text(n, 31)
    t = twin(typed(False, text), False)
    assert t.rep.text_at(None, 5000, 5100) == text[5000:5100].encode()
    s = ctx.text_stats()
    assert s["ranks"] == n and 1 <= s["tiles_written"] <= 2
    assert s["bytes"] == len(text[5000:5100].encode())
    assert t.rep.text_at(None, 4000, 4200) == text[4000:4200].encode()      # across a tile edge
    assert ctx.text_stats()["tiles_written"] == 2
    assert t.rep.text_at() == text.encode()
    assert ctx.text_stats()["tiles_written"] == 3
    assert t.rep.text_info(None, 5000, 5100)["n"] == 100
    assert ctx.text_stats()["tiles_written"] == 0                            # sized only: no write pass


def test_the_device_adapters_read_windows_and_marked_versions():
    """HipDownstream in codepoints, HipDownstreamBytes in UTF-8 bytes; a queued update is decoded
    before the read."""
    for cls, at, win in ((crdt_hip.HipDownstream, 5, (6, 8)), (crdt_hip.HipDownstreamBytes, 6, (7, 10))):
        d = cls.from_str("héllo wörld")
        m = d.mark()
        d.insert(at, " €uro")
        assert d.text_range(0, at) == "héllo" and d.text_range(at) == " €uro wörld"
        assert d.text_at(m) == "héllo wörld" and d.text_at(m, *win) == "wö"
        src = crdt_hip.OpLog()
        src.apply_diff(d.replica.encode_diff([]))
        v = src.version()
        src.insert(0, "»")
        d.apply_update(src.encode_from(v))             # queued, not yet decoded
        assert d.text_range(0, 1 if at == 5 else 2) == "»" and d.text_at(m) == "héllo wörld"
        with pytest.raises(crdt_hip.CrdtHipError):
            d.text_range(0, 99)
        d.replica.close()
