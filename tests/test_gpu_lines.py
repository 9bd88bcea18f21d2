"""The line index on the device (crdt_hip_replica_line_starts / _lines_of, lines.hip).

Every device result is compared with the plain Python model of lines_util over the version's text
(from the CPU oracle, or a recording made when the mark was taken) and, byte for byte, with the host
twin's arrays (a host log fed the same updates, joins and deltas holds the same log slot for slot).
The kernels work in tiles of 4,096 ranks (rank 0 is the document start, so the item at rank r is
the r-th of the document order), wave steps of 64 ranks, chunks of 16 steps and rounds of 256
tiles; the shapes here are the smallest that cross those.  A log typed in one run has rank k equal
to item k, which is how a test puts an item at a rank.
"""
import numpy as np
import pytest

import crdt_hip
import crdt_hip_lines as cl
import join_util as ju
import lines_util as lu
import patch_util as pu
import text_util as tu
import tiles_util as tl
from test_gpu_patches import Twin
from test_patches import KINDS, forks_of, typed

pytestmark = pytest.mark.gpu

TILE = 4096
PLAIN = "abcdefgh  " + tu.WIDE          # text_util.mixed_text's alphabet without the line break


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


def cps_of(text: str) -> np.ndarray:
    return np.frombuffer(text.encode("utf-32-le"), "<u4").copy()


def plain_text(n: int, seed: int) -> list:
    """n codepoints of the four widths, none of them a line break, as a list to put some into."""
    rng = np.random.default_rng(seed)
    return [PLAIN[i] for i in rng.integers(0, len(PLAIN), n)]


def one_run(twin, oracle, fugue: bool, chars, dead) -> tuple:
    """(twin, text now) of a log typed in one run, rank k = chars[k - 1], with the ranks of `dead`
    (a bool array) tombstoned; the text is the oracle's."""
    dead = np.asarray(dead, bool)
    log, _ = tl.build_log(fugue, cps_of("".join(chars)), dead)
    t = twin(log, fugue)
    text = pu.oracle_merge(oracle, t.arrays())[0]
    assert text == "".join(c for c, d in zip(chars, dead) if not d)
    return t, text


def both_all(t: Twin, marks, text: str) -> lu.Model:
    """Every line number, every gap in both units, on the replica and on the host twin."""
    dm, hm = marks if marks else (None, None)
    m = lu.check_all(t.rep, dm, text)
    lu.check_all(t.host, hm, text)
    return m


def both(t: Twin, marks, m: lu.Model, lines, gaps) -> None:
    dm, hm = marks if marks else (None, None)
    lu.check_queries(t.rep, dm, m, lines, gaps)
    lu.check_queries(t.host, hm, m, lines, gaps)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [4094, 4095, 4096, 4097, 8192, 8193])
def test_one_run_documents(ctx, twin, oracle, kind, n):
    """About one item in fifteen is a line break and about 20 % are tombstones.  Every line number,
    and the gaps at and around each tile's first and last rank."""
    fugue = kind == "fugue"
    chars = list(tu.mixed_text(n, n))
    dead = np.random.default_rng(n + 1).random(n) < 0.2
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = lu.Model(text)
    assert m.L > n // 25
    cv = np.concatenate([[0], np.cumsum(~dead)])          # visible items of ranks 1..k
    gaps = {0, 1, m.len - 1, m.len}
    for r in (1, 63, 64, 65, 4094, 4095, 4096, 4097, 8191, 8192, 8193):
        if r <= n:
            gaps |= {int(cv[r - 1]), int(cv[r]), min(int(cv[r]) + 1, m.len), max(int(cv[r - 1]) - 1, 0)}
    both(t, None, m, np.arange(m.L + 2), sorted(gaps))
    lu.check_text_lines(t.rep, None, m)
    s = cl.stats(ctx)
    assert s["ranks"] == n


EDGE_CASES = [("nn", (False, False)), ("nn", (True, False)), ("nn", (False, True)), ("nn", (True, True)),
              ("wn", (False, False)), ("nw", (False, False))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("what,dead2", EDGE_CASES, ids=[f"{w}-{int(a)}{int(b)}" for w, (a, b) in EDGE_CASES])
def test_tile_edges(twin, oracle, kind, what, dead2):
    """Rank 4,095 is the last of tile 0 and rank 4,096 the first of tile 1.  `nn`: a line break at
    each, visible or tombstoned; `wn` / `nw`: a 4-byte codepoint at one and a line break at the
    other.  Every line and every gap in both units, and the bytes inside the wide codepoint."""
    fugue = kind == "fugue"
    n = TILE + 200
    chars = plain_text(n, 3)
    for k in (50, 4000, 4150):
        chars[k - 1] = "\n"
    for k, c in zip((4095, 4096), what):
        chars[k - 1] = "\n" if c == "n" else "😀"
    dead = np.random.default_rng(7).random(n) < 0.1
    dead[[49, 3999, 4149]] = False
    dead[4094], dead[4095] = dead2
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = both_all(t, None, text)
    assert m.L == 3 + sum(1 for c, d in zip(what, dead2) if c == "n" and not d)
    if "w" in what:
        at = int(np.cumsum(~dead)[4094 + what.index("w")]) - 1     # the wide codepoint's index in text
        assert text[at] == "😀"
        for obj in (t.rep, t.host):
            for j in (1, 2, 3):
                lu.assert_refused(obj, "lines_of", [0, int(m.bd[at]) + j], lu.EINVAL, flags=lu.BYTES)


@pytest.mark.parametrize("kind", KINDS)
def test_a_tile_without_a_line_break(twin, oracle, kind):
    """3 x 4,096 + 10 ranks: line breaks only in tile 0 and tile 3, tile 1 has none and tile 2 is
    wholly tombstoned, so the tiles 1, 2 and 3 share one line break prefix.  The line that spans
    them by number, and positions inside tiles 1, 2 and 3."""
    fugue = kind == "fugue"
    n = 3 * TILE + 10
    chars = plain_text(n, 5)
    for k in (10, 2000, 4000, 3 * TILE + 2, 3 * TILE + 7):
        chars[k - 1] = "\n"
    dead = np.random.default_rng(9).random(n) < 0.2
    dead[2 * TILE - 1: 3 * TILE - 1] = True               # ranks 8,192..12,287
    dead[[9, 1999, 3999, 3 * TILE + 1, 3 * TILE + 6]] = False
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = lu.Model(text)
    assert m.L == 5
    cv = np.concatenate([[0], np.cumsum(~dead)])
    gaps = [int(cv[r]) for r in (4095, 4096, 5000, 8191, 8192, 9000, 12287, 12288, 12289, 12290, 12291,
                                 12295, 12296, n)]
    both(t, None, m, [3, 4, 0, 5, 6, 3, 1, 2], gaps)
    st = cl.line_starts(t.rep, [3, 4])[0]
    assert int(st["start"][1]) - int(st["start"][0]) > 3000    # line 3 spans tiles 1 and 2
    both_all(t, None, text)


@pytest.mark.parametrize("kind", KINDS)
def test_wave_and_chunk_edges_of_the_walk(twin, oracle, kind):
    """Line breaks at tile-relative ranks 62, 63, 64, 65 (a 64-rank step's edge), 1,023 and 1,024
    (a 16-step chunk's edge) of tiles 0 and 1, and 200 consecutive ones, so that one step holds many
    and the k-th must be picked; some of them tombstoned.  Every line by number and every gap."""
    fugue = kind == "fugue"
    n = 2 * TILE + 100
    chars = plain_text(n, 11)
    for base in (0, TILE):
        for k in (62, 63, 64, 65, 1023, 1024):
            chars[base + k - 1] = "\n"
    chars[2500:2700] = ["\n"] * 200
    dead = np.random.default_rng(13).random(n) < 0.2
    for base in (0, TILE):
        dead[[base + k - 1 for k in (62, 63, 64, 65, 1023, 1024)]] = False
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = both_all(t, None, text)
    assert m.L > 150
    lu.check_text_lines(t.rep, None, m, [(0, 1), (3, 170), (m.L - 2, 5)])


@pytest.mark.parametrize("kind", KINDS)
def test_marks(twin, kind):
    """A mark at 100 items, then about 9,000 more (the mark's plane ends far below the replica's
    slots), a second mark, then a line break the marks saw is deleted and one is typed: the marks'
    lines are those of their recordings, the lines now have the one and not the other."""
    fugue = kind == "fugue"
    base = tu.mixed_text(100, 3)
    assert base.count("\n") >= 3
    t = twin(typed(fugue, base), fugue)
    dm1, hm1, at1 = t.mark()
    a, b = tu.mixed_text(3000, 12), tu.mixed_text(6000, 13)
    t.edit(lambda l: (l.insert(30, a), l.insert(l.visible_len(), b)))
    mid = base[:30] + a + base[30:] + b
    assert t.rep.info()[0] == 9100
    dm2, hm2, at2 = t.mark()
    assert at1.text == base and at2.text == mid
    both_all(t, (dm1, hm1), base)
    both_all(t, (dm2, hm2), mid)
    p = 3030 + base[30:].index("\n")                       # a break of `base` behind the insert
    assert mid[p] == "\n"
    t.edit(lambda l: (l.remove(p, p + 1), l.insert(5, "\n")))
    now = mid[:5] + "\n" + mid[5:p] + mid[p + 1:]
    assert t.rep.text_at() == now.encode()
    m1 = both_all(t, (dm1, hm1), base)
    m2 = both_all(t, (dm2, hm2), mid)
    m = both_all(t, None, now)
    assert (m1.L, m2.L, m.L) == (base.count("\n"), mid.count("\n"), mid.count("\n"))
    assert m2.starts.tolist() != m.starts.tolist()
    lu.check_text_lines(t.rep, dm1, m1)
    lu.check_text_lines(t.rep, dm2, m2, [(2, 40), (m2.L - 1, 3)])


def test_order_from_the_incremental_path_and_from_rebuilds(twin, oracle):
    base = ju.base_log()
    fa, fb = forks_of(base, False)
    t = twin(base, False)

    def read_only_call(check):
        """`check` makes line calls; they leave the log as it was and the replica as a merge_inc
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
    t.edit(lambda l: l.insert(20, "01\n3456\n89"))  # 10 new items: the incremental path applies
    assert t.rep.merge_inc()[2] == 1
    text = pu.oracle_merge(oracle, t.arrays())[0]
    assert read_only_call(lambda: both_all(t, None, text)) == text
    m = t.mark()
    for sync, fork in ((t.join, fa), (t.apply_diff, fb)):
        sync(fork)                                 # the kept order no longer covers the log
        now = pu.oracle_merge(oracle, t.arrays())[0]
        assert read_only_call(lambda: both_all(t, None, now)) == now
        sync(fork)                                 # (nothing new: the order stays valid)
        assert read_only_call(lambda: both_all(t, m[:2], text)) == now


def test_carries_past_tile_255(ctx):
    """tiles_util's 258-tile shape, whose alphabet holds the line break: k_line_top's three carries
    go through rounds 1 and 2.  The last line break before rank 1,048,576, the first one of tile 256
    and of tile 257 and L + 1 by number; the named gaps by position."""
    doc = tl.Doc("rga", "sprinkled")
    ref = doc.ref
    rep = crdt_hip.Replica(ctx, doc.host)
    try:
        m = lu.Model(ref.text())
        br = np.flatnonzero(ref.live & (ref.cps == 10)) + 1        # ranks of the line breaks, in order
        assert br.size == m.L and m.len == ref.len and m.nbytes == ref.nbytes
        i256, i257 = int(np.searchsorted(br, 256 * TILE)), int(np.searchsorted(br, 257 * TILE))
        assert br[i256 - 1] < 256 * TILE <= br[i256] < 257 * TILE <= br[i257]
        lines = [i256, i256 + 1, i257 + 1, m.L + 1, 0, 1, m.L, i257]   # line k starts behind break k
        want = m.line_starts(lines)
        assert want["start"][:3].tolist() == [int(ref.cv[br[i]]) for i in (i256 - 1, i256, i257)]
        gaps = tl.named_gaps(ref)
        for obj in (rep, doc.host):
            lu.check_queries(obj, None, m, lines, gaps)
        assert cl.stats(ctx) == {**cl.stats(ctx), "queries": len(gaps), "ranks": tl.N}
        for p in tl.inside_wide4(ref)[:3]:
            lu.assert_refused(rep, "lines_of", [p], lu.EINVAL, flags=lu.BYTES)
    finally:
        rep.close()


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_edge_cases(ctx, twin, oracle, kind):
    fugue = kind == "fugue"
    t = twin(pu.new_log(fugue), fugue)             # the empty replica: one line that starts at 0
    for obj in (t.rep, t.host):
        lu.check_all(obj, None, "")
        lu.assert_refused(obj, "line_starts", [2], lu.ERANGE)
        lu.assert_refused(obj, "lines_of", [1], lu.ERANGE)
        lu.assert_refused(obj, "lines_of", [0], lu.EINVAL, flags=2)
    dm0, hm0, _ = t.mark()
    text = "ab\n😀c\n\né€" + tu.mixed_text(300, 21)
    t.edit(lambda l: l.insert(0, text))
    other = twin(t.host.clone(), fugue)            # another replica with the same items
    clone = t.rep.clone()
    t.made.append(clone)
    hmark = t.host.mark()
    foreign = [other.rep.mark(), clone.mark(), hmark]   # ... a clone's, and a host mark
    m = lu.Model(text)
    lu.refusals(t.rep, None, m, foreign)
    lu.refusals(t.host, None, m, [dm0, clone.mark()])   # a device mark on a log
    dm, hm, at = t.mark()
    t.edit(lambda l: l.replace(1, 4, "Z\n\n😀"))
    now = pu.oracle_merge(oracle, t.arrays())[0]
    lu.refusals(t.rep, dm, lu.Model(at.text), foreign)
    lu.refusals(t.rep, None, lu.Model(now), foreign)
    both_all(t, (dm0, hm0), "")                    # an empty version of a replica that holds items
    ctx2 = crdt_hip.Context(0)                     # a replica of another context
    try:
        for name in ("line_starts", "lines_of"):
            lu.assert_refused(t.rep, name, [0], lu.EINVAL, ctx=ctx2._h)
    finally:
        ctx2.close()
    assert t.rep.text_at() == now.encode() and t.rep.encode_diff([]) == t.host.encode_diff([])


def test_line_stats_and_the_device_adapters(ctx, twin):
    n = 2 * TILE + 1000
    text = tu.mixed_text(n, 31)
    t = twin(typed(False, text), False)
    cl.line_starts(t.rep, [0, 5, 9])
    s = cl.stats(ctx)
    assert (s["queries"], s["ranks"]) == (3, n) and s["device_ns"] > 0
    cl.lines_of(t.rep, np.arange(100), bytes=False)
    assert (cl.stats(ctx)["queries"], cl.stats(ctx)["ranks"]) == (100, n)
    assert cl.line_count(t.rep) == text.count("\n") + 1
    assert cl.stats(ctx)["queries"] == 0
    # HipDownstream in codepoints, HipDownstreamBytes in bytes: a queued update is decoded first
    for cls in (crdt_hip.HipDownstream, crdt_hip.HipDownstreamBytes):
        d = cls.from_str("héllo\nwörld\n€nd")
        mk = d.mark()
        src = crdt_hip.OpLog()
        src.apply_diff(d.replica.encode_diff([]))
        v = src.version()
        src.insert(0, "»\n")
        d.apply_update(src.encode_from(v))             # queued, not yet decoded
        assert cl.line_count(d) == 4 and cl.text_lines(d, 1, 2) == "héllo\nwörld\n".encode()
        assert cl.line_count(d, mk) == 3 and cl.text_lines(d, 2, 5, mk) == "€nd".encode()
        of = cl.lines_of(d, [9])[0]
        assert (int(of["line"][0]), int(of["col"][0]), int(of["col_bytes"][0])) == (2, 1, 1)
        d.replica.close()
