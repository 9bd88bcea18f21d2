"""UTF-16 positions on the device (crdt_hip_replica_units_of and the *_utf16 edits and patches,
utf16.hip).

Every device array is compared with the plain Python model of utf16_util over the version's text
(from the CPU oracle, or a recording made when the mark was taken) and, byte for byte, with the host
twin's arrays (a host log fed the same updates, joins and deltas holds the same log slot for slot).
The kernels work in tiles of 4,096 ranks (rank 0 is the document start, so the item at rank r is
the r-th of the document order), wave steps of 64 ranks, chunks of 16 steps (1,024 ranks) and
rounds of 256 tiles; the shapes here are the smallest that cross those.  A log typed in one run has
rank k equal to item k, which is how a test puts an item at a rank.
"""
import ctypes as C
import random

import numpy as np
import pytest

import crdt_hip
import crdt_hip_utf16 as cu
import join_util as ju
import patch_util as pu
import tiles_util as tl
import utf16_util as uu
from test_gpu_patches import Twin
from test_patches import KINDS, forks_of, typed

pytestmark = pytest.mark.gpu

TILE = 4096
NARROW = "abcdefgh é€é€ab  "        # 1, 2 and 3 bytes: one code unit each
ASTRAL = "😀𝄞"                      # 4 bytes: two code units


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


def mixed(n: int, seed: int, astral: float = 0.1) -> list:
    """n characters of the four UTF-8 widths, about `astral` of them of two code units, as a list
    to put some into."""
    rng = np.random.default_rng(seed)
    wide = rng.random(n) < astral
    return [ASTRAL[i % 2] if w else NARROW[i] for w, i in zip(wide, rng.integers(0, len(NARROW), n))]


def one_run(twin, oracle, fugue: bool, chars, dead) -> tuple:
    """(twin, text now) of a log typed in one run, rank k = chars[k - 1], with the ranks of `dead`
    (a bool array) tombstoned; the text is the oracle's."""
    dead = np.asarray(dead, bool)
    log, _ = tl.build_log(fugue, cps_of("".join(chars)), dead)
    t = twin(log, fugue)
    text = pu.oracle_merge(oracle, t.arrays())[0]
    assert text == "".join(c for c, d in zip(chars, dead) if not d)
    return t, text


def both_all(t: Twin, marks, text: str) -> uu.Model:
    """Every gap in the three units, on the replica and on the host twin (each against the model,
    so the two agree byte for byte)."""
    dm, hm = marks if marks else (None, None)
    m = uu.check_all(t.rep, dm, text)
    uu.check_all(t.host, hm, text)
    return m


def both(t: Twin, marks, m: uu.Model, gaps) -> None:
    dm, hm = marks if marks else (None, None)
    uu.check_gaps(t.rep, dm, m, gaps)
    uu.check_gaps(t.host, hm, m, gaps)


def refused_inside(t: Twin, m: uu.Model, at: int) -> None:
    """The positions inside the astral character text[at], in UTF-16 and in bytes, on both sides;
    the gaps on both sides of it are fine."""
    assert uu.units16(m.text[at]) == 2
    for obj in (t.rep, t.host):
        uu.assert_refused(obj, [0, int(m.ud[at]) + 1], uu.UTF16, uu.EINVAL)
        for j in (1, 2, 3):
            uu.assert_refused(obj, [int(m.bd[at]) + j, 0], uu.BYTES, uu.EINVAL)
    both(t, None, m, [at, at + 1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [4094, 4095, 4096, 4097, 8192, 8193])
def test_one_run_documents(ctx, twin, oracle, kind, n):
    """Mixed widths with about one astral in ten and about 20 % tombstones.  Every gap in all three
    units."""
    fugue = kind == "fugue"
    chars = mixed(n, n)
    dead = np.random.default_rng(n + 1).random(n) < 0.2
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = both_all(t, None, text)
    assert m.len + n // 20 < m.n16 < m.nbytes
    s = cu.stats(ctx)
    assert s["ranks"] == n and s["device_ns"] > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rank", [4095, 4096])
@pytest.mark.parametrize("dead_one", [False, True], ids=["visible", "tombstoned"])
def test_an_astral_on_a_tile_edge(twin, oracle, kind, rank, dead_one):
    """Rank 4,095 is the last of tile 0 and rank 4,096 the first of tile 1: an astral codepoint on
    one of them, visible or tombstoned.  Every gap, and the position inside it refused."""
    fugue = kind == "fugue"
    n = TILE + 200
    chars = mixed(n, 3, astral=0.02)
    for k in (4094, 4095, 4096, 4097):
        chars[k - 1] = "x"
    chars[rank - 1] = "😀"
    dead = np.random.default_rng(7).random(n) < 0.1
    dead[4092:4098] = False
    dead[rank - 1] = dead_one
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = both_all(t, None, text)
    at = int(np.cumsum(~dead)[rank - 1]) - 1            # text index of the item of that rank
    if dead_one:
        assert text[at: at + 2] == "xx"                   # (rank - 1 and rank + 1 are neighbours now)
        both(t, None, m, [at, at + 1, at + 2])
    else:
        assert text[at] == "😀"
        refused_inside(t, m, at)


@pytest.mark.parametrize("kind", KINDS)
def test_wave_and_chunk_edges_of_the_walk(twin, oracle, kind):
    """Astral codepoints at tile-relative ranks 62, 63, 64, 65 (a 64-rank step's edge), 1,023 and
    1,024 (a 16-step chunk's edge) of tiles 0 and 1, some neighbours tombstoned.  Every gap, and the
    positions inside each of them refused."""
    fugue = kind == "fugue"
    n = 2 * TILE + 100
    chars = mixed(n, 11, astral=0.05)
    spots = [base + k for base in (0, TILE) for k in (62, 63, 64, 65, 1023, 1024)]
    for r in spots:
        chars[r - 1] = "𝄞"
    dead = np.random.default_rng(13).random(n) < 0.2
    dead[[r - 1 for r in spots]] = False
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = both_all(t, None, text)
    cv = np.cumsum(~dead)
    for r in spots:
        refused_inside(t, m, int(cv[r - 1]) - 1)


@pytest.mark.parametrize("kind", KINDS)
def test_a_wholly_astral_tile_and_a_wholly_dead_one(twin, oracle, kind):
    """3 x 4,096 + 10 ranks: tile 1 (ranks 4,096..8,191) wholly astral and visible, 8,192 code units,
    the largest tile aggregate; tile 2 wholly tombstoned, so tiles 2 and 3 share their prefixes.
    Positions landing in tiles 1 and 3 and on their edges."""
    fugue = kind == "fugue"
    n = 3 * TILE + 10
    chars = mixed(n, 5)
    chars[TILE - 1: 2 * TILE - 1] = ["😀"] * TILE
    dead = np.random.default_rng(9).random(n) < 0.2
    dead[TILE - 1: 2 * TILE - 1] = False
    dead[2 * TILE - 1: 3 * TILE - 1] = True
    dead[[TILE - 2, 3 * TILE - 1, n - 1]] = False
    t, text = one_run(twin, oracle, fugue, chars, dead)
    m = uu.Model(text)
    cv = np.concatenate([[0], np.cumsum(~dead)])
    ranks = (1, 4094, 4095, 4096, 4097, 5000, 6143, 6144, 8190, 8191, 8192, 9000, 12287, 12288, 12289,
             12290, 12295, n)
    gaps = sorted({int(cv[r]) for r in ranks} | {int(cv[r - 1]) for r in ranks} | {0, m.len})
    both(t, None, m, gaps)
    first = int(cv[TILE - 1])                              # text index of rank 4,096
    assert text[first: first + TILE] == "😀" * TILE
    assert int(m.ud[first + TILE] - m.ud[first]) == 2 * TILE
    for at in (first, first + 1, first + 2047, first + TILE - 1):
        refused_inside(t, m, at)
    both_all(t, None, text)


@pytest.mark.parametrize("kind", KINDS)
def test_two_marks_alive_at_once(twin, kind):
    """A mark at 100 items, then 9,000 more (the mark's plane ends far below the replica's slots),
    a second mark, then an astral the marks saw is deleted and one is typed."""
    fugue = kind == "fugue"
    base = "".join(mixed(100, 3))
    t = twin(typed(fugue, base), fugue)
    dm1, hm1, at1 = t.mark()
    a, b = "".join(mixed(3000, 12)), "".join(mixed(6000, 13))
    t.edit(lambda l: (l.insert(30, a), l.insert(l.visible_len(), b)))
    mid = base[:30] + a + base[30:] + b
    assert t.rep.info()[0] == 9100
    dm2, hm2, at2 = t.mark()
    assert at1.text == base and at2.text == mid
    both_all(t, (dm1, hm1), base)
    both_all(t, (dm2, hm2), mid)
    p = 3030 + next(i for i, c in enumerate(base[30:]) if uu.units16(c) == 2)   # an astral of `base`
    t.edit(lambda l: (l.remove(p, p + 1), l.insert(5, "𝄞")))
    now = mid[:5] + "𝄞" + mid[5:p] + mid[p + 1:]
    assert t.rep.text_at() == now.encode()
    m1 = both_all(t, (dm1, hm1), base)
    m2 = both_all(t, (dm2, hm2), mid)
    m = both_all(t, None, now)
    assert m2.n16 == m.n16 and m2.ud.tolist() != m.ud.tolist() and m1.n16 < m2.n16
    for marks, at_text in (((dm1, hm1), base), ((dm2, hm2), mid)):
        dev = uu.check_since(t.rep, marks[0], at_text, now)
        assert pu.same_raw(dev, uu.check_since(t.host, marks[1], at_text, now))


def test_order_from_the_incremental_path_and_from_rebuilds(twin, oracle):
    base = ju.base_log()
    base.insert(3, "😀a𝄞")
    fa, fb = forks_of(base, False)
    fa.insert(0, "𝄞")
    fb.insert(2, "x😀")
    t = twin(base, False)

    def read_only_call(check):
        """`check` makes translation calls; they leave the log as it was and the replica as a
        merge_inc would: the next merge_inc returns what it returns on an untouched clone."""
        clone = t.rep.clone()
        t.made.append(clone)
        before = t.rep.encode_diff([])
        check()
        assert t.rep.encode_diff([]) == before
        got, want = t.rep.merge_inc(text=True), clone.merge_inc(text=True)
        assert (got[0], got[1], got[3]) == (want[0], want[1], want[3])
        return got[3].decode()

    t.rep.merge_inc()                              # the kept order is valid from here on
    t.edit(lambda l: l.insert(20, "01😀3456𝄞89"))  # 10 new items: the incremental path applies
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
        dev = uu.check_since(t.rep, m[0], text, now)
        assert pu.same_raw(dev, uu.check_since(t.host, m[1], text, now))


@pytest.fixture(scope="module")
def big(ctx):
    """tiles_util's 258-tile shape (one kind, one layout), built once."""
    doc = tl.Doc("rga", "sprinkled")
    rep = crdt_hip.Replica(ctx, doc.host)
    yield doc, rep
    rep.close()


def test_carries_past_tile_255(ctx, big):
    """The 258-tile shape: k_unit_top's three carries go through rounds 1 and 2.  The named gaps in
    all three units against the reference's arrays and the host twin."""
    doc, rep = big
    ref = doc.ref
    live = ref.live
    u16 = np.concatenate([[0], np.cumsum((1 + (ref.width == 4)) * live, dtype=np.int64)])   # of ranks 1..k
    ud = np.concatenate([[0], u16[ref.vis]])               # code units of the first v visible items
    gaps = np.asarray(tl.named_gaps(ref), np.int64)
    want = np.zeros(gaps.size, uu.DT)
    want["cp"], want["bytes"], want["utf16"] = gaps, ref.bd[gaps], ud[gaps]
    info = {"len": ref.len, "len_bytes": ref.nbytes, "len_utf16": int(ud[-1])}
    assert info["len"] < info["len_utf16"] < info["len_bytes"]
    for obj in (rep, doc.host):
        for unit in (uu.CP, uu.BYTES, uu.UTF16):
            uu.same(cu.units_of(obj, want[uu.FIELD[unit]], unit), want, info)
    assert cu.stats(ctx) == {**cu.stats(ctx), "queries": gaps.size, "ranks": tl.N}
    for p in tl.inside_wide4(ref)[:3]:
        uu.assert_refused(rep, [p], uu.BYTES, uu.EINVAL)
    for k in tl.WIDE4:
        uu.assert_refused(rep, [int(u16[k - 1]) + 1], uu.UTF16, uu.EINVAL)


@pytest.mark.parametrize("kind", KINDS)
def test_edits_in_utf16_across_a_tile_edge(ctx, twin, oracle, kind):
    """apply_patches_utf16 and replace_utf16 on a replica against the host twin, slot for slot: a
    set whose patches lie on both sides of rank 4,096 with astral text inserted and deleted, applied
    while the kept order is stale (a join came first), then a keystroke."""
    fugue = kind == "fugue"
    n = TILE + 300
    chars = mixed(n, 17)
    for k in (4095, 4096, 4097):
        chars[k - 1] = "😀"
    chars[0] = "q"
    dead = np.random.default_rng(19).random(n) < 0.15
    dead[4090:4100] = False
    dead[0] = False
    t, text = one_run(twin, oracle, fugue, chars, dead)
    t.rep.merge_inc()
    fork = t.host.clone()
    fork.set_agent(7)
    fork.insert(fork.visible_len(), "j😀")         # (at the end: the ranks before it stay)
    t.join(fork)                                   # the kept order no longer covers the log
    text = pu.oracle_merge(oracle, t.arrays())[0]
    m = uu.Model(text)
    e = int(np.cumsum(~dead)[4094]) - 1            # text index of rank 4,095
    assert text[e: e + 3] == "😀😀😀"              # ranks 4,095..4,097
    # ranks 4,095 and 4,096 deleted by one patch, astral text typed by the patch before it
    pset = uu.patches16_at(m, [(3, 6, "𝄞𝄞"), (e, e + 2, "y😀"), (e + 3, e + 3, "end")])
    cp_set = uu.to_cp_patches(text, pset)
    assert cp_set[1][1] == 2 and cp_set != pset
    want = t.host.clone()
    assert cu.apply_patches_utf16(t.rep, pset) == cu.apply_patches_utf16(t.host, pset) == want.apply_patches(cp_set)
    assert ctx.edit_stats()["patches"] == 3 and cu.stats(ctx)["queries"] == 6
    assert t.host.encode_diff([]) == want.encode_diff([])
    now = pu.oracle_merge(oracle, t.arrays())[0]   # (asserts the replica and the host log agree)
    assert now == uu.splice16(text, pset)
    m = both_all(t, None, now)
    k = int(m.ud[now.index("y😀") + 2])
    for obj in (t.rep, t.host):
        cu.replace_utf16(obj, k, k + 2, "z")
        cu.insert_utf16(obj, 0, "𝄞")
        cu.remove_utf16(obj, 2, 3)
    after = pu.oracle_merge(oracle, t.arrays())[0]
    assert after == uu.splice16(now, [(k, 2, "z"), (0, 0, "𝄞"), (2, 1, "")])


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_edge_cases(ctx, twin, oracle, kind):
    fugue = kind == "fugue"
    t = twin(pu.new_log(fugue), fugue)             # the empty replica
    for obj in (t.rep, t.host):
        uu.check_all(obj, None, "")
        for unit in (uu.CP, uu.BYTES, uu.UTF16):
            uu.assert_refused(obj, [1], unit, uu.ERANGE)
        uu.assert_refused(obj, [0], 3, uu.EINVAL)
        assert cu.apply_patches_utf16(obj, []) == (0, 0)
        uu.apply_refused(obj, [(1, 0, "x")], uu.ERANGE)
    dm0, hm0, _ = t.mark()
    text = "a😀b😀c\né€" + "".join(mixed(300, 21))
    for obj in (t.rep, t.host):
        cu.insert_utf16(obj, 0, text)              # the first edit of an empty replica, in UTF-16
    assert pu.oracle_merge(oracle, t.arrays())[0] == text
    other = twin(t.host.clone(), fugue)            # another replica with the same items
    clone = t.rep.clone()
    t.made.append(clone)
    hmark = t.host.mark()
    foreign = [other.rep.mark(), clone.mark(), hmark]   # ... a clone's, and a host mark
    m = uu.Model(text)
    uu.refusals(t.rep, None, m, foreign)
    uu.refusals(t.host, None, m, [dm0, clone.mark()])   # a device mark on a log
    for obj in (t.rep, t.host):
        uu.patch_refusals(obj, text)
    dm, hm, at = t.mark()
    t.edit(lambda l: l.replace(1, 4, "Z\n\n😀"))
    now = pu.oracle_merge(oracle, t.arrays())[0]
    uu.refusals(t.rep, dm, uu.Model(at.text), foreign)
    uu.refusals(t.rep, None, uu.Model(now), foreign)
    both_all(t, (dm0, hm0), "")                    # an empty version of a replica that holds items
    for obj, mk in ((t.rep, dm0), (t.host, hm0)):
        for unit in (uu.CP, uu.BYTES, uu.UTF16):
            uu.assert_refused(obj, [1], unit, uu.ERANGE, mark=mk)
        uu.check_since(obj, mk, "", now)
    L = cu.lib()
    n, nb = C.c_size_t(0), C.c_size_t(0)
    since = L.crdt_hip_replica_patches_since_utf16
    assert since(ctx._h, t.rep._h, dm._h, None, 0, C.byref(n), None, 0, C.byref(nb)) == -6   # ESPACE
    raw = cu.patches_since_utf16_raw(t.rep, dm)
    assert (n.value, nb.value) == (raw[0].size, len(raw[1])) and n.value
    for fm in foreign:
        assert since(ctx._h, t.rep._h, fm._h, None, 0, C.byref(n), None, 0, C.byref(nb)) == -1
    ctx2 = crdt_hip.Context(0)                     # a replica of another context
    try:
        for unit in (uu.CP, uu.BYTES, uu.UTF16):
            uu.assert_refused(t.rep, [0], unit, uu.EINVAL, ctx=ctx2._h)
        assert since(ctx2._h, t.rep._h, dm._h, None, 0, C.byref(n), None, 0, C.byref(nb)) == -1
        assert L.crdt_hip_replica_replace_utf16(ctx2._h, t.rep._h, 0, 1, None, 0) == -1
        assert L.crdt_hip_replica_apply_patches_utf16(ctx2._h, t.rep._h, None, 0, None, 0, None, None) == -1
    finally:
        ctx2.close()
    assert t.rep.text_at() == now.encode() and t.rep.encode_diff([]) == t.host.encode_diff([])


def test_unit_stats_and_the_utf16_adapter(ctx, twin):
    n = 2 * TILE + 1000
    text = "".join(mixed(n, 31))
    t = twin(typed(False, text), False)
    cu.units_of(t.rep, [0, 5, 9], cu.UNIT_CODEPOINTS)
    s = cu.stats(ctx)
    assert (s["queries"], s["ranks"]) == (3, n) and s["device_ns"] > 0
    cu.to_utf16(t.rep, np.arange(100))
    assert (cu.stats(ctx)["queries"], cu.stats(ctx)["ranks"]) == (100, n)
    assert cu.len_utf16(t.rep) == uu.units16(text)
    assert cu.stats(ctx)["queries"] == 0
    # HipDownstreamUtf16 against a Python str held in UTF-16, over a seeded edit script
    d = cu.HipDownstreamUtf16.from_str("héllo 😀\nwörld 𝄞\n€nd")
    s16 = "héllo 😀\nwörld 𝄞\n€nd"
    assert d.len() == uu.units16(s16) and d.NAME == "mi355x-device-utf16"
    rng = random.Random(9)
    for step in range(40):
        m = uu.Model(s16)
        ga, gb = sorted(rng.randrange(m.len + 1) for _ in range(2))
        a, b = int(m.ud[ga]), int(m.ud[min(gb, ga + 4)])
        ins = "".join(rng.choice("ab é€😀𝄞\n") for _ in range(rng.randrange(4)))
        (d.replace, lambda a, b, i: d.insert(a, i), lambda a, b, i: d.remove(a, b))[step % 3](a, b, ins)
        if step % 3 == 1:
            b = a
        if step % 3 == 2:
            ins = ""
        s16 = uu.splice16(s16, [(a, b - a, ins)])
        assert d.len() == uu.units16(s16)
    assert d.text() == s16
    m = uu.Model(s16)
    # a queued update is decoded first; marks, patches, windows, anchors, formats and lines in UTF-16
    mk = d.mark()
    src = crdt_hip.OpLog()
    src.apply_diff(d.replica.encode_diff([]))
    v = src.version()
    src.insert(0, "»𝄞\n")
    d.apply_update(src.encode_from(v))             # queued, not yet decoded
    assert d.len() == m.n16 + 4
    now = "»𝄞\n" + s16
    assert d.patches_since(mk) == [(0, 0, "»𝄞\n")]
    assert uu.splice16(s16, d.patches_since(mk)) == now
    mn = uu.Model(now)
    g1, g2 = 2, mn.len - 3
    assert d.text_range(int(mn.ud[g1]), int(mn.ud[g2])) == now[g1:g2]
    assert d.text_at(mk) == s16 and d.text_at(mk, 0, int(m.ud[4])) == s16[:4]
    anchor = d.anchor_at(int(mn.ud[g2]))
    assert d.resolve(anchor) == int(mn.ud[g2])
    d.insert(0, "😀")
    assert d.resolve(anchor) == int(mn.ud[g2]) + 2 and d.resolve_many([anchor, (5 << 16 | 999, 0)])[1] is None
    now = "😀" + now
    mn = uu.Model(now)
    d.format(int(mn.ud[1]), int(mn.ud[6]), 1, 42)
    sp, pend = d.spans()
    assert pend == 0 and [x for x in sp if x[2]] == [(int(mn.ud[1]), int(mn.ud[6] - mn.ud[1]), {1: 42})]
    line, ch = d.lines_of(mn.ud)
    rows = now.split("\n")
    want = [(r, uu.units16(rows[r][:c])) for r in range(len(rows)) for c in range(len(rows[r]) + 1)]
    assert list(zip(line.tolist(), ch.tolist())) == want
    other = cu.HipDownstreamUtf16.from_str("")
    other.sync_from(d)
    mark_text = other.text()
    other.insert(0, "x𝄞")
    got = d.sync_patches(other)
    assert got == [(0, 0, "x𝄞")] and d.text() == "x𝄞" + mark_text
    c = d.clone()
    assert isinstance(c, cu.HipDownstreamUtf16) and c.len() == d.len()
    for x in (d, other, c):
        x.replica.close()
