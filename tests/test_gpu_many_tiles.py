"""The order passes past tile 255 (text.hip, anchor.hip, format.hip, bytes.hip, patch.hip, edit.hip).

Every kernel that reads the kept document order counts per tile of 4,096 ranks and scans the tile
aggregates in one workgroup, in rounds of 256 tiles with a carry from round to round
(order_tile_scan, block_scan_counts<kOrdTop>, k_patch_top's own loop).  From tile 256 on every tile
prefix is a carry plus a scan within the round, and the byte carry is a 64-bit variable of its own.
The shape here (tiles_util) has 258 tiles of mixed-width text with about 20 % tombstones, so a
dropped, truncated or swapped carry shows: tile 256's prefix is the carry alone, tile 257's the
carry and tile 256's aggregate, no tile's count is 4,096 and no byte prefix equals its codepoint
prefix.  With `dead_edge` tile 254 selects nothing and tile 255 its last rank only, so the prefixes
of tiles 254, 255 and 256 are p, p and p + 1, where a tile search can take the wrong side of the
round's edge.

Every device result is held to three things: the host twin's raw result byte for byte, the numpy
reference of tiles_util (which test_many_tiles.py checks against the host and the oracle on the CPU),
and `ranks` in the call's stats, the items the call streamed.  Exact bytes and integers throughout.
The read-only tests share one replica per kind and layout (a module-scoped fixture parametrised
by both); a host call walks all N items, so the windows of a replica are spread over PARTS tests
and no test takes more than a few host calls.
"""
import pytest

import anchor_util as au
import bytes_util as bu
import crdt_hip
import patch_util as pu
import text_util as tu
import tiles_util as tl
from anchor_util import EINVAL
from crdt_hip import AFTER, BEFORE, DEAD, LIVE
from tiles_util import KINDS, LAYOUTS, N, TILE

pytestmark = pytest.mark.gpu

PARTS = 26      # tests a replica's window pairs are spread over (three pairs, twelve host calls each)
TAIL = 5000     # the items typed after the mark


class World:
    """The document of one kind and layout and a replica that holds it."""

    def __init__(self, ctx, doc: tl.Doc = None, host: crdt_hip.OpLog = None):
        self.doc, self.ref = doc, doc.ref if doc else None
        self.host = doc.host if doc else host
        self.rep = crdt_hip.Replica(ctx, self.host)

    def close(self):
        self.rep.close()


@pytest.fixture(scope="module", params=[(k, l) for k in KINDS for l in LAYOUTS], ids="-".join)
def world(ctx, request):
    """Built once per kind and layout and only read."""
    w = World(ctx, tl.Doc(*request.param))
    yield w
    w.close()


@pytest.fixture(scope="module")
def edited(ctx, world):
    """Another replica of the same document after a mark on it and on its host twin and
    Doc.edit_after_mark, shipped as one wire update; only read from then on."""
    w = World(ctx, world.doc.clone())
    try:
        w.dmark = w.rep.mark()
        w.doc.edit_after_mark(lambda upd: w.rep.apply_updates([upd]))
        yield w
        w.dmark.close()
    finally:
        w.close()


def device_windows(w: World, marks, ref: tl.NRef, part: int, ranks: int) -> None:
    """Part `part` of the reference's window pairs, in codepoints and in bytes: the replica's bytes
    and info against the host twin's and against the slice of the reference's text."""
    dm, hm = marks
    text, bd = ref.text(), ref.boundaries()
    for a, b in tl.window_pairs(ref)[part::PARTS]:
        want = tl.want_window(text, bd, a, b)
        for in_bytes, (x, y) in ((False, (a, b)), (True, (bd[a], bd[b]))):
            dev = tl.read_window(w.rep, dm, x, y, in_bytes, len(want[0]))
            assert w.rep.ctx.text_stats()["ranks"] == ranks
            assert dev == tl.read_window(w.host, hm, x, y, in_bytes, len(want[0]))
            assert dev == want
        tu.check_window(w.rep, dm, text, a, b, bd)


@pytest.mark.parametrize("part", range(PARTS))
def test_windows_now(world, part):
    device_windows(world, (None, None), world.ref, part, N)


@pytest.mark.parametrize("which", ["whole", "inside_257", "255_and_256", "last_of_255", "first_of_256"])
def test_tiles_written(ctx, world, which):
    """The whole text writes 258 tiles, a window inside tile 257 one; the last visible item of tile
    255 and the first of tile 256 write two, each of them alone one (with `dead_edge` the first is
    tile 255's only item, behind a tile that selects nothing)."""
    ref, rep, host = world.ref, world.rep, world.host
    text, bd = ref.text(), ref.boundaries()
    first257, last255 = int(ref.cv[257 * TILE]), int(ref.cv[256 * TILE - 1])
    assert ref.vis[last255 - 1] == 256 * TILE - 1 and ref.vis[last255] == 256 * TILE
    a, b, tiles = {"whole": (0, ref.len, 258), "inside_257": (first257 + 10, first257 + 60, 1),
                   "255_and_256": (last255 - 1, last255 + 1, 2), "last_of_255": (last255 - 1, last255, 1),
                   "first_of_256": (last255, last255 + 1, 1)}[which]
    assert tl.tiles_of(ref, a, b) == tiles
    want = tl.want_window(text, bd, a, b)
    for in_bytes, (x, y) in ((False, (a, b)), (True, (bd[a], bd[b]))):
        dev = tl.read_window(rep, None, x, y, in_bytes, len(want[0]))
        s = ctx.text_stats()
        assert (s["ranks"], s["tiles_written"], s["bytes"]) == (N, tiles, len(want[0]))
        assert dev == tl.read_window(host, None, x, y, in_bytes, len(want[0])) and dev == want


@pytest.mark.parametrize("rank", tl.WIDE4)
def test_windows_refused_inside_a_codepoint(world, rank):
    """A byte boundary 1, 2 or 3 bytes into a named 4-byte codepoint, as a start and as an end, is
    EINVAL on the host and on the device, with the outputs untouched."""
    ref = world.ref
    assert ref.live[rank - 1] and ref.width[rank - 1] == 4
    for p in (int(ref.cb[rank - 1]) + k for k in (1, 2, 3)):
        with pytest.raises(ValueError):
            ref.gap_of_bytes(p)
        for obj in (world.rep, world.host):
            tu.assert_refused(obj, None, p, tu.END, tu.BYTES, tu.EINVAL)
            tu.assert_refused(obj, None, 0, p, tu.BYTES, tu.EINVAL)


def test_windows_refused_past_the_end(world):
    ref = world.ref
    for obj in (world.rep, world.host):
        tu.assert_refused(obj, None, 0, ref.nbytes + 1, tu.BYTES, tu.ERANGE)
        tu.assert_refused(obj, None, ref.len + 1, tu.END, 0, tu.ERANGE)


@pytest.mark.parametrize("part", range(PARTS))
def test_windows_at_the_mark(edited, part):
    """The mark's plane ends at slot N; the replica holds 5,000 slots past it, and ranks the mark
    selected have died since."""
    w = edited
    device_windows(w, (w.dmark, w.doc.hmark), w.doc.at_mark, part, N + TAIL)


def test_texts_after_the_mark(ctx, edited):
    """The mark's text is the recording, the text now the reference's, and the log the host's."""
    w, d = edited, edited.doc
    for marks, ref in (((w.dmark, d.hmark), d.at_mark), ((None, None), d.ref)):
        text, bd = ref.text(), ref.boundaries()
        dev = tl.read_window(w.rep, marks[0], 0, None, False, ref.nbytes)
        assert ctx.text_stats()["ranks"] == N + TAIL
        assert dev == tl.read_window(w.host, marks[1], 0, None, False, ref.nbytes)
        assert dev == tl.want_window(text, bd, 0, ref.len)
    assert d.ref.marked_text() == d.at_mark.text()
    assert w.rep.encode_diff([]) == w.host.encode_diff([])


@pytest.mark.parametrize("unit", ["codepoints", "bytes"])
def test_patches_since_the_mark(ctx, edited, unit):
    """k_patch_top's carries of the `now` items, the deleted ones and the inserted bytes all differ:
    the patches equal the host's array and the reference's, and applied to the recording they give
    the text now."""
    w, d, in_bytes = edited, edited.doc, unit == "bytes"
    want = d.ref.patches(in_bytes)
    name = "patches_since_bytes_raw" if in_bytes else "patches_since_raw"
    raw = getattr(w.rep, name)(w.dmark)
    s = ctx.patch_stats()
    assert (s["patches"], s["ins_bytes"], s["ranks"]) == (3, len(want[2][2].encode()), N + TAIL)
    assert pu.same_raw(raw, getattr(w.host, name)(d.hmark)) and pu.same_raw(raw, tl.raw_patches(want))
    got, rec, now = crdt_hip._patch_list(raw), d.at_mark.text(), d.ref.text()
    if in_bytes:
        assert bu.apply_bytes(rec.encode(), got) == now.encode()
    else:
        assert pu.apply_patches(rec, got) == now


def anchor_stats(ctx, m: int) -> None:
    s = ctx.anchor_stats()
    assert (s["anchors"], s["unknown"], s["ranks"]) == (m, 0, N)


@pytest.mark.parametrize("unit", ["codepoints", "bytes"])
def test_anchors_at_and_back(ctx, world, unit):
    """The named gaps and 100 random ones under both biases, and resolve(anchors_at(p)) == p."""
    ref, rep, host, in_bytes = world.ref, world.rep, world.host, unit == "bytes"
    gaps, bias = tl.anchor_gaps(ref)
    pos = [int(ref.bd[g]) for g in gaps] if in_bytes else gaps
    name = "anchors_at_bytes_raw" if in_bytes else "anchors_at_raw"
    dev = getattr(rep, name)(pos, bias)
    anchor_stats(ctx, len(pos))
    assert dev.tobytes() == getattr(host, name)(pos, bias).tobytes()
    assert dev.tobytes() == ref.anchors_raw(pos, bias, in_bytes).tobytes()
    back = rep.resolve_anchors_raw(dev)
    anchor_stats(ctx, len(pos))
    assert back.tobytes() == host.resolve_anchors_raw(dev).tobytes()
    assert back.tobytes() == ref.positions_raw(crdt_hip._anchor_list(dev)).tobytes()
    assert back["pos_bytes" if in_bytes else "pos"].tolist() == pos


def test_anchors_on_items_around_the_round_edge(ctx, world):
    """Every item within 70 ranks of the first rank of tiles 256 and 257, dead ones included."""
    ref = world.ref
    near = tl.near_anchors(ref)
    got = world.rep.resolve_anchors_raw(near)
    anchor_stats(ctx, len(near))
    assert got.tobytes() == world.host.resolve_anchors_raw(near).tobytes()
    assert got.tobytes() == ref.positions_raw(near).tobytes()
    assert {LIVE, DEAD} == set(got["state"].tolist())


@pytest.mark.parametrize("rank", tl.WIDE4)
def test_anchors_inside_a_codepoint(world, rank):
    """A byte position 1, 2 or 3 bytes into a named 4-byte codepoint, beside a valid one: EINVAL on
    the host and on the device, `out` untouched."""
    ref = world.ref
    for k, bias in ((1, AFTER), (2, BEFORE), (3, AFTER)):
        p = int(ref.cb[rank - 1]) + k
        with pytest.raises(ValueError):
            ref.at(p, bias, True)
        for obj in (world.rep, world.host):
            au.fails(lambda o: obj.anchors_at_bytes_raw([0, p], bias, out=o), EINVAL,
                     au.raw_anchors([(3, 1)] * 2))


def test_spans(ctx, world):
    """tiles_util.format_set: k_fmt_btop's second round has a carry of ten boundaries and a prefix
    inside the round, k_fmt_bpos walks tiles 256 and 257 from their scanned prefixes."""
    formats = tl.format_set(world.ref)
    want, pending, segments = world.ref.spans(formats)
    sp, at, pend = world.rep.spans_raw(formats)
    s = ctx.format_stats()
    hsp, hat, hpend = world.host.spans_raw(formats)
    wsp, wat = tl.raw_spans(want)
    assert (sp.tobytes(), at.tobytes(), pend) == (hsp.tobytes(), hat.tobytes(), hpend)
    assert (sp.tobytes(), at.tobytes(), pend) == (wsp.tobytes(), wat.tobytes(), pending)
    assert (s["formats"], s["pending"], s["segments"], s["spans"], s["ranks"]) == \
        (len(formats), pending, segments, len(want), N)
    assert pending == 1 and segments == 21 and len(want) >= 12


class Edit(World):
    """A replica and a host twin of their own after one apply_patches or apply_patches_bytes call
    with the same patches on both, and a mark on each from before it."""

    def __init__(self, ctx, world: World, call: str, plist):
        super().__init__(ctx, host=world.host.clone())
        try:
            self.marks = self.rep.mark(), self.host.mark()
            self.counts = getattr(self.rep, call)(plist), getattr(self.host, call)(plist)
            self.stats = ctx.edit_stats()
        except BaseException:
            self.close()    # (a failure's traceback keeps this object alive past the context's end,
            raise           # and a replica must be freed before its context)


@pytest.fixture
def byte_edit(ctx, world):
    """tiles_util.byte_patches' four patches in one apply_patches_bytes call: k_bytes_translate
    finds their boundaries against second-round byte prefixes."""
    w = Edit(ctx, world, "apply_patches_bytes", tl.byte_patches(world.ref)[0])
    yield w
    w.close()


@pytest.fixture
def codepoint_edit(ctx, world):
    """test_gpu_edit.test_257_tiles on text where a tile's visible rank is not its rank: the patch
    in tile 256 needs k_edit_top's carry, the one in tile 257 the carry and tile 256's count."""
    w = Edit(ctx, world, "apply_patches", tl.codepoint_patches(world.ref))
    yield w
    w.close()


def test_byte_edits_give_the_hosts_log(world, byte_edit):
    w, want = byte_edit, bu.counts(tl.byte_patches(world.ref)[1])
    assert w.counts[0] == w.counts[1] and w.counts[0] == want
    s = w.stats
    assert (s["patches"], s["items"], s["tombstones"], s["ranks"]) == (4, *want, N)
    assert w.rep.encode_diff([]) == w.host.encode_diff([])


def test_byte_edits_text_and_patches_since(world, byte_edit):
    w, plist_b = byte_edit, tl.byte_patches(world.ref)[0]
    after = bu.apply_bytes(world.ref.text().encode(), plist_b)
    text = w.rep.text_at()
    assert text == w.host.text_at() and text == after
    raw = w.rep.patches_since_bytes_raw(w.marks[0])
    assert pu.same_raw(raw, w.host.patches_since_bytes_raw(w.marks[1]))
    assert pu.same_raw(raw, tl.raw_patches(plist_b))


def test_byte_edit_refused_after_the_edit(world, byte_edit):
    """A second call whose boundary lies 2 bytes into the 4-byte codepoint of rank 1,052,672, where
    the first call left it, beside a valid patch: EINVAL on both sides, and nothing changes."""
    w, plist_b = byte_edit, tl.byte_patches(world.ref)[0]
    state = (w.rep.encode_diff([]), w.rep.info())
    p = int(world.ref.cb[257 * TILE - 1]) + sum(len(i.encode()) - dl for _, dl, i in plist_b[:2])
    assert bu.apply_bytes(world.ref.text().encode(), plist_b)[p: p + 4] == "😀".encode()
    for obj in (w.rep, w.host):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            obj.apply_patches_bytes([(10, 1, "ok"), (p + 2, 0, "x")])
        assert e.value.code == EINVAL
    assert (w.rep.encode_diff([]), w.rep.info()) == state and w.host.encode_diff([]) == state[0]


def test_codepoint_edits_give_the_hosts_log(world, codepoint_edit):
    w = codepoint_edit
    assert w.counts[0] == w.counts[1] and w.counts[0] == bu.counts(tl.codepoint_patches(world.ref)) == (6, 6)
    s = w.stats
    assert (s["patches"], s["items"], s["tombstones"], s["ranks"]) == (4, 6, 6, N)
    assert w.rep.encode_diff([]) == w.host.encode_diff([])


def test_codepoint_edits_text_and_patches_since(world, codepoint_edit):
    w, plist = codepoint_edit, tl.codepoint_patches(world.ref)
    text = w.rep.text_at()
    assert text == w.host.text_at() and text == tl.splice(world.ref.text(), plist).encode()
    raw = w.rep.patches_since_raw(w.marks[0])
    assert pu.same_raw(raw, w.host.patches_since_raw(w.marks[1])) and pu.same_raw(raw, tl.raw_patches(plist))
