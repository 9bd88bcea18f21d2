"""The numpy reference of the 258-tile shape (tiles_util.NRef) against the host calls and the oracle.

test_gpu_many_tiles.py holds the device to two things, the host twin and a reference that does not
use the product.  Before anything runs on a GPU, this file checks that reference: at N = 1,056,000
items against the host OpLog, for both kinds and both layouts, on exactly the windows, anchors,
formats and patches the GPU file uses (tiles_util builds them), and at 300 items against the
oracle-based restatements the rest of the suite trusts (anchor_util.Ref, format_util.FRef).  CPU only.
"""
import random

import pytest

import anchor_util as au
import bytes_util as bu
import crdt_hip
import format_util as fu
import patch_util as pu
import text_util as tu
import tiles_util as tl
from crdt_hip import AFTER, BEFORE, DEAD, LIVE
from tiles_util import KINDS, LAYOUTS, N

PARTS = 4       # the windows of a document are checked in this many tests (a host call walks N items)


@pytest.fixture(scope="module")
def docs():
    """Per (kind, layout): the document, built once and only read."""
    made = {}

    def get(kind, layout):
        if (kind, layout) not in made:
            made[kind, layout] = tl.Doc(kind, layout)
        return made[kind, layout]
    yield get
    made.clear()


@pytest.fixture(scope="module")
def edited():
    """Per (kind, layout): a document after Doc.edit_after_mark, only read."""
    made = {}

    def get(kind, layout):
        if (kind, layout) not in made:
            d = tl.Doc(kind, layout)
            d.edit_after_mark()
            made[kind, layout] = d
        return made[kind, layout]
    yield get
    made.clear()


def host_windows(host, mark, ref: tl.NRef, part: int) -> None:
    """The host's bytes and info of part `part` of the reference's window pairs, in both units."""
    text, bd = ref.text(), ref.boundaries()
    for a, b in tl.window_pairs(ref)[part::PARTS]:
        want = tl.want_window(text, bd, a, b)
        assert tl.read_window(host, mark, a, b, False, len(want[0])) == want
        assert tl.read_window(host, mark, bd[a], bd[b], True, len(want[0])) == want


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_shape(docs, kind, layout):
    """258 tiles; the four named ranks hold a visible 4-byte codepoint; with `dead_edge` the
    exclusive prefixes of tiles 254, 255 and 256 are p, p and p + 1; the whole text and its
    refusals."""
    d = docs(kind, layout)
    ref, host = d.ref, d.host
    assert ref.n == N and N // tl.TILE + 1 == 258
    assert (257 * tl.TILE, 258 * tl.TILE - 1) == (1_052_672, 1_056_767)
    pre = [int(ref.cv[t * tl.TILE - 1]) for t in (254, 255, 256)]   # visible before the tile's ranks
    if layout == "dead_edge":
        assert pre[1] == pre[0] and pre[2] == pre[0] + 1
    assert 0.75 * N < ref.len < 0.85 * N and ref.nbytes > ref.len + 100_000
    text = ref.text()
    assert host.text_at() == text.encode()
    assert host.text_info() == tu.want_info(text, 0, ref.len, ref.boundaries())
    assert (host.visible_len(), host.visible_bytes()) == (ref.len, ref.nbytes)
    for p in tl.inside_wide4(ref):
        with pytest.raises(ValueError):
            ref.gap_of_bytes(p)
        tu.assert_refused(host, None, p, tu.END, tu.BYTES, tu.EINVAL)
        tu.assert_refused(host, None, 0, p, tu.BYTES, tu.EINVAL)
    tu.assert_refused(host, None, 0, ref.nbytes + 1, tu.BYTES, tu.ERANGE)


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_windows_now(docs, kind, layout, part):
    d = docs(kind, layout)
    host_windows(d.host, None, d.ref, part)


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_windows_at_the_mark(edited, kind, layout, part):
    d = edited(kind, layout)
    host_windows(d.host, d.hmark, d.at_mark, part)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_texts_and_patches_after_the_mark(edited, kind, layout):
    d = edited(kind, layout)
    rec, now = d.at_mark.text(), d.ref.text()
    assert d.ref.marked_text() == rec
    assert d.host.text_at(d.hmark) == rec.encode() and d.host.text_at() == now.encode()
    for in_bytes in (False, True):
        want = d.ref.patches(in_bytes)
        raw = (d.host.patches_since_bytes_raw if in_bytes else d.host.patches_since_raw)(d.hmark)
        assert pu.same_raw(raw, tl.raw_patches(want))
        assert len(want) == 3 and [bool(i) for _, _, i in want] == [False, False, True]
    assert pu.apply_patches(rec, d.ref.patches()) == now
    assert bu.apply_bytes(rec.encode(), d.ref.patches(True)) == now.encode()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_anchors(docs, kind, layout):
    d = docs(kind, layout)
    ref, host = d.ref, d.host
    gaps, bias = tl.anchor_gaps(ref)
    for in_bytes in (False, True):
        pos = [int(ref.bd[g]) for g in gaps] if in_bytes else gaps
        want = ref.anchors_raw(pos, bias, in_bytes)
        got = (host.anchors_at_bytes_raw if in_bytes else host.anchors_at_raw)(pos, bias)
        assert got.tobytes() == want.tobytes()
        back = host.resolve_anchors_raw(got)
        assert back.tobytes() == ref.positions_raw(crdt_hip._anchor_list(got)).tobytes()
        assert back["pos_bytes" if in_bytes else "pos"].tolist() == pos
    near = tl.near_anchors(ref)
    got = host.resolve_anchors_raw(near)
    assert got.tobytes() == ref.positions_raw(near).tobytes()
    assert {LIVE, DEAD} == set(got["state"].tolist())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_spans(docs, kind, layout):
    d = docs(kind, layout)
    formats = tl.format_set(d.ref)
    want, pending, segments = d.ref.spans(formats)
    sp, at, pend = d.host.spans_raw(formats)
    wsp, wat = tl.raw_spans(want)
    assert (sp.tobytes(), at.tobytes(), pend) == (wsp.tobytes(), wat.tobytes(), pending)
    fu.assert_layout(sp, at)
    assert pending == 1 and segments == 21 and len(want) >= 12


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_byte_and_codepoint_patches(docs, kind, layout):
    """The two edits of the GPU file on the host: the byte patches translate to the codepoint
    patches, and the text afterwards is the reference's spliced."""
    src = docs(kind, layout)
    text = src.ref.text()
    plist_b, plist_c = tl.byte_patches(src.ref)
    assert plist_b == bu.to_bytes(text, plist_c) and plist_b != plist_c
    d = src.clone()
    m = d.host.mark()
    assert d.host.apply_patches_bytes(plist_b) == bu.counts(plist_c)
    after = bu.apply_bytes(text.encode(), plist_b)
    assert d.host.text_at() == after == pu.apply_patches(text, plist_c).encode()
    assert d.host.patches_since_bytes(m) == plist_b and d.host.patches_since(m) == plist_c
    d = src.clone()
    plist = tl.codepoint_patches(src.ref)
    assert d.host.apply_patches(plist) == bu.counts(plist) == (6, 6)
    assert d.host.text_at() == pu.apply_patches(text, plist).encode()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_300_items_against_the_oracle(oracle, kind, layout):
    """NRef on a 300-item log of the same make against anchor_util.Ref and format_util.FRef: every
    gap in both units, every identity, random formats, and the patches of an edit after a mark
    against patch_util."""
    d = tl.Doc(kind, layout, n=300)
    nref = d.ref
    ref = fu.FRef(oracle, d.host.arrays())
    assert ref.order == list(range(1, 301))
    assert (nref.len, nref.nbytes, nref.boundaries().arr.tolist()) == (ref.len, ref.nbytes, ref.ends)
    assert nref.text() == pu.oracle_merge(oracle, d.host.arrays())[0]
    for in_bytes in (False, True):
        for p, b in zip(*au.all_gaps(ref, in_bytes)):
            assert nref.at(p, b, in_bytes) == ref.at(p, b, in_bytes)
    for p in ref.insides():
        with pytest.raises(ValueError):
            nref.gap_of_bytes(p)
    every = [(i, b) for i in ref.ident for b in (AFTER, BEFORE)] + [(9 << 16 | 77, AFTER)]
    every += [(crdt_hip.EDGE, AFTER), (crdt_hip.EDGE, BEFORE)]
    assert [nref.resolve(a) for a in every] == [ref.resolve(a) for a in every]
    rng = random.Random(7)
    for count, keys in ((1, 1), (12, 3), (60, 3), (200, 5)):
        formats = fu.random_formats(ref, rng, count, keys, absent=0.05)
        want, pending = ref.spans(formats)
        assert nref.spans(formats)[:2] == (want, pending)
        assert d.host.spans_raw(formats)[0].tobytes() == fu.raw_spans(want)[0].tobytes()
    # an edit after a mark: two deletes and a run typed at the end
    at = pu.At(oracle, d.host.arrays())
    nref.take_mark()
    hm = d.host.mark()
    for a, b in ((150, 170), (40, 45)):
        d.host.remove(a, b)
        nref.remove(a, b)
    tail = tl.codepoints(50, 3)
    d.host.insert(d.host.visible_len(), tl.to_str(tail))
    A = d.host.arrays()
    nref.append(tail, [(int(l) << 16) | int(g) for l, g in zip(A.lamport[300:], A.agent[300:])])
    assert nref.patches() == pu.check(oracle, d.host, hm, at, A)
    assert nref.patches(True) == d.host.patches_since_bytes(hm)
    assert nref.marked_text() == at.text
