"""Formats on the host (crdt_hip_oplog_spans): rich-text attribute ranges on anchors, flattened
into spans.

Expected spans are computed without the product (format_util.FRef: gaps, coverage and winners by
brute force over the CPU oracle's document order); every comparison is of exact integers, the raw
arrays byte for byte.  CPU only.
"""
import random

import numpy as np
import pytest

import anchor_util as au
import crdt_hip
import format_util as fu
import patch_util as pu
from crdt_hip import AFTER, BEFORE, EDGE, REMOVE
from edit_util import KINDS
from format_util import EINVAL, ERANGE, ESPACE, fmt, op_of

START, END_ = (EDGE, AFTER), (EDGE, BEFORE)


def ref_of(oracle, log) -> fu.FRef:
    return fu.FRef(oracle, log.arrays())


def typed(text: str, fugue: bool = False) -> crdt_hip.OpLog:
    log = pu.new_log(fugue)
    log.insert(0, text)
    return log


def painted(oracle, log, formats) -> list:
    """[(pos, len, {key: value})] of log.spans, checked against the restatement."""
    fu.check(log, ref_of(oracle, log), formats)
    sp, pend = log.spans(formats)
    assert pend == 0
    return [(p, n, a) for p, n, _, _, a in sp]


@pytest.mark.parametrize("kind", KINDS)
def test_worked_example(oracle, kind):
    log = typed("abcdef", kind == "fugue")
    b, d, c0, c1, e = log.anchors_at([1, 4, 2, 3, 4], [BEFORE, AFTER, BEFORE, AFTER, BEFORE])
    f1 = fmt(b, d, 1, 1, op_of(10, 1))
    f2 = fmt(c0, c1, 1, 0, op_of(11, 2), REMOVE)
    f3 = fmt(START, END_, 2, 0xFF0000, op_of(3, 1))
    col, both = {2: 0xFF0000}, {1: 1, 2: 0xFF0000}
    sp, at, pend = fu.check(log, ref_of(oracle, log), [f1, f2, f3])
    assert (len(sp), len(at), pend) == (5, 7, 0)
    assert painted(oracle, log, [f1, f2, f3]) == [(0, 1, col), (1, 1, both), (2, 1, col), (3, 1, both),
                                                  (4, 2, col)]
    # with F2 older than F1, F1 wins and c stays bold
    assert painted(oracle, log, [f1, f2[:4] + (op_of(9, 2), REMOVE), f3]) == \
        [(0, 1, col), (1, 3, both), (4, 2, col)]
    log.remove(2, 3)                                    # "c" dies: b and d are neighbours
    assert painted(oracle, log, [f3, f2, f1]) == [(0, 1, col), (1, 2, both), (3, 2, col)]
    log.insert(3, "X")                                  # right after "d": outside F1
    assert painted(oracle, log, [f1, f2, f3]) == [(0, 1, col), (1, 2, both), (3, 3, col)]
    f1e = fmt(b, e, 1, 1, op_of(10, 1))                 # had F1 ended BEFORE e, X is bold
    assert painted(oracle, log, [f1e, f2, f3]) == [(0, 1, col), (1, 3, both), (4, 2, col)]


def test_expansion_at_the_start(oracle):
    log = typed("abcdef")
    b_after, c_before, d_after = log.anchors_at([2, 2, 4], [AFTER, BEFORE, AFTER])
    tight, wide = fmt(c_before, d_after, 1, 1, op_of(1, 0)), fmt(b_after, d_after, 1, 1, op_of(1, 0))
    assert painted(oracle, log, [tight]) == painted(oracle, log, [wide]) == [(2, 2, {1: 1})]
    log.insert(2, "X")                                  # between "b" and "c"
    assert painted(oracle, log, [tight]) == [(3, 2, {1: 1})]
    assert painted(oracle, log, [wide]) == [(2, 3, {1: 1})]   # a start AFTER "b" takes it


@pytest.mark.parametrize("kind", KINDS)
def test_shapes_of_ranges(oracle, kind):
    log = typed("0123456789", kind == "fugue")

    def rng(a, b, key, value, op, flags=0):             # [a, b) of the text, not expanding
        s, e = log.anchors_at([a, b], [BEFORE, AFTER])
        return fmt(s, e, key, value, op, flags)
    # nested, overlapping, identical, adjacent
    assert painted(oracle, log, [rng(1, 9, 1, 1, 1 << 16), rng(3, 5, 2, 7, 2 << 16)]) == \
        [(1, 2, {1: 1}), (3, 2, {1: 1, 2: 7}), (5, 4, {1: 1})]
    assert painted(oracle, log, [rng(1, 5, 1, 1, 1 << 16), rng(3, 8, 2, 7, 2 << 16)]) == \
        [(1, 2, {1: 1}), (3, 2, {1: 1, 2: 7}), (5, 3, {2: 7})]
    assert painted(oracle, log, [rng(2, 6, 1, 1, 1 << 16), rng(2, 6, 1, 5, 2 << 16)]) == [(2, 4, {1: 5})]
    assert painted(oracle, log, [rng(2, 4, 1, 1, 1 << 16), rng(4, 6, 2, 1, 2 << 16)]) == \
        [(2, 2, {1: 1}), (4, 2, {2: 1})]
    # two formats of equal key and value that abut: one span; of another value: two
    assert painted(oracle, log, [rng(2, 4, 1, 1, 1 << 16), rng(4, 7, 1, 1, 2 << 16)]) == [(2, 5, {1: 1})]
    assert painted(oracle, log, [rng(2, 4, 1, 1, 1 << 16), rng(4, 7, 1, 2, 2 << 16)]) == \
        [(2, 2, {1: 1}), (4, 3, {1: 2})]
    # REMOVE wins and loses by op; the agent bits decide a tie in lamport
    bold = rng(0, 10, 1, 1, op_of(5, 1))
    assert painted(oracle, log, [bold, rng(4, 6, 1, 0, op_of(5, 2), REMOVE)]) == \
        [(0, 4, {1: 1}), (6, 4, {1: 1})]
    assert painted(oracle, log, [bold, rng(4, 6, 1, 0, op_of(5, 0), REMOVE)]) == [(0, 10, {1: 1})]
    assert painted(oracle, log, [rng(4, 6, 1, 9, op_of(5, 2)), bold]) == \
        [(0, 4, {1: 1}), (4, 2, {1: 9}), (6, 4, {1: 1})]
    assert painted(oracle, log, [rng(0, 10, 1, 0, op_of(9, 0), REMOVE), bold]) == []
    # inverted and collapsed ranges cover nothing, and are no error
    s, e = log.anchors_at([6, 2], [BEFORE, AFTER])
    same = log.anchors_at([3], AFTER)[0]
    assert painted(oracle, log, [fmt(s, e, 1, 1, 1), fmt(same, same, 1, 1, 2),
                                 fmt(END_, START, 1, 1, 3), fmt(START, START, 2, 2, 4)]) == []
    # EDGE anchors: the whole document, whatever is typed at either end later
    whole = fmt(START, END_, 3, 3, 7)
    assert painted(oracle, log, [whole]) == [(0, 10, {3: 3})]
    log.insert(10, "z")
    log.insert(0, "a")
    assert painted(oracle, log, [whole]) == [(0, 12, {3: 3})]
    assert log.spans([]) == ([], 0)


@pytest.mark.parametrize("kind", KINDS)
def test_tombstones_and_runs(oracle, kind):
    fugue = kind == "fugue"
    log = typed("aaaXXXbbb", fugue)
    a0, a1, b0, b1, x0, x1 = log.anchors_at([0, 3, 6, 9, 3, 6], [BEFORE, AFTER] * 3)
    two = [fmt(a0, a1, 1, 1, 1 << 16), fmt(b0, b1, 1, 1, 2 << 16)]
    assert painted(oracle, log, two) == [(0, 3, {1: 1}), (6, 3, {1: 1})]   # X | empty set | X
    log.remove(3, 6)
    assert painted(oracle, log, two) == [(0, 6, {1: 1})]                   # X | all-dead Y | X
    other = two + [fmt(x0, x1, 2, 2, 3 << 16)]                             # a set on the dead only
    assert painted(oracle, log, other) == [(0, 6, {1: 1})]
    log.remove(0, 6)                                                       # all items dead
    assert log.visible_len() == 0
    assert painted(oracle, log, other + [fmt(START, END_, 5, 5, 9)]) == []
    empty = pu.new_log(fugue)                                              # an empty log
    assert empty.spans(other + [fmt(START, END_, 5, 5, 9)]) == ([], 3)


@pytest.mark.parametrize("kind", KINDS)
def test_pending(oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    fk = pu.jf.fork if fugue else pu.ju.fork
    a, b = fk(base, 1, 61, 40), fk(base, 2, 62, 30)
    ra = ref_of(oracle, a)
    formats = fu.random_formats(ra, random.Random(5), 120, 4)
    assert fu.check(a, ra, formats)[2] == 0
    sp, at, pend = fu.check(b, ref_of(oracle, b), formats)   # b lacks a's new items
    assert 0 < pend < len(formats) and len(sp)
    b.apply_diff(a.encode_diff(b.state_vector()))
    assert fu.check(b, ref_of(oracle, b), formats)[2] == 0
    only = [fmt((op_of(9, 77), AFTER), END_, 1, 1, 1), fmt(START, (op_of(9, 78), BEFORE), 1, 1, 2)]
    assert b.spans(only) == ([], 2)


@pytest.mark.parametrize("kind", KINDS)
def test_random_against_the_restatement(oracle, kind):
    fugue = kind == "fugue"
    log = pu.base_log(fugue)                            # ~300 items, multi-byte, tombstones
    A = log.arrays()
    if fugue:
        assert A.side.any()                             # left children are among the items
    ref = ref_of(oracle, log)
    assert ref.nbytes > ref.len
    for seed, count, keys in ((1, 1, 1), (2, 7, 2), (3, 64, 1), (4, 200, 5), (5, 1000, 70)):
        sp, at, _ = fu.check(log, ref, fu.random_formats(ref, random.Random(seed), count, keys))
        if count >= 200:
            assert len(sp) > 5 and (sp["len_bytes"] > sp["len"]).any()
            assert (sp["pos_bytes"] > sp["pos"]).any()


def test_multibyte_positions(oracle):
    log = typed("a€😀éz")                                # 1, 3, 4, 2, 1 bytes
    s, e = log.anchors_at([1, 4], [BEFORE, AFTER])
    sp, at, _ = fu.check(log, ref_of(oracle, log), [fmt(s, e, 1, 1, 1)])
    assert sp.tolist() == [(1, 1, 3, 9, 0, 1)] and at.tolist() == [(1, 1, 0)]
    assert log.spans([fmt(s, e, 1, 1, 1)]) == ([(1, 3, 1, 9, {1: 1})], 0)


@pytest.mark.parametrize("kind", KINDS)
def test_errors_leave_outputs_untouched(oracle, kind):
    """EINVAL, ERANGE and ESPACE; EBADLOG needs a malformed log (a cycle), which the update, join and
    delta paths all refuse to build."""
    log = pu.base_log(kind == "fugue")
    n = log.visible_len()
    s, e = log.anchors_at([3, n - 3], [BEFORE, AFTER])
    good = fmt(s, e, 1, 1, op_of(4, 1))
    before = log.encode_diff([])
    for formats, code in fu.bad_formats(good):
        fu.fails(log, formats, code)
    # the per-format checks run in array order, the duplicate check after them all
    dup_then_bad = [good, fmt(s, e, 2, 2, op_of(4, 1)), fmt(s, e, 1, 1, 1 << 48)]
    fu.fails(log, dup_then_bad, EINVAL)
    many = np.zeros(65537, crdt_hip.FORMAT_DTYPE)
    many["start"]["id"], many["end"]["id"] = EDGE, EDGE
    many["op"] = np.arange(65537)
    fu.fails(log, many, ERANGE)
    assert log.spans_raw(many[:65536])[0].size == 0     # 65,536 are fine: (AFTER, AFTER) covers nothing
    # ESPACE sizes both outputs, and the second call succeeds
    formats = [good, fmt(START, END_, 2, 2, op_of(1, 1))]
    L, arr = crdt_hip.lib(), crdt_hip._formats_pack(formats)
    import ctypes as C
    ns, na, pend = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
    sp, at = fu.outs(2, 3)
    was = (sp.tobytes(), at.tobytes())
    for out, cap, attrs, acap in ((None, 0, None, 0), (sp.ctypes.data, 2, at.ctypes.data, 3),
                                  (sp.ctypes.data, 3, None, 0)):
        assert L.crdt_hip_oplog_spans(log._h, arr.ctypes.data, 2, out, cap, C.byref(ns), attrs, acap,
                                      C.byref(na), C.byref(pend)) == ESPACE
        assert (ns.value, na.value, pend.value) == (3, 4, 77) and (sp.tobytes(), at.tobytes()) == was
    fu.fails(log, formats, ESPACE, (sp, at))
    sp, at = fu.outs(3, 4)
    got = log.spans_raw(formats, out=(sp, at))
    want = log.spans_raw(formats)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert log.encode_diff([]) == before


@pytest.mark.parametrize("kind", KINDS)
def test_convergence(oracle, kind):
    """Two forks that sync to the same items in different slots, given the same format set in a
    different array order, return identical bytes."""
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    fk = pu.jf.fork if fugue else pu.ju.fork
    a, b = fk(base, 1, 61, 60), fk(base, 2, 62, 45)
    fa = fu.random_formats(ref_of(oracle, a), random.Random(8), 90, 3, op0=1000)
    fb = fu.random_formats(ref_of(oracle, b), random.Random(9), 90, 3, op0=2000)
    a.apply_diff(b.encode_diff(a.state_vector()))
    b.apply_diff(a.encode_diff(b.state_vector()))
    assert a.encode_diff([]) != b.encode_diff([])       # the same items, in different slots
    union = fa + fb
    ga = fu.check(a, ref_of(oracle, a), union)
    shuffled = list(union)
    random.Random(10).shuffle(shuffled)
    gb = fu.check(b, ref_of(oracle, b), shuffled)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()
    assert ga[2] == gb[2] == 0 and len(ga[0]) > 5


def test_host_adapter():
    a = crdt_hip.HipMerge.from_str("hello world")
    b = a.clone()
    a.set_agent(1)
    b.set_agent(2)
    bold = a.format(0, 5, 1, 1)
    link = b.format(3, 8, 2, 7, expand=b.START | b.END)
    assert bold & 0xFFFF == 1 and link & 0xFFFF == 2 and bold >> 16 == link >> 16
    b.insert(8, "ZZ")                                   # at the expanding end of b's link
    assert b.spans() == ([(3, 7, {2: 7})], 0)
    assert a.sync_formats_from(b) == 1 and a.sync_formats_from(b) == 0
    assert a.spans() == ([(0, 3, {1: 1}), (3, 2, {1: 1, 2: 7}), (5, 3, {2: 7})], 0)
    a.sync_from(b)
    b.sync_from(a)
    b.sync_formats_from(a)
    assert a.spans() == b.spans() == ([(0, 3, {1: 1}), (3, 2, {1: 1, 2: 7}), (5, 5, {2: 7})], 0)
    off = a.unformat(0, 2, 1)
    assert off >> 16 > bold >> 16 and a.spans()[0][0] == (2, 1, {1: 1})
    assert a.unformat(0, 1, 2) >> 16 == (off >> 16) + 1   # the adapter's own clock moves on


def test_two_slots_of_one_identity_the_lower_wins():
    """Of two slots of a malformed log that share an identity, a format's anchors name the lower one."""
    log = au.shared_identity_log()
    on_b = fmt((au.SHARED, BEFORE), (au.SHARED, AFTER), 7, 9, op_of(1, 0))
    assert log.spans([on_b]) == ([(1, 1, 1, 1, {7: 9})], 0)
    log.remove(1, 2)
    assert log.spans([on_b]) == ([], 0)
    assert log.text_at() == b"acx"
