"""Text windows on the host (crdt_hip_oplog_text_at): a range of the document, now or at a mark.

The host call is the definition the device call is held to.  A version's text comes from the CPU
oracle or from a recording made when the mark was taken; a window of it is a Python slice
(text_util).  CPU only.
"""
import random

import pytest

import crdt_hip
import join_util as ju
import patch_util as pu
import text_util as tu
from test_patches import KINDS, forks_of, typed


@pytest.mark.parametrize("kind", KINDS)
def test_whole_document_is_the_oracles(oracle, kind):
    fugue = kind == "fugue"
    base = pu.base_log(fugue)
    a, b = forks_of(base, fugue)
    a.join(b)
    for log in (pu.new_log(fugue), typed(fugue), base, b, a):
        text = pu.oracle_merge(oracle, log.arrays())[0]
        assert log.text_at() == text.encode("utf-8")
        assert log.text_at(None, 0, None, bytes=True) == text.encode("utf-8")
        assert log.text_info() == tu.want_info(text, 0, len(text))
        assert log.visible_len() == len(text)


def small_doc(fugue: bool) -> tuple:
    """A 40-codepoint document of all four UTF-8 widths with tombstones in it, typed in pieces so
    that the document order is not the slot order."""
    log = pu.new_log(fugue)
    log.insert(0, "abc€déf😀ghij")
    log.insert(4, "😀xyé€ zw😀😀qé")
    log.insert(0, "é€tuv")
    log.insert(log.visible_len(), "klm€n😀opé€rs 😀é€zz")
    log.remove(2, 4)
    log.remove(10, 12)
    log.remove(30, 33)
    assert log.visible_len() == 40 and log.arrays().deleted.sum() == 7
    return log


@pytest.mark.parametrize("kind", KINDS)
def test_every_small_window(oracle, kind):
    log = small_doc(kind == "fugue")
    text = pu.oracle_merge(oracle, log.arrays())[0]
    assert {len(c.encode()) for c in text} == {1, 2, 3, 4}
    bd = tu.boundaries(text)
    for a in range(41):
        for b in range(a, 41):
            tu.check_window(log, None, text, a, b, bd)
    # every byte window: on two boundaries the byte slice, off one EINVAL
    data, on = text.encode("utf-8"), set(bd)
    for x in range(len(data) + 1):
        for y in range(x, len(data) + 1):
            if x in on and y in on:
                assert log.text_at(None, x, y, bytes=True) == data[x:y]
            else:
                tu.assert_refused(log, None, x, y, tu.BYTES, tu.EINVAL)
    assert log.text_at(None, 7, None) == text[7:].encode()          # TEXT_END
    assert log.text_at(None, bd[7], None, bytes=True) == text[7:].encode()


@pytest.mark.parametrize("kind", KINDS)
def test_history_over_30_steps(oracle, kind):
    """Edits, updates, a join and a delta; a mark and a recording after each step.  At the end
    every mark still reads its recording, windows of it are slices of the recording, and
    patches_since(mark) applied to text_at(mark) is the text now."""
    fugue = kind == "fugue"
    rng = random.Random(7 if fugue else 8)
    log = pu.base_log(fugue)
    fa, fb = forks_of(log, fugue)
    marks = []
    for step in range(30):
        if step == 11:
            log.join(fa)
        elif step == 23:
            log.apply_diff(fb.encode_diff(log.state_vector()))
        elif step % 3 == 1:                       # an update: edits made elsewhere, one wire update
            src = log.clone()
            v = src.version()
            ju.random_edits(src, rng, 4)
            log.apply_update(src.encode_from(v))
        else:
            ju.random_edits(log, rng, 4)
        marks.append((log.mark(), pu.oracle_merge(oracle, log.arrays())[0]))
    now = pu.oracle_merge(oracle, log.arrays())[0]
    assert log.text_at() == now.encode()
    assert len({t for _, t in marks}) > 20
    for m, rec in marks:
        assert log.text_at(m) == rec.encode()
        assert log.text_info(m) == tu.want_info(rec, 0, len(rec))
        bd = tu.boundaries(rec)
        for _ in range(6):
            a = rng.randint(0, len(rec))
            b = rng.randint(a, len(rec))
            tu.check_window(log, m, rec, a, b, bd)
        assert pu.apply_patches(log.text_at(m).decode(), log.patches_since(m)) == now


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_in_their_order(kind):
    fugue = kind == "fugue"
    log = small_doc(fugue)
    text = log.text_at().decode()
    bd = tu.boundaries(text)
    nb, inside = bd[-1], next(x for x in range(bd[-1]) if x not in set(bd))
    m = log.mark()
    other = log.clone().mark()                     # a clone is another owner
    ok = tu.raw(log, m, 0, tu.END, 0, nb)
    assert ok[0] == 0 and ok[1] == text.encode() and ok[2] == nb
    # each refusal alone
    tu.assert_refused(log, other, 0, 1, 0, tu.EINVAL)
    tu.assert_refused(log, None, 0, 1, 2, tu.EINVAL)
    tu.assert_refused(log, None, 0, 1, 3, tu.EINVAL)
    tu.assert_refused(log, None, 0, 1, 0, tu.EINVAL, null_len=True)
    tu.assert_refused(log, None, 5, 4, 0, tu.EINVAL)
    tu.assert_refused(log, None, 41, tu.END, 0, tu.ERANGE)
    tu.assert_refused(log, None, 0, 41, 0, tu.ERANGE)
    tu.assert_refused(log, None, nb + 1, tu.END, tu.BYTES, tu.ERANGE)
    tu.assert_refused(log, None, 0, nb + 1, tu.BYTES, tu.ERANGE)
    tu.assert_refused(log, None, inside, tu.END, tu.BYTES, tu.EINVAL)
    tu.assert_refused(log, None, 0, inside, tu.BYTES, tu.EINVAL)
    # two faults in one call: the earlier check's code
    tu.assert_refused(log, other, 41, tu.END, 0, tu.EINVAL)                 # 1 before 4
    tu.assert_refused(log, None, 41, tu.END, 2, tu.EINVAL)                  # 2 before 4
    tu.assert_refused(log, None, 41, tu.END, 0, tu.EINVAL, null_len=True)   # 2 before 4
    tu.assert_refused(log, None, 45, 42, 0, tu.EINVAL)                      # 3 before 4
    tu.assert_refused(log, None, inside, nb + 1, tu.BYTES, tu.ERANGE)       # 4 before 5
    tu.assert_refused(log, None, 41, tu.END, 0, tu.ERANGE, cap=0)           # 4 before 7
    tu.assert_refused(log, None, inside, tu.END, tu.BYTES, tu.EINVAL, cap=0)  # 5 before 7
    # ESPACE: one byte short, and no buffer at all; *out_len and *info are set, out is untouched
    want = tu.want_info(text, 3, 30)
    for kw in ({"cap": want["n_bytes"] - 1}, {"cap": 64, "null_out": True}):
        rc, buf, n, inf = tu.raw(log, m, 3, 30, 0, **kw)
        assert rc == tu.ESPACE and n == want["n_bytes"] and inf == want
        assert buf == bytes([tu.CANARY]) * kw["cap"]
    rc, buf, n, inf = tu.raw(log, m, 3, 30, 0, want["n_bytes"], info=False)   # info may be NULL
    assert rc == 0 and buf == text[3:30].encode() and n == want["n_bytes"]
    # empty windows, an empty version and an empty log are ok, with no buffer
    for start in (0, 17, 40):
        assert tu.raw(log, None, start, start, 0, 0)[::2] == (0, 0)
    empty = pu.new_log(fugue)
    m0 = empty.mark()
    assert tu.raw(empty, None, 0, tu.END, 0, 0)[::2] == (0, 0)
    tu.assert_refused(empty, None, 1, tu.END, 0, tu.ERANGE)
    empty.insert(0, "later")
    assert empty.text_at(m0) == b"" and empty.text_info(m0)["len"] == 0
    tu.assert_refused(empty, m0, 0, 1, 0, tu.ERANGE)
    # nothing in the log changed, and the marks still read the same
    assert log.text_at(m) == text.encode()


def test_the_adapter_reads_windows_and_marked_versions():
    d = crdt_hip.HipMerge.from_str("héllo wörld")
    m = d.mark()
    d.insert(5, " €uro")
    assert d.text_range(0, 5) == "héllo" and d.text_range(5) == " €uro wörld"
    assert d.text_at(m) == "héllo wörld" and d.text_at(m, 6, 8) == "wö"
    with pytest.raises(crdt_hip.CrdtHipError):
        d.text_range(0, 99)
