"""Byte-offset edits and patches on the host (crdt_hip_oplog_apply_patches_bytes / _replace_bytes /
_patches_since_bytes / _visible_bytes).

The result of a byte edit is defined through the codepoint call: a clone that got the same patches
in codepoints, one crdt_hip_oplog_replace each, must hold the same log slot for slot
(edit_util.same_logs).  The byte patch lists come from a plain Python string model
(bytes_util.to_bytes), and every parity test asserts that its byte list differs from its codepoint
list, so that none passes by treating bytes as codepoints.  A rejected call returns its code and
leaves the log as it was.  CPU only.
"""
import random

import pytest

import bytes_util as bu
import crdt_hip
import edit_util as eu
import patch_util as pu
from conftest import trace_path
from edit_util import KINDS
from test_patches import TEXT, typed


def both(oracle, log: crdt_hip.OpLog, text: str, plist) -> tuple:
    """apply_patches_bytes on `log`, the codepoint replace loop on a clone: the same log, and the
    model's text.  Returns (the new text, the byte patch list)."""
    plist_b = bu.to_bytes(text, plist)
    ref = log.clone()
    eu.replace_loop(ref, plist)
    assert log.visible_bytes() == bu.blen(text)
    assert log.apply_patches_bytes(plist_b) == bu.counts(plist)
    eu.same_logs(log, ref)
    want = eu.model_apply(text, plist)
    assert bu.apply_bytes(text.encode(), plist_b) == want.encode()
    if oracle is not None:
        assert pu.oracle_merge(oracle, log.arrays())[0] == want
    assert log.visible_len() == len(want) and log.visible_bytes() == bu.blen(want)
    return want, plist_b


@pytest.mark.parametrize("kind", KINDS)
def test_single_edits(oracle, kind):
    fugue = kind == "fugue"
    n = len(TEXT)
    i2, i3, i4 = TEXT.index("é"), TEXT.index("€"), TEXT.index("😀")
    cases = [(0, 0, "é"), (n, 0, "end€"), (n - 5, 5, ""), (0, n, ""),
             (i2 + 1, 1, "X"), (i2, 1, "x"), (i2 - 1, 2, "ß"),          # next to a 2-byte character
             (i3 + 1, 2, "Y"), (i3, 1, "E"), (i3 - 1, 1, ""),           # a 3-byte one
             (i4 + 1, 1, "z"), (i4, 1, ""), (i4 - 1, 3, "€😀"), (i4 + 1, 0, "é")]   # a 4-byte one
    seen_c, seen_b = [], []
    for p in cases:
        _, pb = both(oracle, typed(fugue), TEXT, [p])
        seen_c += [p]
        seen_b += pb
    assert sum(a != b for a, b in zip(seen_c, seen_b)) >= 10
    log = pu.new_log(fugue)                            # the empty log
    assert log.visible_bytes() == 0
    assert both(oracle, log, "", [(0, 0, "héllo")])[0] == "héllo"
    assert log.apply_patches_bytes([]) == (0, 0)
    assert both(oracle, log, "héllo", [(5, 0, "!")])[1] == [(6, 0, "!")]


@pytest.mark.parametrize("kind", KINDS)
def test_replace_insert_remove_are_one_patch_each(kind):
    fugue = kind == "fugue"
    log, ref = typed(fugue), typed(fugue)
    b = lambda k: bu.blen(TEXT[:k])                    # noqa: E731
    assert b(3) != 3
    log.insert_bytes(b(3), "aé")                       # TEXT[:3] + "aé" + TEXT[3:]
    log.remove_bytes(0, b(2))                          # drops "hé"
    log.replace_bytes(b(5), b(7), "€")                 # "laélo" is as long as "héllo"
    before = log.encode_diff([])
    log.replace_bytes(4, 4, "")                        # Upstream::replace of nothing: a no-op
    assert log.encode_diff([]) == before
    eu.replace_loop(ref, [(3, 0, "aé"), (0, 2, ""), (5, 2, "€")])
    eu.same_logs(log, ref)
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        log.remove_bytes(3, 2)
    assert e.value.code == -2


@pytest.mark.parametrize("kind", KINDS)
def test_many_patches(kind):
    text, plist = bu.aeu(3000)
    log = typed(kind == "fugue", text)
    want, plist_b = both(None, log, text, plist)
    assert want == "a€" * 3000 + "a"
    assert plist_b[0] == (1, 2, "€") and plist_b[-1] == (1 + 4 * 2999, 2, "€")
    assert all(a != b for a, b in zip(plist[1:], plist_b[1:])) and plist[0] != plist_b[0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_patch_sets_between_joins(oracle, kind, seed):
    fugue = kind == "fugue"
    rng = random.Random(140 + seed)
    log = eu.two_agent_log(fugue, rng.randint(2000, 4000), seed)
    log.set_agent(5)
    other = log.clone()
    other.set_agent(6)
    for step in range(3):
        log.insert(0, "é")                             # a multi-byte character before every patch
        text = pu.oracle_merge(oracle, log.arrays())[0]
        plist = bu.shifted(eu.random_patches(rng, len(text) - 1, rng.choice([1, 20, 200])))
        text, plist_b = both(oracle, log, text, plist)
        assert all(a[0] != b[0] for a, b in zip(plist, plist_b))
        # a join in between: the next call takes the order from the log, not from the index
        eu.replace_loop(other, eu.random_patches(rng, other.visible_len(), 10))
        log.join(other)
    assert log.arrays().n > 2000


@pytest.mark.parametrize("kind", KINDS)
def test_rejected_calls_change_nothing(kind):
    log = typed(kind == "fugue")
    before = (log.encode_diff([]), log.encode_from(0), log.version(), log.visible_len(),
              log.visible_bytes())
    for name, rows, ins, code in bu.rejections(TEXT):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            log.apply_patches_bytes(*bu.raw(rows, ins))
        assert e.value.code == code, name
        assert (log.encode_diff([]), log.encode_from(0), log.version(), log.visible_len(),
                log.visible_bytes()) == before, name
    for k in (1, 2, 3):                                # the same through replace_bytes
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            log.replace_bytes(bu.inside(TEXT, "😀") + k, bu.inside(TEXT, "😀") + 4, "")
        assert e.value.code == -1
    assert log.encode_diff([]) == before[0]
    # the lamport bound comes after the boundary check
    big = pu.new_log(kind == "fugue")
    big.join(crdt_hip.LogArrays([0], [0xFFFFFFF0], [1], [0], [ord("é")],
                                side=[0] if kind == "fugue" else None))
    snap = big.encode_diff([])
    for pos, code in ((1, -1), (2, -2)):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            big.apply_patches_bytes([(pos, 0, "x" * 15)])
        assert e.value.code == code and big.encode_diff([]) == snap
    assert big.apply_patches_bytes([(2, 0, "x" * 14)]) == (14, 0)


def check_since(oracle, log, mark, text_at_mark: str) -> list:
    """patches_since_bytes against to_bytes of patches_since through the text at the mark, and the
    byte splice of the mark's UTF-8 against the UTF-8 now."""
    got = log.patches_since_bytes(mark)
    assert got == bu.to_bytes(text_at_mark, log.patches_since(mark))
    now = pu.oracle_merge(oracle, log.arrays())[0]
    assert bu.apply_bytes(text_at_mark.encode(), got) == now.encode()
    for (p0, _, i0), (p1, _, _) in zip(got, got[1:]):  # they never touch, in bytes
        assert p1 > p0 + bu.blen(i0)
    pu.assert_raw(log.patches_since_bytes_raw(mark))
    return got


@pytest.mark.parametrize("kind", KINDS)
def test_patches_since_bytes(oracle, kind):
    fugue = kind == "fugue"
    log = typed(fugue)
    m = log.mark()
    assert log.patches_since_bytes(m) == []            # nothing changed
    i2 = TEXT.index("é")
    log.replace(i2, i2 + 1, "€")                       # D and I items interleave into one run
    log.replace(i2 + 1, i2 + 2, "ß")
    log.insert(i2 + 1, "😀")
    got = check_since(oracle, log, m, TEXT)
    assert got == [(i2, 3, "€😀ß")]
    log.insert(len(TEXT) + 1, "tail")
    assert check_since(oracle, log, m, TEXT)[1] == (bu.blen(TEXT) + 6, 0, "tail")
    # seeded edits, a join and a delta after a mark on a log of two agents
    log = eu.two_agent_log(fugue, 1500, 31)
    log.insert(0, "é")
    m = log.mark()
    at = pu.oracle_merge(oracle, log.arrays())[0]
    fork = log.clone()
    fork.set_agent(9)
    rng = random.Random(8)
    eu.replace_loop(log, bu.shifted(eu.random_patches(rng, len(at) - 1, 60)))
    eu.replace_loop(fork, bu.shifted(eu.random_patches(rng, len(at) - 1, 60)))
    got = check_since(oracle, log, m, at)
    assert len(got) >= 3 and got != log.patches_since(m)
    log.join(fork)
    got = check_since(oracle, log, m, at)
    assert len(got) >= 3 and all(a[0] != b[0] for a, b in zip(got, log.patches_since(m)))


def test_rustcode_windows_in_bytes():
    """Real data: the stretches of rustcode in which byte and codepoint offsets differ, applied one
    patch per call through replace_bytes from a trace that went through chars_to_bytes, against
    the codepoint replay."""
    cp_trace = crdt_hip.Trace(trace_path("rustcode"))
    b_trace = crdt_hip.Trace(trace_path("rustcode"))
    b_trace.chars_to_bytes()
    assert "÷" in cp_trace.patch(4400)[2]
    assert cp_trace.patch(4401)[1] == 1 and b_trace.patch(4401)[1] == 2
    assert cp_trace.patch(6233)[1] == 8 and b_trace.patch(6233)[1] == 9
    log, ref = crdt_hip.OpLog(), crdt_hip.OpLog()
    if cp_trace.start_content:
        log.insert(0, cp_trace.start_content)
        ref.insert(0, cp_trace.start_content)
    done = 0
    for first, last, differs in bu.RUSTCODE_WINDOWS:
        assert cp_trace.patch(differs) != b_trace.patch(differs)
        bu.replay(cp_trace, log, done, first)
        bu.replay(cp_trace, ref, done, last)
        for i in range(first, last):
            pos, dele, ins = b_trace.patch(i)
            log.replace_bytes(pos, pos + dele, ins)
        eu.same_logs(log, ref)
        done = last
