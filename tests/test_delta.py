"""Host delta sync (crdt_hip_oplog_state_vector / encode_diff / apply_diff), CPU only.

The reference's Yrs Downstream exchanges a state vector and a diff against it
(rope.rs:252-255: state_vector(), encode_diff_v1(&sv), apply_update).  Here the state vector and
the delta's bytes are compared with plain Python restatements (delta_util), and the log after an
apply with the Python union of the two logs (join_util.union), slot for slot, and through the CPU
oracle's merge.
"""
import random
import struct

import numpy as np
import pytest

import crdt_hip
import delta_util as du
import join_fugue_util as jf
from join_util import (assert_same_log, assert_unique_identities, crafted, fork, random_edits,
                       to_anchor)


@pytest.fixture(scope="module")
def forks():
    base, nb, a, b = du.scripted_forks()
    c = fork(base, 3, 33, 60)
    assert_unique_identities(a.arrays(), b.arrays(), c.arrays())
    du.assert_cases(base.arrays(), a.arrays(), b.arrays())
    return base, nb, a, b, c


def sync(dst: crdt_hip.OpLog, src: crdt_hip.OpLog) -> tuple:
    return dst.apply_diff(src.encode_diff(dst.state_vector()))


def raises(code, fn, *args):
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)


def test_state_vector_and_bytes_equal_the_restatement(forks):
    base, nb, a, b, c = forks
    for log, peer in ((a, b), (b, a), (c, a), (base, a)):
        arrs = log.arrays()
        assert log.state_vector() == du.state_vector(arrs)
        for sv in ([], du.state_vector(peer.arrays()), du.state_vector(arrs)):
            assert log.encode_diff(sv) == du.encode_diff(arrs, sv)
    # against its own vector a log sends no item, and still every tombstone
    own = du.decode_diff(a.encode_diff(a.state_vector()))
    assert own["n"] == 0 and sum(own["rcount"]) == int(a.arrays().deleted.sum()) > 0
    # against the empty vector: the whole log, in slot order, and no range
    whole = du.decode_diff(a.encode_diff([]))
    assert whole["key"] == du.keys(a.arrays()) and whole["r"] == 0
    # the peer's vector covers the base: only the fork's own items travel
    d = du.decode_diff(b.encode_diff(a.state_vector()))
    assert d["n"] == b.arrays().n - nb and d["r"] > 0


def test_apply_equals_the_union(oracle, forks):
    _, _, a, b, _ = forks
    want, added, tomb = du.union(a.arrays(), b.arrays())
    assert added > 0 and tomb > 0
    dst = a.clone()
    v0 = dst.version()
    delta = b.encode_diff(dst.state_vector())
    assert dst.apply_diff(delta) == (added, tomb)
    assert_same_log(dst.arrays(), want, oright=False)
    assert (dst.arrays().origin_right[a.arrays().n:] == 0xFFFFFFFF).all()
    assert oracle.merge(to_anchor(dst.arrays())) == oracle.merge(to_anchor(want))
    # newly tombstoned ids and appended tombstones went to the delete ops
    assert (dst.version() >> 32, (dst.version() - v0) & 0xFFFFFFFF) == (
        want.n, tomb + int(want.deleted[a.arrays().n:].sum()))
    v = dst.version()
    assert dst.apply_diff(delta) == (0, 0)
    assert dst.version() == v
    assert_same_log(dst.arrays(), want, oright=False)
    # the same log as the host join with origin_right absent
    hj = a.clone()
    src = b.arrays()
    hj.join(crdt_hip.LogArrays(src.parent, src.lamport, src.agent, src.deleted, src.cp))
    assert_same_log(dst.arrays(), hj.arrays())
    # positional edits go on after an apply (the resolver index is rebuilt)
    dst.insert(0, "!")
    assert oracle.merge(to_anchor(dst.arrays())).startswith(b"!")


def test_stale_vector(oracle, forks):
    _, _, a, b, c = forks
    dst = a.clone()
    old = dst.state_vector()
    dst.join(c)
    delta = b.encode_diff(old)         # made before dst took c; b has taken c since
    b2 = b.clone()
    b2.join(c)
    delta2 = b2.encode_diff(old)       # carries c's items too: dst holds them already
    want, added, tomb = du.union(dst.arrays(), b.arrays())
    d1 = dst.clone()
    assert d1.apply_diff(delta) == (added, tomb)
    assert_same_log(d1.arrays(), want, oright=False)
    want2, added2, tomb2 = du.union(dst.arrays(), b2.arrays())
    assert du.decode_diff(delta2)["n"] > added2 == added
    assert dst.apply_diff(delta2) == (added2, tomb2)
    assert_same_log(dst.arrays(), want2, oright=False)
    assert oracle.merge(to_anchor(dst.arrays())) == oracle.merge(to_anchor(want))


def test_three_peers_in_a_ring(oracle, forks):
    _, _, a, b, c = forks
    peers = [a.clone(), b.clone(), c.clone()]
    for _ in range(4):
        moved = 0
        for i in range(3):
            dst, src = peers[i], peers[(i + 1) % 3]
            delta = src.encode_diff(dst.state_vector())
            got = dst.apply_diff(delta)
            moved += got[0] + got[1]
        if not moved:
            break
    assert moved == 0
    for i in range(3):      # no delta carries anything: no item, and no tombstone that is news
        dst, src = peers[i], peers[(i + 2) % 3]
        assert du.decode_diff(src.encode_diff(dst.state_vector()))["n"] == 0
    texts = {oracle.merge(to_anchor(p.arrays())) for p in peers}
    assert len(texts) == 1
    sets = []
    for p in peers:
        d = du.decode_diff(p.encode_diff([]))
        sets.append(sorted(zip(d["key"], d["pkey"], d["cp"])))
    assert sets[0] == sets[1] == sets[2] and len(sets[0]) == peers[0].arrays().n


def test_range_edges():
    arrs = du.range_edges()
    log = du.host_log(arrs)
    assert_same_log(log.arrays(), arrs, oright=False)
    data = log.encode_diff(du.range_edges_sv())
    assert data == du.encode_diff(arrs, du.range_edges_sv())
    assert du.ranges(data) == du.range_edges_want()
    assert du.decode_diff(data)["key"] == [(22 << 16) | 3]
    # applied to a copy without the tombstones: the ranges delete the covered ones, and the one
    # item that travels (the copy holds it) brings its own tombstone
    live = du.host_log(crafted(arrs.parent, arrs.lamport, arrs.agent, arrs.cp))
    assert live.apply_diff(data) == (0, int(arrs.deleted.sum()))
    assert_same_log(live.arrays(), arrs, oright=False)
    # the ranges alone leave that item alive
    d = du.decode_diff(data)
    live = du.host_log(crafted(arrs.parent, arrs.lamport, arrs.agent, arrs.cp))
    assert live.apply_diff(du.pack(1, [], [], [], d["rkey"], d["rcount"])) == (0, int(arrs.deleted.sum()) - 1)
    assert live.arrays().deleted.tolist() == [x if i != 11 else 0 for i, x in enumerate(arrs.deleted.tolist())]


def test_agent_and_lamport_edges():
    #                parent        lamport          agent               cp
    arrs = crafted([0, 1, 0, 3], [0, 1, 0, 7], [0, 0, 65535, 65535], [97, 98, 99, 100], [1, 0, 0, 1])
    log = du.host_log(arrs)
    assert log.state_vector() == [(0, 1), (65535, 7)] == du.state_vector(arrs)
    only0 = du.host_log(crafted([0], [0], [0], [97]))
    assert only0.state_vector() == [(0, 0)]                  # a lamport-0 item still has an entry
    for sv in ([], [(0, 0)], [(0, 1)], [(65535, 0)], [(0, 1), (65535, 7)]):
        assert log.encode_diff(sv) == du.encode_diff(arrs, sv)
    assert du.ranges(log.encode_diff([(0, 0)])) == [(0, 1)]   # identity 0: agent 0, lamport 0
    assert only0.apply_diff(log.encode_diff(only0.state_vector())) == (3, 1)
    assert_same_log(only0.arrays(), arrs, oright=False)
    many = crdt_hip.OpLog.synth_agents(3000, 64, 7)
    M = many.arrays()
    assert len(many.state_vector()) == 64 and many.state_vector() == du.state_vector(M)
    half = [(ag, lam // 2) for ag, lam in du.state_vector(M)][::2]
    for sv in ([], half, du.state_vector(M)):
        assert many.encode_diff(sv) == du.encode_diff(M, sv)
    empty = crdt_hip.OpLog()
    assert empty.state_vector() == []
    assert empty.apply_diff(many.encode_diff([])) == (M.n, 0)
    assert_same_log(empty.arrays(), M, oright=False)
    assert empty.encode_diff([]) == many.encode_diff([])


def test_fugue(oracle):
    base, nb, a, b = jf.scripted_forks((20, 20))
    A, B = a.arrays(), b.arrays()
    assert a.state_vector() == du.state_vector(A)
    for sv in ([], du.state_vector(B), du.state_vector(A)):
        assert a.encode_diff(sv) == du.encode_diff(A, sv)
    assert struct.unpack_from("<2I", a.encode_diff([]))[1] == 2
    want, added, tomb = du.union(A, B)
    dst = a.clone()
    delta = b.encode_diff(dst.state_vector())
    d = du.decode_diff(delta)
    assert any(c & du.SIDE for c in d["cp"])                  # left children travel
    assert dst.apply_diff(delta) == (added, tomb)
    jf.assert_same_log(dst.arrays(), want)
    assert (dst.arrays().side[A.n:] == 1).any()               # ... and keep their side
    assert jf.merged(oracle, dst.arrays()) == jf.merged(oracle, want)
    assert dst.apply_diff(delta) == (0, 0)
    # the kinds do not mix, whatever the contents
    rga = crdt_hip.OpLog(agent=5)
    rga.insert(0, "abc")
    before = rga.arrays()
    raises(du.EINVAL, rga.apply_diff, delta)
    raises(du.EINVAL, dst.apply_diff, rga.encode_diff([]))
    raises(du.EINVAL, crdt_hip.OpLog(fugue=True).apply_diff, crdt_hip.OpLog().encode_diff([]))
    assert_same_log(rga.arrays(), before)
    # a left child of the document start
    k = (9 << 16) | 7
    raises(du.EBADLOG, dst.apply_diff, du.pack(2, [k], [du.START], [120 | du.SIDE], [], []))
    raises(du.EBADLOG, dst.apply_diff, du.pack(2, [(0xFFFFFFFF << 16) | 7], [du.START], [120], [], []))
    jf.assert_same_log(dst.arrays(), want)


def rejections(dst_arrs: crdt_hip.LogArrays, src_arrs: crdt_hip.LogArrays) -> list:
    """(name, error code, bytes): every rejection of apply_diff, made by editing the bytes of the
    restated delta of src against dst's vector.  src holds new items whose parents are new too,
    and tombstones dst lacks."""
    good = du.encode_diff(src_arrs, du.state_vector(dst_arrs))
    d = du.decode_diff(good)
    assert d["n"] >= 3 and d["r"] >= 1
    child = next(i for i in range(1, d["n"]) if d["pkey"][i] == d["key"][i - 1])   # a new parent
    out = []

    def case(name, code, **edits):
        e = {k: list(v) if isinstance(v, list) else v for k, v in d.items()}
        for k, fn in edits.items():
            fn(e[k])
        out.append((name, code, du.repack(e)))

    def setv(i, v):
        return lambda col: col.__setitem__(i, v)

    out.append(("magic", du.EINVAL, b"XXXX" + good[4:]))
    out.append(("version", du.EINVAL, good[:4] + struct.pack("<I", 3) + good[8:]))
    out.append(("other_kind", du.EINVAL, good[:4] + struct.pack("<I", 2) + good[8:]))
    out.append(("truncated", du.EINVAL, good[:-4]))
    out.append(("short_header", du.EINVAL, good[:12]))
    out.append(("oversized", du.EINVAL, good + b"\0\0\0\0"))
    out.append(("n_too_large", du.EINVAL, good[:8] + struct.pack("<I", 0x0FFFFFFF) + good[12:]))
    case("zero_count", du.EINVAL, rcount=setv(0, 0))
    case("dup_item", du.EBADLOG, key=setv(1, d["key"][0]))
    case("unknown_parent", du.EBADLOG, pkey=setv(0, (0x7FFF << 16) | 9))
    case("parent_after_item", du.EBADLOG, pkey=setv(child - 1, d["key"][child]))
    case("identity_too_large", du.EBADLOG, key=setv(0, 1 << 50))
    case("reserved_cp_bits", du.EBADLOG, cp=setv(0, d["cp"][0] | (1 << 25)))
    case("range_unknown", du.EBADLOG, rkey=setv(0, (0x7FFF << 16) | 9))
    case("range_runs_off", du.EBADLOG, rcount=setv(0, d["rcount"][0] + 5000))
    case("range_huge", du.EBADLOG, rcount=setv(0, 0xFFFFFFFF))
    # a range whose first item is known and whose second is not: the base agent's last item
    top0 = int(dst_arrs.lamport[dst_arrs.agent == 0].max())
    assert top0 == int(src_arrs.lamport[src_arrs.agent == 0].max())
    case("range_past_the_end", du.EBADLOG, rkey=setv(0, top0 << 16), rcount=setv(0, 2))
    # an item dst holds, sent again with another codepoint / parent
    k = du.keys(dst_arrs)
    held = next(i for i in range(dst_arrs.n) if dst_arrs.parent[i])
    pk = k[int(dst_arrs.parent[held]) - 1]
    cpw = int(dst_arrs.cp[held])
    out.append(("shared_cp", du.EBADLOG, du.pack(1, [k[held]], [pk], [cpw ^ 1], [], [])))
    out.append(("shared_parent", du.EBADLOG, du.pack(1, [k[held]], [du.START], [cpw], [], [])))
    out.append(("shared_parent_unknown", du.EBADLOG, du.pack(1, [k[held]], [(0x7FFF << 16) | 9], [cpw], [], [])))
    return out


def fugue_rejections(dst_arrs: crdt_hip.LogArrays) -> list:
    k = du.keys(dst_arrs)
    held = next(i for i in range(dst_arrs.n) if dst_arrs.parent[i])
    pk = k[int(dst_arrs.parent[held]) - 1]
    cpw = int(dst_arrs.cp[held]) | (du.SIDE if dst_arrs.side[held] else 0)
    new = (0x7000 << 16) | 77
    return [("shared_side", du.EBADLOG, du.pack(2, [k[held]], [pk], [cpw ^ du.SIDE], [], [])),
            ("left_of_start", du.EBADLOG, du.pack(2, [new], [du.START], [120 | du.SIDE], [], [])),
            ("lamport_max", du.EBADLOG, du.pack(2, [(0xFFFFFFFF << 16) | 7], [pk], [120], [], [])),
            ("rga_delta", du.EINVAL, du.pack(1, [new], [pk], [120], [], []))]


def test_rejections_change_nothing(forks):
    _, _, a, b, _ = forks
    A = a.arrays()
    cases = rejections(A, b.arrays())
    assert len({name for name, _, _ in cases}) == len(cases) >= 19
    dst = a.clone()
    v = dst.version()
    for name, code, data in cases:
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            dst.apply_diff(data)
        assert e.value.code == code, (name, str(e.value))
        assert dst.version() == v, name
        assert_same_log(dst.arrays(), A)
    _, _, fa, _ = jf.scripted_forks()
    FA = fa.arrays()
    for name, code, data in fugue_rejections(FA):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            fa.apply_diff(data)
        assert e.value.code == code, (name, str(e.value))
        jf.assert_same_log(fa.arrays(), FA)
    # the log still takes the good delta
    want, added, tomb = du.union(A, b.arrays())
    assert sync(dst, b) == (added, tomb)
    assert_same_log(dst.arrays(), want, oright=False)


def test_espace_and_unsorted_vectors(forks):
    import ctypes as C
    _, _, a, b, _ = forks
    L = crdt_hip.lib()
    n = C.c_size_t(0)
    assert L.crdt_hip_oplog_state_vector(a._h, None, 0, C.byref(n)) == du.ESPACE and n.value == 2
    out = (crdt_hip.SvEntry * 2)()
    n.value = 0
    assert L.crdt_hip_oplog_state_vector(a._h, out, 1, C.byref(n)) == du.ESPACE and n.value == 2
    assert L.crdt_hip_oplog_state_vector(a._h, out, 2, C.byref(n)) == 0
    assert [(e.agent, e.lamport) for e in out] == a.state_vector()
    want = a.encode_diff([])
    need = C.c_size_t(0)
    assert L.crdt_hip_oplog_encode_diff(a._h, None, 0, None, 0, C.byref(need)) == du.ESPACE
    assert need.value == len(want) == 16 + 20 * a.arrays().n
    buf = C.create_string_buffer(len(want))
    need.value = 0
    assert L.crdt_hip_oplog_encode_diff(a._h, None, 0, buf, len(want) - 1, C.byref(need)) == du.ESPACE
    assert need.value == len(want)
    assert L.crdt_hip_oplog_encode_diff(a._h, None, 0, buf, len(want), C.byref(need)) == 0
    assert buf.raw == want
    for sv in ([(2, 5), (1, 5)], [(1, 5), (1, 6)], [(65536, 1)], [(1, 1), (70000, 1)]):
        raises(du.EINVAL, a.encode_diff, sv)
    assert a.encode_diff([(1, 5), (2, 0xFFFFFFFF)]) == du.encode_diff(a.arrays(), [(1, 5), (2, 0xFFFFFFFF)])


def test_hipmerge_sync_from(oracle, forks):
    _, _, a, b, _ = forks
    x, y = crdt_hip.HipMerge(a.clone()), crdt_hip.HipMerge(b.clone())
    want, added, tomb = du.union(a.arrays(), b.arrays())
    got = x.sync_from(y)
    assert got[:2] == (added, tomb) and got[2] == len(du.encode_diff(b.arrays(), du.state_vector(a.arrays())))
    assert got[2] < len(b.encode_diff([]))
    assert_same_log(x.log.arrays(), want, oright=False)
    assert x.sync_from(y)[:2] == (0, 0)
