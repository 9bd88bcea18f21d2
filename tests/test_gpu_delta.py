"""Device delta sync (crdt_hip_replica_state_vector / encode_diff / apply_diff, delta.hip).

The reference's Yrs Downstream exchanges a state vector and a diff against it
(rope.rs:252-255: state_vector(), encode_diff_v1(&sv), apply_update).  The device calls must give
the host's bytes, byte for byte, and the host's log, slot for slot: a delta against the empty
vector is the whole log in identity-anchored form, so `rep.encode_diff([])` reads a replica's log
back.  Expected results are computed without the product (delta_util restatements, join_util.union,
the CPU oracle).  Besides the ~300-item forks of the CPU file, one pair of ~2,500-item logs makes
every kernel run several 256-thread blocks, with a 700-slot tombstone range across block
boundaries.
"""
import random

import numpy as np
import pytest

import crdt_hip
import delta_util as du
import join_fugue_util as jf
from edit_util import ALPHABET
from join_util import (assert_same_log, assert_unique_identities, base_log, fork, to_anchor,
                       visible)
from test_delta import fugue_rejections, rejections

pytestmark = pytest.mark.gpu


def expect(oracle, arrs):
    """(text, digest, info) of a log, by the oracle."""
    if arrs.side is not None:
        return jf.expect(oracle, arrs)
    text = oracle.merge(to_anchor(arrs))
    cps, nbytes = visible(arrs)
    assert nbytes == len(text) and cps == len(text.decode())
    return text, oracle.tree_digest(text), (arrs.n, cps, nbytes)


def check(oracle, rep, arrs):
    text, dig, info = expect(oracle, arrs)
    got_text, got_dig = rep.merge()
    assert got_text == text
    assert got_dig == dig
    assert rep.info() == info


@pytest.fixture
def mk(ctx):
    """Replica factory that closes what it made when the test ends (a replica must be freed
    before its context)."""
    made = []

    def make(init=None):
        r = init if isinstance(init, crdt_hip.Replica) else crdt_hip.Replica(ctx, init)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


@pytest.fixture(scope="module")
def forks():
    base, nb, a, b = du.scripted_forks()
    c = fork(base, 3, 33, 60)
    assert_unique_identities(a.arrays(), b.arrays(), c.arrays())
    du.assert_cases(base.arrays(), a.arrays(), b.arrays())
    return base, nb, a, b, c


@pytest.fixture(scope="module")
def big():
    x, y = du.big_log()
    X, Y = x.arrays(), y.arrays()
    assert 2300 < X.n < 2900 and 2300 < Y.n < 2900
    d = du.decode_diff(du.encode_diff(Y, du.state_vector(X)))
    assert max(d["rcount"]) >= 700 and d["n"] > 512       # one range across block boundaries
    return x, y


@pytest.fixture(scope="module")
def fforks():
    _, _, a, b = jf.scripted_forks((20, 20))
    return a, b


def host_sync(dst, src):
    out = dst.clone()
    got = out.apply_diff(src.encode_diff(out.state_vector()))
    return out, got


def test_state_vector(mk, forks, big, fforks):
    _, _, a, b, c = forks
    many = crdt_hip.OpLog.synth_agents(3000, 64, 7)
    for log in (a, b, c, many) + big + fforks:
        want = du.state_vector(log.arrays())
        assert log.state_vector() == want
        assert mk(log).state_vector() == want
    assert len(du.state_vector(many.arrays())) == 64
    assert mk().state_vector() == []
    edges = du.host_log(du.join_util.crafted([0, 1, 0, 3], [0, 1, 0, 7], [0, 0, 65535, 65535],
                                             [97, 98, 99, 100], [1, 0, 0, 1]))
    assert mk(edges).state_vector() == [(0, 1), (65535, 7)]
    assert mk(du.host_log(du.join_util.crafted([0], [0], [0], [97]))).state_vector() == [(0, 0)]


@pytest.mark.parametrize("pair", ["forks", "big", "fugue", "agents64", "edges"])
def test_encode_bytes_equal_the_hosts(ctx, mk, forks, big, fforks, pair):
    if pair == "forks":
        log, peer = forks[2], forks[3]
    elif pair == "big":
        peer, log = big
    elif pair == "fugue":
        log, peer = fforks
    elif pair == "agents64":
        log = crdt_hip.OpLog.synth_agents(3000, 64, 7)
        peer = du.host_log(log.arrays())
        peer.remove(0, 40)
        log, peer = peer, log
    else:
        log = du.host_log(du.range_edges())
        peer = du.host_log(du.join_util.crafted([0], [1], [1], [97]))
    arrs = log.arrays()
    rep = mk(log)
    before = (rep.merge(), rep.info())
    vectors = [[], du.state_vector(peer.arrays()), du.state_vector(arrs)]
    if pair == "agents64":
        vectors.append([(ag, lam // 2) for ag, lam in du.state_vector(arrs)][::2])
    if pair == "edges":
        vectors.append(du.range_edges_sv())
    for sv in vectors:
        want = du.encode_diff(arrs, sv)
        assert log.encode_diff(sv) == want
        got = rep.encode_diff(sv)
        assert got == want
        d = du.decode_diff(got)
        st = ctx.delta_stats()
        assert (st["items"], st["ranges"], st["table_slots"]) == (d["n"], d["r"], 0)
    if pair == "edges":
        assert du.ranges(rep.encode_diff(du.range_edges_sv())) == du.range_edges_want()
    assert (rep.merge(), rep.info()) == before             # encode_diff leaves the replica as it was
    assert mk(crdt_hip.OpLog(fugue=pair == "fugue")).encode_diff([]) == crdt_hip.OpLog(
        fugue=pair == "fugue").encode_diff([])


@pytest.mark.parametrize("contraction", [1, 2])
@pytest.mark.parametrize("pair", ["forks", "big", "fugue"])
def test_apply_equals_the_union_slot_for_slot(ctx, mk, oracle, forks, big, fforks, pair, contraction):
    a, b = {"forks": forks[2:4], "big": big, "fugue": fforks}[pair]
    A, B = a.arrays(), b.arrays()
    want, added, tomb = du.union(A, B)
    assert added > 0 and tomb > 0
    hj, got = host_sync(a, b)
    assert got == (added, tomb)
    ctx.set_param("contraction", contraction)
    try:
        dst, src = mk(a), mk(b)
        src_before = (src.merge(), src.info(), src.encode_diff([]))
        delta = src.encode_diff(dst.state_vector())
        assert delta == du.encode_diff(B, du.state_vector(A))
        assert dst.apply_diff(delta) == (added, tomb)
        st = ctx.delta_stats()
        d = du.decode_diff(delta)
        assert (st["items"], st["ranges"], st["table_slots"]) == (d["n"], d["r"], A.n)
        check(oracle, dst, want)
        # slot for slot: the replica's whole log, read back as a delta
        assert dst.encode_diff([]) == hj.encode_diff([]) == du.encode_diff(want, [])
        assert (src.merge(), src.info(), src.encode_diff([])) == src_before
        # a replica uploaded from the host's log merges the same
        up = mk(hj)
        assert up.merge() == dst.merge() and up.info() == dst.info()
    finally:
        ctx.set_param("contraction", 0)


def test_past_1024_block_counts(mk):
    """262,444 items are 1,026 blocks of 256: the one-workgroup scans of the block counts take a
    second round of 1,024 with the carry of the first, in the encode (items, range heads and ends)
    and in the apply (new items).  Slots 262,201..262,430 are tombstoned: blocks 1,024 and 1,025.
    Device against the host twin, byte for byte."""
    n = 262144 + 300
    text = (ALPHABET * (n // len(ALPHABET) + 1))[:n]
    live = crdt_hip.OpLog()
    live.insert(0, text)
    log = live.clone()
    log.remove(262200, 262430)
    whole = log.encode_diff([])
    rep = mk(log)
    assert rep.encode_diff([]) == whole
    # against the vector of the same items: nothing but the range, its head and end past block 1,024
    ranges = log.encode_diff(live.state_vector())
    assert du.decode_diff(ranges)["n"] == 0 and list(du.decode_diff(ranges)["rcount"]) == [230]
    assert rep.encode_diff(live.state_vector()) == ranges
    first = crdt_hip.OpLog()
    first.insert(0, text[:100])
    for held in (crdt_hip.OpLog(), first):
        k = held.view().n
        dst = mk(held if k else None)
        assert dst.apply_diff(whole) == held.apply_diff(whole) == (n - k, 0)
        assert dst.encode_diff([]) == held.encode_diff([]) == whole
    dst = mk(live)
    assert dst.apply_diff(ranges) == live.apply_diff(ranges) == (0, 230)
    assert dst.encode_diff([]) == live.encode_diff([]) == whole


def test_device_and_host_deltas_cross(mk, oracle, forks, fforks):
    for a, b in (forks[2:4], fforks):
        want, added, tomb = du.union(a.arrays(), b.arrays())
        ra, rb = mk(a), mk(b)
        # a device delta applied on the host
        h = a.clone()
        assert h.apply_diff(rb.encode_diff(h.state_vector())) == (added, tomb)
        # a host delta applied on the device
        assert ra.apply_diff(b.encode_diff(ra.state_vector())) == (added, tomb)
        assert ra.encode_diff([]) == h.encode_diff([]) == du.encode_diff(want, [])
        check(oracle, ra, want)


def test_stale_vector_and_idempotence(mk, oracle, forks):
    _, _, a, b, c = forks
    dst = mk(a)
    old = dst.state_vector()
    assert dst.join(mk(c))[0] > 0
    b2 = b.clone()
    b2.join(c)
    delta = mk(b2).encode_diff(old)                         # carries c's items: dst holds them
    ac = a.clone()
    ac.join(c)
    want, added, tomb = du.union(ac.arrays(), b2.arrays())
    assert du.decode_diff(delta)["n"] > added > 0
    assert dst.apply_diff(delta) == (added, tomb)
    check(oracle, dst, want)
    whole = dst.encode_diff([])
    assert whole == du.encode_diff(want, [])
    before = (dst.merge(), dst.info())
    assert dst.apply_diff(delta) == (0, 0)
    assert dst.encode_diff([]) == whole and (dst.merge(), dst.info()) == before
    # tombstones alone: the peer's own vector, ranges only
    a2 = a.clone()
    a2.remove(3, 9)
    ra = mk(a)
    delta = mk(a2).encode_diff(ra.state_vector())
    assert du.decode_diff(delta)["n"] == 0
    assert ra.apply_diff(delta) == (0, 6)
    check(oracle, ra, a2.arrays())
    # into an empty replica: the whole log
    empty = mk()
    assert empty.apply_diff(whole) == (want.n, 0)
    assert empty.encode_diff([]) == whole
    check(oracle, empty, want)


def test_previous_slot_flag_is_recomputed_both_ways(mk, oracle):
    """As test_gpu_join's: src = [base, X, S, Y] with Y typed after X, dst = [base, S].  X and Y
    become neighbours in dst (Y follows its parent's slot there, not in src), and X follows the
    base's last slot in src only."""
    base = base_log(70, seed=3)
    n = base.visible_len()
    d, e = base.clone(), base.clone()
    d.set_agent(2)
    e.set_agent(3)
    d.insert(n, "X")
    e.insert(5, "S")
    src = d.clone()
    src.join(e)
    src.set_agent(2)
    src.insert(n + 2, "Y")
    dst = base.clone()
    dst.join(e)
    S, D = src.arrays(), dst.arrays()
    nb = base.arrays().n
    assert S.parent[nb + 2] == nb + 1 and S.parent[nb] == nb
    want, added, tomb = du.union(D, S)
    assert added == 2 and want.parent[D.n + 1] == D.n + 1 and want.parent[D.n] == nb
    rd, rs = mk(dst), mk(src)
    assert rd.apply_diff(rs.encode_diff(rd.state_vector())) == (2, 0)
    check(oracle, rd, want)
    text = oracle.merge(to_anchor(want)).decode()
    assert text.endswith("XY") and oracle.merge_naive(to_anchor(want)).decode() == text
    assert rd.encode_diff([]) == du.encode_diff(want, [])


def test_rejections_change_nothing(mk, forks, fforks):
    _, _, a, b, _ = forks
    A = a.arrays()
    dst = mk(a)
    before = (dst.merge(), dst.info(), dst.encode_diff([]))
    for name, code, data in rejections(A, b.arrays()):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            dst.apply_diff(data)
        assert e.value.code == code, (name, str(e.value))
        assert (dst.merge(), dst.info(), dst.encode_diff([])) == before, name
    fa = fforks[0]
    fdst = mk(fa)
    fbefore = (fdst.merge(), fdst.info(), fdst.encode_diff([]))
    for name, code, data in fugue_rejections(fa.arrays()):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            fdst.apply_diff(data)
        assert e.value.code == code, (name, str(e.value))
        assert (fdst.merge(), fdst.info(), fdst.encode_diff([])) == fbefore, name
    with pytest.raises(crdt_hip.CrdtHipError) as e:
        dst.apply_diff(fdst.encode_diff([]))
    assert e.value.code == du.EINVAL and "Fugue" in str(e.value)
    for sv in ([(2, 5), (1, 5)], [(65536, 1)]):
        with pytest.raises(crdt_hip.CrdtHipError) as e:
            dst.encode_diff(sv)
        assert e.value.code == du.EINVAL
    # a replica of another context
    other = crdt_hip.Context(0)
    foreign = crdt_hip.Replica(other, a)
    try:
        L = crdt_hip.lib()
        import ctypes as C
        n = C.c_size_t(0)
        assert L.crdt_hip_replica_state_vector(dst.ctx._h, foreign._h, None, 0, C.byref(n)) == du.EINVAL
        assert L.crdt_hip_replica_encode_diff(dst.ctx._h, foreign._h, None, 0, None, 0, C.byref(n)) == du.EINVAL
        # the ESPACE convention of both output calls
        assert L.crdt_hip_replica_state_vector(dst.ctx._h, dst._h, None, 0, C.byref(n)) == du.ESPACE
        assert n.value == 2
        assert L.crdt_hip_replica_encode_diff(dst.ctx._h, dst._h, None, 0, None, 0, C.byref(n)) == du.ESPACE
        assert n.value == len(before[2])
        buf = C.create_string_buffer(n.value)
        assert L.crdt_hip_replica_encode_diff(dst.ctx._h, dst._h, None, 0, buf, n.value - 1,
                                              C.byref(n)) == du.ESPACE
    finally:
        foreign.close()   # before its context
        other.close()
    # dst still takes the good delta
    want, added, tomb = du.union(A, b.arrays())
    assert dst.apply_diff(b.encode_diff(dst.state_vector())) == (added, tomb)
    assert dst.encode_diff([]) == du.encode_diff(want, [])


def test_after_an_apply(ctx, mk, oracle, forks):
    _, _, a, b, _ = forks
    dst, src = mk(a), mk(b)
    text_a = oracle.merge(to_anchor(a.arrays()))
    assert dst.merge_inc(text=True)[2:] == (0, text_a)
    src_before = (src.merge(), src.info())
    dst.apply_diff(src.encode_diff(dst.state_vector()))
    assert (src.merge(), src.info()) == src_before
    want, _, _ = du.union(a.arrays(), b.arrays())
    t = expect(oracle, want)
    cps, nbytes, path, text = dst.merge_inc(text=True)
    assert (path, text, cps, nbytes) == (0, t[0], t[2][1], t[2][2])
    cl = mk(dst.clone())
    assert cl.merge() == t[:2] and cl.info() == t[2]


def test_hipdownstream_sync_from(oracle, forks):
    _, _, a, b, _ = forks
    ctx = crdt_hip.HipMerge.context()
    made = [crdt_hip.HipDownstream(crdt_hip.Replica(ctx)) for _ in range(4)]
    x, y, x2, y2 = made
    try:
        for r in (x, x2):
            r.apply_update(a.encode_from(0))
        for r in (y, y2):
            r.apply_update(b.encode_from(0))
        want, added, tomb = du.union(a.arrays(), b.arrays())
        got = x.sync_from(y)
        assert got[:2] == (added, tomb) == x2.merge_from(y2)
        assert got[2] == len(du.encode_diff(b.arrays(), du.state_vector(a.arrays())))
        assert x.text() == x2.text() == oracle.merge(to_anchor(want)).decode()
        assert x.len() == x2.len() == visible(want)[0]
        assert x.sync_from(y)[:2] == (0, 0)
    finally:
        for r in made:
            r.replica.close()
