"""k_doctree at its run-count, key-width and text-size edges, against the oracle (exact: bytes,
tree digest, pre-order; no tolerances).

The edges, as tests/doctree_util.py derives them from doctree_lds_bytes and plan_level1
(engine.hip), and the run counts the device reported at them (st["runs"]):

  narrow bound   10,846 runs stay on k_doctree (rcap 10,848: 162,752 B of the 162,816 B budget);
                 10,847 (162,864 B) go to k_doctree_wide.  st["runs"] 10845 / 10846 / 10847 for
                 every shape, with 64-bit and with 32-bit keys.
  J bounds       12,288 -> 12,289 runs: k_doctree_wide -> k_doctree_wide17; 17,408 -> 17,409:
                 LDS level 1 -> global level 1.  st["runs"] 12287 .. 12289 and 17407 .. 17409.
  wide bound     by LDS bytes the wide instances would hold 18,086 runs (156,768 B at 17,408),
                 so J = 17 ends the LDS path first and the byte bound has no cases of its own.
  tile cuts      4095 / 4096 / 4097 and 8191 / 8192 / 8193 runs; R = 2 is a 4096-item typed chain
                 (with every item visible a second run exists only as a tile cut), R = 3 a fork.
  mixed waves    st["runs"] 35,528 (large document of 10,846 runs), 35,528 (10,847) and 36,971
                 (12,289), equal to the per-document predictions at their base slots.
  fused text     162,304 B (kDocLds - 512) fuse; 162,305 B are expanded by k_expand.
  clamp bound    the largest text whose dyn_bytes formula stays within kDocLds: 129,351 B for
                 the typed run (11 runs, 42,112 slots), 103,757 B for the bush (8,009 runs).
                 Above it and up to the fused bound phase C may refuse the document (from about
                 137 KB of text it always does): results only.
  2^18           262,143 B stay on the LDS level 1, 262,144 B take the global one.
  text step      1 byte: DocInfo::text_cap is the exact count of visible UTF-8 bytes (no rounding
                 in Engine::plan or upload), so "the next size up" is one codepoint a byte wider.
  tile table     a document of 1022 whole tiles (max_doc_slots / 4096 + 2 == kDocTiles) stages
                 from the tile segments, one of 1023 does not.
  Fugue          20,000 items, agents 1..5: 12,655 rows, k_doctree_wide17 under doctree_k32.

The stage_launches the path assertions read are the host's account of the plan it ran (Engine::
finish_wave), so they pin plan_level1 against tests/doctree_util.py; what the kernels computed
is pinned by the bytes, digests and orders.  The file takes about 4 s on an MI355X.
"""
import functools

import numpy as np
import pytest

import crdt_hip
import doctree_util as du
from doctree_util import to_anchor
from oracle_bind import Oracle
from test_fugue import random_fugue
from test_gpu_merge import _level1_cases

pytestmark = pytest.mark.gpu

NARROW = du.narrow_max()                      # the largest run count on 64-bit keys
J_NARROW = du.KDOC_J_NARROW * du.KDOC_THREADS  # 12288: J = 12 -> J = 17
J_MAX = du.KDOC_J * du.KDOC_THREADS            # 17408: the LDS level 1 ends
# (the wide instances' LDS bound lies above J_MAX, tests/test_doctree_shapes.py: no edge of its own)
assert du.lds_max(True) == J_MAX
EDGES = [4096, 8192, NARROW, J_NARROW, J_MAX]
WIDE_EDGES = [NARROW, J_NARROW, J_MAX]
L23 = (1 << 23) - 2                            # the greatest lamport of the 32-bit key layout


def _run_count_cases():
    cases = []
    for e in EDGES:
        for r in (e - 1, e, e + 1):
            cases += [(s, r, 3) for s in sorted(du.SHAPES)]
    for e in WIDE_EDGES:
        for r in (e - 1, e, e + 1):
            cases += [(s, r, 255) for s in sorted(du.SHAPES)]
    cases += [("bush", 2, 3), ("bush", 3, 3)]
    rng = np.random.default_rng(0xED6E)
    cases += [("bush", int(r), 3) for r in rng.integers(4, J_MAX + 1, 12)]
    return cases


@functools.lru_cache(maxsize=None)
def _oracle():
    return Oracle()


def _reference(log):
    """(text, order, digest) of the oracle (Fugue logs: the Fugue oracle)."""
    o = _oracle()
    a = to_anchor(log)
    text, order = (o.merge_fugue if log.side is not None else o.merge)(a, want_order=True)
    return text, order, o.tree_digest(text)


@functools.lru_cache(maxsize=None)
def _shape_case(shape, R, agents, seed=1):
    log = du.SHAPES[shape](R, seed, agents)
    return (log,) + _reference(log)


@pytest.fixture(scope="module")
def ctxs():
    """One context on default parameters and one with doctree_k32 = 1."""
    cs = {0: crdt_hip.Context(0), 1: crdt_hip.Context(0)}
    cs[1].set_param("doctree_k32", 1)
    yield cs
    for c in cs.values():
        c.close()


def _k32_ctx():
    c = crdt_hip.Context(0)
    c.set_param("doctree_k32", 1)
    return c


def _merge_all_ways(c, log, ref):
    """One document through merge_batch (stats), merge (bytes) and merge_order; returns the stats."""
    text, order, digest = ref
    dig, lens, st = c.merge_batch([log], stats=True)
    assert lens[0] == len(text) and dig[0] == digest
    got, d = c.merge(log)
    assert got == text and d == digest
    assert np.array_equal(c.merge_order(log), order)
    return st


def _assert_path(st, lds1):
    sl = st["stage_launches"]
    if lds1:
        # (two launches per LDS wave: k_doctotals and the k_doctree instance)
        assert sl["doctree"] == 2 and sl["walk1"] == 0, sl
    else:
        assert sl["walk1"] > 0, sl


# ---- a. run-count edges, one document per merge -------------------------------------------------
@pytest.mark.parametrize("k32", [0, 1])
@pytest.mark.parametrize("shape,R,agents", _run_count_cases())
def test_run_count_edges(ctxs, shape, R, agents, k32):
    log, text, order, digest = _shape_case(shape, R, agents)
    runs = du.predicted_runs(log.parent)
    assert runs == R
    st = _merge_all_ways(ctxs[k32], log, (text, order, digest))
    print(f"runs {shape} R={R} A={agents} k32={k32}: {st['runs']}")
    assert st["runs"] == runs  # the case sits where it claims
    _assert_path(st, du.plan(runs, len(text), du.doc_slots(log.n), bool(k32)).lds1)


# ---- b. mixed waves -----------------------------------------------------------------------------
SMALL = [("bush", 3), ("ladder", 100), ("comb64", 4096), ("bush", 4097), ("ladder", 8192),
         ("bush", 8193)]


@pytest.mark.parametrize("big", [NARROW, NARROW + 1, J_NARROW + 1])
def test_mixed_waves_follow_their_largest_document(ctxs, big):
    """Small documents are dragged onto the instance their large neighbour needs: k_doctree at
    the narrow bound, k_doctree_wide one run above it, k_doctree_wide17 at 12289."""
    cases = [_shape_case("bush", big, 3, 2)] + [_shape_case(s, r, 3, 2) for s, r in SMALL]
    logs = [c[0] for c in cases]
    c = ctxs[0]
    dig, lens, st = c.merge_batch(logs, stats=True)
    base = runs = rmax = 0
    for i, (log, text, _, digest) in enumerate(cases):
        assert lens[i] == len(text) and dig[i] == digest, i
        r = du.predicted_runs(log.parent, base)   # in order, each padded to 64 slots
        runs, rmax = runs + r, max(rmax, r)
        base += du.doc_slots(log.n)
    print(f"runs mixed big={big}: {st['runs']} (predicted {runs})")
    assert st["waves"] == 1 and st["runs"] == runs
    p = du.plan(rmax, max(len(x[1]) for x in cases), max(du.doc_slots(x[0].n) for x in cases))
    assert p.lds1 and (p.wide, p.j) == {NARROW: (False, 12), NARROW + 1: (True, 12),
                                        J_NARROW + 1: (True, 17)}[big]
    _assert_path(st, True)
    # resident replicas, merged twice: the learnt plan and merge_async take the same wave
    # (no `runs` here: the rotation moves the tile boundaries)
    b = c.batch(logs, replicas=2, relabel="rotate", seed=9)
    for it in range(2):
        dig, lens, st = b.merge()
        for r in range(b.docs):
            assert lens[r] == len(cases[r % len(cases)][1]), (it, r)
            assert dig[r] == cases[r % len(cases)][3], (it, r)
        assert st["stage_launches"]["walk1"] == 0
    b.close()


# ---- c. the 32-bit key layout -------------------------------------------------------------------
def _family(log):
    par = log.parent.astype(np.int64)
    return par, np.bincount(par, minlength=log.n + 1)


def _leaf_siblings(log, k=2):
    """Ids of k leaf items of one sibling group (each a run head of one item)."""
    par, nk = _family(log)
    ids = np.arange(1, log.n + 1)
    leaf = nk[ids] == 0
    cnt = np.bincount(par[leaf], minlength=log.n + 1)
    p = int(np.flatnonzero(cnt >= k)[3])
    return [int(x) for x in ids[leaf & (par == p)][:k]]


def _leaf_singleton(log):
    """A leaf that is its parent's only child and not in the slot after it: a head, alone."""
    par, nk = _family(log)
    ids = np.arange(1, log.n + 1)
    return int(ids[(nk[ids] == 0) & (nk[par] == 1) & (par != ids - 1)][0])


def _second_of_a_pair(log):
    """The second item of a typed pair that ends its run: not a head."""
    par, nk = _family(log)
    ids = np.arange(1, log.n + 1)
    ok = (nk[ids] == 0) & (par == ids - 1) & (nk[par] == 1) & (ids % du.SCAN_TILE != 0)
    return int(ids[ok][5])


def _with_keys(log, keys):
    out = log.copy()
    for i, (lam, agent) in keys.items():
        out.lamport[i - 1], out.agent[i - 1] = lam, agent
    ids = out.lamport.astype(np.uint64) << np.uint64(16) | out.agent.astype(np.uint64)
    assert np.unique(ids).size == out.n
    return out


@functools.lru_cache(maxsize=None)
def _base5000(agents=255):
    return du.bush(5000, 4, agents)


def _misfits(log, at):
    """Three logs, each with one key beyond the 32-bit layout on item at[0], and on its sibling
    at[1] a key that differs from it only in bits the compression drops, so that a kernel that
    truncated would reorder the two.  (Lamport 2^23 - 1 is kept out of the layout only because
    with agent 255 it would compress to the Fugue content row's 0x7FFFFFFF; its sibling here
    is that neighbour.  Next to 0xFFFFFFFE only a lamport that is itself too wide compresses to
    a greater key.)"""
    x, y = at
    top = int(log.lamport.max()) + 10
    return {
        "agent256": _with_keys(log, {x: (top, 256), y: (top, 1)}),
        "lamport2^23-1": _with_keys(log, {x: (L23 + 1, 255), y: (L23 + 1, 254)}),
        "lamport0xFFFFFFFE": _with_keys(log, {x: (0xFFFFFFFE, 0), y: (0x00FFFFFE, 1)}),
    }


def test_key32_keys_that_fit_stay_on_the_lds_path(ctxs):
    log = _base5000()
    assert int(log.agent.max()) == 254
    a, b = _leaf_siblings(log)
    s = _leaf_singleton(log)
    variants = {
        "agent255": _with_keys(log, {a: (int(log.lamport[a - 1]), 255)}),
        "lamport2^23-2": _with_keys(log, {a: (L23, 0), b: (L23, 255), s: (L23, 7)}),
    }
    for name, v in variants.items():
        st = _merge_all_ways(ctxs[1], v, _reference(v))
        assert st["stage_launches"]["walk1"] == 0, name
        assert st["runs"] == 5000


@pytest.mark.parametrize("which", ["agent256", "lamport2^23-1", "lamport0xFFFFFFFE"])
def test_key32_keys_that_do_not_fit_take_the_global_path(ctxs, which):
    base = _base5000()
    bad = _misfits(base, _leaf_siblings(base))[which]
    ref = _reference(bad)
    if which != "lamport2^23-1":
        # the case is sensitive: sorting by the truncated keys gives another order
        cut = bad.copy()
        cut.lamport[:] = (bad.lamport << np.uint32(8)) | (bad.agent & np.uint16(0xFF))
        cut.agent[:] = 0
        assert not np.array_equal(_reference(cut)[1], ref[1])
    # 64-bit keys hold them all
    st = _merge_all_ways(ctxs[0], bad, ref)
    assert st["stage_launches"]["walk1"] == 0
    # 32-bit keys: the load phase flags the document (C_ERR bit 32), the wave is merged again
    # on the global path; first on a context that has learnt nothing (run_wave's redo) ...
    c = _k32_ctx()
    st = _merge_all_ways(c, bad, ref)
    assert st["stage_launches"]["walk1"] > 0
    # ... then behind a document of the same shape whose keys fit and whose plan is learnt
    st = _merge_all_ways(c, base, _reference(base))
    assert st["stage_launches"]["walk1"] == 0
    for _ in range(2):
        st = _merge_all_ways(c, bad, ref)
        assert st["stage_launches"]["walk1"] > 0
    c.close()


def test_key32_misfit_in_a_resident_batch_merged_twice():
    """The redo of merge_async_finish must not run on a stale plan: both merges of the batch
    give the oracle's digests."""
    base = _base5000()
    bad = _misfits(base, _leaf_siblings(base))["agent256"]
    refs = [_reference(bad), _reference(base)]
    c = _k32_ctx()
    b = c.batch([bad, base], replicas=2, relabel="rotate", seed=3)
    for it in range(2):
        dig, lens, st = b.merge()
        for r in range(b.docs):
            assert lens[r] == len(refs[r % 2][0]) and dig[r] == refs[r % 2][2], (it, r)
        assert st["stage_launches"]["walk1"] > 0, it
    b.close()
    c.close()


def test_key32_wide_key_inside_a_run_is_not_sorted(ctxs):
    """Only the heads' keys are sorted: the same wide keys on the second item of a typed pair
    leave the document on the LDS path."""
    base = _base5000()
    x = _second_of_a_pair(base)
    for lam, agent in ((int(base.lamport.max()) + 10, 256), (L23 + 1, 255), (0xFFFFFFFE, 0)):
        v = _with_keys(base, {x: (lam, agent)})
        st = _merge_all_ways(ctxs[1], v, _reference(v))
        assert st["stage_launches"]["walk1"] == 0, (lam, agent)
        assert st["runs"] == 5000


def test_key32_fugue_neighbour_of_the_content_row(ctxs):
    """Fugue rows on 32-bit keys: a node with left children whose right child has lamport
    2^23 - 2 and agent 255 compresses to 0x7FFFFEFF, next to its content row's 0x7FFFFFFF."""
    f = random_fugue(20000, 31, agents=5, cps=(0x61, 0xE9, 0x4E2D, 0x1F600))
    agent = f.agent + 1                                   # agents 1..5
    lp = f.parent[f.side == 1]
    v = int(lp[f.deleted[lp - 1] == 0][100])              # a visible node with left children
    extra = [(v, 0, L23, 255), (v, 0, L23, 254), (v, 0, L23 - 1, 255), (v, 1, L23, 253)]
    k = len(extra)
    log = crdt_hip.LogArrays(
        np.r_[f.parent, [e[0] for e in extra]], np.r_[f.lamport, [e[2] for e in extra]],
        np.r_[agent, [e[3] for e in extra]], np.r_[f.deleted, np.zeros(k, np.uint8)],
        np.r_[f.cp, np.full(k, 0x58, np.uint32)], side=np.r_[f.side, [e[1] for e in extra]])
    assert not log.deleted[v - 1]  # (its content row holds text)
    st = _merge_all_ways(ctxs[1], log, _reference(log))
    print(f"runs fugue 20000 items k32=1: {st['runs']}")
    assert st["stage_launches"]["walk1"] == 0


def test_key32_level1_cases_and_64_agents(ctxs):
    o = _oracle()
    logs = _level1_cases()
    dig, lens = ctxs[1].merge_batch(logs)
    for i, lg in enumerate(logs):
        ref = o.merge(to_anchor(lg)) if lg.n else b""
        assert lens[i] == len(ref) and dig[i] == o.tree_digest(ref), i
    log = crdt_hip.OpLog.synth_agents(200000, 64, 0x5EED0009).arrays()
    _merge_all_ways(ctxs[1], log, _reference(log))


# ---- d. text-size edges -------------------------------------------------------------------------
TEXT_SHAPES = {"typed": du.typed_run, "bush": du.bush_text}
KNOBS = [(0, 2), (0, 1), (0, 0), (1, 2)]   # (text_scatter, stile_text)
T_LABELS = ["120000", "clamp", "clamp+1", "150000", "fuse", "fuse+1", "200000", "2^18-1", "2^18"]


@functools.lru_cache(maxsize=None)
def _clamp_edge(shape):
    """The largest text of this shape on which the dyn_bytes clamp does not bite.  (The bound
    depends on the document's runs and slots, which the shape sizes by its text bucket.)"""
    T = 120_000
    for _ in range(4):
        log = TEXT_SHAPES[shape](T, 1)
        T2 = du.unclamped_max_text(du.predicted_runs(log.parent), du.doc_slots(log.n))
        if du._bucket(T2) == du._bucket(T):
            return T2
        T = T2
    return T


def _text_size(shape, label):
    """Text sizes are exact on the host (DocInfo::text_cap = the visible bytes, no rounding),
    so the next size up is one more byte: one codepoint a byte wider."""
    return {"120000": 120_000, "clamp": _clamp_edge(shape), "clamp+1": _clamp_edge(shape) + 1,
            "150000": 150_000, "fuse": du.fuse_max_text(), "fuse+1": du.fuse_max_text() + 1,
            "200000": 200_000, "2^18-1": (1 << 18) - 1, "2^18": 1 << 18}[label]


@functools.lru_cache(maxsize=None)
def _text_case(shape, T):
    log = TEXT_SHAPES[shape](T, 1)
    text, _, digest = _reference(log)
    assert len(text) == T
    return log, text, digest


@pytest.fixture(scope="module")
def knob_ctxs():
    cs = {}
    for scatter, stile in KNOBS:
        cs[scatter, stile] = c = crdt_hip.Context(0)
        c.set_param("text_scatter", scatter)
        c.set_param("stile_text", stile)
    yield cs
    for c in cs.values():
        c.close()


@pytest.mark.parametrize("knobs", KNOBS)
@pytest.mark.parametrize("label", T_LABELS)
@pytest.mark.parametrize("shape", sorted(TEXT_SHAPES))
def test_text_size_edges(knob_ctxs, shape, label, knobs):
    T = _text_size(shape, label)
    log, text, digest = _text_case(shape, T)
    runs = du.predicted_runs(log.parent)
    p = du.plan(runs, T, du.doc_slots(log.n))
    # the case sits on the edge its label names
    want = {"clamp": (True, True), "clamp+1": (True, False), "fuse": (True, False),
            "fuse+1": (False, False), "2^18-1": (False, False), "2^18": (False, False)}
    if label in want:
        assert (p.fuse, p.unclamped) == want[label]
    assert p.lds1 == (label != "2^18")
    c = knob_ctxs[knobs]
    for it in range(3):  # (from the second merge on: the learnt plan, where the knobs act)
        dig, lens, st = c.merge_batch([log], stats=True)
        sl = st["stage_launches"]
        print(f"text {shape} T={T} knobs={knobs} merge {it}: runs {st['runs']} "
              f"expand {sl['expand']} walk1 {sl['walk1']} text {sl['text']}")
        assert lens[0] == T and dig[0] == digest, it
        assert st["runs"] == runs
        assert (sl["walk1"] == 0) == (T < (1 << 18)), sl
        if p.unclamped:
            assert sl["expand"] == 0, sl          # fused, and phase C cannot refuse
        elif not p.fuse:
            assert sl["expand"] > 0, sl
        # (fused but clamped: phase C may refuse the document and the wave is redone)
    got, d = c.merge(log)
    assert got == text and d == digest


# ---- e. the tile-table edge ---------------------------------------------------------------------
def test_tile_table_edge():
    """max_doc_slots / 4096 + 2 == kDocTiles: the text is staged from the tile segments and
    fused; one tile more and the plan must not stage from them."""
    c = crdt_hip.Context(0)
    for tiles, stile in ((du.KDOC_TILES - 2, True), (du.KDOC_TILES - 1, False)):
        log = du.tile_edge_doc(tiles, 1)
        slots = du.doc_slots(log.n)
        assert slots // du.SCAN_TILE + 2 == (du.KDOC_TILES if stile else du.KDOC_TILES + 1)
        text, _, digest = _reference(log)
        assert 90_000 < len(text) < 110_000
        assert du.plan(2000, len(text), slots).stile_text == stile
        for it in range(2):
            dig, lens, st = c.merge_batch([log], stats=True)
            assert lens[0] == len(text) and dig[0] == digest, (tiles, it)
            if stile:
                assert st["stage_launches"]["expand"] == 0, st["stage_launches"]
        got, d = c.merge(log)
        assert got == text and d == digest
    c.close()
