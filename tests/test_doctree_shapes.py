"""The k_doctree edge shapes on the CPU: the generators of tests/doctree_util.py give what they
promise, the oracles agree on them (multi-agent lamport ties included), and the constants the
edge arithmetic transcribes are still the ones in engine.hip."""
import os
import re

import numpy as np
import pytest

import doctree_util as du
from conftest import PKG
from doctree_util import SHAPES, to_anchor

RUNS = [2, 3, 64, 65, 1000]
AGENTS = [1, 3, 255]


@pytest.mark.parametrize("agents", AGENTS)
@pytest.mark.parametrize("R", RUNS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_generator_properties(shape, R, agents):
    for seed in (1, 2):
        log = SHAPES[shape](R, seed, agents)
        assert du.predicted_runs(log.parent) == R
        assert du.group_sizes(log.parent).max() <= 64
        assert not log.deleted.any()
        ids = log.lamport.astype(np.uint64) << np.uint64(16) | log.agent.astype(np.uint64)
        assert np.unique(ids).size == log.n, "identities repeat"
        assert (log.agent < agents).all()
        plam = np.r_[np.uint32(0), log.lamport][log.parent]
        assert (log.lamport > plam).all(), "a child's lamport must exceed its parent's"
        groups, tied = du.tie_share(log)
        # (one agent cannot tie: two items of one agent never share a lamport)
        if agents >= 2:
            assert 10 * tied >= groups, (groups, tied)
        assert len(log.cp.tobytes()) and sum(len(chr(c).encode()) for c in log.cp) < 100_000


def test_generators_cover_every_group_size_and_utf8_width():
    log = du.bush(5000, 3, 3)
    assert set(du.GROUP_SIZES) <= set(du.group_sizes(log.parent).tolist())
    assert {len(chr(c).encode()) for c in log.cp} == {1, 2, 3, 4}
    lad = du.ladder(1001, 3, 3)
    sizes = du.group_sizes(lad.parent)
    assert set(sizes[sizes > 0].tolist()) == {1, 2}  # (1: the document start's only child)
    comb = du.comb64(1 + 64 * 20, 3, 3)
    sizes = du.group_sizes(comb.parent)
    assert set(sizes[sizes > 0].tolist()) == {64}


def test_predicted_runs_moves_with_the_base_slot():
    """A typed chain has one head per tile boundary it crosses, wherever the document starts."""
    chain = np.arange(5000, dtype=np.uint32)
    assert du.predicted_runs(chain) == 2
    assert du.predicted_runs(chain, base_slot=8192 - 5000) == 3   # items 904 and 5000
    assert du.predicted_runs(chain, base_slot=8191 - 5000) == 2   # item 905
    assert du.predicted_runs(chain, base_slot=4095) == 3           # items 1 and 4097


@pytest.mark.parametrize("R", [3, 65, 1000, 2000])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_oracles_agree_on_the_shapes(oracle, shape, R):
    for agents in (3, 255):
        log = SHAPES[shape](R, 5, agents)
        a = to_anchor(log)
        assert oracle.merge(a) == oracle.merge_naive(a), (shape, R, agents)
        flog = SHAPES[shape](R, 5, agents, fugue=True)
        assert R < 1000 or flog.side.any()
        text, order = oracle.merge_fugue(to_anchor(flog), want_order=True)
        ref = du.fugue_order(flog)
        assert np.array_equal(order, ref), (shape, R, agents)
        assert text == "".join(chr(c) for c in flog.cp[ref - 1]).encode()


def test_text_shapes_hold_the_bytes_they_claim(oracle):
    for T in (120_000, 150_001, (1 << 18) - 1):
        for log in (du.typed_run(T, 1), du.bush_text(T, 1)):
            text = oracle.merge(to_anchor(log))
            assert len(text) == T
            assert 0.1 < log.deleted.mean() < 0.25
    a, b = du.bush_text(150_000, 1), du.bush_text(150_001, 1)
    assert np.array_equal(a.parent, b.parent) and np.array_equal(a.deleted, b.deleted)


def test_edge_arithmetic():
    """The edges the GPU tests sit on, and that each predicate flips once (so "the largest" is
    well defined)."""
    wide = [du.plan(r, 0, 0).wide for r in range(1, 17410)]
    assert wide == sorted(wide)
    assert du.narrow_max() < du.KDOC_J_NARROW * du.KDOC_THREADS  # LDS, not J, ends k_doctree
    assert not du.plan(du.narrow_max(), 0, 0).wide and du.plan(du.narrow_max() + 1, 0, 0).wide
    for k32 in (False, True):
        lds = [du.plan(r, 0, 0, k32).lds1 for r in range(1, 20000)]
        assert lds == sorted(lds, reverse=True)
        # the wide instances' LDS bound lies above J = 17: the run-count bound ends the LDS path
        assert du.lds_max(k32) == du.KDOC_J * du.KDOC_THREADS
    assert du.plan(10, du.fuse_max_text(), 4096).fuse
    assert not du.plan(10, du.fuse_max_text() + 1, 4096).fuse
    t = du.unclamped_max_text(8000, 65536)
    assert du.plan(8000, t, 65536).unclamped and not du.plan(8000, t + 1, 65536).unclamped
    assert du.plan(10, (1 << 18) - 1, 4096).lds1 and not du.plan(10, 1 << 18, 4096).lds1


# what tests/doctree_util.py transcribes, as engine.hip spells it
PINNED = [
    (r"constexpr uint32_t kDocLds = 163840 - 1024;", "KDOC_LDS", 163840 - 1024),
    (r"#define CRDT_DOC_J 17\b", "KDOC_J", 17),
    (r"constexpr int kDocJNarrow = 12;", "KDOC_J_NARROW", 12),
    (r"#define CRDT_DOC_LOG2S 2\b", "KDOC_LOG2S", 2),
    (r"constexpr uint32_t kDocTiles = 1024;", "KDOC_TILES", 1024),
    (r"constexpr int kDocThreads = 1024;", "KDOC_THREADS", 1024),
]


@pytest.mark.parametrize("pattern,name,value", PINNED)
def test_engine_constants_are_the_transcribed_ones(pattern, name, value):
    with open(os.path.join(PKG, "csrc", "engine.hip")) as f:
        src = f.read()
    assert getattr(du, name) == value
    assert re.search(pattern.replace(" ", r"\s+"), src), (
        f"engine.hip no longer has `{pattern}`: update tests/doctree_util.py ({name}) and "
        "revisit the edge list of tests/test_gpu_doctree_edges.py, whose cases sit on "
        "thresholds computed from this constant")
