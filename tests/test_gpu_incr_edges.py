"""GPU tests of the incremental merge at its thresholds (csrc/incr.hip: k_inc, inc_forest,
inc_search, inc_splice_tile, inc_lookback), the kept order compared with the CPU oracle's.

test_gpu_incr.py compares the merged text, in which tombstones weigh nothing.  Here every case of
incr_util.py runs on a replica and a host log fed the same update bytes, and after every batch the
observer (incr_util.Pair.check) compares the text and counters, the position of every identity
the log holds under both biases (the rank of every slot, dead ones included), the text at every
earlier mark and the patches since it with a model on the oracle's order, and asserts the path
the merge took.  Then one more keystroke is typed and everything is compared again.

The cases by the constant they stand next to:
  kIncMax 4096 and inc_forest<1|2|4>      A (m = 1 .. 4097: one paste, m roots, split chunks; Fugue)
  run contraction at thread/wave/instance  A chunks (heads at 0, 1, 2, 64Q - 1 .. 64Q + 1, 1023 ..)
  kIncThinGroup 32, kIncGroupMax 1024     B
  tile seams of the splice                C (n0 = 4094 .. 8192, ranks 4094..4097 live or dead)
  the staging area cwl, two text passes   D
  the look-back's second window           E (66 tiles)
  kIncScan, kSearchRound, kIncSearchers, kIncHard, root_before's tie rule, I_MAXKEY's carry   F
  the Fugue left-child bits across growth and idle calls, Fugue roots that need a search      G
  20 seeded random histories, RGA and Fugue                                                   H
test_incr_edges.py holds what each case claims about its input and why a wrong order would show.
"""
import pytest

import incr_util as iu

pytestmark = pytest.mark.gpu

CASES = iu.all_cases()


def _section(letter: str) -> list:
    return [n for n in CASES if n.startswith(letter + "-")]


def _run(ctx, oracle, name):
    iu.run_case(iu.build(CASES[name]), oracle, ctx)


@pytest.mark.parametrize("name", _section("A"))
def test_batch_sizes_and_forest_instances(ctx, oracle, name):
    _run(ctx, oracle, name)


@pytest.mark.parametrize("name", _section("B"))
def test_sibling_groups(ctx, oracle, name):
    _run(ctx, oracle, name)


@pytest.mark.parametrize("name", _section("C"))
def test_tile_seams_of_the_splice(ctx, oracle, name):
    _run(ctx, oracle, name)


@pytest.mark.parametrize("name", _section("D"))
def test_full_staging_area(ctx, oracle, name):
    _run(ctx, oracle, name)


@pytest.mark.parametrize("name", _section("E"))
def test_look_back_past_one_window(ctx, oracle, name):
    _run(ctx, oracle, name)


@pytest.mark.parametrize("name", _section("F"))
def test_searched_roots(ctx, oracle, name):
    _run(ctx, oracle, name)


@pytest.mark.parametrize("name", _section("G"))
def test_fugue_state(ctx, oracle, name):
    _run(ctx, oracle, name)


@pytest.mark.parametrize("name", _section("H"))
def test_seeded_differential(ctx, oracle, name):
    _run(ctx, oracle, name)
