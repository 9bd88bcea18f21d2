"""CPU twin of test_gpu_incr_edges.py: every case builder of incr_util.py against the host log alone.

Three things are settled here, before a GPU sees a case.  The model is sound: the host log's
resolve_anchors_raw, text_at(mark) and patches_since(mark) agree with it at every step.  The case
is what it says it is: its item count, roots, sibling groups, losing roots and run heads are read
back from the update bytes.  And it is discriminating: where a case is aimed at the search or at
root_before's tie rule, the order a kernel without that rule would give (every root right after
its parent; the tie rule reversed) is computed from the oracle's order, and what the observer
compares must differ under it.
"""
import pytest

import incr_util as iu

CASES = iu.all_cases()


def _hook(pair, st, before, ref):
    n0, maxkey = before
    if n0 == 0:
        return
    facts = iu.batch_facts(n0, maxkey, st.updates)
    for k, want in st.claims.items():
        if k == "heads":
            if st.claims.get("heads_exact"):
                assert facts["heads"] == want
            else:
                assert set(want) <= set(facts["heads"]), sorted(set(want) - set(facts["heads"]))
        elif k == "min_new_left":
            assert facts["new_left"] >= want
        elif k != "heads_exact":
            assert facts[k] == want, (k, facts[k], want)
    if not st.wrong:
        return
    arrs = pair.host.arrays()
    at = pair.marks[-2][1]      # the version the step was applied to
    assert at.n == n0
    right = iu.shown(arrs, ref.order, at)
    for name in st.wrong:
        order = (iu.naive_order if name == "naive" else iu.tie_reversed_order)(arrs, ref.order, n0)
        assert sorted(order) == sorted(ref.order)
        wrong = iu.shown(arrs, order, at)
        seen = {k for k in right if right[k] != wrong[k]}
        assert set(st.sees) <= seen, (name, seen)
        assert not st.only or set(st.sees) == seen, (name, seen)


@pytest.mark.parametrize("name", list(CASES))
def test_case_on_the_host_log(oracle, name):
    iu.run_case(iu.build(CASES[name]), oracle, None, _hook)


def test_every_constant_has_a_case_on_each_side():
    """incr.hip's thresholds, each at its last passing and first failing value."""
    for name in ("A-paste-4096", "A-paste-4097",                      # kIncMax
                 "A-chunks-1024", "A-chunks-1025", "A-singles-2048", "A-singles-2049",  # inc_forest<Q>
                 "B-children-1024", "B-children-1025",                # kIncGroupMax
                 "B-roots-32-shared", "B-roots-33-distinct",          # kIncThinGroup
                 "F-many-16", "F-many-17",                            # kIncSearchers
                 "F-many-256", "F-many-257",                          # kIncHard
                 "F-scan-65535", "F-scan-65536",                      # kIncScan
                 "F-scan-4095", "F-scan-4096",                        # kSearchRound
                 "D-paste", "D-singles", "E-66-tiles"):
        assert name in CASES
