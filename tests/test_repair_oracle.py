"""The oracle of tests/repair_cases.py without a GPU: (a) where every pairwise angular gap exceeds 1e-9 rad -- nine orders
of magnitude above the ~1e-15 error of a float64 arctan2 -- the contract's exact order IS the reference's
``np.argsort(np.arctan2(...))`` of the closed sequence around ``coords.mean(axis=0)``, duplicate dropped (integer
coordinates below 2^20: every order of summation gives numpy's centre bits; the generator asserts both preconditions);
(b) the tie rules on rings worked by hand; and the adversarial pairs really defeat the naive comparators."""
import numpy as np
import pytest

import repair_cases as rc
import simplify_cases as sc


@pytest.mark.parametrize("n", [3, 4, 5, 13, 63, 64, 65, 130, 300, 1000])
def test_exact_order_is_numpys_where_the_angles_are_separated(n):
    for seed in range(3):
        ring = rc.separated_grid_ring(n, 1000 * n + seed)
        assert rc.resort_order(ring) == rc.numpy_order(ring), (n, seed)
    closed = np.vstack([ring, ring[:1]])                             # given closed: the duplicate follows its twin
    order = rc.resort_order(closed)
    assert [k for k in order if k != n] == rc.numpy_order(ring) and order[order.index(0) + 1] == n


def test_tie_rules_on_hand_worked_rings():
    assert sorted(rc.SPECIAL) == sorted(rc.SPECIAL_ORDER)
    for name, want in rc.SPECIAL_ORDER.items():
        assert rc.resort_order(rc.SPECIAL[name]) == want, name
    # arctan2's conventions, vector by vector
    assert rc.exact_compare((0.0, 0.0), (1.0, 0.0)) == -1            # the centre itself: angle 0, length 0
    assert rc.exact_compare((1.0, 0.0), (1.0, 1e-300)) == -1
    assert rc.exact_compare((1.0, -1e-300), (1.0, 0.0)) == -1
    assert rc.exact_compare((-1.0, 0.0), (-1.0, 1e-300)) == 1        # the negative x ray is +pi: last
    assert rc.exact_compare((-1.0, -0.0), (-1.0, 1e-300)) == 1       # either zero
    assert rc.exact_compare((-1.0, -1e-300), (5.0, -7.0)) == -1      # just past the ray: first
    assert rc.exact_compare((-3.0, 0.0), (-2.0, 0.0)) == 1 and rc.exact_compare((2.0, 2.0), (2.0, 2.0), 3, 7) == -1


def test_passed_through_and_expected_tensors():
    for ring in ([], [(1, 1)], [(1, 1), (2, 5)], [(1, 1), (2, 5), (1, 1)]):
        assert rc.resort_order(ring) == list(range(len(ring)))
    rings = [rc.SPECIAL["bow_tie"], [(7, 7)], rc.SPECIAL["collinear"], [(0, 0), (4, 0), (4, 4), (0, 4)]]
    want = rc.expected_resort(rings, select=[True, True, False, True])
    assert want["vertex_index"].tolist() == [0, 2, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    rep = rc.expected_repair(rings)
    assert rep["status"].tolist() == [1, 2, 2, 0] and rep["counters"].tolist() == [3, 1, 2]
    assert rep["reason_before"][0, 0] == sc.TOUCH and rep["reason_after"][0].tolist() == [sc.OK, -1, -1]
    assert rep["reason_after"][1, 0] == sc.TOO_FEW and rep["vertex_index"].tolist() == [0, 2, 1, 3, 4, 7, 8, 6, 5, 9, 10, 11, 12]


def test_a_shuffled_convex_ring_comes_back_convex():
    for n, seed in ((7, 1), (64, 2), (300, 3)):
        ring = rc.convex_ring(n, seed)
        back = rc.shuffled(ring, seed)[rc.resort_order(rc.shuffled(ring, seed))]
        assert sc.ring_simple_exact(back)[0] and sc.area2(back) > 0  # valid and counter-clockwise
        assert sorted(map(tuple, back.tolist())) == sorted(map(tuple, ring.tolist()))


@pytest.mark.parametrize("kind", ["cross", "atan2"])
def test_the_naive_comparators_fail_on_the_adversarial_pairs(kind):
    pairs = rc.naive_failures(kind)                                  # asserts the failures itself
    assert len(pairs) == 6
    for ring in rc.naive_failure_rings(kind):
        order = rc.resort_order(ring)
        assert sorted(order) == list(range(6)) and order[0] in (3, 5) and order[-1] == 1
