"""The nearest-boundaries oracle of tests/nearest_cases.py on the CPU: the hand-worked cases, its consistency with the
join's oracles (the candidates ARE the join's pairs; with k at least the largest count the kept set is the join), and the
erosion mask against its direct definition."""
import numpy as np
import pytest

import buffered_count_cases as bc
import nearest_cases as nc
import polygon_join_cases as pc


def test_unit_square_inside_outside_and_on_an_edge():
    rings, points = nc.hand_unit_square()
    r = nc.nearest(points, rings, 2, 0.0, "intersects")
    assert r["count"].tolist() == [1, 0, 1, 1] and r["counters"].tolist() == [3, 3, 0, 1]
    assert r["polygon"].tolist() == [[0, 1], [1, 1], [0, 1], [0, 1]]              # 1 = P, the padding
    assert r["dist2"][:, 0].tolist() == [0.0625, np.inf, 0.0, 0.0] and np.all(np.isinf(r["dist2"][:, 1]))
    assert r["inside"][:, 0].tolist() == [True, False, False, True] and not r["inside"][:, 1].any()
    assert nc.signed_distance(r)[:, 0].tolist() == [-0.25, np.inf, 0.0, 0.0]
    # open set, no buffer: the on-ring points are out
    assert nc.nearest(points, rings, 2, 0.0, "contains")["count"].tolist() == [1, 0, 0, 0]
    # grown by 1/2: the outside point is a candidate of the closed set and not of the open one; dist2 is to the ring itself
    r = nc.nearest(points, rings, 1, 0.5, "intersects")
    assert r["count"].tolist() == [1, 1, 1, 1] and r["dist2"][1, 0] == 0.25 and not r["inside"][1, 0]
    assert nc.signed_distance(r)[1, 0] == 0.5
    assert nc.nearest(points, rings, 1, 0.5, "contains")["count"].tolist() == [1, 0, 1, 1]


def test_nested_rings_the_deeper_one_first():
    rings, points = nc.hand_nested()
    r = nc.nearest(points, rings, 2, 0.5, "intersects")
    assert r["polygon"].tolist() == [[0, 1], [0, 1]]
    assert r["dist2"].tolist() == [[4.0, 1.0], [0.25, 0.25]] and r["inside"].tolist() == [[True, True], [True, False]]
    assert nc.signed_distance(r).tolist() == [[-2.0, -1.0], [-0.5, 0.5]]
    r1 = nc.nearest(points, rings, 1, 0.5, "intersects")
    assert r1["polygon"].tolist() == [[0], [0]] and r1["count"].tolist() == [2, 2] and r1["counters"].tolist() == [4, 2, 2, 2]


def test_identical_polygons_tie_and_the_lower_id_wins():
    rings, points = nc.hand_twins()
    r = nc.nearest(points, rings, 3)
    assert r["polygon"].tolist() == [[1, 0, 2]] and r["dist2"].tolist() == [[2.25, 0.25, 0.25]] and r["inside"].all()
    assert nc.nearest(points, rings, 2)["polygon"].tolist() == [[1, 0]]
    assert nc.min_key_gap(points, rings, 0.0, "intersects") == 0.0


def test_a_point_on_a_shared_vertex_has_two_zero_keys():
    rings, points = nc.hand_shared_vertex()
    r = nc.nearest(points, rings, 2)
    assert r["polygon"].tolist() == [[0, 1]] and r["dist2"].tolist() == [[0.0, 0.0]] and r["inside"].tolist() == [[False, True]]
    assert not np.signbit(nc.signed_distance(r)[0, 0]) and nc.signed_distance(r)[0, 1] == 0.0      # -0.0 and +0.0: by value
    assert nc.nearest(points, rings, 1)["polygon"].tolist() == [[0]]
    assert nc.nearest(points, rings, 2, 0.0, "contains")["count"].tolist() == [0]


@pytest.mark.parametrize("pred", pc.PREDICATES)
@pytest.mark.parametrize("d", pc.D_CASES)
def test_candidates_are_the_joins_pairs_on_the_named_cases(pred, d):
    rings, _, points, _, _ = pc.cases()
    ref = pc.reference("cases", d)
    c = nc.candidates(points, rings, d, pred)
    got = np.stack([c["point"], c["polygon"]], axis=1)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    assert np.array_equal(got, ref["f64"][pred])
    # and, away from the band of the decision boundary, the exact rational oracle's
    assert np.array_equal(pc.without(got, ref["undecided"]), pc.without(ref["exact"][pred], ref["undecided"]))
    # dist2 against the exact one: within the float64 oracle's recorded error
    for i, p, d2 in zip(c["point"], c["polygon"], c["dist2"]):
        exact = ref["exact"]["dist2"][(int(i), int(p))]
        assert abs(d2 - float(exact)) <= 4 * pc.E_REF * float(exact), (i, p)


@pytest.mark.parametrize("pred", pc.PREDICATES)
def test_with_k_at_least_max_count_the_kept_set_is_the_join(pred):
    rings, points = bc.scene_field()
    dists = np.linspace(0.0, 2.0, len(rings))
    full = nc.nearest(points, rings, 16, dists, pred)
    assert 1 < full["counters"][3] <= 16 and full["counters"][2] == 0 and full["counters"][0] == full["counters"][1]
    assert np.array_equal(nc.kept_pairs(full, len(rings)), pc.join_f64(points, rings, dists)[pred])
    assert np.array_equal(full["count"], np.bincount(pc.join_f64(points, rings, dists)[pred][:, 0], minlength=len(points)))


def test_oracle_is_self_consistent():
    rings, points = bc.scene_field()
    dists = np.linspace(0.0, 2.0, len(rings))
    full = nc.nearest(points, rings, 16, dists)
    for k in (1, 3):
        r = nc.nearest(points, rings, k, dists)
        assert np.array_equal(r["polygon"], np.where(np.arange(16)[None, :k] < full["count"][:, None], full["polygon"][:, :k], len(rings)))
        assert np.array_equal(r["dist2"], full["dist2"][:, :k]) and np.array_equal(r["inside"], full["inside"][:, :k])
        assert np.array_equal(r["count"], full["count"])             # before the cap
        assert r["counters"].tolist() == [full["counters"][0], int(np.minimum(full["count"], k).sum()), int((full["count"] > k).sum()),
                                          full["counters"][3]]
    # a row is in key order: inside (negative, deepest first), then outside, the padding last
    s = np.where(full["inside"], -full["dist2"], full["dist2"])
    assert np.all(s[:, :-1][np.isfinite(s[:, 1:])] <= s[:, 1:][np.isfinite(s[:, 1:])]) and np.all(np.isinf(s[:, 1:][np.isinf(s[:, :-1])]))
    # shuffling the polygons permutes the ids and nothing else: no two keys of a point tie in this scene
    assert nc.min_key_gap(points, rings, dists, "intersects") > 0.0
    perm = np.random.default_rng(2).permutation(len(rings))
    other = nc.nearest(points, [rings[p] for p in perm], 3, dists[perm])
    assert np.array_equal(np.append(perm, len(rings))[other["polygon"]], nc.nearest(points, rings, 3, dists)["polygon"])


def test_stack_scene_has_the_counts_it_states():
    for k in (1, 3, 16):
        rings, points, counts = nc.scene_stack(k)
        r = nc.nearest(points, rings, k)
        assert r["count"].tolist() == counts.tolist()
        assert {0, 1, k - 1, k, k + 1, 32, 33, nc.STACK_COPIES} <= set(counts.tolist())
        assert r["counters"].tolist() == [int(counts.sum()), int(np.minimum(counts, k).sum()), int((counts > k).sum()), nc.STACK_COPIES]
        # the last point of the stack, x = 39.5 / 64: 32.5 / 64 from the left side of copy 7 and 31.5 / 64 from its right side,
        # the other way round in copy 8 -- a tie at the deepest key, and the lower id first
        last = int(np.argmax(counts))
        assert r["polygon"][last, :2].tolist() == [7, 8][:k] and r["dist2"][last, 0] == (31.5 / 64) ** 2
        assert nc.nearest(points, rings, 2)["dist2"][last].tolist() == [(31.5 / 64) ** 2] * 2


def test_erosion_mask_is_the_direct_definition_on_the_hand_cases():
    """in a square shrunk by d (closed): inside, and at least d from every side"""
    def direct(pt, x0, y0, side, d):
        x, y = pt - nc.ORIGIN
        return min(x - x0, x0 + side - x, y - y0, y0 + side - y) >= d and x0 < x < x0 + side and y0 < y < y0 + side
    scenes = ((nc.hand_unit_square(), [(0.0, 0.0, 1.0)]), (nc.hand_nested(), [(0.0, 0.0, 4.0), (1.0, 1.0, 2.0)]),
              (nc.hand_twins(), [(0.0, 0.0, 1.0), (-1.0, -1.0, 3.0), (0.0, 0.0, 1.0)]),
              (nc.hand_shared_vertex(), [(0.0, 0.0, 1.0), (1.0, 1.0, 1.0)]))
    n_in = 0
    for (rings, points), squares in scenes:
        r = nc.nearest(points, rings, len(rings), 0.0, "intersects")
        for d in (0.0, 0.125, 0.25, 0.5, 1.0, 2.0, 2.5):
            mask = nc.erosion_mask(r, d)
            for i in range(len(points)):
                want = {p for p, sq in enumerate(squares) if direct(points[i], *sq, d)}
                got = {int(p) for p, m in zip(r["polygon"][i], mask[i]) if m}
                # d = 0: a point ON the ring with a true parity is in the mask and not strictly inside: the closed set
                if d == 0.0:
                    got -= {int(p) for p, d2 in zip(r["polygon"][i], r["dist2"][i]) if d2 == 0.0}
                assert got == want, (d, i)
                n_in += len(want)
    assert n_in > 10
