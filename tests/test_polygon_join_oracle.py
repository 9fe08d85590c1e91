"""The two oracles of tests/polygon_join_cases.py against each other (CPU, no product import): the float64 oracle equals
the exact one outside the undecided band under both predicates, the undecided pairs stay below the cap, E_REF is what
the float64 oracle's dist2 really deviates by, and the two predicates relate as their definitions say."""
import numpy as np
import pytest

import polygon_join_cases as pc

RUNS = [("cases", d) for d in pc.D_CASES] + [("batch", r) for r in pc.BATCH_RATIOS]


def rows(a):
    return {(int(x), int(y)) for x, y in a}


@pytest.mark.parametrize("which,d", RUNS)
def test_float64_oracle_equals_exact_outside_the_band_and_the_cap_holds(which, d):
    ref = pc.reference(which, d)
    undecided = rows(ref["undecided"])
    for pred in pc.PREDICATES:
        f64 = rows(ref["f64"][pred])
        if which == "cases":
            assert f64 - undecided == rows(ref["exact"][pred]) - undecided, pred
        else:                        # the exact oracle saw the near-boundary pairs only: every one of them must agree
            near = rows(ref["f64"]["near"])
            assert (f64 & near) - undecided == rows(ref["exact"][pred]) - undecided, pred
        assert len(f64) > 0
        print(which, d, pred, "pairs", len(f64), "undecided", len(undecided))
        assert len(undecided) <= pc.MAX_UNDECIDED * len(f64), (which, d, pred, len(undecided), len(f64))


def _dist2_error(points, rings, dists, exact_dist2):
    worst = 0.0
    by_ring = {}
    for (i, p), d2 in exact_dist2.items():
        if d2 is not None:
            by_ring.setdefault(p, []).append((i, d2))
    for p, items in by_ring.items():
        idx = np.array([i for i, _ in items])
        _, _, got, _ = pc.match_f64(points[idx], rings[p], float(dists[p]))
        for g, (_, want) in zip(got, items):
            if want == 0:
                assert g == 0.0                                       # on the ring: exact in float64 on these coordinates
            else:
                worst = max(worst, abs(float((pc.Fraction(float(g)) - want) / want)))
    return worst


def test_float64_oracle_dist2_error():
    rings, _, points, _, _ = pc.cases()
    worst = _dist2_error(points, rings, pc.reference("cases", 0.25)["dists"], pc.reference("cases", 0.25)["exact"]["dist2"])
    brings, bpoints = pc.batch()
    rng = np.random.default_rng(5)
    f64 = pc.reference("batch", 0.05)["f64"]
    sample = np.concatenate([f64["intersects"][rng.choice(len(f64["intersects"]), 1500, replace=False)], f64["near"]])
    dists = pc.reference("batch", 0.05)["dists"]
    exact = pc.join_exact(bpoints, brings, dists, only=sample)
    worst = max(worst, _dist2_error(bpoints, brings, dists, exact["dist2"]))
    print("largest relative error of the float64 dist2:", worst)
    assert worst <= pc.E_REF
    assert pc.BAND == max(8 * pc.E_REF, 4 * pc.ULP)
    # the sampled pairs of the batch agree with float64 as well (they are far from the boundary)
    und = rows(exact["undecided"])
    assert rows(sample) & rows(f64["contains"]) - und == rows(exact["contains"]) - und


@pytest.mark.parametrize("which,d", RUNS)
def test_contains_is_a_subset_of_intersects(which, d):
    f64 = pc.reference(which, d)["f64"]
    assert rows(f64["contains"]) <= rows(f64["intersects"])
    if which == "cases":
        exact = pc.reference(which, d)["exact"]
        assert rows(exact["contains"]) <= rows(exact["intersects"])


def test_without_a_buffer_the_predicates_differ_by_the_on_ring_points():
    rings, _, points, labels, _ = pc.cases()
    ref = pc.reference("cases", 0.0)
    on_ring = {k for k, d2 in ref["exact"]["dist2"].items() if d2 is not None and d2 == 0}
    assert len(on_ring) >= 3 * 20                                     # vertices and edge midpoints of every real ring
    assert len(ref["undecided"]) == 0
    for src in ("exact", "f64"):
        assert rows(ref[src]["intersects"]) - rows(ref[src]["contains"]) == on_ring, src
    # with d > 0 the on-ring points are in under both
    ref = pc.reference("cases", 0.25)
    assert on_ring <= rows(ref["exact"]["contains"])


def test_the_inputs_are_what_the_issue_asks_for():
    rings, names, points, labels, owner = pc.cases()
    assert {"square", "l_shape", "star5", "regular13", "regular25", "star63", "star64", "star65", "star200", "square_closed",
            "empty", "point", "segment", "collinear4"} <= set(names)
    assert all(n + "_cw" in names for n in names[:10])
    assert [len(pc.mc.open_ring(r)) for r, n in zip(rings, names) if n in ("star63", "star64", "star65", "star200")] == [63, 64, 65, 200]
    for d in pc.D_CASES:                                              # degenerate rings match nothing
        ex = pc.reference("cases", d)["exact"]
        degenerate = {names.index(n) for n in ("empty", "point", "segment")}
        assert not {p for _, p in rows(ex["intersects"])} & degenerate
    assert labels[-1] == "far" and not any(i == len(points) - 1 for i, _ in rows(pc.reference("cases", 0.25)["f64"]["intersects"]))
    notch = labels.index("l_shape:notch")
    assert not any(i == notch for i, _ in rows(pc.reference("cases", 0.25)["exact"]["intersects"]))
    brings, bpoints = pc.batch()
    n_verts = np.array([len(pc.mc.open_ring(r)) for r in brings])
    assert 1900 <= len(brings) <= 2100 and 49_000 <= len(bpoints) <= 51_000
    assert (n_verts == 64).sum() >= 2 and (n_verts == 65).sum() >= 2 and 25 <= (n_verts > 65).sum() <= 40
    pairs = pc.reference("batch", 0.05)["f64"]["contains"]
    per_point = np.bincount(pairs[:, 0], minlength=len(bpoints))
    per_polygon = np.bincount(pairs[:, 1], minlength=len(brings))
    assert (per_point >= 3).sum() > 100 and (per_polygon[n_verts >= 3] == 0).sum() >= 5
