"""The oracle of the ring-rasterisation tests, checked on the CPU: it agrees with the hand-worked image, with the integer
raster of contour_cases.py, with the exact-rational predicate of polygon_join_cases.py on every case, and it inverts the
contour oracle on the admitted labels of a Voronoi scene."""
import numpy as np
import pytest

import contour_cases as cc
import morphology_cases as mc
import rasterize_cases as rc


@pytest.mark.parametrize("predicate", rc.PREDICATES)
def test_hand_worked_image(predicate):
    c = rc.cases()[0]
    assert c["name"] == "hand8"
    want = rc.expected(c, predicate, "lowest")
    assert np.array_equal(want["image"], rc.hand_image(predicate))
    assert want["n_covered"].tolist() == ([9, 10] if predicate == "intersects" else [1, 1])
    assert want["counters"]["n_overlaps"] == 0 and want["counters"]["n_clipped"] == 0


def _integer_rings():
    rings = [rc.HAND_SQUARE, rc.HAND_TRIANGLE, [[1, 1], [3, 3], [5, 5]], [[0, 0], [6, 2], [3, 7], [1, 4]]]
    rings += rc.rings_of(cc.expected(cc.voronoi_small()))[0][:12]
    return [np.asarray(r, np.float64) for r in rings]


def test_oracle_equals_the_integer_raster_on_integer_rings():
    """closed <-> "intersects", strict <-> "contains" (contour_cases.raster walks the ring's bounding box)"""
    rings = _integer_rings()
    shape = (100, 100)
    masks = rc.masks_f64(rings, shape)
    for ring, m in zip(rings, masks):
        closed, strict = cc.raster([(int(x), int(y)) for x, y in ring])
        for name, want in (("intersects", closed), ("contains", strict)):
            got = {(int(i % shape[1]), int(i // shape[1])) for i in m[name]}
            assert got == want, (ring.tolist(), name)


@pytest.mark.parametrize("name", [c["name"] for c in rc.cases()])
def test_float64_oracle_equals_the_exact_rational_one(name):
    c = next(c for c in rc.cases() if c["name"] == name)
    f64 = rc.reference(name)
    exact = rc.masks_exact(c["rings"], c["shape"], c["scale"], c["translation"])
    for p, (a, b) in enumerate(zip(f64, exact)):
        for predicate in rc.PREDICATES:
            assert np.array_equal(a[predicate], b[predicate]), (name, p, predicate)


def test_cases_hold_what_they_are_for():
    by = {c["name"]: c for c in rc.cases()}
    sizes = [len(mc.open_ring(r)) for n in ("tier_edges", "ring4096") for r in by[n]["rings"]]
    assert sorted(sizes) == [3, 64, 64, 65, 4096]
    _, ws = rc.widths(8)
    assert {1, 63, 64, 65, 7, 8, 9} <= set(ws)
    w = rc.expected(by["widths"], "intersects", "lowest")
    cols = [int((w["image"] == k + 1).any(0).sum()) for k in range(len(ws))]
    assert cols == ws                                                # each rectangle covers exactly that many columns
    assert rc.expected(by["sliver"], "intersects", "lowest")["counters"]["n_empty"] == 1
    col = {p: rc.expected(by["collinear"], p, "lowest") for p in rc.PREDICATES}
    assert col["intersects"]["n_covered"].tolist() == [5, 5] and col["contains"]["n_covered"].tolist() == [0, 0]
    deg = rc.expected(by["degenerate"], "intersects", "lowest")
    assert deg["counters"]["n_degenerate"] == 4 and deg["counters"]["n_empty"] == 4 and deg["n_covered"].tolist() == [0, 0, 0, 0, 16]
    out = rc.expected(by["outside_and_clipped"], "intersects", "lowest")
    assert out["counters"]["n_clipped"] == 6 and out["n_covered"][0] == 0 and (out["n_covered"][1:] > 0).all()
    lo = rc.expected(by["nested_twins_shared_edge"], "intersects", "lowest")
    hi = rc.expected(by["nested_twins_shared_edge"], "intersects", "highest")
    assert lo["counters"]["n_overlaps"] == hi["counters"]["n_overlaps"] > 0 and not np.array_equal(lo["image"], hi["image"])
    assert lo["n_won"][2] == 0 and hi["n_won"][1] < hi["n_covered"][1]        # the twin with the losing index wins nothing
    assert (lo["image"][1:13, 12] == 1).all() and (hi["image"][1:13, 12] == 4).all()      # the shared edge x = 12


def test_oracle_round_trip_on_the_admitted_labels():
    """image -> contour oracle -> raster oracle -> image.  voronoi_small() meets the condition under the oracle alone (at
    least half of the labels present are admitted), so no other scene was needed."""
    img = cc.voronoi_small()
    want = cc.expected(img)
    ok = cc.admitted(img, want["by_label"])
    assert len(ok) >= 0.5 * len(want["by_label"]), (len(ok), len(want["by_label"]))
    rings, labels = rc.rings_of(want, set(ok))
    masks = rc.masks_f64(rings, img.shape)
    got = rc.resolve(masks, rings, img.shape, (1.0, 1.0), (0.0, 0.0), labels, "intersects", "lowest")
    assert np.array_equal(got["image"], np.where(np.isin(img, ok), img, 0))
    assert got["counters"]["n_overlaps"] == 0 and got["counters"]["n_empty"] == 0
    assert np.array_equal(got["n_covered"], np.asarray([(img == lab).sum() for lab in labels]))
