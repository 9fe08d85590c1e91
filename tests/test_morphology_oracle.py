"""The oracle of the boundary morphology tests, checked on the CPU (no product code is imported).

* Hull: the float64 oracle's hull vertex set and hull area equal ``scipy.spatial.ConvexHull`` (``.vertices``, ``.volume``)
  on every non-degenerate case -- the one outside pin available without shapely -- and the committed
  tests/golden/morphology_small.npz holds what scipy said, for machines without scipy.
* Float64 against exact: the same hull, and the five float quantities within the recorded ``E_REF``.

Largest relative deviation of the float64 oracle from the exact one, per column, over the named cases, their copies on
slide coordinates, the degenerate rings and the 1 000-ring batch (measured here, recorded as
``morphology_cases.E_REF``, the yardstick of tests/test_gpu_morphology.py):

    area 0    hull_area 0    envelope_area 0    rect_area 2.22e-16 (recorded as 2.3e-16)    radius 2.45e-16 (recorded as 2.5e-16)

(the three areas are sums of exactly representable products of translated coordinates: exact in float64).
"""
import math
import os

import numpy as np
import pytest

import morphology_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morphology_small.npz")


def test_hull_equals_scipy():
    spatial = pytest.importorskip("scipy.spatial")
    f64, _ = mc.reference("cases")
    for (name, ring), got in zip(mc.cases(), f64):
        if name not in mc.NON_DEGENERATE:
            continue
        pts = mc.open_ring(ring)
        hull = spatial.ConvexHull(pts)
        # as coordinates: of repeated vertices scipy and the oracle may name different copies
        assert {tuple(pts[i]) for i in hull.vertices} == {tuple(pts[i]) for i in got["hull"]}, name
        assert len(got["hull"]) == got["n_hull"] == len({tuple(pts[i]) for i in hull.vertices}), name
        assert abs(got["hull_area"] - hull.volume) <= mc.scipy_area_tolerance(pts), (name, got["hull_area"], hull.volume)


def test_golden_file_holds_scipys_numbers():
    g = np.load(GOLDEN)
    f64, _ = mc.reference("cases")
    by_name = {name: (ring, got) for (name, ring), got in zip(mc.cases(), f64)}
    assert len(g["names"]) == len(mc.NON_DEGENERATE) - 2
    for p, name in enumerate(g["names"]):
        ring, got = by_name[str(name)]
        b, e = g["ring_offsets"][p], g["ring_offsets"][p + 1]
        assert np.array_equal(g["xy"][b:e], ring), name
        verts = g["scipy_hull_vertices"][g["scipy_hull_offsets"][p]:g["scipy_hull_offsets"][p + 1]]
        pts = mc.open_ring(ring)
        assert {tuple(pts[i]) for i in verts} == {tuple(pts[i]) for i in got["hull"]}, name
        assert abs(got["hull_area"] - g["scipy_hull_area"][p]) <= mc.scipy_area_tolerance(pts), name


@pytest.mark.parametrize("which", ["cases", "batch"])
def test_float64_oracle_agrees_with_exact(which):
    f64, exact = mc.reference(which)
    worst = {c: 0.0 for c in mc.FLOAT_COLS}
    for p, (got, ex) in enumerate(zip(f64, exact)):
        assert got["n_hull"] == ex["n_hull"] and got["hull"] == ex["hull"], p
        want = mc.exact_floats(ex)
        for c in mc.FLOAT_COLS:
            if math.isnan(want[c]):
                assert math.isnan(got[c]), (p, c)
            else:
                worst[c] = max(worst[c], mc.rel_dev(got[c], want[c]))
    print(f"e_ref[{which}] =", worst)
    for c in mc.FLOAT_COLS:
        assert worst[c] <= mc.E_REF[c], (c, worst[c], mc.E_REF[c])


def test_expected_shapes_of_the_cases():
    f64 = dict(zip((name for name, _ in mc.cases()), mc.reference("cases")[0]))
    r = {name: mc.ratios(*(f64[name][c] for c in mc.FLOAT_COLS)) for name in f64}
    assert r["l_shape"][1] > 1 and r["star5"][1] > 1                              # convexity
    assert r["square_ccw"][1] == 1 and np.array_equal(r["square_ccw"], r["square_cw"])
    assert np.array_equal(r["square_ccw"], r["square_closed"]) and np.array_equal(r["square_ccw"], r["square_edge_vertices"])
    assert np.array_equal(r["square_ccw"], r["square_repeated"])
    assert r["rect_10x1_rot30"][2] < 0.5                                          # elongation
    for name, support in (("rect_10x1_rot30", 2), ("obtuse", 2)):                 # the circle on the longest chord
        ring = mc.open_ring(dict(mc.cases())[name])
        longest = max(math.dist(a, b) for a in ring for b in ring)
        assert math.isclose(f64[name]["radius"], longest / 2, rel_tol=1e-12), name
    acute = dict(mc.cases())["acute"]
    assert f64["acute"]["radius"] > max(math.dist(a, b) for a in acute for b in acute) / 2 * 1.01   # three support points
    assert [f64[n]["n_hull"] for n in mc.DEGENERATE] == [0, 1, 2, 2, 1]
    assert f64["segment"]["radius"] == 2.5 and f64["collinear5"]["area"] == 0 and f64["collinear5"]["rect_area"] == 0
    assert len(mc.open_ring(dict(mc.cases())["star_max"])) == mc.MAX_VERTS
    assert len(mc.batch()) == 1000
