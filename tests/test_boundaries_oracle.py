"""The oracle of the cell boundary tests against scipy (CPU): on every case the exact monotone-chain hull has the vertex
set of ``scipy.spatial.ConvexHull`` (Qhull), it starts at the lowest point and runs counter-clockwise, the degenerate rule
is the reference's, and the seeded real-coordinate cells have identical float64 and exact hulls."""
import numpy as np
import pytest
from scipy.spatial import ConvexHull, QhullError

import boundaries_cases as bc


def all_cells():
    cells = {("scene", c): p for c, p in bc.scene_cells().items()}
    cells.update({("real", c): p for c, p in bc.real_cells().items()})
    cells[("parabola", 0)] = bc.parabola()
    return cells


def test_hull_vertex_set_is_qhulls():
    compared = 0
    for key, pts in all_cells().items():
        got = bc.hull(pts)
        try:
            qh = ConvexHull(pts)
        except (QhullError, ValueError):                             # collinear, duplicate or too few points: Qhull itself raises
            assert got is None, key
            continue
        assert got is not None, key
        assert {tuple(v) for v in got} == {tuple(pts[i] + 0.0) for i in qh.vertices}, key
        assert len(got) == len({tuple(v) for v in got}) == len(qh.vertices), key
        compared += 1
    assert compared >= len(bc.ROUTE_SIZES) + 8


def test_rings_start_lowest_and_run_counter_clockwise():
    for key, pts in all_cells().items():
        ring = bc.hull(pts)
        if ring is None:
            continue
        assert tuple(ring[0]) == min(map(tuple, ring)), key
        nxt, prv = np.roll(ring, -1, 0), np.roll(ring, 1, 0)
        turn = (ring[:, 0] - prv[:, 0]) * (nxt[:, 1] - ring[:, 1]) - (ring[:, 1] - prv[:, 1]) * (nxt[:, 0] - ring[:, 0])
        assert (turn > 0).all(), key                                 # strictly convex: no vertex on an edge


def test_degenerate_rule_is_the_references():
    hulls = bc.scene_hulls()
    for c, pts in bc.tiny_cells().items():
        distinct = np.unique(pts + 0.0, axis=0)
        collinear = len(distinct) < 3 or np.linalg.matrix_rank(distinct[1:] - distinct[0]) < 2
        assert (hulls[c] is None) == bool(collinear), c
    assert [c for c in sorted(bc.tiny_cells()) if hulls[c] is not None] == [5, 6, 7, 8]
    assert len(hulls[6]) == 4 and len(hulls[7]) == 4 and len(hulls[8]) == 3
    assert len(hulls[40]) == 200 and len(hulls[41]) == 100
    assert len(bc.hull(bc.parabola())) == 5000 > bc.CHUNK_MAX_HULL


def test_real_coordinate_cells_have_identical_float64_and_exact_hulls():
    for c, pts in bc.real_cells().items():
        exact, f64 = bc.hull(pts), bc.hull_f64(pts)
        assert exact is not None and f64 is not None and np.array_equal(exact.view(np.uint64), f64.view(np.uint64)), c


def test_chaikin_doubles_the_vertices_and_keeps_convexity():
    ring = bc.scene_hulls()[41]
    for s in (1, 3):
        out = bc.chaikin(ring, s)
        assert out.shape == (len(ring) << s, 2)
        nxt, prv = np.roll(out, -1, 0), np.roll(out, 1, 0)
        turn = (out[:, 0] - prv[:, 0]) * (nxt[:, 1] - out[:, 1]) - (out[:, 1] - prv[:, 1]) * (nxt[:, 0] - out[:, 0])
        assert (turn >= -1e-6 * np.abs(turn).max()).all()
    assert np.array_equal(bc.chaikin(ring, 0), ring)


def test_scene_is_inside_the_exact_range_and_interleaved():
    xy, ids = bc.scene()
    assert np.abs(xy).max() < bc.LIMIT and np.array_equal(xy, np.round(xy))
    assert (ids < 0).sum() == 500 and (np.diff(ids) < 0).sum() > 1000
    assert sorted(set(ids[ids >= 0])) == sorted(bc.scene_cells())
