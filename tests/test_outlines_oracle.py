"""The concave outline oracle of tests/outline_cases.py on the CPU: its exactness conditions hold for every committed case
and connectivity, the sequential peel of the reference and the parallel fixed point leave the same triangles (asserted
inside check_case), the crescent is really concave, and the pruning agrees with a recorded run of the reference's
``_CellOutline.refine`` (tests/golden/outlines_small.npz, written by tests/golden/make_outlines_golden.py)."""
import math
import os

import numpy as np
import pytest

import outline_cases as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outlines_small.npz")


@pytest.mark.parametrize("connectivity", oc.CONNECTIVITIES)
def test_conditions_hold_and_the_peel_is_order_independent(connectivity):
    for c, pts in oc.scene_cells().items():
        oc.check_case(pts, connectivity)


@pytest.mark.parametrize("connectivity", oc.CONNECTIVITIES)
def test_conditions_hold_for_the_cells_at_the_point_limit(connectivity):
    for c, pts in oc.big_cells().items():
        info = oc.check_case(pts, connectivity)
        assert info["triangles"] > 2 * len(pts) - 200 and len(np.unique(pts, axis=0)) == len(pts) == oc.MAX_POINTS - 1 + c
    assert len(np.unique(oc.too_big_cell(), axis=0)) == oc.MAX_POINTS + 1


def test_the_cases_show_what_they_are_for():
    cells = oc.cells()
    assert oc.outline(cells[1]) is not None and len(oc.outline(cells[1])) == 3
    assert all(oc.outline(cells[2], k) is None for k in oc.CONNECTIVITIES)              # thin: pruned away
    assert len(oc.outline(cells[4])) == 4
    assert all(oc.outline(cells[c]) is None for c in (5, 6, 7))
    for k in oc.CONNECTIVITIES:
        assert 0 < oc.outline_area(cells[9], k) < oc.hull_area(cells[9])                # the crescent is concave
    for c, touching in ((10, True), (11, False)):                                       # the neck severed at connectivity 1
        st = oc.State(cells[c])
        comps = oc.components(st, oc.prune_sequential(st, 1.0)[0])
        assert len(comps) == 2
        shared = set(st.simplices[comps[0][1]].ravel().tolist()) & set(st.simplices[comps[1][1]].ravel().tolist())
        assert len(shared) == (1 if touching else 0), c
    st = oc.State(cells[8])
    assert len(cells[8]) - len(st.points) == 15 and st.d_max > 0                        # duplicates, and d_max is not theirs


def test_rings_are_open_counter_clockwise_from_the_lowest_vertex():
    for c, pts in oc.cells().items():
        ring = oc.outline(pts, 1.0)
        if ring is None:
            continue
        assert len({tuple(v) for v in ring}) == len(ring) >= 3
        assert tuple(ring[0]) == min(tuple(v) for v in ring)
        area2 = float((ring[:, 0] * np.roll(ring[:, 1], -1) - np.roll(ring[:, 0], -1) * ring[:, 1]).sum())
        assert area2 > 0 and math.isclose(area2 / 2, oc.outline_area(pts, 1.0), rel_tol=1e-12)


def largest_cycle(points, rim):
    """polygonize, for edges that cross nowhere: drop dangles, trace the faces, -> the edges of the largest one"""
    edges = {tuple(sorted((tuple(points[a]), tuple(points[b])))) for a, b in rim}
    while True:
        deg = {}
        for u, v in edges:
            deg[u] = deg.get(u, 0) + 1
            deg[v] = deg.get(v, 0) + 1
        keep = {e for e in edges if deg[e[0]] > 1 and deg[e[1]] > 1}
        if keep == edges:
            break
        edges = keep
    nbrs = {}
    for u, v in edges:
        nbrs.setdefault(u, []).append(v)
        nbrs.setdefault(v, []).append(u)
    for u in nbrs:
        nbrs[u].sort(key=lambda w: math.atan2(w[1] - u[1], w[0] - u[0]))
    seen, best = set(), (0.0, None)
    for start in [(u, v) for u in nbrs for v in nbrs[u]]:
        if start in seen:
            continue
        face, (u, v) = [], start
        while (u, v) not in seen:
            seen.add((u, v))
            face.append((u, v))
            ring = nbrs[v]
            u, v = v, ring[(ring.index(u) - 1) % len(ring)]                             # the next edge clockwise: interior left
        area2 = sum(a[0] * b[1] - b[0] * a[1] for a, b in face)
        if area2 > best[0]:
            best = (area2, {tuple(sorted(e)) for e in face})
    return best[1]


def test_the_pruning_agrees_with_a_run_of_the_reference():
    g = np.load(GOLDEN)
    assert np.array_equal(g["connectivities"], oc.CONNECTIVITIES)
    cells = oc.cells()
    assert len(g["cell_ids"]) >= 10
    for c in g["cell_ids"].tolist():
        assert np.array_equal(g[f"points_{c}"], cells[c]), c                            # the fixture is of these cells
        for k, conn in enumerate(oc.CONNECTIVITIES):
            assert float(g[f"d_max_{c}_{k}"]) == oc.State(cells[c]).d_max, (c, conn)
            ring = oc.outline(cells[c], conn)
            want = largest_cycle(g[f"points_{c}"], g[f"rim_{c}_{k}"])
            if ring is None:
                assert want is None, (c, conn)
                continue
            got = {tuple(sorted((tuple(a), tuple(b)))) for a, b in zip(ring, np.roll(ring, -1, axis=0))}
            assert got == want, (c, conn)
