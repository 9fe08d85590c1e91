"""The ring layer on the device (csrc/rings.h): morphology and the polygon join count "entries", "open vertices" and
"route" the same way.

Eight rings: a 64- and a 65-vertex star, each open, closed with its first vertex, reversed, and reversed and closed.  The
closed 64-vertex ring has 65 entries and must still take the register route; the closed 65-vertex ring has 66 and takes
the LDS route like its open twin.  A closed ring must give the bits of its open twin in ``polygon_props`` and the points
of its open twin in ``points_in_polygons``; both must agree with the float64 oracles, which drop the closing vertex
themselves.  A unit that counted entries instead of open vertices, or chose the route from another number than the one
it loads, would differ from its twin or from the oracle here.
"""
import functools

import numpy as np
import pytest
import torch

import morphology_cases as mc
import polygon_join_cases as pjc

pytestmark = pytest.mark.gpu

SEEDS = {64: 6401, 65: 6501}
DISTS = (0.0, 0.25)
TWINS = ((0, 1), (2, 3), (4, 5), (6, 7))                             # (open, closed)


@functools.lru_cache(maxsize=None)
def inputs() -> tuple:
    """(rings, points): per n the ring open, closed, reversed, reversed and closed, all at SLIDE; about 500 points over the
    rings' bounds grown by 1, and every ring's first vertex"""
    rings = []
    for n, seed in SEEDS.items():
        base = mc.star_ring(n, seed) + mc.quantize(mc.SLIDE)
        for ring in (base, base[::-1]):
            rings += [np.ascontiguousarray(ring), np.concatenate([ring, ring[:1]])]
    lo = np.min([r.min(0) for r in rings], axis=0) - 1.0
    hi = np.max([r.max(0) for r in rings], axis=0) + 1.0
    points = mc.quantize(np.random.default_rng(65).uniform(lo, hi, (500, 2)))
    return tuple(rings), np.concatenate([points, np.asarray([r[0] for r in rings])])


@functools.lru_cache(maxsize=None)
def join_reference(d: float) -> dict:
    """the float64 join and the pairs the exact oracle has within the undecided band"""
    rings, points = inputs()
    dists = np.full(len(rings), d)
    f64 = pjc.join_f64(points, rings, dists)
    return {"f64": f64, "undecided": pjc.join_exact(points, rings, dists, only=f64["near"])["undecided"]}


def test_the_inputs_are_what_the_test_is_about():
    rings, points = inputs()
    assert [len(r) for r in rings] == [64, 65, 64, 65, 65, 66, 65, 66]
    assert [len(mc.open_ring(r)) for r in rings] == [64, 64, 64, 64, 65, 65, 65, 65]
    for d in DISTS:
        ref = join_reference(d)
        assert len(ref["f64"]["contains"]) > 500                     # every ring holds many of the points
        assert len(ref["undecided"]) == 0                            # these seeds: within pjc.MAX_UNDECIDED, and nothing to leave out


def test_polygon_props_of_a_closed_ring_are_its_open_twins(cuda):
    from segger_amd import morphology as mo
    rings, _ = inputs()
    offsets, xy = mc.to_csr(rings)
    got = {k: v.cpu().numpy() for k, v in mo.polygon_props(torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda)).items()}
    for p, ring in enumerate(rings):
        want = mc.props_f64(ring)
        assert got["n_hull"][p] == want["n_hull"], p
        assert np.array_equal(got["bounds"][p], np.asarray(want["bounds"])), p
        for c in mc.FLOAT_COLS:
            dev = mc.rel_dev(float(got[c][p]), want[c])
            print(p, c, dev)
            assert dev <= mc.tolerance(c), (p, c, float(got[c][p]), want[c])
    for a, b in TWINS:
        for c in mc.FLOAT_COLS + ("bounds", "n_hull"):
            assert np.asarray(got[c][a]).tobytes() == np.asarray(got[c][b]).tobytes(), (a, b, c)


@pytest.mark.parametrize("d", DISTS)
@pytest.mark.parametrize("pred", pjc.PREDICATES)
def test_points_in_a_closed_ring_are_those_in_its_open_twin(cuda, pred, d):
    from segger_amd import geometry as ge
    rings, points = inputs()
    offsets, xy = pjc.to_csr(rings)
    ei = ge.points_in_polygons(torch.from_numpy(points).to(cuda), torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda),
                               buffer=d, predicate=pred)
    got = ei.t().cpu().numpy()
    by_ring = [set(got[got[:, 1] == p, 0].tolist()) for p in range(len(rings))]
    for a, b in TWINS:
        assert by_ring[a] == by_ring[b] and len(by_ring[a]) > 50, (a, b, sorted(by_ring[a] ^ by_ring[b])[:10])
    ref = join_reference(d)
    g = {tuple(r) for r in pjc.without(got, ref["undecided"]).tolist()}
    w = {tuple(r) for r in pjc.without(ref["f64"][pred], ref["undecided"]).tolist()}
    assert g == w, ("extra", sorted(g - w)[:10], "missing", sorted(w - g)[:10])
