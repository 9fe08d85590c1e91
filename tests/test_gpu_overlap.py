"""segger_amd.overlap on the device against the exact oracles of tests/overlap_cases.py: pairs and the first two counters
EQUAL to the oracle's, every area within the DERIVED bound 2^-52 (T S + 16 T W H) -- any-order summation of T terms errs by
at most (T - 1) u S, a term is about a dozen operations on translated coordinates and carries at most 16 u W H, u = 2^-53,
doubled; T and S come from the exact oracle, W and H are the pair's joint extent -- identical bits across runs, orders,
tiers and grids, and the chains from the project's three sources of rings."""
import numpy as np
import pytest
import torch

import overlap_cases as oc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def to_dev(rings):
    return tuple(torch.from_numpy(t).to(dev()) for t in oc.csr(rings))


def run(rings_a, rings_b, **kw):
    from segger_amd import polygon_overlaps
    out = polygon_overlaps(*to_dev(rings_a), *to_dev(rings_b), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_boxes(n, seed):
    rng = np.random.default_rng(seed)
    return [np.array([(0, a), (b, 0), (100, c), (d, 100)], np.float64) for a, b, c, d in rng.integers(1, 100, (n, 4))]


@pytest.fixture(scope="module")
def batches():
    """(name, A, B, the exact join) -- computed once, never changed"""
    import simplify_cases as sc
    hand_a, hand_b = [v[0] for v in oc.HAND.values()], [v[1] for v in oc.HAND.values()]
    vor = sc.voronoi_rings()[:10]                                    # pixel contours: vertical and horizontal edges only
    shifted = [r + np.array([3.0, 2.0]) for r in vor]
    s1, s2 = oc.scene(300, 1), oc.scene(300, 2)
    whole = oc.rect(-200, -200, 4200, 4200)
    out = [("hand", hand_a, hand_b), ("boundaries",) + oc.boundary_sets(), ("pixel_identical", vor, vor), ("pixel_shifted", vor, shifted),
           ("scene", s1, s2), ("wide_a", s1[:150] + [whole], s2[:150]), ("wide_both", [whole] + s1[:100], s2[:100] + [whole[::-1]]),
           ("stacked", oc.scene(40, 3, extent=1), oc.scene(40, 4, extent=1)), ("same_boxes", same_boxes(30, 5), same_boxes(30, 6))]
    return [(name, a, b, oc.expected(a, b)) for name, a, b in out]


def check(got, want, what):
    assert np.array_equal(got["pairs"], want["pairs"]), (what, got["pairs"].shape, want["pairs"].shape)
    assert got["counters"][0] == len(want["candidates"]) and got["counters"][1] == want["pairs"].shape[1], (what, got["counters"])
    err = np.abs(got["area"] - want["area"])
    worst = int(np.argmax(err - want["tol"])) if len(err) else 0
    assert (err <= want["tol"]).all(), (what, want["pairs"][:, worst], got["area"][worst], want["area"][worst], want["tol"][worst])


@pytest.mark.parametrize("route", (None, "large"))
def test_pairs_counters_and_areas_against_the_exact_oracle(batches, route):
    lds = 0
    for name, a, b, want in batches:
        got = run(a, b, _route=route)
        check(got, want, (name, route))
        assert (got["area"] <= np.minimum(got["area_a"][got["pairs"][0]], got["area_b"][got["pairs"][1]])).all() and (got["area"] >= 0).all()
        lds += int(got["counters"][2])
        if route == "large":
            assert got["counters"][2] == got["counters"][0]
        if name.startswith("wide"):
            assert got["counters"][3] == (2 if name == "wide_both" else 1)
    assert lds > 0


def test_hand_cases_one_by_one():
    for name, (a, b, area, hit) in oc.HAND.items():
        got = run([a], [b])
        assert got["pairs"].shape[1] == int(hit), name
        if hit and area is not None:
            assert got["area"][0] == area, (name, got["area"])       # small integers: every term is exact


def test_identical_bits_across_runs_orders_tiers_and_grids(batches):
    for name in ("scene", "boundaries", "wide_a"):
        _, a, b, want = next(x for x in batches if x[0] == name)
        base = run(a, b)
        for kw in ({}, {"_route": "large"}, {"cells_per_polygon": 0.1}, {"cells_per_polygon": 4.0}, {"cells_per_polygon": 37.0}):
            other = run(a, b, **kw)
            assert other["pairs"].tobytes() == base["pairs"].tobytes() and other["area"].tobytes() == base["area"].tobytes(), (name, kw)
            assert other["counters"][0] == base["counters"][0]
        rng = np.random.default_rng(9)
        pa, pb = rng.permutation(len(a)), rng.permutation(len(b))
        got = run([a[i] for i in pa], [b[i] for i in pb])
        back = np.stack([pa[got["pairs"][0]], pb[got["pairs"][1]]])
        order = np.lexsort((back[1], back[0]))
        assert np.array_equal(back[:, order], base["pairs"]) and got["area"][order].tobytes() == base["area"].tobytes(), name


def test_swapped_sets_give_transposed_pairs(batches):
    for name, a, b, want in batches:
        if name not in ("hand", "scene", "pixel_shifted"):
            continue
        got = run(b, a)
        order = np.lexsort((got["pairs"][0], got["pairs"][1]))
        assert np.array_equal(got["pairs"][::-1][:, order], want["pairs"]), name
        assert (np.abs(got["area"][order] - want["area"]) <= want["tol"]).all(), name


def test_polygons_in_polygons_is_the_pair_set(batches):
    from segger_amd import polygons_in_polygons
    _, a, b, want = next(x for x in batches if x[0] == "scene")
    got = polygons_in_polygons(*to_dev(a), *to_dev(b))
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want["pairs"])
    assert np.array_equal(polygons_in_polygons(*to_dev(a), *to_dev(b), predicate="intersects").cpu().numpy(), want["pairs"])
    with pytest.raises(ValueError, match="'contains' is not built"):
        polygons_in_polygons(*to_dev(a), *to_dev(b), predicate="contains")


def test_match_polygons_equals_its_restatement(batches):
    from segger_amd import match_polygons, polygon_overlaps
    _, a, b, want = next(x for x in batches if x[0] == "scene")
    out = polygon_overlaps(*to_dev(a), *to_dev(b))
    got = {k: v.cpu().numpy() for k, v in match_polygons(out).items()}
    ref = oc.match_numpy(*(out[k].cpu().numpy() for k in ("pairs", "area", "area_a", "area_b")))
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert (got["best_b"] == -1).any() and (got["n_overlapping"] > 1).any()
    # a constructed tie: a0 meets b0, b1, b2 with IoU 1/3, 1/3, 1/7; b1 meets a0 and a1 with IoU 1/3 each
    tie = {"pairs": torch.tensor([[0, 0, 0, 1], [0, 1, 2, 1]], device=dev()), "area": torch.tensor([2.0, 2.0, 1.0, 2.0], dtype=torch.float64, device=dev()),
           "area_a": torch.tensor([4.0, 4.0, 9.0], dtype=torch.float64, device=dev()), "area_b": torch.tensor([4.0, 4.0, 4.0], dtype=torch.float64, device=dev())}
    m = match_polygons(tie)
    assert m["best_b"].tolist() == [0, 1, -1] and m["best_a"].tolist() == [0, 0, 0] and m["n_overlapping"].tolist() == [3, 1, 0]
    assert m["best_iou"].tolist() == [2.0 / 6.0, 2.0 / 6.0, 0.0] and m["n_overlapping_b"].tolist() == [1, 2, 1]
    ref = oc.match_numpy(*(tie[k].cpu().numpy() for k in ("pairs", "area", "area_a", "area_b")))
    assert all(np.array_equal(m[k].cpu().numpy(), ref[k]) for k in ref)


def test_one_full_pair_of_4096_vertex_rings():
    """1.7e7 edge pairs on one wave.  B is A from another start vertex, reversed: the exact area is A's.  T and S are too many
    terms for Fraction; they come from the float64 formula, S scaled DOWN by 1e-9 so that its rounding cannot widen the bound."""
    a = oc.star(oc.MAX_VERTS, 77, scale=1 << 20)
    b = np.roll(a, -1000, 0)[::-1].copy()
    exact = abs(oc.shoelace2(oc.ints(a))) / 2.0
    _, T, S = oc.area_formula_f64(a, b, rows=128)
    ext = a.max(0) - a.min(0)
    tol = 2.0 ** -52 * (T * S * (1 - 1e-9) + 16.0 * T * ext[0] * ext[1])
    got = run([a], [b])
    assert got["pairs"].tolist() == [[0], [0]] and got["counters"].tolist()[:3] == [1, 1, 1]
    assert abs(got["area"][0] - exact) <= tol, (got["area"][0], exact, tol)
    assert got["area"][0] <= got["area_a"][0]


def test_refusals_and_empty_sets():
    from segger_amd import polygon_overlaps
    tri, long_ring = oc.star(3, 1), oc.star(oc.MAX_VERTS + 1, 5, scale=1 << 20)
    with pytest.raises(ValueError, match="set B: polygon 1 has 4097 vertices"):
        run([tri], [tri, long_ring])
    with pytest.raises(ValueError, match="set A: polygon 0 has 4097 vertices"):
        run([long_ring], [tri])
    off, xy = to_dev([tri, oc.SQUARE])
    bad = off.clone()
    bad[1] = 99
    with pytest.raises(ValueError, match="set B: ring_offsets of polygon 0"):
        polygon_overlaps(off, xy, bad, xy)
    nan = xy.clone()
    nan[2, 0] = float("nan")
    with pytest.raises(ValueError, match="set A: xy holds a non-finite"):
        polygon_overlaps(off, nan, off, xy)
    none = (torch.zeros(1, dtype=torch.int64, device=dev()), torch.empty(0, 2, dtype=torch.float64, device=dev()))
    for args in ((*none, off, xy), (off, xy, *none), (*none, *none)):
        out = polygon_overlaps(*args)
        assert out["pairs"].shape == (2, 0) and out["pairs"].dtype == torch.int64 and out["area"].shape == (0,)
        assert out["counters"].tolist() == [0, 0, 0, 0]
    assert polygon_overlaps(off, xy, *none)["area_a"].shape == (2,)
    out = run([tri[:2], tri[:1]], [tri])                              # rings of 2 and 1 vertices pair with nothing
    assert out["pairs"].shape == (2, 0) and out["counters"].tolist()[:2] == [0, 0]


def identity_bound(n_a, n_b, box):
    """the bound with what is known without an oracle: T <= n_a n_b terms, each at most W H in magnitude"""
    T, wh = n_a * n_b, (box[2] - box[0]) * (box[3] - box[1])
    return 2.0 ** -52 * (T * (T * wh) + 16.0 * T * wh)


def test_chain_label_contours_simplified_against_unsimplified():
    import contour_cases as cc
    from segger_amd import label_contours, match_polygons, polygon_overlaps, polygon_props, simplify_rings
    c = label_contours(torch.from_numpy(cc.voronoi_small()).to(dev()))
    s = simplify_rings(c["ring_offsets"], c["xy"], 0.0)
    assert s["xy"].shape[0] <= c["xy"].shape[0]                       # tolerance 0 drops collinear vertices only, if any are left
    out = polygon_overlaps(s["ring_offsets"], s["xy"], c["ring_offsets"], c["xy"])
    m = match_polygons(out)
    n = c["ring_offsets"].numel() - 1
    assert m["best_b"].tolist() == list(range(n)) and m["best_a"].tolist() == list(range(n))      # every label matches itself
    diag = out["pairs"][0] == out["pairs"][1]
    n_a, n_b = (torch.diff(t["ring_offsets"]).cpu().numpy() for t in (s, c))
    box = polygon_props(c["ring_offsets"], c["xy"])["bounds"].cpu().numpy()
    tol = np.array([identity_bound(n_a[i], n_b[i], box[i]) for i in range(n)])
    area = out["area"][diag].cpu().numpy()
    assert (np.abs(area - out["area_b"].cpu().numpy()) <= tol).all()                  # tolerance 0 drops no area: IoU 1
    assert (np.abs(m["best_iou"].cpu().numpy() - 1.0) <= 4 * tol / area).all() and bool((m["best_iou"] <= 1.0).all())
    assert bool((out["area"][~diag] == 0).all())                      # neighbours share pixel-chain borders at most


def test_chain_hulls_against_outlines_of_the_same_cells():
    import outline_cases as ocs
    from segger_amd import cell_boundaries, cell_outlines, polygon_overlaps, polygon_props
    xy, cell, keep = (torch.from_numpy(np.asarray(t)).to(dev()) for t in ocs.scene())
    hulls = cell_boundaries(xy, cell, ocs.N_CELLS, keep=keep)
    outl = cell_outlines(xy, cell, ocs.N_CELLS, keep=keep)
    out = polygon_overlaps(hulls["ring_offsets"], hulls["xy"], outl["ring_offsets"], outl["xy"])
    a, b = out["pairs"]
    assert bool((out["area"] <= torch.minimum(out["area_a"][a], out["area_b"][b])).all())
    same = hulls["cell_ids"][a] == outl["cell_ids"][b]                # an outline lies inside the hull of the same transcripts
    assert int(same.sum()) == outl["cell_ids"].numel()
    n_a, n_b = torch.diff(hulls["ring_offsets"])[a[same]].cpu().numpy(), torch.diff(outl["ring_offsets"])[b[same]].cpu().numpy()
    box = polygon_props(hulls["ring_offsets"], hulls["xy"])["bounds"][a[same]].cpu().numpy()      # the hull's box holds the outline
    tol = np.array([identity_bound(x, y, bx) for x, y, bx in zip(n_a, n_b, box)])
    assert (np.abs((out["area"][same] - out["area_b"][b[same]]).cpu().numpy()) <= tol).all()
