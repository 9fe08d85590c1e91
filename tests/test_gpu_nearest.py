"""segger_amd.nearest on the device against the CPU oracle of tests/nearest_cases.py.  ``polygon``, ``inside``, ``count`` and
the counters are EQUAL to the oracle, and ``dist2`` is BIT-equal: every operation is an IEEE float64 add, multiply, divide
or minimum in the oracle's order, contraction is off, and the coordinates are multiples of 2^-11 near ORIGIN, as the
join's.  The scenes stay below a few thousand points and sit on the kernels' own boundaries: the ring routes, the
wave-chunk edge of the cell walk, the cap k and the lane / wave threshold of the selection."""
import numpy as np
import pytest
import torch

import buffered_count_cases as bc
import nearest_cases as nc
import polygon_join_cases as pc

pytestmark = pytest.mark.gpu

KEYS = ("polygon", "dist2", "inside", "count", "counters")
DTYPES = {"polygon": torch.int32, "dist2": torch.float64, "inside": torch.bool, "count": torch.int32, "counters": torch.int64}


def tensors(cuda, points, rings):
    offsets, xy = pc.to_csr(rings)
    return (torch.from_numpy(np.ascontiguousarray(points)).to(cuda), torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda))


def run(cuda, points, rings, k, buffer=None, predicate="intersects", **kw):
    from segger_amd import nearest
    if isinstance(buffer, np.ndarray):
        buffer = torch.from_numpy(buffer).to(cuda)
    return nearest.nearest_boundaries(*tensors(cuda, points, rings), k, buffer=buffer, predicate=predicate, **kw)


def assert_equal(got, want, what=""):
    for name in KEYS:
        g = got[name].cpu().numpy()
        assert got[name].dtype == DTYPES[name] and got[name].is_cuda, (what, name)
        assert g.shape == want[name].shape, (what, name, g.shape, want[name].shape)
        if name == "dist2":                                          # bit for bit; +inf in the padding
            g, w = g.view(np.uint64), np.ascontiguousarray(want[name]).view(np.uint64)
        else:
            w = want[name]
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def check(cuda, points, rings, k, buffer=None, predicate="intersects", **kw):
    want = nc.nearest(points, rings, k, 0.0 if buffer is None else buffer, predicate)
    got = run(cuda, points, rings, k, buffer, predicate, **kw)
    print(predicate, "k", k, dict(zip(nc.COUNTER_NAMES, got["counters"].tolist())), "oracle", want["counters"].tolist())
    assert_equal(got, want, (predicate, k))
    return got, want


def test_public_names():
    import segger_amd
    from segger_amd import nearest, neighbors
    assert segger_amd.nearest is nearest and nearest.COUNTER_NAMES == nc.COUNTER_NAMES
    assert segger_amd.nearest_boundaries is nearest.nearest_boundaries and segger_amd.signed_distance is nearest.signed_distance
    assert segger_amd.prediction_graph_nearest is neighbors.prediction_graph_nearest


def test_hand_worked_cases(cuda):
    for scene, d in ((nc.hand_unit_square, 0.0), (nc.hand_unit_square, 0.5), (nc.hand_nested, 0.5), (nc.hand_twins, 0.0),
                     (nc.hand_shared_vertex, 0.0)):
        rings, points = scene()
        for pred in pc.PREDICATES:
            for k in (1, 2, 3):
                check(cuda, points, rings, k, d, pred)
    rings, points = nc.hand_shared_vertex()
    got = run(cuda, points, rings, 2)
    assert got["polygon"].tolist() == [[0, 1]] and got["dist2"].tolist() == [[0.0, 0.0]] and got["inside"].tolist() == [[False, True]]


@pytest.mark.parametrize("pred", pc.PREDICATES)
@pytest.mark.parametrize("d", pc.D_CASES)
def test_ring_routes_3_64_65_4096_vertices(cuda, pred, d):
    rings, points, _ = bc.scene_routes()
    got, want = check(cuda, points, rings, 3, d, pred)
    first = np.bincount(want["polygon"][:, 0], minlength=5)[:4]      # every route did rank first somewhere;
    assert np.all(first[1:] > 0) and (first[0] > 0) == (d > 0.0 or pred == "intersects")      # the open triangle holds no point


def test_cells_of_0_1_63_64_65_points(cuda):
    rings, points, _ = bc.scene_clusters()
    got, want = check(cuda, points, rings, 2, 0.0, "contains")
    assert np.bincount(nc.kept_pairs(want, len(rings))[:, 1], minlength=6).tolist() == [1, 63, 64, 65, 0, 193]
    check(cuda, points, rings, 1, 0.25, "intersects")


@pytest.mark.parametrize("k", [1, 3, 16])
def test_candidates_0_1_k_minus_1_k_k_plus_1_and_above_the_lane_threshold(cuda, k):
    from segger_amd import _lib
    rings, points, counts = nc.scene_stack(k, _lib.NEAREST_LANE_MAX)
    got, want = check(cuda, points, rings, k)
    assert got["count"].tolist() == counts.tolist() and {0, 1, k - 1, k, k + 1, _lib.NEAREST_LANE_MAX, _lib.NEAREST_LANE_MAX + 1} <= set(counts.tolist())
    c = dict(zip(nc.COUNTER_NAMES, got["counters"].tolist()))
    assert c == {"n_pairs": int(counts.sum()), "n_kept": int(np.minimum(counts, k).sum()), "n_truncated_points": int((counts > k).sum()),
                 "max_count": nc.STACK_COPIES}
    # the same points among many others: the wave route next to lanes that take the lane route
    rng = np.random.default_rng(k)
    more = np.concatenate([points, nc.at(*rng.integers(-64, 192, (300, 2)) / 128.0)])
    check(cuda, more[rng.permutation(len(more))], rings, k)


def test_ties_duplicate_polygons_on_ring_points_and_a_mixed_buffer(cuda):
    rings, names, points, _, _ = pc.cases()
    rings = list(rings) + [rings[0], rings[3], rings[3]]
    buf = np.where(np.arange(len(rings)) % 2 == 0, 0.0, 0.25)
    buf[-3:] = (buf[0], buf[3], buf[3])                              # a duplicate carries its twin's buffer
    for pred in pc.PREDICATES:
        for k in (1, 2, 3):
            got, want = check(cuda, points, rings, k, buf, pred)
    zero = want["dist2"] == 0.0
    assert zero.sum() > 10 and want["inside"][zero].any() and not want["inside"][zero].all()        # s = 0 with either parity
    twin = (want["polygon"][:, :2] == np.array([3, len(rings) - 2])).all(axis=1)                    # a tie: the lower id first
    assert twin.sum() > 5 and np.array_equal(want["dist2"][twin, 0], want["dist2"][twin, 1])


def test_same_bytes_for_any_grid_point_order_and_polygon_order(cuda):
    rings, points = bc.scene_field()
    buf = np.linspace(2.0, 6.0, len(rings))
    base, want = check(cuda, points, rings, 3, buf)
    assert want["counters"][2] > 0 and want["counters"][3] > 3       # some points are truncated
    again = run(cuda, points, rings, 3, buf)
    for ppc in (0.25, 8.0, 500.0):
        other = run(cuda, points, rings, 3, buf, points_per_cell=ppc)
        for name in KEYS:
            assert torch.equal(base[name], other[name]) and torch.equal(base[name], again[name]), (ppc, name)
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(points))
    other = run(cuda, points[perm], rings, 3, buf)
    for name in ("polygon", "dist2", "inside", "count"):
        assert torch.equal(base[name][torch.from_numpy(perm).to(cuda)], other[name]), ("points", name)
    assert torch.equal(base["counters"], other["counters"])
    # no two keys of a point tie in this scene (the oracle, on the CPU), so the polygon ids decide nothing
    assert nc.min_key_gap(points, rings, buf, "intersects") > 0.0
    pperm = rng.permutation(len(rings))
    other = run(cuda, points, [rings[p] for p in pperm], 3, buf[pperm])
    back = torch.from_numpy(np.append(pperm, len(rings))).to(cuda)
    assert torch.equal(back[other["polygon"].long()].int(), base["polygon"])
    for name in ("dist2", "inside", "count", "counters"):
        assert torch.equal(base[name], other[name]), ("polygons", name)


@pytest.mark.parametrize("pred", pc.PREDICATES)
def test_with_k_16_the_kept_pairs_equal_points_in_polygons(cuda, pred):
    from segger_amd import geometry as ge
    rings, points = bc.scene_field()
    t = tensors(cuda, points, rings)
    got = run(cuda, points, rings, 16, 1.5, pred)
    ei = ge.points_in_polygons(*t, buffer=1.5, predicate=pred)
    assert 1 < int(got["counters"][3]) <= 16 and int(got["counters"][2]) == 0
    pairs = torch.from_numpy(nc.kept_pairs({"polygon": got["polygon"].cpu().numpy()}, len(rings))).to(cuda)
    assert torch.equal(pairs.t(), ei) and int(got["counters"][0]) == ei.shape[1] > int(ei[0].unique().numel()) > 1000
    assert torch.equal(got["count"].long(), torch.bincount(ei[0], minlength=len(points)))


def test_prediction_graph_nearest_and_shape_with_max_k(cuda):
    from segger_amd import neighbors
    rings, points = bc.scene_field()
    t = tensors(cuda, points, rings)
    for max_k, max_dist in ((1, 0.0), (3, 1.5), (16, 1.5)):
        want = nc.kept_pairs(nc.nearest(points, rings, max_k, max_dist, "intersects"), len(rings))
        ei = neighbors.prediction_graph_nearest(*t, max_k=max_k, max_dist=max_dist)
        assert ei.dtype == torch.int64 and ei.is_cuda and np.array_equal(ei.cpu().numpy(), want.T)
        assert int(torch.bincount(ei[0]).max()) == min(max_k, int(nc.nearest(points, rings, 1, max_dist)["counters"][3]))
    ratio = 0.6                                                      # grown so far that neighbours overlap
    dists = nc.field_dists(rings, ratio)
    everything = neighbors.prediction_graph_shape(*t, buffer_ratio=ratio)
    assert torch.equal(everything, neighbors.prediction_graph_shape(*t, buffer_ratio=ratio, max_k=None))
    assert int(torch.bincount(everything[0]).max()) > 2
    for max_k in (1, 2, 16):
        want = nc.kept_pairs(nc.nearest(points, rings, max_k, dists, "contains"), len(rings))
        ei = neighbors.prediction_graph_shape(*t, buffer_ratio=ratio, max_k=max_k)
        assert np.array_equal(ei.cpu().numpy(), want.T) and int(torch.bincount(ei[0]).max()) == min(max_k, int(torch.bincount(everything[0]).max()))
    assert torch.equal(neighbors.prediction_graph_shape(*t, buffer_ratio=ratio, max_k=16), everything)


def test_empty_inputs_degenerate_rings_and_k_out_of_range(cuda):
    rings, points = bc.scene_field()
    r = run(cuda, points[:0], rings, 3)
    assert r["polygon"].shape == (0, 3) and r["count"].numel() == 0 and r["counters"].tolist() == [0] * 4
    r = run(cuda, points[:7], [], 2)
    assert r["polygon"].tolist() == [[0, 0]] * 7 and bool(torch.isinf(r["dist2"]).all()) and not bool(r["inside"].any())
    assert r["count"].tolist() == [0] * 7 and r["counters"].tolist() == [0] * 4
    for name in KEYS:
        assert r[name].dtype == DTYPES[name] and r[name].is_cuda
    odd = [np.zeros((0, 2)), points[:1], points[:2], rings[0], np.concatenate([points[:2], points[:1]])]
    got, want = check(cuda, points, odd, 2, 1.0)
    assert set(np.unique(want["polygon"]).tolist()) == {3, 5}        # fewer than 3 vertices match nothing
    t = tensors(cuda, points, rings)
    from segger_amd import nearest, neighbors
    for bad in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError, match="SEGGER_NEAREST_MAX_K = 16"):
            nearest.nearest_boundaries(*t, bad)
    with pytest.raises(ValueError, match="SEGGER_NEAREST_MAX_K = 16"):
        neighbors.prediction_graph_nearest(*t, max_k=17)
    with pytest.raises(ValueError, match="buffer must be finite and >= 0"):
        neighbors.prediction_graph_nearest(*t, max_dist=-1.0)


def test_signed_distance_within_one_ulp(cuda):
    from segger_amd import nearest
    rings, points = bc.scene_field()
    got, want = check(cuda, points, rings, 3, 1.5)
    sd = nearest.signed_distance(got).cpu().numpy()
    ref = nc.signed_distance(want)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(sd)) and np.all(sd[~fin] == np.inf) and fin.sum() > 1000
    assert np.all(np.abs(sd[fin] - ref[fin]) <= np.spacing(np.abs(ref[fin])))       # two faithful square roots: one ulp
    assert np.array_equal(np.sign(sd[fin]), np.sign(ref[fin])) and (sd[fin] < 0).any() and (sd[fin] > 0).any()
