"""segger_amd.repair on the device against the oracle of tests/repair_cases.py: every tensor of resort_rings and
repair_rings EQUAL to the exact sequential oracle on both LDS tiers, at every ring size where the kernel changes its padded
size, its chunk count or its tier; the hand-worked tie rings and the pairs that defeat a float cross product or a float
atan2 key; the CSR shapes; the permutation, identity and validity properties; the three ``on_failure`` modes; and the
chain label_contours -> simplify_rings -> scramble -> repair_rings -> polygon_props / points_in_polygons."""
import numpy as np
import pytest
import torch

import repair_cases as rc
import simplify_cases as sc

pytestmark = pytest.mark.gpu
ROUTES = (None, "large")


def dev():
    return torch.device("cuda:0")


def upload(rings):
    return tuple(torch.from_numpy(t).to(dev()) for t in sc.csr(rings))


def run(rings, select=None, route=None):
    from segger_amd import resort_rings
    off, xy = upload(rings)
    if select is not None:
        select = torch.as_tensor(np.asarray(select, bool), device=dev())
    return {k: v.cpu().numpy() for k, v in resort_rings(off, xy, select, _route=route).items()}


def assert_equal(got, want, what):
    assert np.array_equal(got["vertex_index"], want["vertex_index"]), (what, got["vertex_index"][:16], want["vertex_index"][:16])
    assert got["xy"].tobytes() == want["xy"].tobytes(), (what, "xy")  # the input's bytes


@pytest.fixture(scope="module")
def sized():
    """the rings of rc.SIZES with their oracle result -- computed once, never changed"""
    rings = rc.sized_rings()
    assert [len(r) for r in rings] == list(rc.SIZES)
    return rings, rc.expected_resort(rings)


@pytest.fixture(scope="module")
def special():
    rings = list(rc.SPECIAL.values()) + rc.naive_failure_rings("cross") + rc.naive_failure_rings("atan2")
    want = rc.expected_resort(rings)
    off = sc.csr(rings)[0]
    for p, name in enumerate(rc.SPECIAL):                            # the oracle itself is pinned to the hand-worked orders
        assert (want["vertex_index"][off[p]:off[p + 1]] - off[p]).tolist() == rc.SPECIAL_ORDER[name]
    return rings, want


@pytest.mark.parametrize("route", ROUTES)
def test_every_size_equals_the_oracle(sized, route):
    rings, want = sized
    got = run(rings, route=route)
    assert_equal(got, want, route)
    off = sc.csr(rings)[0]
    for p in range(len(rings)):                                      # per ring, a permutation of its range
        assert np.array_equal(np.sort(got["vertex_index"][off[p]:off[p + 1]]), np.arange(off[p], off[p + 1])), p


def test_single_rings_at_the_tier_boundary_and_the_cap(sized):
    rings, _ = sized
    for n in (256, 257, 4096):
        ring = rings[rc.SIZES.index(n)]
        assert_equal(run([ring]), rc.expected_resort([ring]), n)
    closed = np.vstack([rings[-1], rings[-1][:1]])                   # 4097 entries of 4096 vertices
    assert_equal(run([closed]), rc.expected_resort([closed]), "4096 closed")


def test_a_ring_above_the_cap_is_refused():
    from segger_amd import repair_rings, resort_rings
    off, xy = upload([rc.SPECIAL["bow_tie"], sc.star_ring(rc.MAX_VERTS + 1, 5)])
    for fn in (resort_rings, repair_rings):
        with pytest.raises(ValueError, match="polygon 1 has 4097 vertices"):
            fn(off, xy)


@pytest.mark.parametrize("route", ROUTES)
def test_ties_and_adversarial_pairs_equal_the_oracle(special, route):
    rings, want = special
    assert_equal(run(rings, route=route), want, route)


def test_csr_shapes(special):
    from segger_amd import resort_rings
    few = [np.zeros((0, 2)), np.array([(7.0, 7.0)]), np.array([(7.0, 7.0), (8.0, 9.0)]), np.array([(7.0, 7.0), (8.0, 9.0), (7.0, 7.0)])]
    rings = [rc.SPECIAL["bow_tie"]] + few + [rc.SPECIAL["negative_x_ray"]]
    want = rc.expected_resort(rings)
    assert want["vertex_index"][4:10].tolist() == list(range(4, 10))  # fewer than 3 open vertices: passed through
    assert_equal(run(rings), want, "few")
    # P = 0
    out = resort_rings(torch.zeros(1, dtype=torch.int64, device=dev()), torch.empty(0, 2, dtype=torch.float64, device=dev()))
    assert out["xy"].shape == (0, 2) and out["vertex_index"].shape == (0,) and out["vertex_index"].dtype == torch.int64
    # select all false: nothing launched, the input itself
    rings, want_all = special
    off, xy = upload(rings)
    out = resort_rings(off, xy, torch.zeros(len(rings), dtype=torch.bool, device=dev()))
    assert out["xy"].data_ptr() == xy.data_ptr() and out["vertex_index"].tolist() == list(range(xy.shape[0]))
    # select mixed (bool and uint8): unselected rings bit-identical, vertex_index the identity there
    select = np.arange(len(rings)) % 3 != 1
    want = rc.expected_resort(rings, select)
    assert_equal(run(rings, select), want, "mixed")
    got = resort_rings(off, xy, torch.from_numpy(select.astype(np.uint8)).to(dev()))
    assert_equal({k: v.cpu().numpy() for k, v in got.items()}, want, "mixed uint8")
    o = sc.csr(rings)[0]
    for p in np.flatnonzero(~select):
        assert got["vertex_index"][o[p]:o[p + 1]].tolist() == list(range(o[p], o[p + 1]))
        assert torch.equal(got["xy"][o[p]:o[p + 1]], xy[o[p]:o[p + 1]])
    assert not np.array_equal(want["vertex_index"], want_all["vertex_index"])


def test_properties(sized):
    from segger_amd import polygon_props, resort_rings, rings_simple
    rings, _ = sized
    off, xy = upload(rings)
    a, b = resort_rings(off, xy), resort_rings(off, xy)
    assert all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in a)     # the same bytes from run to run
    assert torch.equal(a["xy"], xy[a["vertex_index"]])
    # shuffled convex rings come back valid and counter-clockwise
    convex = [rc.shuffled(rc.convex_ring(n, 20 + n), n) for n in (3, 7, 64, 100, 300, 1000)]
    off, xy = upload(convex)
    assert not bool(rings_simple(off, xy)[0][2:].any())
    out = resort_rings(off, xy)
    assert bool(rings_simple(off, out["xy"])[0].all())
    area = polygon_props(off, out["xy"])["area"]
    assert bool((area > 0).all())
    assert area.cpu().numpy().tolist() == pytest.approx([sc.area2(rc.convex_ring(n, 20 + n)) / 2.0 for n in (3, 7, 64, 100, 300, 1000)],
                                                        rel=1e-12)


def test_repair_rings_modes():
    from segger_amd import repair_rings
    square = np.array([(0, 0), (4, 0), (4, 4), (0, 4)], np.float64)
    rings = [square, rc.SPECIAL["bow_tie"], rc.SPECIAL["collinear"], rc.shuffled(rc.convex_ring(50, 9), 9), np.array([(7.0, 7.0)]),
             rc.SPECIAL["bow_tie_closed"] + 10.0]
    want = rc.expected_repair(rings)
    assert want["status"].tolist() == [0, 1, 2, 1, 2, 1]
    off, xy = upload(rings)
    out = repair_rings(off, xy, on_failure="keep")
    assert out["status"].dtype == torch.int8 and out["reason_after"].dtype == torch.int32 and "kept" not in out
    for k, v in want.items():
        assert np.array_equal(out[k].cpu().numpy(), v) and out[k].cpu().numpy().tobytes() == v.tobytes(), k
    with pytest.raises(ValueError, match="polygon 2 is still invalid after the re-sort .edges 0 and"):
        repair_rings(off, xy)
    with pytest.raises(ValueError, match="polygon 2 is still invalid after the re-sort .fewer than 3"):
        repair_rings(*upload(rings[:2][::-1] + rings[4:5]))
    drop = repair_rings(off, xy, on_failure="drop")
    assert drop["kept"].tolist() == [0, 1, 3, 5] and drop["kept"].dtype == torch.int64
    keep_rows = np.concatenate([np.arange(want["ring_offsets"][p], want["ring_offsets"][p + 1]) for p in (0, 1, 3, 5)])
    assert drop["ring_offsets"].tolist() == [0, 4, 8, 58, 63]
    assert np.array_equal(drop["vertex_index"].cpu().numpy(), want["vertex_index"][keep_rows])
    assert drop["xy"].cpu().numpy().tobytes() == want["xy"][keep_rows].tobytes()
    assert np.array_equal(drop["status"].cpu().numpy(), want["status"])                     # status and reasons stay [P]
    # nothing invalid: no sort, the input tensor itself
    off, xy = upload([square, square + 5.0])
    out = repair_rings(off, xy)
    assert out["xy"] is xy and out["status"].tolist() == [0, 0] and out["counters"].tolist() == [0, 0, 0]
    assert out["vertex_index"].tolist() == list(range(8)) and repair_rings(off, xy, on_failure="drop")["kept"].tolist() == [0, 1]
    empty = repair_rings(torch.zeros(1, dtype=torch.int64, device=dev()), torch.empty(0, 2, dtype=torch.float64, device=dev()))
    assert empty["status"].shape == (0,) and empty["reason_after"].shape == (0, 3) and empty["counters"].tolist() == [0, 0, 0]


def test_chain_from_a_label_image():
    import contour_cases as cc
    from segger_amd import label_contours, points_in_polygons, polygon_props, repair_rings, rings_simple, simplify_rings
    img = torch.from_numpy(cc.voronoi_small()).to(dev())
    c = label_contours(img)
    s = simplify_rings(c["ring_offsets"], c["xy"], 0.5)
    o = s["ring_offsets"].tolist()
    rings = [s["xy"][a:b].cpu().numpy() for a, b in zip(o[:-1], o[1:])]
    scrambled = [rc.shuffled(r, p) if p % 3 == 0 else r for p, r in enumerate(rings)]
    want = rc.expected_repair(scrambled)
    assert (want["status"] == 1).sum() >= 3 and (want["status"] == 0).sum() >= 3             # both answers occur
    off, xy = upload(scrambled)
    out = repair_rings(off, xy, on_failure="keep")
    for k, v in want.items():
        assert np.array_equal(out[k].cpu().numpy(), v), k
    assert out["xy"].cpu().numpy().tobytes() == want["xy"].tobytes()
    good = repair_rings(off, xy, on_failure="drop")
    assert bool(rings_simple(good["ring_offsets"], good["xy"])[0].all())
    repaired = torch.from_numpy(want["status"] == 1).to(dev())
    area = polygon_props(out["ring_offsets"], out["xy"])["area"]
    before = polygon_props(s["ring_offsets"], s["xy"])["area"]
    assert bool((area[repaired] > 0).all())                          # counter-clockwise
    convex = torch.isclose(area[repaired], before[repaired].abs(), rtol=1e-12)
    assert bool(convex.any())                                        # a cell that is star-shaped around its centre is itself again
    pts = torch.rand(2000, 2, dtype=torch.float64, device=dev()) * img.shape[0]
    pairs = points_in_polygons(pts, good["ring_offsets"], good["xy"])
    assert pairs.shape[0] == 2 and pairs.shape[1] > 0 and int(pairs[1].max()) < good["kept"].numel()
