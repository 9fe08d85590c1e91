"""segger_amd.boundaries.cell_outlines on the device against the oracle of tests/outline_cases.py.

Every coordinate of the cases is a multiple of 1/16 and a cell spans fewer than 2^11 such steps, so the device's float64
orient2d and incircle are exact, scipy's triangulation is unique (tests/test_outlines_oracle.py asserts both), and the
device's rings must equal the oracle's vertex for vertex and bit for bit -- start vertex and orientation included.  One
scene of about 40 cells is shared: 3 points kept and 3 points pruned away, 4 points, fewer than 3 distinct, collinear,
duplicates, a crescent, two blobs whose neck the peel severs (touching at a vertex, and apart), 63 / 64 / 65 and
255 / 256 / 257 points (the route threshold), random clouds; absent and negative ids, a mask, shuffled rows.
"""
import os

import numpy as np
import pytest
import torch

import boundaries_cases as bc
import morphology_cases as mc
import outline_cases as oc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outlines_small.npz")
KEYS = ("ring_offsets", "xy", "cell_ids", "n_transcripts")


def run(cuda, xy, ids, n_cells=None, **kw):
    from segger_amd import boundaries as bd
    out = bd.cell_outlines(torch.from_numpy(np.ascontiguousarray(xy)).to(cuda), torch.from_numpy(np.ascontiguousarray(ids)).to(cuda),
                           n_cells, **kw)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def assert_same(got, want, label=""):
    offsets, xy, cell_ids, n_tx, n_dropped = want
    assert np.array_equal(got["cell_ids"], cell_ids), label
    assert np.array_equal(got["n_transcripts"], n_tx), label
    assert np.array_equal(got["ring_offsets"], offsets), label
    assert got["xy"].shape == xy.shape and np.array_equal(got["xy"].view(np.uint64), xy.view(np.uint64)), label
    assert got["n_dropped"] == n_dropped, label
    assert got["ring_offsets"].dtype == np.int64 and got["xy"].dtype == np.float64
    assert got["cell_ids"].dtype == np.int32 and got["n_transcripts"].dtype == np.int64


def scene_run(cuda, **kw):
    xy, ids, keep = oc.scene()
    return run(cuda, xy, ids, oc.N_CELLS, keep=torch.from_numpy(keep).to(cuda), **kw)


@pytest.fixture(scope="module")
def scene_result(cuda):
    return scene_run(cuda)


@pytest.mark.parametrize("connectivity", oc.CONNECTIVITIES)
def test_scene_rings_equal_the_oracle_bit_for_bit(cuda, connectivity):
    got = scene_run(cuda, connectivity=connectivity)
    assert_same(got, oc.expected(oc.scene_cells(), connectivity), connectivity)
    assert not {2, 5, 6, 7} & set(got["cell_ids"].tolist()) and got["n_dropped"] >= 4      # thin, 2 distinct, collinear, 1 point


@pytest.mark.parametrize("connectivity", oc.CONNECTIVITIES)
def test_cells_at_the_point_limit_equal_the_oracle_bit_for_bit(cuda, connectivity):
    cells = oc.big_cells()
    xy = np.concatenate(list(cells.values()))
    ids = np.concatenate([np.full(len(p), c, dtype=np.int32) for c, p in cells.items()])
    assert_same(run(cuda, xy, ids, connectivity=connectivity), oc.expected(cells, connectivity), connectivity)


def test_refusal_above_the_point_limit_and_rows_staged_in_rounds(cuda):
    from segger_amd import _lib
    big = oc.too_big_cell()
    with pytest.raises(_lib.SeggerAmdError, match=rf"1 cells have more than {oc.MAX_POINTS} distinct points.*cell 3 among them"):
        run(cuda, np.concatenate([big, oc.cells()[1]]), np.concatenate([np.full(len(big), 3), np.zeros(3)]).astype(np.int32))
    # more rows than the staging area of 2 MAX_POINTS holds, few distinct points: staged in rounds, not refused; the
    # duplicated points count 0 in d_max
    pts = oc.cells()[13]
    many = np.random.default_rng(2).permutation(np.concatenate([pts] + [pts[:40]] * 110))      # 4463 rows, 63 distinct
    got = run(cuda, many, np.zeros(len(many), dtype=np.int32))
    assert oc.outline(many, 2.0) is not None and len(many) > 2 * oc.MAX_POINTS
    assert_same(got, oc.expected({0: many}, 2.0))


def test_same_bytes_for_three_row_orders_and_mask_and_negative_ids(cuda, scene_result):
    xy, ids, keep = oc.scene()
    for perm in (np.random.default_rng(11).permutation(len(ids)), np.argsort(ids, kind="stable"), np.arange(len(ids))[::-1]):
        got = run(cuda, xy[perm], ids[perm], oc.N_CELLS, keep=torch.from_numpy(keep[perm].copy()).to(cuda))
        for k in KEYS:
            assert np.array_equal(got[k].view(np.uint8), scene_result[k].view(np.uint8)), k
        assert got["n_dropped"] == scene_result["n_dropped"]
    # the mask applied by hand, int64 ids, float32 coordinates (exact for this grid), the id domain found on the device
    sel = keep & (ids >= 0)
    got = run(cuda, xy[sel].astype(np.float32), ids[sel].astype(np.int64))
    for k in KEYS:
        assert np.array_equal(got[k], scene_result[k]), k
    unmasked = run(cuda, xy, ids, oc.N_CELLS)                                # the masked rows of cell 14 now count
    q = unmasked["cell_ids"].tolist().index(14)
    assert unmasked["n_transcripts"][q] == 64 + 100 and scene_result["n_transcripts"][scene_result["cell_ids"].tolist().index(14)] == 64


@pytest.mark.parametrize("smoothing", [1, 3])
def test_smoothing_has_the_bits_of_numpys_iteration(cuda, scene_result, smoothing):
    got = scene_run(cuda, smoothing=smoothing)
    assert_same(got, oc.expected(oc.scene_cells(), 2.0, smoothing), smoothing)
    assert np.array_equal(np.diff(got["ring_offsets"]), np.diff(scene_result["ring_offsets"]) << smoothing)


def test_golden_scene_matches_the_recorded_run_of_the_reference(cuda):
    import test_outlines_oracle as too
    g = np.load(GOLDEN)
    ids = g["cell_ids"].tolist()
    xy = np.concatenate([g[f"points_{c}"] for c in ids])
    cell = np.concatenate([np.full(len(g[f"points_{c}"]), c, dtype=np.int32) for c in ids])
    for k, conn in enumerate(g["connectivities"].tolist()):
        got = run(cuda, xy, cell, connectivity=conn)
        rings = {int(c): got["xy"][got["ring_offsets"][q]:got["ring_offsets"][q + 1]] for q, c in enumerate(got["cell_ids"])}
        for c in ids:
            want = too.largest_cycle(g[f"points_{c}"], g[f"rim_{c}_{k}"])
            if want is None:
                assert c not in rings, (c, conn)
                continue
            ring = rings[c]
            assert {tuple(sorted((tuple(a), tuple(b)))) for a, b in zip(ring, np.roll(ring, -1, axis=0))} == want, (c, conn)


def test_polygon_props_and_points_in_polygons_take_the_rings_as_they_are(cuda, scene_result):
    from segger_amd import geometry as ge
    from segger_amd import morphology as mo
    off, ring_xy = torch.from_numpy(scene_result["ring_offsets"]).to(cuda), torch.from_numpy(scene_result["xy"]).to(cuda)
    area = mo.polygon_props(off, ring_xy)["area"].cpu().numpy()
    cells = oc.scene_cells()
    kept = scene_result["cell_ids"].tolist()
    for q, c in enumerate(kept):
        assert mc.rel_dev(float(area[q]), oc.outline_area(cells[c], 2.0)) <= mc.tolerance("area"), c
    # the centroid of a triangle of the oracle's kept component lies strictly inside its cell's ring
    probes, owner = [], []
    for q, c in enumerate(kept):
        st = oc.State(cells[c])
        alive, _ = oc.prune_sequential(st, 2.0)
        _, tris = max(oc.components(st, alive), key=lambda x: x[0])
        probes.append(st.points[st.simplices[tris[0]]].mean(0))
        owner.append(q)
    pairs = ge.points_in_polygons(torch.from_numpy(np.array(probes)).to(cuda), off, ring_xy).cpu().numpy()
    found = set(zip(pairs[0].tolist(), pairs[1].tolist()))
    assert all((i, q) in found for i, q in enumerate(owner))


def test_segmentation_wrappers_agree_with_cell_outlines(cuda):
    from segger_amd import boundaries as bd
    from segger_amd import postprocess as pp
    from test_gpu_boundaries import fake_result
    from test_postprocess import fake_predictions
    res, xy, row, enc, counted = fake_result(cuda)
    xy = xy / 4.0                                                            # still a grid
    got = bd.segmentation_outlines(res, torch.from_numpy(xy).to(cuda), 40, smoothing=1, connectivity=1.0)
    want = run(cuda, xy[row[counted]], enc[counted].astype(np.int32), 40, smoothing=1, connectivity=1.0)
    for k in KEYS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert got["n_dropped"] == want["n_dropped"] and len(want["cell_ids"]) > 20
    acc = pp.SegmentationAccumulator(4000, cuda)
    for b in fake_predictions(0):
        acc.update(*b)
    sxy = torch.from_numpy(np.random.default_rng(8).integers(-2000, 2000, (4000, 2)).astype(np.float64) / 8).to(cuda)
    a, b = acc.outlines(sxy, connectivity=1.0), bd.segmentation_outlines(acc.segmentation(), sxy, connectivity=1.0)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert a["cell_ids"].numel() > 0


def test_errors_raise_and_name_what_was_found(cuda):
    from segger_amd import _lib
    xy, ids, keep = oc.scene()
    bad = ids.copy()
    first = int(np.flatnonzero(ids == 13)[0])
    bad[first] = oc.N_CELLS + 3
    with pytest.raises(_lib.SeggerAmdError, match=rf"1 kept rows have a cell id outside \[0, {oc.N_CELLS}\)"):
        run(cuda, xy, bad, oc.N_CELLS)
    broken = xy.copy()
    broken[first, 1] = np.nan
    with pytest.raises(_lib.SeggerAmdError, match="0 kept rows have a cell id.*and 1 a NaN or infinite coordinate"):
        run(cuda, broken, ids, oc.N_CELLS)
    got = run(cuda, np.zeros((0, 2)), np.zeros(0, dtype=np.int32))
    assert got["ring_offsets"].tolist() == [0] and got["xy"].shape == (0, 2) and got["n_dropped"] == 0


def ring_checks(ring, pts):
    """simple, counter-clockwise, made of input points, no larger than the hull"""
    assert len({tuple(v) for v in ring}) == len(ring) >= 3
    assert {tuple(v) for v in ring} <= {tuple(v) for v in pts}
    a, b = ring, np.roll(ring, -1, axis=0)
    area = 0.5 * float((a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]).sum())
    h = bc.hull_f64(pts)
    hull_area = 0.5 * float((h[:, 0] * np.roll(h[:, 1], -1) - np.roll(h[:, 0], -1) * h[:, 1]).sum())
    assert 0 < area <= hull_area * (1 + 1e-12)
    d = b - a                                                                # no two non-adjacent edges cross

    def side(i, p):                                                          # of edge i, for every point of p
        return d[i, 0] * (p[:, 1] - a[i, 1]) - d[i, 1] * (p[:, 0] - a[i, 0])

    for i in range(len(ring)):
        s1 = side(i, a) * side(i, b)                                         # edge j straddles the line of edge i
        s2 = (d[:, 0] * (a[i, 1] - a[:, 1]) - d[:, 1] * (a[i, 0] - a[:, 0])) * (d[:, 0] * (b[i, 1] - a[:, 1]) - d[:, 1] * (b[i, 0] - a[:, 0]))
        assert not ((s1 < 0) & (s2 < 0)).any(), i
    return area


def test_real_float32_coordinates_structurally(cuda):
    """qhull is tolerance-based off the grid and equality with it is not claimed: the ring is simple, counter-clockwise,
    made of input points, within the hull, and the call returns"""
    cells = {c: p.astype(np.float32).astype(np.float64) for c, p in bc.real_cells().items()}
    xy = np.concatenate(list(cells.values()))
    ids = np.concatenate([np.full(len(p), c, dtype=np.int32) for c, p in cells.items()])
    got = run(cuda, xy.astype(np.float32), ids)
    assert len(got["cell_ids"]) + got["n_dropped"] == len(cells) and len(got["cell_ids"]) >= 4
    for q, c in enumerate(got["cell_ids"].tolist()):
        ring_checks(got["xy"][got["ring_offsets"][q]:got["ring_offsets"][q + 1]], cells[c])


def test_co_circular_grid_points_are_triangulated_consistently(cuda):
    """a full 9 x 9 lattice: every unit square is co-circular; nothing is peeled at connectivity 2, so the outline is the
    lattice's border with all of its 32 vertices, area 64"""
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(9.0)), -1).reshape(-1, 2)
    got = run(cuda, np.random.default_rng(0).permutation(g), np.zeros(81, dtype=np.int32))
    ring = got["xy"]
    assert got["ring_offsets"].tolist() == [0, 32] and ring_checks(ring, g) == 64.0
    assert tuple(ring[0]) == (0.0, 0.0) and tuple(ring[1]) == (1.0, 0.0)
