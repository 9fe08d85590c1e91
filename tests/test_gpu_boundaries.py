"""segger_amd.boundaries on the device against the exact oracle of tests/boundaries_cases.py.

Every coordinate of the scene is an integer below 2^20, so the device's float64 orientation test is exact and its rings
must equal the oracle's vertex for vertex and bit for bit -- start vertex and orientation included -- as must the
smoothed rings equal numpy's iteration of the reference's formula on the same hull.  One scene is shared by the tests: the
tiny cells (0, 1, 2 points, collinear, duplicates, exactly 3, a 5 x 5 grid, duplicated extremes), the route boundaries
(63, 64, 65, 4095, 4096, 4097 points), a chunked cell of 9000 points with a hull of 200, and a hull of 100 on the LDS
route; the rows are interleaved at random, with unassigned rows and ids that own no row.
"""
import os

import numpy as np
import pytest
import torch

import boundaries_cases as bc
import morphology_cases as mc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundaries_small.npz")
KEYS = ("ring_offsets", "xy", "cell_ids", "n_transcripts")


def run(cuda, xy, ids, n_cells=None, **kw):
    from segger_amd import boundaries as bd
    out = bd.cell_boundaries(torch.from_numpy(np.ascontiguousarray(xy)).to(cuda), torch.from_numpy(np.ascontiguousarray(ids)).to(cuda),
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


@pytest.fixture(scope="module")
def scene_result(cuda):
    xy, ids = bc.scene()
    return run(cuda, xy, ids, bc.N_CELLS)


def test_scene_rings_equal_the_exact_oracle_bit_for_bit(scene_result):
    want = bc.expected(bc.scene_cells(), bc.scene_hulls())
    assert_same(scene_result, want)
    sizes = dict(zip(scene_result["cell_ids"].tolist(), np.diff(scene_result["ring_offsets"]).tolist()))
    assert sizes[6] == 4 and sizes[7] == 4 and sizes[5] == 3 and sizes[40] == 200 and sizes[41] == 100
    assert scene_result["n_dropped"] == 5 and not {0, 1, 2, 3, 4, 9} & set(sizes)
    routes = dict(zip(scene_result["cell_ids"].tolist(), scene_result["n_transcripts"].tolist()))
    assert [routes[20 + 2 * k] for k in range(6)] == list(bc.ROUTE_SIZES) and routes[40] == 9000


def test_bookkeeping_does_not_depend_on_the_order_of_the_rows(cuda, scene_result):
    xy, ids = bc.scene()
    for perm in (np.random.default_rng(11).permutation(len(ids)), np.argsort(ids, kind="stable"), np.arange(len(ids))[::-1]):
        got = run(cuda, xy[perm], ids[perm], bc.N_CELLS)
        for k in KEYS:
            assert np.array_equal(got[k].view(np.uint8), scene_result[k].view(np.uint8)), k
        assert got["n_dropped"] == scene_result["n_dropped"]
    # the id domain found on the device, int64 ids, float32 coordinates (exact for these integers), a mask instead of -1
    keep = ids >= 0
    got = run(cuda, xy.astype(np.float32), np.where(keep, ids, 3).astype(np.int64), keep=torch.from_numpy(keep).to(cuda))
    for k in KEYS:
        assert np.array_equal(got[k], scene_result[k]), k


@pytest.mark.parametrize("smoothing", [1, 3])
def test_smoothing_has_the_bits_of_numpys_iteration(cuda, scene_result, smoothing):
    xy, ids = bc.scene()
    got = run(cuda, xy, ids, bc.N_CELLS, smoothing=smoothing)
    assert_same(got, bc.expected(bc.scene_cells(), bc.scene_hulls(), smoothing), smoothing)
    assert np.array_equal(np.diff(got["ring_offsets"]), np.diff(scene_result["ring_offsets"]) << smoothing)


def test_real_coordinates_in_general_position(cuda):
    cells = bc.real_cells()
    xy = np.concatenate(list(cells.values()))
    ids = np.concatenate([np.full(len(p), c, dtype=np.int32) for c, p in cells.items()])
    perm = np.random.default_rng(1).permutation(len(ids))
    got = run(cuda, xy[perm], ids[perm])
    assert_same(got, bc.expected(cells, {c: bc.hull(p) for c, p in cells.items()}))
    again = run(cuda, xy, ids, smoothing=2)
    assert_same(again, bc.expected(cells, {c: bc.hull(p) for c, p in cells.items()}, 2))


def test_polygon_props_takes_the_rings_as_they_are(cuda, scene_result):
    from segger_amd import morphology as mo
    props = mo.polygon_props(torch.from_numpy(scene_result["ring_offsets"]).to(cuda), torch.from_numpy(scene_result["xy"]).to(cuda))
    area, n_hull = props["area"].cpu().numpy(), props["n_hull"].cpu().numpy()
    hulls = bc.scene_hulls()
    for q, c in enumerate(scene_result["cell_ids"].tolist()):
        assert n_hull[q] == len(hulls[c]), c
        assert mc.rel_dev(float(area[q]), bc.area2_exact(hulls[c]) / 2) <= mc.tolerance("area"), c


def test_points_in_polygons_finds_every_interior_transcript_in_its_own_ring(cuda):
    from segger_amd import boundaries as bd
    from segger_amd import geometry as ge
    cells = {c: p for c, p in bc.scene_cells().items() if len(p) <= 100}            # tiny cells, 63 .. 65, the circle of 100
    xy = np.concatenate(list(cells.values()))
    ids = np.concatenate([np.full(len(p), c, dtype=np.int32) for c, p in cells.items()])
    pts, cell = torch.from_numpy(xy).to(cuda), torch.from_numpy(ids).to(cuda)
    out = bd.cell_boundaries(pts, cell, bc.N_CELLS)
    pairs = ge.points_in_polygons(pts, out["ring_offsets"], out["xy"]).cpu().numpy()
    found = set(zip(pairs[0].tolist(), pairs[1].tolist()))
    hulls, kept = bc.scene_hulls(), out["cell_ids"].cpu().numpy().tolist()
    checked = 0
    for q, c in enumerate(kept):
        rows = np.flatnonzero(ids == c)
        inner = rows[~bc.on_boundary(xy[rows], hulls[c])]
        assert all((int(i), q) in found for i in inner), c
        assert not any((int(i), q) in found for i in rows if i not in set(inner.tolist())), c      # "contains" is the open set
        checked += len(inner)
    assert checked > 150


def fake_result(cuda, n_slide=3000, seed=4):
    """a segmentation result with every threshold case: above, equal (kept), below, NaN similarity, NaN threshold"""
    rng = np.random.default_rng(seed)
    row = np.sort(rng.choice(n_slide, 2400, replace=False))
    enc = rng.integers(-1, 40, len(row))
    thr = rng.choice([0.25, 0.5, np.nan], len(row), p=[0.45, 0.45, 0.1])
    sim = rng.choice([0.125, 0.25, 0.5, 0.75, np.nan], len(row)).astype(np.float32)
    xy = rng.integers(-500, 500, (n_slide, 2)).astype(np.float64)
    res = {"row_index": torch.from_numpy(row).to(cuda), "cell_encoding": torch.from_numpy(enc).to(cuda),
           "similarity": torch.from_numpy(sim).to(cuda), "similarity_threshold": torch.from_numpy(thr).to(cuda)}
    with np.errstate(invalid="ignore"):
        counted = (enc >= 0) & (sim.astype(np.float64) >= thr)
    assert (sim[counted] == thr[counted]).sum() > 100 and np.isnan(sim).sum() > 100 and np.isnan(thr).sum() > 100
    return res, xy, row, enc, counted


def test_segmentation_wrapper_applies_the_threshold_rule(cuda):
    from segger_amd import boundaries as bd
    res, xy, row, enc, counted = fake_result(cuda)
    got = bd.segmentation_boundaries(res, torch.from_numpy(xy).to(cuda), 40, smoothing=1)
    want = run(cuda, xy[row[counted]], enc[counted].astype(np.int32), 40, smoothing=1)
    for k in KEYS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert got["n_dropped"] == want["n_dropped"]
    cells = {int(c): xy[row[counted & (enc == c)]] for c in set(enc[counted].tolist())}
    assert_same({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()},
                bc.expected(cells, {c: bc.hull(p) for c, p in cells.items()}, 1))


def test_accumulator_boundaries_sit_beside_expression(cuda):
    from segger_amd import boundaries as bd
    from segger_amd import postprocess as pp
    from test_postprocess import fake_predictions
    acc = pp.SegmentationAccumulator(4000, cuda)
    for b in fake_predictions(0):
        acc.update(*b)
    xy = torch.from_numpy(np.random.default_rng(8).integers(-2000, 2000, (4000, 2)).astype(np.float64)).to(cuda)
    got = acc.boundaries(xy)
    seg = acc.segmentation()
    want = bd.segmentation_boundaries(seg, xy)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    expr = acc.expression()
    kept = (seg["cell_encoding"] >= 0) & (seg["similarity"].double() >= seg["similarity_threshold"])
    direct = bd.cell_boundaries(xy[seg["row_index"][kept]], seg["cell_encoding"][kept])
    for k in KEYS:
        assert torch.equal(got[k], direct[k]), k
    assert int(got["n_transcripts"].sum()) <= expr["n_kept"] and got["cell_ids"].numel() + got["n_dropped"] == expr["cell_ids"].numel()
    pos = torch.searchsorted(expr["cell_ids"], got["cell_ids"])
    assert torch.equal(expr["cell_count"][pos], got["n_transcripts"])


def test_errors_raise_and_name_what_was_found(cuda):
    from segger_amd import _lib
    xy, ids = bc.scene()
    bad = ids.copy()
    first = int(np.flatnonzero(ids == 6)[0])
    bad[first] = bc.N_CELLS + 3
    with pytest.raises(_lib.SeggerAmdError, match=rf"1 kept rows have a cell id outside \[0, {bc.N_CELLS}\)"):
        run(cuda, xy, bad, bc.N_CELLS)
    got = run(cuda, xy, bad, bc.N_CELLS, keep=torch.from_numpy(bad < bc.N_CELLS).to(cuda))       # masked out: not an error
    assert np.array_equal(got["cell_ids"], bc.expected(bc.scene_cells(), bc.scene_hulls())[2])
    for value in (np.nan, np.inf, -np.inf):
        broken = xy.copy()
        broken[first, 1] = value
        with pytest.raises(_lib.SeggerAmdError, match="0 kept rows have a cell id.*and 1 a NaN or infinite coordinate"):
            run(cuda, broken, ids, bc.N_CELLS)
    par = bc.parabola()
    with pytest.raises(_lib.SeggerAmdError, match=r"1 cells of more than 4096 transcripts.*cell 2 among them"):
        run(cuda, np.concatenate([par, bc.tiny_cells()[5]]), np.concatenate([np.full(len(par), 2), np.full(3, 0)]).astype(np.int32))
    got = run(cuda, par[:bc.MAX_VERTS], np.zeros(bc.MAX_VERTS, dtype=np.int32))                   # a full buffer of hull: one round
    assert np.array_equal(got["ring_offsets"], [0, bc.MAX_VERTS]) and np.array_equal(got["xy"], bc.hull(par[:bc.MAX_VERTS]))


def test_no_rows_and_no_polygons(cuda):
    got = run(cuda, np.zeros((0, 2)), np.zeros(0, dtype=np.int32))
    assert got["ring_offsets"].tolist() == [0] and got["xy"].shape == (0, 2) and got["cell_ids"].shape == (0,) and got["n_dropped"] == 0
    got = run(cuda, np.zeros((4, 2)), np.array([-1, -1, 2, 2], dtype=np.int32))
    assert got["ring_offsets"].tolist() == [0] and got["xy"].shape == (0, 2) and got["n_dropped"] == 1


def test_golden_scipy_hulls_are_reproduced(cuda):
    g = np.load(GOLDEN)
    got = run(cuda, g["xy"], g["cell"], int(g["n_cells"]))
    assert np.array_equal(got["cell_ids"], g["scipy_cell_ids"])
    for q, c in enumerate(got["cell_ids"]):
        ring = got["xy"][got["ring_offsets"][q]:got["ring_offsets"][q + 1]]
        verts = g["scipy_hull_vertices"][g["scipy_hull_offsets"][q]:g["scipy_hull_offsets"][q + 1]]
        assert {tuple(v) for v in ring} == {tuple(g["xy"][i]) for i in verts}, c
        area = 0.5 * abs(float((ring[:, 0] * np.roll(ring[:, 1], -1) - np.roll(ring[:, 0], -1) * ring[:, 1]).sum()))
        assert abs(area - g["scipy_hull_area"][q]) <= mc.scipy_area_tolerance(ring), c
