"""cell_outlines(large_cells="global") on the device: the route through global memory for cells above the LDS budget
(segger_cell_outlines_large, csrc/outlines_large.hip) against tests/outline_cases.py and, where co-circular points make the
triangulation a matter of choice, the canonical oracle of tests/outline_large_cases.py.  Everything is bit for bit on
ring_offsets, xy, cell_ids, n_transcripts and n_dropped: a ring has the same bytes whichever route produced it.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import outline_cases as oc
import outline_large_cases as lc
from test_gpu_outlines import KEYS, assert_same, run

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outlines_large.npz")


def same_bytes(a, b, label=""):
    for k in KEYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (k, label)
    assert a["n_dropped"] == b["n_dropped"], label


def scene_run(cuda, **kw):
    xy, ids, keep = oc.scene()
    return run(cuda, xy, ids, oc.N_CELLS, keep=torch.from_numpy(keep).to(cuda), **kw)


def entry_point(cuda, xy, ids, n_cells, large_rows, keep=None):
    """segger_cell_outlines_large through _lib -> (counters by name, ring_offsets, xy, cell_ids)"""
    from segger_amd import _lib
    from segger_amd import boundaries as bd
    n = len(ids)
    txy, tid = torch.from_numpy(np.ascontiguousarray(xy)).to(cuda), torch.from_numpy(np.ascontiguousarray(ids)).to(cuda)
    mask = None if keep is None else torch.from_numpy(keep.astype(np.uint8)).to(cuda)
    _, offs, out, cell_ids, n_tx, counters = bd._outputs(cuda, n, n_cells, 0, _lib.OUTLINE_LARGE_COUNTERS)
    ws, ws_bytes = _lib.workspace("segger_cell_outlines_large_workspace_bytes", cuda, n, n_cells, large_rows)
    _lib.call("segger_cell_outlines_large", cuda, txy.data_ptr(), tid.data_ptr(), _lib.ptr(mask), n, n_cells, 2.0, 0, offs.data_ptr(),
              out.data_ptr(), n, cell_ids.data_ptr(), n_tx.data_ptr(), counters.data_ptr(), ws.data_ptr(), ws_bytes,
              _lib.OUTLINE_MAX_POINTS, large_rows)
    c = dict(zip(bd.LARGE_OUTLINE_COUNTER_NAMES, counters.tolist()))
    K = c["n_kept"]
    return c, offs[:K + 1].cpu().numpy(), out[:c["n_vertices"]].cpu().numpy(), cell_ids[:K].cpu().numpy()


def stack(cells):
    return (np.concatenate(list(cells.values())), np.concatenate([np.full(len(p), c, dtype=np.int32) for c, p in cells.items()]))


@pytest.mark.parametrize("smoothing", [0, 2])
@pytest.mark.parametrize("connectivity", oc.CONNECTIVITIES)
def test_every_shared_case_on_the_global_route(cuda, connectivity, smoothing):
    got = scene_run(cuda, connectivity=connectivity, smoothing=smoothing, large_cells="global", _lds_max_points=0)
    assert_same(got, oc.expected(oc.scene_cells(), connectivity, smoothing), (connectivity, smoothing))
    same_bytes(got, scene_run(cuda, connectivity=connectivity, smoothing=smoothing), (connectivity, smoothing))


# ---------------------------------------------------------------- the component rule, across routes ---
def tie_cell(n, seed, delta):
    """a cloud and its mirror image, 1200 grid steps up and `delta` to the right: congruent, so every area ties exactly"""
    a = oc.cloud(n, seed, 300)
    return np.concatenate([a, a * [-1.0, 1.0] + [delta / oc.GRID, 1200.0 / oc.GRID]])


def three_clouds(ns, seed):
    """three clouds side by side, the small one first: the triangulation starts there, at point 0"""
    out, x = [], 0.0
    for i, (n, half) in enumerate(zip(ns, (150, 300, 200))):
        out.append(oc.cloud(n, seed + i, half, ((x + half) / oc.GRID, 0.0)))
        x += 2 * half + 350
    return np.concatenate(out)


# name -> (points, connectivity, the two best areas tie).  Triangle numbers (the triangulation's growth replayed on the host,
# not part of the test): tie_128 240 triangles, the winner's root 73 against 32; tie_340 662 triangles, roots 86 against 6;
# later_240 462 triangles, the largest component's root 66, the first component's 0; later_330 643 triangles, 86 after 0.
# So in every case the kept component is not the first found, and on the global route another wave holds it.
COMPONENT_CASES = {
    "tie_128": (lambda: tie_cell(64, 7, 28), 0.5, True),
    "tie_340": (lambda: tie_cell(170, 0, -8), 0.5, True),
    "later_240": (lambda: three_clouds((50, 110, 80), 2), 1.0, False),
    "later_330": (lambda: three_clouds((70, 150, 110), 1), 1.0, False),
}


def ring_by_the_component_rule(points, connectivity):
    """-> (the oracle's ring under the device's rule: the larger area, then the lower lowest vertex; the components as
    (twice the area, lowest vertex), best first)"""
    st = oc.State(points)
    alive, _ = oc.prune_sequential(st, connectivity)
    comps = sorted(((area2, int(st.simplices[ts].min()), ts) for area2, ts in oc.components(st, alive)), key=lambda c: c[:2])
    comps.sort(key=lambda c: -c[0])                                          # stable: equal areas stay by lowest vertex
    return st.points[oc.ring_of(st, comps[0][2])], [c[:2] for c in comps]


@pytest.mark.parametrize("name", COMPONENT_CASES)
def test_the_component_rule_gives_the_same_ring_on_every_route(cuda, name):
    make, connectivity, tie = COMPONENT_CASES[name]
    pts = make()
    rows, small = len(pts), name in ("tie_128", "later_240")
    assert (rows <= 256) == small and len(np.unique(pts, axis=0)) == rows
    ring, comps = ring_by_the_component_rule(pts, connectivity)
    if tie:                                                                  # every condition of exactness but the last one
        with pytest.raises(AssertionError, match="components of equal area"):
            oc.check_case(pts, connectivity)
        assert comps[0][0] == comps[1][0] > comps[2][0] and comps[0][1] < comps[1][1]
    else:
        assert oc.check_case(pts, connectivity)["components"] >= 3 and np.array_equal(ring, oc.outline(pts, connectivity))
        assert comps[0][1] > 0 and min(c[1] for c in comps) == 0             # point 0, where the growth starts, is elsewhere
    assert small or len(oc.State(pts).simplices) > 256
    want = (np.array([0, len(ring)]), ring, np.array([0], dtype=np.int32), np.array([rows]), 0)
    xy, ids = np.random.default_rng(5).permutation(pts), np.zeros(rows, dtype=np.int32)
    lds = run(cuda, xy, ids, 1, connectivity=connectivity)
    glob = run(cuda, xy, ids, 1, connectivity=connectivity, large_cells="global", _lds_max_points=0)
    assert_same(lds, want, (name, "default"))
    assert_same(glob, want, (name, "global"))
    same_bytes(lds, glob, name)


@pytest.fixture(scope="module")
def limit_cells():
    """the two cells at the limit, one of 2049 points above it, a small cell; id 3 is absent"""
    cells = {0: oc.big_cells()[0], 1: oc.big_cells()[1], 2: oc.cells()[1] + [700.0, 0.0], 4: lc.limit_cell() + [0.0, 300.0]}
    for k in oc.CONNECTIVITIES:
        oc.check_case(cells[4], k)
    return cells


def test_the_limit_one_cell_above_it_goes_through_global_memory(cuda, limit_cells):
    from segger_amd import _lib
    xy, ids = stack(limit_cells)
    want = oc.expected(limit_cells, 2.0)
    assert 4 in want[2].tolist()
    assert_same(run(cuda, xy, ids, 6, large_cells="global"), want, "default threshold")
    assert_same(run(cuda, xy, ids, 6, large_cells="global", _lds_max_points=0), want, "every cell")
    with pytest.raises(_lib.SeggerAmdError, match=rf"1 cells have more than {oc.MAX_POINTS} distinct points.*cell 4 among them"):
        run(cuda, xy, ids, 6)
    with pytest.raises(_lib.SeggerAmdError, match=rf"1 cells have more than {oc.MAX_POINTS} distinct points.*cell 4 among them"):
        run(cuda, xy, ids, 6, large_cells="refuse")


@pytest.mark.parametrize("name", lc.GOLDEN_CASES)
def test_ids_beyond_16_bits(cuda, name):
    """edge_ids: 11 500 points, 22 967 triangles, directed-edge ids up to 68 900.  vertex_ids: 65 537 points, 130 935
    triangles.  The expected ring is recorded (tests/golden/make_outlines_large_golden.py: the Python oracle takes 15 s).
    GPU time of the entry point, MI355X, median of 20 (profiles/outlines_large_cells.json): about 0.17 s at 11 500 points
    (interpolated between 51 ms at 4096 and 261 ms at 16 384; the test's call took 0.19 s) and 1.44 s at 65 537."""
    g = np.load(GOLDEN)
    pts = getattr(lc, name + "_cell")()
    assert len(pts) == int(g[name + "_points"]) and int(g[name + "_triangles"]) > (21846 if name == "edge_ids" else 2 * 65536 - 300)
    got = run(cuda, np.random.default_rng(1).permutation(pts), np.zeros(len(pts), dtype=np.int32), 1, large_cells="global")
    ring = g[name + "_ring"]
    assert got["ring_offsets"].tolist() == [0, len(ring)] and np.array_equal(got["xy"].view(np.uint64), ring.view(np.uint64))
    assert got["n_transcripts"].tolist() == [len(pts)] and got["n_dropped"] == 0
    a, b = got["xy"], np.roll(got["xy"], -1, axis=0)
    assert 0.5 * float((a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]).sum()) == float(g[name + "_area"])


def test_rows_against_distinct_points_three_orders_and_a_mask(cuda):
    cells = {0: lc.repeated_cell(), 1: lc.many_rows_few_points(), 2: oc.cells()[9]}
    assert len(cells[0]) > 2 * oc.MAX_POINTS and len(np.unique(cells[0], axis=0)) == oc.MAX_POINTS + 1
    assert len(cells[1]) > oc.MAX_POINTS == len(np.unique(cells[1], axis=0))
    xy, ids = stack(cells)
    extra = oc.cloud(200, 6, 900)                                            # masked-out rows in the large cell's id
    xy, ids = np.concatenate([xy, extra]), np.concatenate([ids, np.zeros(200, dtype=np.int32)])
    keep = np.concatenate([np.ones(len(ids) - 200, dtype=bool), np.zeros(200, dtype=bool)])
    want = lc.expected(cells, 2.0)
    assert want[2].tolist() == [0, 1, 2]
    first = None
    for perm in (np.random.default_rng(11).permutation(len(ids)), np.argsort(ids, kind="stable"), np.arange(len(ids))[::-1]):
        got = run(cuda, xy[perm], ids[perm], 3, keep=torch.from_numpy(keep[perm].copy()).to(cuda), large_cells="global")
        assert_same(got, want)
        first = first or got
        same_bytes(got, first)
    # the cell of 2048 distinct points and 2500 rows stayed on the LDS route: the counters show one large cell, of 2049
    # points, with a slice of its 4097 rows -- sized for both cells above 2048 rows, as the wrapper sizes it
    c, offs, out, kept = entry_point(cuda, xy, ids, 3, len(cells[0]) + len(cells[1]), keep=keep)
    assert (c["n_large_cells"], c["n_large_points"], c["n_large_rows"], c["n_refused"]) == (1, oc.MAX_POINTS + 1, len(cells[0]), 0)
    assert np.array_equal(offs, first["ring_offsets"]) and np.array_equal(out.view(np.uint64), first["xy"].view(np.uint64))
    # and the default call gives that cell the same bytes
    alone = run(cuda, cells[1], np.zeros(len(cells[1]), dtype=np.int32), 1)
    lo, hi = first["ring_offsets"][1], first["ring_offsets"][2]
    assert np.array_equal(alone["xy"].view(np.uint64), first["xy"][lo:hi].view(np.uint64))


def test_capacity_one_row_short_refuses_the_cell_and_returns(cuda, limit_cells):
    from segger_amd import _lib
    from segger_amd import boundaries as bd
    xy, ids = stack(limit_cells)
    need = len(limit_cells[4])

    def entry(large_rows):
        return entry_point(cuda, xy, ids, 6, large_rows)

    c, offs, out, kept = entry(need)
    assert (c["n_refused"], c["n_large_cells"], c["n_large_points"], c["n_large_rows"]) == (0, 1, need, need)
    assert kept.tolist() == [0, 1, 2, 4]
    c2, offs2, out2, kept2 = entry(need - 1)
    assert (c2["n_refused"], c2["refused_cell"] - 1, c2["n_large_cells"], c2["n_large_rows"]) == (1, 4, 0, 0)
    assert kept2.tolist() == [0, 1, 2] and np.array_equal(offs2, offs[:4])
    assert np.array_equal(out2.view(np.uint64), out[:offs[3]].view(np.uint64))


def test_segmentation_wrappers_pass_the_keyword_through(cuda):
    from segger_amd import boundaries as bd
    from segger_amd import postprocess as pp
    from test_gpu_boundaries import fake_result
    from test_postprocess import fake_predictions
    res, xy, row, enc, counted = fake_result(cuda)
    xy = xy / 4.0
    kw = dict(connectivity=1.0, large_cells="global", _lds_max_points=0)
    got = bd.segmentation_outlines(res, torch.from_numpy(xy).to(cuda), 40, **kw)
    want = run(cuda, xy[row[counted]], enc[counted].astype(np.int32), 40, **kw)
    plain = run(cuda, xy[row[counted]], enc[counted].astype(np.int32), 40, connectivity=1.0)
    for k in KEYS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]) and np.array_equal(want[k], plain[k]), k
    assert got["n_dropped"] == want["n_dropped"] and len(want["cell_ids"]) > 20
    acc = pp.SegmentationAccumulator(4000, cuda)
    for b in fake_predictions(0):
        acc.update(*b)
    sxy = torch.from_numpy(np.random.default_rng(8).integers(-2000, 2000, (4000, 2)).astype(np.float64) / 8).to(cuda)
    a, b = acc.outlines(sxy, **kw), bd.segmentation_outlines(acc.segmentation(), sxy, **kw)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert a["cell_ids"].numel() > 0
