"""segger_amd.geometry.points_in_polygons and neighbors.prediction_graph_shape on the device against the oracles of
tests/polygon_join_cases.py.

The named cases are compared pair for pair with the exact (rational) oracle, the batch with the float64 oracle; pairs
the exact oracle has within the undecided band (polygon_join_cases.BAND: 8 x E_REF, at least 4 float64 ulp, relative on
dist2 against d*d) are left out on both sides.  Everything else is an equality of tensors: the output is defined to be
bit-identical from call to call, for every grid, and for a polygon or a point whatever else is in the batch.
"""
import numpy as np
import pytest
import torch

import polygon_join_cases as pc

pytestmark = pytest.mark.gpu


def join(cuda, points, rings, buffer=None, predicate="contains", dtype=torch.float64, **kw):
    """points_in_polygons of numpy inputs -> the [2, E] device tensor"""
    from segger_amd import geometry as ge
    offsets, xy = pc.to_csr(rings)
    if isinstance(buffer, np.ndarray):
        buffer = torch.from_numpy(buffer).to(cuda)
    return ge.points_in_polygons(torch.from_numpy(np.ascontiguousarray(points)).to(cuda, dtype), torch.from_numpy(offsets).to(cuda),
                                 torch.from_numpy(xy).to(cuda), buffer=buffer, predicate=predicate, **kw)


def pairs(ei) -> np.ndarray:
    return ei.t().cpu().numpy()


def assert_sorted_unique(ei):
    a = pairs(ei)
    assert ei.dtype == torch.int64 and ei.dim() == 2 and ei.shape[0] == 2
    key = a[:, 0] * (int(a[:, 1].max()) + 1 if len(a) else 1) + a[:, 1]
    assert np.all(np.diff(key) > 0)                                   # sorted by (point, polygon), no duplicates


def assert_same_pairs(got, want, undecided, what):
    got, want = pc.without(got, undecided), pc.without(want, undecided)
    g, w = {tuple(r) for r in got.tolist()}, {tuple(r) for r in want.tolist()}
    assert g == w, (what, "extra", sorted(g - w)[:10], "missing", sorted(w - g)[:10])


@pytest.fixture(scope="module")
def case_runs(cuda):
    rings, _, points, _, _ = pc.cases()
    return {(pred, d): join(cuda, points, rings, buffer=d, predicate=pred) for pred in pc.PREDICATES for d in pc.D_CASES}


@pytest.fixture(scope="module")
def batch_runs(cuda):
    rings, points = pc.batch()
    return {r: join(cuda, points, rings, buffer=pc.batch_dists(r)) for r in pc.BATCH_RATIOS}


@pytest.mark.parametrize("d", pc.D_CASES)
@pytest.mark.parametrize("pred", pc.PREDICATES)
def test_cases_equal_the_exact_oracle(case_runs, pred, d):
    ref = pc.reference("cases", d)
    ei = case_runs[(pred, d)]
    assert_sorted_unique(ei)
    _, names, _, labels, _ = pc.cases()
    print(pred, d, "pairs", ei.shape[1], "oracle", len(ref["exact"][pred]), "undecided", len(ref["undecided"]))
    got = pairs(ei)
    want = ref["exact"][pred]
    g, w = {tuple(r) for r in pc.without(got, ref["undecided"]).tolist()}, {tuple(r) for r in pc.without(want, ref["undecided"]).tolist()}
    assert g == w, ([(labels[i], names[p]) for i, p in sorted(g - w)[:10]], [(labels[i], names[p]) for i, p in sorted(w - g)[:10]])


@pytest.mark.parametrize("ratio", pc.BATCH_RATIOS)
def test_batch_equals_the_float64_oracle(batch_runs, ratio):
    ref = pc.reference("batch", ratio)
    ei = batch_runs[ratio]
    assert_sorted_unique(ei)
    print(ratio, "pairs", ei.shape[1], "oracle", len(ref["f64"]["contains"]), "undecided", len(ref["undecided"]))
    assert_same_pairs(pairs(ei), ref["f64"]["contains"], ref["undecided"], ratio)


def test_batch_intersects_equals_the_float64_oracle(cuda):
    rings, points = pc.batch()
    ref = pc.reference("batch", 0.05)
    ei = join(cuda, points, rings, buffer=ref["dists"], predicate="intersects")
    assert_sorted_unique(ei)
    assert_same_pairs(pairs(ei), ref["f64"]["intersects"], ref["undecided"], "intersects")


def test_two_calls_and_every_grid_give_identical_tensors(cuda, batch_runs):
    rings, points = pc.batch()
    d = pc.batch_dists(0.05)
    assert torch.equal(join(cuda, points, rings, buffer=d), batch_runs[0.05])
    for ppc in (0.5, 2.0, 16.0):
        assert torch.equal(join(cuda, points, rings, buffer=d, points_per_cell=ppc), batch_runs[0.05]), ppc
    crings, _, cpoints, _, _ = pc.cases()                             # the far point stretches this grid: clamped border cells
    want = join(cuda, cpoints, crings, buffer=0.25)
    for ppc in (0.5, 16.0):
        assert torch.equal(join(cuda, cpoints, crings, buffer=0.25, points_per_cell=ppc), want), ppc


def test_permutations_relabel_the_pairs(cuda, batch_runs):
    rings, points = pc.batch()
    d = pc.batch_dists(0.05)
    want = {tuple(r) for r in pairs(batch_runs[0.05]).tolist()}
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(points))                               # new point i is old point perm[i]
    got = join(cuda, points[perm], rings, buffer=d)
    assert_sorted_unique(got)
    assert {(int(perm[i]), p) for i, p in pairs(got).tolist()} == want
    qerm = rng.permutation(len(rings))
    got = join(cuda, points, [rings[q] for q in qerm], buffer=d[qerm])
    assert_sorted_unique(got)
    assert {(i, int(qerm[p])) for i, p in pairs(got).tolist()} == want


def test_each_case_alone_equals_its_rows(cuda, case_runs):
    rings, names, points, _, _ = pc.cases()
    full = pairs(case_runs[("contains", 0.25)])
    for k, name in enumerate(names):
        alone = pairs(join(cuda, points, [rings[k]], buffer=0.25))
        rows = full[full[:, 1] == k]
        assert np.array_equal(alone[:, 0], rows[:, 0]) and np.all(alone[:, 1] == 0), name


def test_short_and_long_rings_alone_equal_their_rows(cuda, batch_runs):
    rings, points = pc.batch()
    d = pc.batch_dists(0.05)
    n_verts = np.array([len(pc.mc.open_ring(r)) for r in rings])
    full = pairs(batch_runs[0.05])
    for keep in (np.flatnonzero(n_verts <= 64), np.flatnonzero(n_verts > 64)):          # the register and the LDS route
        assert len(keep) > 25
        got = pairs(join(cuda, points, [rings[p] for p in keep], buffer=d[keep]))
        new_id = np.full(len(rings), -1)
        new_id[keep] = np.arange(len(keep))
        rows = full[new_id[full[:, 1]] >= 0]
        assert np.array_equal(got, np.stack([rows[:, 0], new_id[rows[:, 1]]], axis=1))


def test_prediction_graph_shape(cuda, batch_runs):
    from segger_amd import geometry as ge, morphology as mo, neighbors as nb
    rings, points = pc.batch()
    offsets, xy = (torch.from_numpy(a).to(cuda) for a in pc.to_csr(rings))
    tx = torch.from_numpy(points).to(cuda)
    area = mo.polygon_props(offsets, xy)["area"]
    d = torch.sqrt(area / np.pi) * 0.05
    d = torch.where(area.isnan(), torch.zeros_like(d), d)
    got = nb.prediction_graph_shape(tx, offsets, xy)                                      # the default ratio
    assert torch.equal(got, ge.points_in_polygons(tx, offsets, xy, buffer=d, predicate="contains"))
    assert_same_pairs(pairs(got), pc.reference("batch", 0.05)["f64"]["contains"], pc.reference("batch", 0.05)["undecided"], "shape")
    # float32 positions: the same result as their float64 copy
    tx32 = tx.sub(tx.min(0).values).float()                                               # slide coordinates lose bits in float32
    offsets0, xy0 = offsets, xy - tx.min(0).values
    assert torch.equal(nb.prediction_graph_shape(tx32, offsets0, xy0), nb.prediction_graph_shape(tx32.double(), offsets0, xy0))
    # no buffer: the points on a ring stay out
    rings_c, _, cpoints, _, _ = pc.cases()
    co, cxy = (torch.from_numpy(a).to(cuda) for a in pc.to_csr(rings_c))
    got = nb.prediction_graph_shape(torch.from_numpy(cpoints).to(cuda), co, cxy, buffer_ratio=0.0)
    ref = pc.reference("cases", 0.0)
    on_ring = {k for k, d2 in ref["exact"]["dist2"].items() if d2 is not None and d2 == 0}
    assert on_ring and not on_ring & {tuple(r) for r in pairs(got).tolist()}
    assert {tuple(r) for r in pairs(got).tolist()} == {tuple(r) for r in ref["exact"]["contains"].tolist()}


def test_bad_offsets_and_empty_inputs(cuda):
    from segger_amd import geometry as ge
    rings, _, points, _, _ = pc.cases()
    offsets, xy = pc.to_csr(rings[:4])
    pts = torch.from_numpy(points).to(cuda)
    xy_d = torch.from_numpy(xy).to(cuda)
    for bad, where in ((offsets.copy(), 2), (offsets.copy(), 3)):
        if where == 2:
            bad[2] = bad[1] - 1                                        # descending
        else:
            bad[4] = len(xy) + 5                                       # beyond the vertices
        with pytest.raises(ValueError, match=rf"ring_offsets of polygon {1 if where == 2 else 3} are"):
            ge.points_in_polygons(pts, torch.from_numpy(bad).to(cuda), xy_d, buffer=0.25)
    with pytest.raises(ValueError, match="non-finite"):
        ge.points_in_polygons(torch.cat([pts, pts.new_tensor([[float("nan"), 0.0]])]), torch.from_numpy(offsets).to(cuda), xy_d)
    with pytest.raises(ValueError, match="buffer must be finite"):
        ge.points_in_polygons(pts, torch.from_numpy(offsets).to(cuda), xy_d, buffer=torch.tensor([0.1, -0.1, 0.1, 0.1], device=cuda))
    for ei in (ge.points_in_polygons(pts[:0], torch.from_numpy(offsets).to(cuda), xy_d),
               ge.points_in_polygons(pts, torch.zeros(1, dtype=torch.int64, device=cuda), xy_d[:0]),
               ge.points_in_polygons(pts, torch.zeros(3, dtype=torch.int64, device=cuda), xy_d[:0])):
        assert ei.shape == (2, 0) and ei.dtype == torch.int64 and ei.is_cuda


def test_predict_step_runs_on_the_shape_graph(cuda):
    from segger_amd import LitISTEncoder, TX_NB_BD, neighbors as nb
    from segger_amd.synthetic import C1, make_graph
    b, aux = make_graph(C1, return_aux=True)
    centres = b["bd"].pos.double()
    ang = torch.arange(13, dtype=torch.float64) * (2 * np.pi / 13)
    radius = 0.05 * float((centres.max(0).values - centres.min(0).values).max())
    xy = (centres[:, None, :] + radius * torch.stack([ang.cos(), ang.sin()], 1)[None]).reshape(-1, 2)
    offsets = torch.arange(centres.shape[0] + 1, dtype=torch.int64) * 13
    ei = nb.prediction_graph_shape(b["tx"].pos.to(cuda), offsets.to(cuda), xy.to(cuda))
    assert ei.shape[1] > 0 and int(ei[0].max()) < b["tx"].pos.shape[0] and int(ei[1].max()) < centres.shape[0]
    b[TX_NB_BD]["edge_index"] = ei.cpu()
    torch.manual_seed(0)
    m = LitISTEncoder(n_genes=C1.n_genes, in_channels=128)
    m.model._materialize_bd(C1.bd_dim, "cpu")
    m = m.to(cuda).eval()
    m.set_similarities(aux["tx_similarity"].to(cuda), aux["bd_similarity"].to(cuda))
    tx_index, seg, sim, gene = m.predict_step(b.to(cuda), 0)
    assert sim.numel() > 0 and bool(torch.isfinite(sim).all()) and bool((seg >= 0).any())
