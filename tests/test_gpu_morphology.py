"""segger_amd.morphology on the device against the oracles of tests/morphology_cases.py.

The yardstick is the exact (rational) oracle: ``n_hull`` equal, the five float quantities within ``8 x E_REF`` relative
(E_REF = the float64 oracle's own deviation from the exact one, morphology_cases.E_REF) with a floor of 4 float64 ulp --
the margin covers a different but fixed summation and projection order, not a wrong vertex.  The three areas of the cases
are sums of exactly representable products, so a wrong hull vertex shows as a ``hull_area`` outside 4 ulp.
"""
import math
import os

import numpy as np
import pytest
import torch

import morphology_cases as mc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morphology_small.npz")
KERNEL_COLS = mc.FLOAT_COLS


def run(cuda, rings):
    """polygon_props of a list of rings -> dict of numpy arrays"""
    from segger_amd import morphology as mo
    offsets, xy = mc.to_csr(rings)
    out = mo.polygon_props(torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda))
    return {k: v.cpu().numpy() for k, v in out.items()}


def raw_props(cuda, rings):
    """the kernel's [P, 12] table, bit for bit"""
    got = run(cuda, rings)
    return np.concatenate([np.stack([got[c] for c in KERNEL_COLS], 1), got["centroid"], got["bounds"],
                           got["n_hull"][:, None].astype(np.float64)], axis=1)


@pytest.fixture(scope="module")
def case_results(cuda):
    return run(cuda, [ring for _, ring in mc.cases()])


@pytest.fixture(scope="module")
def batch_results(cuda):
    return run(cuda, list(mc.batch()))


def check_against_exact(got, exact, f64, labels):
    worst = {c: 0.0 for c in mc.FLOAT_COLS}
    failures = []
    for p, (ex, ref, label) in enumerate(zip(exact, f64, labels)):
        if got["n_hull"][p] != ex["n_hull"]:
            failures.append((label, "n_hull", int(got["n_hull"][p]), ex["n_hull"]))
        want = mc.exact_floats(ex)
        for c in mc.FLOAT_COLS:
            if math.isnan(want[c]):
                if not math.isnan(got[c][p]):
                    failures.append((label, c, got[c][p], "nan"))
                continue
            dev = mc.rel_dev(float(got[c][p]), want[c])
            worst[c] = max(worst[c], dev)
            if dev > mc.tolerance(c):
                failures.append((label, c, float(got[c][p]), want[c], dev))
        if ex["n_hull"]:
            assert np.array_equal(got["bounds"][p], np.asarray(ref["bounds"])), label             # min / max: exact
            extent = 1.0 + max(ref["bounds"][2] - ref["bounds"][0], ref["bounds"][3] - ref["bounds"][1])
            assert np.allclose(got["centroid"][p], ref["centroid"], rtol=0, atol=1e-10 * extent), label
    print("largest kernel-vs-exact relative deviation:", worst)
    assert not failures, failures[:10]


def test_cases_agree_with_the_exact_oracle(case_results):
    f64, exact = mc.reference("cases")
    check_against_exact(case_results, exact, f64, [name for name, _ in mc.cases()])


def test_batch_agrees_with_the_exact_oracle(batch_results):
    f64, exact = mc.reference("batch")
    check_against_exact(batch_results, exact, f64, list(range(len(exact))))


def test_cases_one_by_one_equal_the_concatenated_run(cuda, case_results):
    want = np.concatenate([np.stack([case_results[c] for c in KERNEL_COLS], 1), case_results["n_hull"][:, None]], axis=1)
    for p, (name, ring) in enumerate(mc.cases()):
        got = run(cuda, [ring])
        row = np.concatenate([[got[c][0] for c in KERNEL_COLS], [got["n_hull"][0]]])
        assert np.array_equal(row, want[p], equal_nan=True), name


def test_float32_features_are_the_float64_result_rounded_once(cuda, case_results):
    from segger_amd import morphology as mo
    offsets, xy = mc.to_csr([ring for _, ring in mc.cases()])
    o, v = torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda)
    f32 = mo.morphology_features(o, v)
    f64 = mo.morphology_features(o, v, torch.float64)
    assert f32.dtype == torch.float32 and f32.shape == (len(mc.cases()), 4)
    assert np.array_equal(f32.cpu().numpy().view(np.uint32), f64.float().cpu().numpy().view(np.uint32))
    want = np.stack([case_results[c] for c in ("area", "convexity", "elongation", "circularity")], 1)
    assert np.array_equal(f64.cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(mo.morphology_features(o, v.float(), torch.float64).cpu().numpy()[:2], want[:2])     # any float dtype in


def test_degenerate_rows_follow_ieee_division(case_results):
    f64 = mc.reference("cases")[0]
    names = [name for name, _ in mc.cases()]
    for name in mc.DEGENERATE:
        p = names.index(name)
        want = mc.ratios(*(f64[p][c] for c in mc.FLOAT_COLS))
        got = np.array([case_results[c][p] for c in ("area", "convexity", "elongation", "circularity")])
        assert np.array_equal(got, want, equal_nan=True), (name, got, want)
        assert case_results["n_hull"][p] == f64[p]["n_hull"], name
    p = names.index("empty")
    assert all(math.isnan(case_results[c][p]) for c in mc.FLOAT_COLS) and np.isnan(case_results["centroid"][p]).all()
    p = names.index("segment")                                       # 0 / 0, 0 / envelope, 0 / r^2
    assert math.isnan(case_results["convexity"][p]) and case_results["elongation"][p] == 0 and case_results["circularity"][p] == 0
    p = names.index("point")                                         # everything 0 / 0
    assert all(math.isnan(case_results[c][p]) for c in ("convexity", "elongation", "circularity"))


def test_invariances(cuda, case_results):
    names = [name for name, _ in mc.cases()]
    base = ["l_shape", "star5", "rect_10x1_rot30", "regular13", "star63", "star65", "star200", "square_edge_vertices"]
    variants, owner = [], []
    for name in base:
        ring = dict(mc.cases())[name]
        shift = mc.quantize(np.array([-31000.5, 88000.125]))
        for v in (ring[::-1], np.roll(ring, 5, axis=0), np.roll(ring[::-1], 2, axis=0), np.concatenate([ring, ring[:1]]),
                  ring + shift):
            variants.append(np.ascontiguousarray(v))
            owner.append(names.index(name))
    got = run(cuda, variants)
    exact = mc.reference("cases")[1]
    for q, p in enumerate(owner):
        assert got["n_hull"][q] == case_results["n_hull"][p] == exact[p]["n_hull"], (names[p], q % 5)
        want = mc.exact_floats(exact[p])                              # the same exact quantities for every variant
        for c in mc.FLOAT_COLS:
            assert mc.rel_dev(float(got[c][q]), want[c]) <= mc.tolerance(c), (names[p], q % 5, c)
        if q % 5 != 4:                                               # the same vertices: the same bounds
            assert np.array_equal(got["bounds"][q], case_results["bounds"][p])


def test_reproducible_and_independent_of_position_in_the_batch(cuda):
    rings = list(mc.batch())
    first, second = raw_props(cuda, rings), raw_props(cuda, rings)
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    perm = np.random.default_rng(3).permutation(len(rings))
    shuffled = raw_props(cuda, [rings[i] for i in perm])
    assert np.array_equal(shuffled.view(np.uint64), first[perm].view(np.uint64))


def test_routes(cuda, batch_results):
    rings = list(mc.batch())
    n = np.array([len(mc.open_ring(r)) for r in rings])
    assert (n > 64).sum() >= 30 and (n == 64).sum() + (n == 65).sum() >= 2 and (n <= 64).sum() >= 800
    full = np.stack([batch_results[c] for c in KERNEL_COLS] + [batch_results["n_hull"].astype(np.float64)], 1)
    for pick in (np.flatnonzero(n > 64), np.flatnonzero(n <= 64)):
        got = run(cuda, [rings[i] for i in pick])
        part = np.stack([got[c] for c in KERNEL_COLS] + [got["n_hull"].astype(np.float64)], 1)
        assert np.array_equal(part.view(np.uint64), full[pick].view(np.uint64))


def test_bad_offsets_are_reported_and_nothing_runs_for_no_polygons(cuda):
    from segger_amd import morphology as mo
    xy = torch.rand(10, 2, dtype=torch.float64, device=cuda)
    for offsets, where in (([0, 5, 3, 10], 1), ([0, 4, 11], 1), ([-1, 4, 10], 0)):
        with pytest.raises(ValueError, match=f"polygon {where}"):
            mo.polygon_props(torch.tensor(offsets, device=cuda), xy)
    out = mo.polygon_props(torch.zeros(1, dtype=torch.int64, device=cuda), xy[:0])
    assert out["area"].shape == (0,) and out["centroid"].shape == (0, 2) and out["bounds"].shape == (0, 4)
    assert out["n_hull"].dtype == torch.int32 and mo.morphology_features(torch.zeros(1, dtype=torch.int64, device=cuda), xy).shape == (0, 4)


def test_rings_from_padded_round_trips(cuda, case_results):
    from segger_amd import morphology as mo
    names = ["regular13", "regular25", "triangle", "star63"]
    rings = [dict(mc.cases())[n] for n in names]
    padded = np.full((len(rings), 64, 2), np.nan)
    for p, r in enumerate(rings):
        padded[p, :len(r)] = r
    counts = torch.tensor([len(r) for r in rings], device=cuda)
    offsets, xy = mo.rings_from_padded(torch.from_numpy(padded).to(cuda), counts)
    want_offsets, want_xy = mc.to_csr(rings)
    assert np.array_equal(offsets.cpu().numpy(), want_offsets) and np.array_equal(xy.cpu().numpy(), want_xy)
    got = mo.polygon_props(offsets, xy)
    all_names = [name for name, _ in mc.cases()]
    for p, name in enumerate(names):
        assert float(got["area"][p]) == case_results["area"][all_names.index(name)], name


def test_anndata_features_gains_x_morphology_only_when_given_boundaries(cuda):
    from segger_amd import features as ft
    from segger_amd import morphology as mo
    from segger_amd import postprocess as pp
    from test_postprocess import fake_predictions
    acc = pp.SegmentationAccumulator(4000, cuda)
    for b in fake_predictions(0):
        acc.update(*b)
    expr = acc.expression()
    n_cells = int(expr["indptr"].numel()) - 1
    rings = [mc.star_ring(13, 500 + p) + mc.quantize(mc.SLIDE + [3.0 * p, 2.0 * p]) for p in range(n_cells)]
    offsets, xy = mc.to_csr(rings)
    offsets, xy = torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda)
    kw = dict(cells_clusters_n_neighbors=5, genes_clusters_n_neighbors=3)
    plain = ft.anndata_features(expr, 6, 20, 30, **kw)
    with_bd = ft.anndata_features(expr, 6, 20, 30, boundaries=(offsets, xy), **kw)
    assert set(with_bd) == set(plain) | {"X_morphology"} and "X_morphology" not in plain
    for key, value in plain.items():
        assert torch.equal(with_bd[key], value), key
    assert with_bd["X_morphology"].dtype == torch.float32
    assert torch.equal(with_bd["X_morphology"], mo.morphology_features(offsets, xy))
    with pytest.raises(ValueError, match="boundary rings"):
        ft.anndata_features(expr, 6, 20, 30, boundaries=(offsets[:-1], xy), **kw)


def test_encoder_runs_on_four_wide_morphology_input(oracle, cuda):
    from segger_amd import LitISTEncoder
    from segger_amd import morphology as mo
    from segger_amd.synthetic import SyntheticSpec, make_graph
    spec = SyntheticSpec(n_tx=1000, n_bd=100, k_tx=5, n_graphs=1, seed=3, bd_dim=4)
    b, aux = make_graph(spec, return_aux=True)
    centres = b["bd"]["pos"].double().numpy()
    rings = [mc.star_ring(13 if p % 2 else 25, 900 + p, 4.0 + 0.05 * p) + centres[p] for p in range(len(centres))]
    offsets, xy = mc.to_csr(rings)
    bd_x = mo.morphology_features(torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda))
    assert bd_x.shape == (len(centres), 4) and bool(torch.isfinite(bd_x).all())
    b["bd"]["x"] = bd_x.cpu()
    torch.manual_seed(1)
    m = LitISTEncoder(n_genes=spec.n_genes, in_channels=128, hidden_channels=64, out_channels=64, n_heads=2)
    m.model._materialize_bd(4, "cpu")
    sd = {k: v.detach().clone().double() for k, v in m.state_dict().items()}
    m = m.to(cuda).eval()
    z = m(b.to(cuda))
    z_ref = oracle.ist_encoder_forward(sd, b.x_dict, b.edge_index_dict, b.pos_dict, b.batch_dict, n_heads=2)
    for k in ("tx", "bd"):
        assert bool(torch.isfinite(z[k]).all())
        err = (z[k].double().cpu() - z_ref[k]).abs().max().item()
        assert err < 5e-5, f"{k}: max abs err {err}"


def test_golden_scipy_hulls_are_reproduced(cuda):
    from segger_amd import morphology as mo
    g = np.load(GOLDEN)
    got = mo.polygon_props(torch.from_numpy(g["ring_offsets"]).to(cuda), torch.from_numpy(g["xy"]).to(cuda))
    n_hull, hull_area = got["n_hull"].cpu().numpy(), got["hull_area"].cpu().numpy()
    for p, name in enumerate(g["names"]):
        ring = mc.open_ring(g["xy"][g["ring_offsets"][p]:g["ring_offsets"][p + 1]])
        verts = g["scipy_hull_vertices"][g["scipy_hull_offsets"][p]:g["scipy_hull_offsets"][p + 1]]
        assert n_hull[p] == len({tuple(ring[i]) for i in verts}), name
        assert abs(hull_area[p] - g["scipy_hull_area"][p]) <= mc.scipy_area_tolerance(ring), name
