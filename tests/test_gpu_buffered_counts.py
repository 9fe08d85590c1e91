"""segger_amd.buffered_counts on the device against the CPU oracle of tests/buffered_count_cases.py.  Every returned tensor
and every counter is EQUAL to the oracle -- no tolerance: the counts are integers, the rows are sorted, and the predicate
is the float64 arithmetic of the join in its order, on coordinates that are multiples of 2^-11.  The scenes stay below a
few thousand points and sit on the kernel's own boundaries: the ring routes, the wave-chunk edge of the cell walk, the
histogram tiers and the touched list."""
import numpy as np
import pytest
import torch

import buffered_count_cases as bc
import polygon_join_cases as pc

pytestmark = pytest.mark.gpu

KEYS = ("indptr", "indices", "counts", "cell_count", "counters")
DTYPES = {"indptr": torch.int64, "indices": torch.int32, "counts": torch.int32, "cell_count": torch.int64, "counters": torch.int64}


def consts():
    from segger_amd import _lib
    return dict(touched=_lib.BCOUNT_TOUCHED, small_genes=_lib.BCOUNT_SMALL_GENES)


def run(cuda, points, gene, rings, n_genes, buffer=None, predicate="contains", gene_dtype=torch.int64, **kw):
    from segger_amd import buffered_counts as bcm
    offsets, xy = pc.to_csr(rings)
    if isinstance(buffer, np.ndarray):
        buffer = torch.from_numpy(buffer).to(cuda)
    return bcm.buffered_counts(torch.from_numpy(np.ascontiguousarray(points)).to(cuda), torch.from_numpy(np.asarray(gene)).to(cuda, gene_dtype),
                               torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda), n_genes, buffer=buffer,
                               predicate=predicate, **kw)


def assert_equal(got, want, what=""):
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert got[k].dtype == DTYPES[k] and got[k].is_cuda, (what, k)
        assert g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k, g[:20], want[k][:20])


def check(cuda, points, gene, rings, n_genes, buffer=None, predicate="contains", **kw):
    d = 0.0 if buffer is None else buffer
    want = bc.buffered_counts(points, gene, rings, n_genes, d, predicate, **consts())
    got = run(cuda, points, gene, rings, n_genes, buffer, predicate, **kw)
    print(predicate, "n_genes", n_genes, dict(zip(bc.COUNTER_NAMES, got["counters"].tolist())), "oracle", want["counters"].tolist())
    assert_equal(got, want, (predicate, n_genes))
    return got, want


@pytest.mark.parametrize("pred", pc.PREDICATES)
def test_ring_routes_3_64_65_4096_vertices(cuda, pred):
    rings, points, gene = bc.scene_routes()
    got, want = check(cuda, points, gene, rings, 50, 0.5, pred)
    assert np.all(np.diff(want["indptr"]) > 0)                       # every route did count something


def test_cells_of_0_1_63_64_65_points(cuda):
    rings, points, gene = bc.scene_clusters()
    got, want = check(cuda, points, gene, rings, 7, 0.0)
    assert want["cell_count"].tolist() == [1, 63, 64, 65, 0, 193]
    check(cuda, points, gene, rings, 7, 0.25, "intersects")


def test_tier_edges_1_2048_2049_and_the_cap(cuda):
    from segger_amd import _lib
    rings, points = bc.scene_field()
    routes = bc.scene_routes()
    for n_genes in (1, _lib.BCOUNT_SMALL_GENES, _lib.BCOUNT_SMALL_GENES + 1, _lib.BCOUNT_MAX_GENES):
        gene = bc.field_genes(n_genes)
        gene[:3] = n_genes - 1                                       # the last slot of the histogram is used
        got, want = check(cuda, points, gene, rings, n_genes, 1.5)
        assert want["counters"][4] == (len(rings) if n_genes > _lib.BCOUNT_SMALL_GENES else 0)
        # the long-ring route of the tier: at the cap, the workgroup that fills the LDS
        check(cuda, routes[1], routes[2] * (n_genes // 50), routes[0], n_genes, 0.5)


def test_one_gene_above_the_cap_raises(cuda):
    from segger_amd import _lib
    rings, points = bc.scene_field()
    with pytest.raises(ValueError, match=rf"SEGGER_BCOUNT_MAX_GENES = {_lib.BCOUNT_MAX_GENES}"):
        run(cuda, points, bc.field_genes(5), rings, _lib.BCOUNT_MAX_GENES + 1)


def test_touched_list_overflow_no_hit_and_one_shared_gene(cuda):
    from segger_amd import _lib
    T = _lib.BCOUNT_TOUCHED
    for n_distinct, n_genes in ((T, T), (T + 1, T + 1), (T + 50, T + 50), (T + 50, _lib.BCOUNT_SMALL_GENES + 1)):
        rings, points, gene, _ = bc.scene_overflow(n_distinct)
        got, want = check(cuda, points, gene, rings, n_genes)
        assert np.diff(want["indptr"]).tolist() == [n_distinct, 1, 0]
        assert want["counters"][3] == (1 if n_distinct > T else 0) == int(got["counters"][3])
    assert int(got["counters"][3]) != 0


def test_duplicate_polygons_and_mixed_buffers_on_ring_points(cuda):
    rings, names, points, _, _ = pc.cases()
    rings = list(rings) + [rings[0], rings[3], rings[3]]
    gene = np.arange(len(points)) % 11
    buf = np.where(np.arange(len(rings)) % 2 == 0, 0.0, 0.25)
    buf[-3:] = (buf[0], buf[3], buf[3])                              # a duplicate carries its twin's buffer
    for pred in pc.PREDICATES:
        got, want = check(cuda, points, gene, rings, 11, buf, pred)
        g = bc.dense({k: got[k].cpu().numpy() for k in KEYS}, 11)
        assert np.array_equal(g[3], g[-1]) and np.array_equal(g[3], g[-2]) and g[3].sum() > 0      # duplicates: the same rows
        assert np.array_equal(g[0], g[-3])
    zero = bc.buffered_counts(points, gene, rings, 11, 0.0, "contains")
    closed = bc.buffered_counts(points, gene, rings, 11, 0.0, "intersects")
    assert closed["counters"][0] > zero["counters"][0]               # points exactly on a ring are in the scene


def test_gene_out_of_range_moves_n_bad_and_nothing_else(cuda):
    rings, points = bc.scene_field()
    gene = bc.field_genes(40).astype(np.int64)
    bad = np.arange(len(gene)) % 9 == 0
    gene_bad = gene.copy()
    gene_bad[bad] = np.resize(np.array([-1, 40, 41, 2 ** 31, 2 ** 40 + 3, -2 ** 33]), int(bad.sum()))
    got, want = check(cuda, points, gene_bad, rings, 40, 1.5)
    assert want["counters"][2] > 0 and int(got["counters"][2]) == want["counters"][2]
    without = run(cuda, points[~bad], gene[~bad], rings, 40, 1.5)
    for k in ("indptr", "indices", "counts", "cell_count"):
        assert torch.equal(got[k], without[k]), k
    assert int(got["counters"][0]) - int(got["counters"][2]) == int(without["counters"][0])
    small = run(cuda, points, np.clip(gene_bad, -5, 45), rings, 40, 1.5, gene_dtype=torch.int16)
    for k in KEYS:
        assert torch.equal(got[k], small[k]), k


@pytest.mark.parametrize("dtype,lo,hi", [(torch.int8, -128, 127), (torch.uint8, 0, 255)])
def test_narrow_gene_dtypes_with_n_genes_beyond_their_range(cuda, dtype, lo, hi):
    """n_genes and the -1 of "out of range" must not wrap in the dtype of ``gene``: the same bytes as the int64 run"""
    from segger_amd import _lib
    rings, points = bc.scene_field()
    gene = np.random.default_rng(21).integers(lo, hi + 1, len(points))
    gene[:4] = (lo, hi, 0, 100)
    for n_genes in (100, 128, 256, 500, _lib.BCOUNT_MAX_GENES):
        wide, want = check(cuda, points, gene, rings, n_genes, 1.5)
        narrow = run(cuda, points, gene, rings, n_genes, 1.5, gene_dtype=dtype)
        for k in KEYS:
            assert torch.equal(wide[k], narrow[k]), (n_genes, k)
        assert (want["counters"][2] > 0) == (lo < 0 or hi >= n_genes) and want["counters"][1] > 0


def test_same_bytes_for_any_grid_point_order_and_polygon_order(cuda):
    rings, points = bc.scene_field()
    gene = bc.field_genes(300)
    buf = np.linspace(0.0, 2.0, len(rings))
    base, _ = check(cuda, points, gene, rings, 300, buf)
    for ppc in (0.25, 8.0, 500.0):
        other = run(cuda, points, gene, rings, 300, buf, points_per_cell=ppc)
        for k in KEYS:
            assert torch.equal(base[k], other[k]), (ppc, k)
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(points))
    other = run(cuda, points[perm], gene[perm], rings, 300, buf)
    for k in KEYS:
        assert torch.equal(base[k], other[k]), ("points", k)
    pperm = rng.permutation(len(rings))
    other = run(cuda, points, gene, [rings[p] for p in pperm], 300, buf[pperm])
    a = bc.dense({k: base[k].cpu().numpy() for k in KEYS}, 300)
    b = bc.dense({k: other[k].cpu().numpy() for k in KEYS}, 300)
    assert np.array_equal(a[pperm], b) and torch.equal(base["counters"], other["counters"])
    assert torch.equal(base["cell_count"][torch.from_numpy(pperm).to(cuda)], other["cell_count"])


def test_equals_the_composition_of_the_join_and_a_bincount(cuda):
    from segger_amd import geometry as ge
    rings, points = bc.scene_field()
    n_genes = 120
    gene = bc.field_genes(n_genes)
    offsets, xy = pc.to_csr(rings)
    t = [torch.from_numpy(a).to(cuda) for a in (points, offsets, xy, gene)]
    for pred in pc.PREDICATES:
        got = run(cuda, points, gene, rings, n_genes, 1.5, pred)
        ei = ge.points_in_polygons(t[0], t[1], t[2], buffer=1.5, predicate=pred)
        dense = torch.bincount(ei[1] * n_genes + t[3][ei[0]], minlength=len(rings) * n_genes).view(len(rings), n_genes)
        assert int(got["counters"][0]) == ei.shape[1] > int(ei[0].unique().numel()) > 1000      # some points lie in two grown rings
        row, col = dense.nonzero(as_tuple=True)
        assert torch.equal(got["indices"].long(), col) and torch.equal(got["counts"].long(), dense[row, col])
        assert torch.equal(got["indptr"][1:], torch.cumsum(torch.bincount(row, minlength=len(rings)), 0))
        assert torch.equal(got["cell_count"], dense.sum(1))


def test_filter_boundaries_and_the_region_sum_on_a_2x2_grid(cuda):
    from segger_amd import buffered_counts as bcm
    rings, points = bc.scene_field()
    n_genes = 60
    gene = bc.field_genes(n_genes)
    gene[::17] = n_genes + 2
    buf = np.linspace(0.5, 2.0, len(rings))
    want = bc.buffered_counts_regions(points, gene, rings, n_genes, bc.REGION_GRID, buf, bc.REGION_OVERLAP)
    assert want["kept"].min() >= 1 and want["counts"].sum() > len(points) // 2       # on the oracle: nothing was dropped
    offsets, xy = pc.to_csr(rings)
    t_off, t_xy = torch.from_numpy(offsets).to(cuda), torch.from_numpy(xy).to(cuda)
    for x0, y0, x1, y1 in bc.REGION_GRID:
        outset = (x0 - bc.REGION_OVERLAP, y0 - bc.REGION_OVERLAP, x1 + bc.REGION_OVERLAP, y1 + bc.REGION_OVERLAP)
        keep = bcm.filter_boundaries(t_off, t_xy, (x0, y0, x1, y1), outset)
        assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), bc.filter_boundaries(rings, (x0, y0, x1, y1), outset))
    got = bcm.buffered_counts_regions(torch.from_numpy(points).to(cuda), torch.from_numpy(gene).to(cuda), t_off, t_xy, n_genes,
                                      torch.tensor(bc.REGION_GRID), torch.from_numpy(buf).to(cuda), overlap=bc.REGION_OVERLAP)
    for k in ("indptr", "indices", "counts", "cell_count", "kept"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    c = dict(zip(bcm.COUNTER_NAMES, got["counters"].tolist()))
    assert (c["n_pairs"], c["n_bad"], c["nnz"]) == (want["n_pairs"], want["n_bad"], len(want["indices"])) and c["n_bad"] > 0


def test_empty_inputs_and_degenerate_rings(cuda):
    rings, points = bc.scene_field()
    gene = bc.field_genes(9)
    r = run(cuda, points[:0], gene[:0], rings, 9)
    assert r["indptr"].tolist() == [0] * (len(rings) + 1) and r["indices"].numel() == 0 and r["counters"].tolist() == [0] * 5
    r = run(cuda, points, gene, [], 9)
    assert r["indptr"].tolist() == [0] and r["cell_count"].numel() == 0
    odd = [np.zeros((0, 2)), points[:1], points[:2], rings[0], np.concatenate([points[:2], points[:1]])]
    check(cuda, points, gene, odd, 9, 1.0)


def test_the_chain_into_expression_features_and_scipy(cuda):
    from segger_amd import buffered_counts as bcm, features
    rings, points = bc.scene_field()
    n_genes = 30
    gene = bc.field_genes(n_genes)
    gene[::25] = -1
    got = run(cuda, points, gene, rings, n_genes, 1.5)
    f = features.expression_features(got, embedding_size=4, cells_min_counts=1, genes_min_counts=1)
    assert f["X_pca"].shape == (len(rings), 4) and bool(torch.isfinite(f["X_pca"]).all())
    m = bcm.buffered_counts_to_scipy(got, n_genes)
    c = dict(zip(bcm.COUNTER_NAMES, got["counters"].tolist()))
    assert m.dtype == np.uint32 and m.shape == (len(rings), n_genes) and m.has_sorted_indices
    assert int(m.sum()) == c["n_pairs"] - c["n_bad"] == int(got["cell_count"].sum()) and c["n_bad"] > 0
