"""Contamination scoring on the device (``segger_amd.validation``, ``csrc/contamination.hip``) against the float64 numpy
oracles of tests/contamination_cases.py, every case, every row, every entry.

Bounds, all derived, none tuned:

* ``counts`` / ``freq``: integers, and one float64 product rounded once to float32: bit-equal.
* ``contamination``, ``contaminated``, ``total``: integers, equal (the generator keeps every ``q_self`` at least 1e-6 from
  the cutoff); ``percent_contamination``: ``(100.0 * c) / max(t, 1)`` of equal integers in float64: equal.
* the three ``q`` layers: ``|got - ref| <= 2^-23 |ref| + 1e-12`` -- one float32 rounding (2^-24 relative) of a float64
  result whose summation order differs from numpy's by at most T terms of 2^-53; together they sum to 1 within the same
  bound where the gene is known and are exactly 0 where it is not.
* ``contamination_flow``: float64 on both sides, sums of non-negative terms in different orders: 1e-9 relative, entry by
  entry (an entry that is zero is zero on both sides).
* ``reference_table``: float64 on both sides: 1e-12 relative; ``n`` and ``n_cells`` equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segger_amd import phenograph as pg                                # noqa: E402
from segger_amd import postprocess as pp                               # noqa: E402
from segger_amd import validation as va                                # noqa: E402
from segger_amd.neighbors import knn_grid                              # noqa: E402

import contamination_cases as cc                                       # noqa: E402

NAMES = [s[0] for s in cc.SPECS]
Q_LAYERS = ("q_self", "q_neighbor", "q_background")
EXACT = ("contamination", "contaminated", "total", "percent_contamination")


def device_inputs(case, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    expr = {"indptr": t(case["indptr"]), "indices": t(case["indices"]), "counts": t(case["counts"]),
            "gene_ids": torch.arange(cc.N_COLS, dtype=torch.int32, device=dev), "centroid": t(case["xy"])}
    return expr, t(case["labels"]), t(case["weight"]), t(case["gene_map"])


@pytest.fixture(scope="module")
def runs(cuda):
    """name -> (case, oracle, device inputs, result): every case is run once and shared, never modified"""
    out = {}
    for name, (case, oracle) in cc.cases().items():
        expr, labels, weight, gene_map = device_inputs(case, cuda)
        got = va.calculate_contamination(expr, labels, weight, gene_map, n_neighbors=case["k"],
                                         max_neighbor_distance=case["max_distance"], **case["params"])
        out[name] = (case, oracle, (expr, labels, weight, gene_map), got)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_frequencies_are_bit_equal(cuda, runs, name):
    case, oracle, (expr, labels, _, _), got = runs[name]
    freq, counts = va.neighbor_frequencies(expr["centroid"], labels, case["k"], case["n_types"], case["max_distance"])
    assert counts.dtype == torch.int32 and freq.dtype == torch.float32
    assert np.array_equal(counts.cpu().numpy(), oracle["counts"])
    assert np.array_equal(freq.cpu().numpy(), oracle["freq"])
    assert torch.equal(got["neighbor_frequencies"], freq)
    raw, _ = va.neighbor_frequencies(expr["centroid"], labels, case["k"], case["n_types"], case["max_distance"], normalize=False)
    assert np.array_equal(raw.cpu().numpy(), oracle["counts"].astype(np.float32))


@pytest.mark.parametrize("name", NAMES)
def test_posterior_matches_the_oracle(runs, name):
    case, oracle, _, got = runs[name]
    for key in EXACT:
        want = oracle[key]
        assert got[key].dtype == {np.dtype("int32"): torch.int32, np.dtype("int64"): torch.int64,
                                  np.dtype("float64"): torch.float64}[want.dtype], key
        assert np.array_equal(got[key].cpu().numpy(), want), key
    known = ~oracle["missing"]
    total = np.zeros(len(known))
    for key in Q_LAYERS:
        q = got[key]
        assert q.dtype == torch.float32
        q, want = q.cpu().numpy().astype(np.float64), oracle[key]
        err = np.abs(q - want)
        bound = 2.0 ** -23 * np.abs(want) + 1e-12
        assert np.all(err <= bound), (key, float((err / bound).max()))
        assert np.all(q[~known] == 0.0), key
        total += q
    assert np.all(np.abs(total[known] - 1.0) <= 2.0 ** -23 + 1e-12)
    assert np.all(got["contamination"].cpu().numpy()[~known] == 0)


@pytest.mark.parametrize("name", NAMES)
def test_flow_matches_the_oracle(runs, name):
    case, oracle, (expr, labels, weight, gene_map), got = runs[name]
    flow = va.contamination_flow(expr, got["contamination"], labels, weight, gene_map)
    assert flow.dtype == torch.float64 and tuple(flow.shape) == oracle["flow"].shape
    assert np.allclose(flow.cpu().numpy(), oracle["flow"], rtol=1e-9, atol=0.0)       # entry by entry; zeros are exact
    assert torch.equal(flow, va.contamination_flow(expr, got["contamination"], labels, weight, gene_map))
    if name == NAMES[0]:
        with pytest.raises(ValueError, match="No shared genes"):
            va.contamination_flow(expr, got["contamination"], labels, weight, torch.full_like(gene_map, -1))


@pytest.mark.parametrize("name", NAMES)
def test_same_bits_again_and_from_a_permuted_search(cuda, runs, name):
    case, _, (expr, labels, weight, gene_map), got = runs[name]
    kw = dict(n_neighbors=case["k"], max_neighbor_distance=case["max_distance"], **case["params"])
    again = va.calculate_contamination(expr, labels, weight, gene_map, **kw)
    n = len(case["xy"])
    perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(cuda)
    nbr_p, dist_p = knn_grid(expr["centroid"][perm], case["k"], return_dist=True)
    back = torch.cat([perm, perm.new_full((1,), n)])                  # the padding id stays the padding id
    nbr, dist = torch.empty_like(nbr_p), torch.empty_like(dist_p)
    nbr[perm], dist[perm] = back[nbr_p.long()].int(), dist_p
    permuted = va.calculate_contamination(expr, labels, weight, gene_map, knn=(nbr, dist), **kw)
    for key, value in got.items():
        assert torch.equal(value, again[key]), key
        assert torch.equal(value, permuted[key]), key


@pytest.mark.parametrize("name", ["t3_maxdist", "t33_g600"])
def test_reference_table_matches_the_oracle(runs, name):
    case, _, (expr, labels, _, _), _ = runs[name]
    T = case["n_types"]
    want = cc.reference_table_oracle(case["indptr"], case["indices"], case["counts"], case["labels"], T, cc.N_COLS, min_counts=2)
    got = va.reference_table(expr["indptr"], expr["indices"], expr["counts"], labels, T, n_genes=cc.N_COLS)
    assert int(want["n"].sum()) > 100
    for key in ("n", "n_cells"):
        assert got[key].dtype == torch.int64 and np.array_equal(got[key].cpu().numpy(), want[key]), key
    for key in ("me", "pc", "weight"):
        assert got[key].dtype == torch.float64
        assert np.allclose(got[key].cpu().numpy(), want[key], rtol=1e-12, atol=0.0), key
    inferred = va.reference_table(expr["indptr"], expr["indices"], expr["counts"], labels, T)["weight"]      # n_genes = max + 1
    assert torch.equal(got["weight"][:, :inferred.shape[1]], inferred)


def test_empty_matrix_and_no_cells(cuda):
    i32 = dict(dtype=torch.int32, device=cuda)
    expr = {"indptr": torch.zeros(4, dtype=torch.int64, device=cuda), "indices": torch.zeros(0, **i32),
            "counts": torch.zeros(0, **i32), "gene_ids": torch.arange(5, **i32),
            "centroid": torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0]], dtype=torch.float64, device=cuda)}
    out = va.calculate_contamination(expr, torch.tensor([0, 1, -1], **i32), torch.ones(2, 5, dtype=torch.float64, device=cuda),
                                     n_neighbors=2)
    assert out["q_self"].numel() == 0 and out["total"].tolist() == [0, 0, 0] and out["percent_contamination"].tolist() == [0.0] * 3
    assert out["neighbor_frequencies"].tolist() == [[0.5, 0.5], [0.5, 0.5], [1.0, 0.0]]


def _chain(t, dev):
    """expression_matrix -> phenograph labels -> reference_table on the same matrix -> calculate_contamination"""
    n, G = len(t["xy"]), cc.TISSUE_GENES
    m = len(t["tx_cell"])
    result = {"cell_encoding": torch.from_numpy(t["tx_cell"]).to(dev), "gene": torch.from_numpy(t["tx_gene"]).to(dev),
              "similarity": torch.ones(m, dtype=torch.float32, device=dev),
              "similarity_threshold": torch.zeros(m, dtype=torch.float64, device=dev),
              "row_index": torch.arange(m, dtype=torch.int64, device=dev)}
    tx_xy = torch.from_numpy(t["xy"][t["tx_home"]]).to(dev)
    expr = pp.expression_matrix(result, xy=tx_xy, n_cells=n, n_genes=G)
    assert int(expr["cell_ids"].numel()) == n and int(expr["gene_ids"].numel()) == G
    rows = torch.repeat_interleave(torch.arange(n, device=dev), expr["indptr"].diff())
    total = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, rows, expr["counts"].double())
    dense = torch.zeros(n, G, dtype=torch.float64, device=dev)
    dense[rows, expr["indices"].long()] = torch.log1p(expr["counts"].double() / total[rows] * 1e4)
    labels = pg.phenograph(dense, 15, 1.0, min_size=10)
    T = int(labels.max()) + 1
    assert 2 <= T <= 256
    table = va.reference_table(expr["indptr"], expr["indices"], expr["counts"], labels, T, n_genes=G)
    out = va.calculate_contamination(expr, labels, table["weight"])
    return float(out["percent_contamination"].mean()), T


def test_end_to_end_swapped_segmentation_scores_worse(cuda):
    clean = cc.tissue(2000, seed=1)
    swapped = cc.swap_fraction(clean, 0.2)
    a, ta = _chain(clean, cuda)
    b, tb = _chain(swapped, cuda)
    assert b > a
