"""The CPU oracles of tests/contamination_cases.py on their own (no GPU): hand-computed values on a 3-cell example, the
frequency oracle against ``scipy.sparse.csr_matrix`` on the KDTree output (the reference's own construction), both input
margins for every case, and the semantic check -- moving 20 % of every cell's counts to the nearest cell of the other type
raises the mean ``percent_contamination`` and puts the flow table's weight off the diagonal."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial import cKDTree

import contamination_cases as cc


def test_three_cells_by_hand():
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [10.0, 0.0]])
    labels = np.array([0, 1, 0], dtype=np.int32)
    freq, counts = cc.neighbor_frequencies_oracle(xy, labels, 2, 2, max_distance=5.0)
    assert counts.tolist() == [[1, 1], [1, 1], [1, 0]]                  # cell 2 is 9 away from its nearest: only itself
    assert freq.dtype == np.float32 and freq.tolist() == [[0.5, 0.5], [0.5, 0.5], [1.0, 0.0]]
    # cell 0: gene 0 x 3, gene 1 x 1; cell 1: gene 1 x 4; cell 2: gene 0 x 2.  L = [[1, 0], [0, 2]] (eps = 0).
    indptr = np.array([0, 2, 3, 4], dtype=np.int64)
    indices = np.array([0, 1, 1, 0], dtype=np.int32)
    cnt = np.array([3, 1, 4, 2], dtype=np.int32)
    weight = np.array([[1.0, 0.0], [0.0, 2.0]])
    gene_map = np.array([0, 1], dtype=np.int32)
    out = cc.contamination_oracle(indptr, indices, cnt, gene_map, labels, freq, weight, eps=0.0)
    # A = [2/3, 1/3], back = A @ L = [2/3, 2/3], alpha_background * back = 1/30
    # (0, g0): self 0.8 * 1, neigh 0.15 * (0.5 * L[1, 0] = 0), back 1/30 -> / (5/6): 0.96, 0, 0.04
    # (0, g1): self 0.8 * L[0, 1] = 0, neigh 0.15 * (0.5 * 2) = 0.15, back 1/30 -> / (11/60): 0, 9/11, 2/11: flagged
    # (1, g1): self 0.8 * 2, neigh 0.15 * (0.5 * L[0, 1] = 0), back 1/30 -> / (49/30): 48/49, 0, 1/49
    # (2, g0): freq [1, 0] with the own slot zeroed: neigh 0 -> as (0, g0)
    assert np.allclose(out["q_self"], [0.96, 0.0, 48 / 49, 0.96], rtol=1e-15, atol=0)
    assert np.allclose(out["q_neighbor"], [0.0, 9 / 11, 0.0, 0.0], rtol=1e-15, atol=0)
    assert np.allclose(out["q_background"], [0.04, 2 / 11, 1 / 49, 0.04], rtol=1e-14, atol=0)
    assert out["contamination"].tolist() == [0, 1, 0, 0]
    assert out["contaminated"].tolist() == [1, 0, 0] and out["total"].tolist() == [4, 4, 2]
    assert out["percent_contamination"].tolist() == [25.0, 0.0, 0.0]
    # W = weight^T row-normalised = identity; cell 0 gives 25 % to donor 1; host type 0 = cells 0 and 2: mean 12.5
    flow = cc.flow_oracle(indptr, indices, cnt, out["contamination"], gene_map, labels, weight)
    assert flow.tolist() == [[0.0, 0.0], [12.5, 0.0]]
    with pytest.raises(ValueError, match="No shared genes"):
        cc.flow_oracle(indptr, indices, cnt, out["contamination"], np.array([-1, -1], dtype=np.int32), labels, weight)
    # a cell without a type: P_self = eps, every type is a neighbouring type; a gene the table lacks: zeros, never flagged
    out = cc.contamination_oracle(indptr, indices, cnt, np.array([0, -1], dtype=np.int32), np.array([-1, 1, 0], dtype=np.int32),
                                  freq, weight, eps=0.0)
    assert out["q_self"][0] == 0.0 and out["contamination"].tolist() == [3, 0, 0, 0]
    assert out["q_self"][1] == out["q_neighbor"][1] == out["q_background"][1] == 0.0 and bool(out["missing"][1])
    # labelled cells are 1 and 2: A = [1/2, 1/2], back[g0] = 1/2; (0, g0): neigh 0.15 * 0.5 * 1, back 0.05 * 0.5
    assert np.isclose(out["q_neighbor"][0], 0.075 / 0.1, rtol=1e-15) and np.isclose(out["q_background"][0], 0.25, rtol=1e-15)


def test_reference_table_by_hand():
    # cells 0, 1 of type 0, cell 2 of type 1, cell 3 unlabelled; 2 genes
    indptr = np.array([0, 2, 3, 5, 6], dtype=np.int64)
    indices = np.array([0, 1, 0, 0, 1, 1], dtype=np.int32)
    cnt = np.array([3, 1, 2, 1, 4, 9], dtype=np.int32)
    kind = np.array([0, 0, 1, -1], dtype=np.int32)
    t = cc.reference_table_oracle(indptr, indices, cnt, kind, 2, 2, min_counts=2)
    assert t["n"].tolist() == [[2, 0], [0, 1]] and t["n_cells"].tolist() == [2, 1]
    me00 = (np.log1p(3 / (4 / 1e4)) + np.log1p(2 / (2 / 1e4))) / 2
    assert np.allclose(t["me"], [[me00, 0.0], [0.0, np.log1p(4 / (5 / 1e4))]], rtol=1e-15)
    assert t["pc"].tolist() == [[1.0, 0.0], [0.0, 1.0]] and np.array_equal(t["weight"], t["pc"] * t["me"])


@pytest.mark.parametrize("name", ["t1_k1", "t64_k_is_n", "t256_g7"])
def test_frequency_oracle_is_the_references_csr_matrix(name):
    case, oracle = cc.cases()[name]                                     # cases without unlabelled cells: csr_matrix accepts them
    n, k, md = len(case["xy"]), case["k"], case["max_distance"]
    dist, idx = cKDTree(case["xy"]).query(case["xy"], k=k)
    host = np.repeat(np.arange(n, dtype=np.int32), k)
    neigh, dists = idx.reshape(-1), dist.reshape(-1)
    if md is not None:
        host, neigh = host[dists <= md], neigh[dists <= md]
    cols = case["labels"][neigh].astype(np.int32)
    mat = sp.csr_matrix((np.ones_like(cols, dtype=np.int32), (host, cols)), shape=(n, case["n_types"]))
    assert np.array_equal(mat.toarray(), oracle["counts"])
    sums = np.asarray(mat.sum(1)).ravel().astype(np.float64)
    sums[sums == 0] = 1.0
    assert np.array_equal(np.asarray(mat.multiply(1.0 / sums[:, None]).todense()).astype(np.float32), oracle["freq"])


def test_margins_and_coverage_of_every_case():
    seen_lengths, seen_types, routes = set(), set(), set()
    for name, (case, oracle) in cc.cases().items():
        cc.check_margins(case, oracle)
        assert case["xy"].astype(np.float32).astype(np.float64).tolist() == case["xy"].tolist(), name      # float32-exact
        lengths = np.diff(case["indptr"])
        seen_lengths.update(lengths.tolist())
        seen_types.add(case["n_types"])
        missing_row = len(cc.ROW_LENGTHS)
        assert oracle["missing"][case["indptr"][missing_row]:case["indptr"][missing_row + 1]].all(), name
        assert oracle["contaminated"][missing_row] == 0 and oracle["total"][missing_row] > 0
        T, G = case["weight"].shape
        tp = (T + 3) // 4 * 4
        routes.add((G * (tp if (tp // 4) % 2 else tp + 4) + 4 * tp) * 4 <= 65536)
        if case["max_distance"] is not None and name in ("t3_maxdist", "t256_g7"):                          # the isolated cell
            assert oracle["counts"][-1].sum() == 1
    assert set(cc.ROW_LENGTHS) <= seen_lengths and seen_types == {1, 3, 33, 64, 65, 256}
    assert routes == {True, False}                                      # the table in LDS and through L2
    assert {c["k"] for c, _ in cc.cases().values()} >= {1, 48} and len(cc.cases()["t64_k_is_n"][0]["xy"]) == 48
    assert any((c["labels"] < 0).any() for c, _ in cc.cases().values())
    assert cc.cases()["t65_no_back"][0]["params"]["alpha_background"] == 0.0
    assert np.all(cc.cases()["t65_no_back"][1]["q_background"] == 0.0)


def test_swapping_counts_raises_contamination():
    clean = cc.tissue(400, seed=0)
    swapped = cc.swap_fraction(clean, 0.2)
    assert len(swapped["tx_cell"]) == len(clean["tx_cell"]) and (swapped["tx_cell"] != np.sort(clean["tx_cell"])).mean() > 0.1
    a, b = cc.tissue_scores(clean, clean["kind"]), cc.tissue_scores(swapped, swapped["kind"])
    assert b["percent_contamination"].mean() > a["percent_contamination"].mean() + 5.0
    flow = b["flow"]
    assert flow[0, 1] > flow[1, 1] and flow[1, 0] > flow[0, 0] and min(flow[0, 1], flow[1, 0]) > 5.0
