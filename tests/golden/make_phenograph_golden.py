"""Writes tests/golden/phenograph_small.npz (CPU; needs sklearn and networkx): for the real-valued kNN cases the inputs and
``sklearn.neighbors.NearestNeighbors(algorithm="brute")``'s neighbours and distances; for the Louvain quality cases the
graph and the modularity of ``networkx.community.louvain_communities`` for seeds 0..4.  Data only.

    python tests/golden/make_phenograph_golden.py
"""
import os
import sys

import networkx as nx
import numpy as np
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import phenograph_cases as pc                                          # noqa: E402


def main():
    out = {}
    for name, (d, mean) in pc.REAL_CASES.items():
        X = pc.mixture_case(700, d, mean, seed=11 + d)
        dist, idx = NearestNeighbors(n_neighbors=pc.REAL_K, algorithm="brute").fit(X.astype(np.float64)).kneighbors(
            X.astype(np.float64))
        D = np.sort(pc.dist2_f64(X), axis=1)
        gap_ok = (D[:, pc.REAL_K] - D[:, pc.REAL_K - 1]) > 2.0 * pc.knn_tau(X)
        print(f"{name}: rows with a gap above 2 tau: {gap_ok.mean():.4f}")
        if mean == 0.0:
            assert gap_ok.mean() >= 0.95, "the neighbour-set check would go vacuous"
        out[f"X_{name}"], out[f"sk_dist_{name}"], out[f"sk_idx_{name}"] = X, dist, idx.astype(np.int32)
    cases = pc.louvain_cases()
    for name in pc.QUALITY_CASES:
        indptr, indices, weight, gamma = cases[name]
        rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
        G = nx.Graph()
        G.add_nodes_from(range(len(indptr) - 1))
        G.add_weighted_edges_from((int(u), int(v), float(x)) for u, v, x in zip(rows, indices, weight) if u < v)
        qs = []
        for seed in range(5):
            parts = nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=seed)
            labels = np.empty(len(indptr) - 1, dtype=np.int64)
            for c, part in enumerate(parts):
                labels[list(part)] = c
            # networkx's PARTITION, measured by the evaluator every other Q in the tests comes from (clusters numbered by
            # their smallest vertex, exact fixed-point sums): one partition has one value, to the bit
            qs.append(pc.modularity_exact(weight, rows, indices.astype(np.int64), labels, gamma))
            assert abs(qs[-1] - nx.community.modularity(G, parts, weight="weight", resolution=gamma)) <= 1e-12
        print(f"{name}: networkx Q {qs}")
        out[f"indptr_{name}"], out[f"indices_{name}"], out[f"weight_{name}"] = indptr, indices, weight
        out[f"gamma_{name}"], out[f"nxq_{name}"] = np.float64(gamma), np.asarray(qs)
    np.savez_compressed(pc.GOLDEN, **out)
    print(pc.GOLDEN, os.path.getsize(pc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
