"""The oracles of tests/phenograph_cases.py checked on the CPU, before the device is compared with them: the kNN oracle
against sklearn's brute force, the Jaccard oracle against plain set arithmetic, the Louvain restatement against the
networkx quality bar of the golden file (its worst seed minus its own seed-to-seed spread), and the relabelling against
the reference's rule written with pandas-free counting."""
import numpy as np
import pytest

import phenograph_cases as pc


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.GOLDEN)


@pytest.fixture(scope="module")
def louvain_runs():
    return {name: (case, pc.louvain_oracle(*case[:3], case[3])) for name, case in pc.louvain_cases().items()}


def test_knn_oracle_agrees_with_sklearn(golden):
    neighbors = pytest.importorskip("sklearn.neighbors")
    for name, (d, mean) in pc.REAL_CASES.items():
        X = golden[f"X_{name}"]
        assert np.array_equal(X, pc.mixture_case(700, d, mean, seed=11 + d))           # the golden holds the generator's inputs
        idx, d2 = pc.knn_oracle(X, pc.REAL_K)
        dist, sk_idx = neighbors.NearestNeighbors(n_neighbors=pc.REAL_K, algorithm="brute").fit(
            X.astype(np.float64)).kneighbors(X.astype(np.float64))
        assert np.array_equal(sk_idx, golden[f"sk_idx_{name}"])
        # sklearn's own expanded form (float64) differs from the direct sum by its cancellation: |x|^2 * 2^-50
        assert np.abs(dist ** 2 - d2).max() <= (X.astype(np.float64) ** 2).sum(axis=1).max() * 2.0 ** -46
        if mean == 0.0:
            assert np.array_equal(np.sort(idx, axis=1), np.sort(sk_idx, axis=1))
    X = pc.lattice_case(60, 2, seed=1, span=1)                                        # ties everywhere: by index
    idx, d2 = pc.knn_oracle(X, 7)
    assert (np.diff(d2, axis=1) >= 0).all() and ((np.diff(d2, axis=1) > 0) | (np.diff(idx, axis=1) > 0)).all()


def test_centred_cases_keep_the_neighbour_set_check_alive(golden):
    for name, (d, mean) in pc.REAL_CASES.items():
        if mean == 0.0:
            X = golden[f"X_{name}"]
            D = np.sort(pc.dist2_f64(X), axis=1)
            assert ((D[:, pc.REAL_K] - D[:, pc.REAL_K - 1]) > 2 * pc.knn_tau(X)).mean() >= 0.95


def test_jaccard_oracle_against_brute_force_sets():
    idx = pc.knn_oracle(pc.mixture_case(80, 3, 0.0, seed=4), 5)[0]
    indptr, indices, weight = pc.jaccard_oracle(idx)
    n = len(idx)
    A = np.zeros((n, n), dtype=bool)
    A[np.repeat(np.arange(n), idx.shape[1]), idx.reshape(-1)] = True
    A = (A | A.T) | np.eye(n, dtype=bool)                                             # closed neighbourhoods
    rows = np.repeat(np.arange(n), np.diff(indptr))
    assert np.array_equal(np.argwhere(A & ~np.eye(n, dtype=bool)), np.stack([rows, indices], axis=1))
    want = [(A[u] & A[v]).sum() / (A[u] | A[v]).sum() for u, v in zip(rows, indices)]
    assert np.array_equal(weight, np.asarray(want))


def test_louvain_oracle_quality_structure_and_bits(golden, louvain_runs):
    pytest.importorskip("networkx")
    for name, ((indptr, indices, weight, gamma), (labels, q, stats)) in louvain_runs.items():
        assert abs(q - pc.modularity_f64(indptr, indices, weight, labels, gamma)) <= 1e-12, name
        comp = pc.components(indptr, indices)
        assert all(len(set(comp[labels == c].tolist())) == 1 for c in set(labels.tolist())), name
        assert stats["rounds"] <= pc.MAX_ROUNDS * max(stats["levels"], 1)
        again = pc.louvain_oracle(indptr, indices, weight, gamma)
        assert np.array_equal(labels, again[0]) and q == again[1]
        if name in pc.QUALITY_CASES:
            nxq = golden[f"nxq_{name}"]
            print(f"{name}: oracle Q {q:.6f}, networkx {nxq.min():.6f} .. {nxq.max():.6f}")
            assert q >= nxq.min() - (nxq.max() - nxq.min()), name
    assert pc.same_partition(louvain_runs["ring"][1][0], np.arange(48) // 6)
    assert pc.same_partition(louvain_runs["triangles"][1][0], [0, 0, 0, 1, 1, 1])
    assert louvain_runs["edgeless"][1][1] == 0.0 and len(set(louvain_runs["edgeless"][1][0].tolist())) == 7


def test_networkx_numbers_in_the_golden_are_networkx_s(golden):
    nx = pytest.importorskip("networkx")
    indptr, indices, weight, gamma = pc.louvain_cases()["planted300"]
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    G = nx.Graph()
    G.add_nodes_from(range(len(indptr) - 1))
    G.add_weighted_edges_from((int(u), int(v), float(x)) for u, v, x in zip(rows, indices, weight) if u < v)
    parts = nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=0)
    assert abs(nx.community.modularity(G, parts, weight="weight", resolution=gamma) - golden["nxq_planted300"][0]) <= 1e-12
    labels = np.empty(len(indptr) - 1, dtype=np.int64)
    for c, part in enumerate(parts):
        labels[list(part)] = c
    # the golden holds networkx's partition measured by modularity_exact: one partition, one value, to the bit
    assert pc.modularity_exact(weight, rows, indices.astype(np.int64), labels, gamma) == golden["nxq_planted300"][0]


def test_relabelling_rule_and_the_min_size_quirk():
    labels = np.array([4, 4, 4, 1, 1, 8, 8, 3])                       # sizes 3, 2, 2, 1; the tie goes to vertex 3's cluster
    assert pc.relabel_oracle(labels, -1).tolist() == [0, 0, 0, 1, 1, 2, 2, 3]
    assert pc.relabel_oracle(labels, 1).tolist() == [0, 0, 0, 1, 1, 2, 2, -1]
    assert pc.relabel_oracle(labels, 2).tolist() == [0, 0, 0, -1, -1, -1, -1, -1]
    # the quirk: ranks are taken before the filter, so survivors keep their rank even when a bigger cluster... cannot be
    # filtered (size > min_size is monotone in rank) -- what the quirk leaves is that labels are NOT renumbered after it
    assert pc.relabel_oracle(np.array([0, 1, 1, 2, 2, 2]), 5).tolist() == [-1] * 6
