"""Phenograph clustering on the device (``segger_amd.phenograph``, ``csrc/phenograph.hip``) against the numpy oracles of
tests/phenograph_cases.py and the sklearn / networkx numbers of tests/golden/phenograph_small.npz.

Bounds, all derived, none tuned:

* lattice kNN cases (|x| <= 8 integers, d <= 256): every product and sum is an integer below 2^24, exact in fp32, so
  ``idx`` and ``dist2`` EQUAL the float64 oracle, ties by index.
* real-valued kNN: a returned neighbour may be farther than the true k-th only by the fp32 expanded form's error,
  ``tau_i = 4 (d + 3) 2^-24 (|x_i|^2 + max_j |x_j|^2)`` (``phenograph_cases.knn_tau``); the returned ``dist2`` is a direct
  fp32 sum of d squares: ``2 d 2^-24`` relative.  Rows whose true gap ``d2_{k+1} - d2_k`` exceeds ``2 tau_i`` must return
  sklearn's neighbour set (at least 95 % of the rows of the centred cases: asserted by the golden's generator).
* Jaccard: integers and one float64 division: bit-equal.  Louvain: the partition of the numpy restatement, ``Q`` within
  1e-12 of it and of ``Q`` recomputed from the labels; on the quality cases ``Q`` is no lower than networkx's worst seed
  minus networkx's own seed-to-seed spread."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segger_amd import _lib                                            # noqa: E402
from segger_amd import features as ft                                  # noqa: E402
from segger_amd import phenograph as pg                                # noqa: E402
from segger_amd import postprocess as pp                               # noqa: E402

import phenograph_cases as pc                                          # noqa: E402
from test_postprocess import fake_predictions                          # noqa: E402


def on(cuda, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays)


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.GOLDEN)


@pytest.fixture(scope="module")
def louvain_ref():
    """name -> (case, oracle labels, oracle Q): computed once, shared, never modified"""
    return {name: (case,) + pc.louvain_oracle(*case[:3], case[3])[:2] for name, case in pc.louvain_cases().items()}


# ------------------------------------------------------------------ kNN ---
LATTICE = [(1, 3, 1), (2, 4, 2), (5, 1, 5), (6, 5, 5), (127, 31, 10), (128, 32, 33), (129, 33, 64), (300, 128, 10),
           (1000, 256, 10), (1000, 4, 2), (300, 3, 1), (64, 5, 64), (65, 16, 64)]                   # (N, d, k)


@pytest.mark.parametrize("n,d,k", LATTICE)
def test_knn_lattice_is_exact(cuda, n, d, k):
    X = pc.lattice_case(n, d, seed=n + d + k, span=8 if d > 5 else 2)                              # low d: many duplicates
    want_idx, want_d2 = pc.knn_oracle(X, k)
    idx, d2 = pg.knn_bruteforce(on(cuda, X)[0], k)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (n, k)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), want_d2)


def test_knn_more_copies_than_k(cuda):
    """k + 3 copies of row 0 at the end: the lowest indices win, and the late copies do not find themselves"""
    k, n = 5, 200
    X = pc.lattice_case(n, 7, seed=3, copies=k + 2)
    want_idx, want_d2 = pc.knn_oracle(X, k)
    assert n - 1 not in want_idx[n - 1]                                # self dropped out of its own row
    idx, d2 = pg.knn_bruteforce(on(cuda, X)[0], k)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(d2.cpu().numpy(), want_d2.astype(np.float32))
    assert (d2[n - 1] == 0).all() and idx[n - 1].tolist() == [0] + list(range(n - k - 2, n - k + 2))


@pytest.mark.parametrize("name", list(pc.REAL_CASES))
def test_knn_real_valued(cuda, golden, name):
    X, k = golden[f"X_{name}"], pc.REAL_K
    n, d = X.shape
    idx_t, d2_t = pg.knn_bruteforce(on(cuda, X)[0], k)
    idx, d2 = idx_t.cpu().numpy().astype(np.int64), d2_t.cpu().numpy().astype(np.float64)
    D = pc.dist2_f64(X)
    tau = pc.knn_tau(X)
    kth = np.sort(D, axis=1)
    true_d2 = np.take_along_axis(D, idx, axis=1)
    excess = (true_d2 - kth[:, k - 1:k]).max(axis=1)
    print(f"{name}: worst excess over the k-th true distance / tau = {(excess / tau).max():.3e}")
    assert (excess <= tau).all()
    rel = np.abs(d2 - true_d2) / np.maximum(true_d2, np.finfo(np.float64).tiny)
    print(f"{name}: dist2 relative error {rel[true_d2 > 0].max():.3e} against {2 * d * pc.U24:.3e}")
    assert (np.abs(d2 - true_d2) <= 2 * d * pc.U24 * true_d2).all()
    order = d2_t.cpu().numpy().view(np.int32).astype(np.int64) * (1 << 32) + idx       # (dist2 bits, idx), dist2 >= 0
    assert (np.diff(order, axis=1) > 0).all()                          # sorted, and no index twice in a row
    assert all(len(set(row)) == k for row in idx.tolist())
    if pc.REAL_CASES[name][1] == 0.0:
        clear = (kth[:, k] - kth[:, k - 1]) > 2 * tau
        assert clear.mean() >= 0.95
        got, want = np.sort(idx[clear], axis=1), np.sort(golden[f"sk_idx_{name}"].astype(np.int64)[clear], axis=1)
        assert np.array_equal(got, want)


def test_knn_bits_call_to_call_and_on_a_side_stream(cuda, golden):
    X = on(cuda, golden["X_mix128"])[0]
    a = pg.knn_bruteforce(X, 10)
    b = pg.knn_bruteforce(X, 10)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        c = pg.knn_bruteforce(X, 10)
    side.synchronize()
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1].view(torch.int32), other[1].view(torch.int32))


# ------------------------------------------------------------------ Jaccard ---
def jaccard_tables():
    rng = np.random.default_rng(9)
    knn = pc.knn_oracle(pc.mixture_case(150, 4, 0.0, seed=2), 6)[0]                  # mutual and one-way edges
    star = np.stack([np.arange(600), np.zeros(600, dtype=np.int64)], axis=1)         # everyone names vertex 0
    only_self = np.arange(40).reshape(-1, 1)
    isolated = np.stack([np.arange(50), np.arange(50)], axis=1)
    isolated[:20, 1] = rng.integers(0, 20, 20)                                       # vertices 20.. stay isolated
    return {"knn": knn, "star": star, "k1": only_self, "isolated": isolated}


@pytest.mark.parametrize("name", ["knn", "star", "k1", "isolated"])
def test_jaccard_graph_bit_equal(cuda, name):
    table = jaccard_tables()[name].astype(np.int32)
    indptr, indices, weight = pc.jaccard_oracle(table)
    got = pg.jaccard_graph(on(cuda, table)[0])
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float64
    assert np.array_equal(got[0].cpu().numpy(), indptr) and np.array_equal(got[1].cpu().numpy(), indices)
    assert np.array_equal(got[2].cpu().numpy().view(np.int64), weight.view(np.int64))
    if name == "k1":
        assert not indptr.any() and got[1].numel() == 0
    if name == "star":
        assert indptr[1] == 599
    rows = np.repeat(np.arange(len(table)), np.diff(indptr))
    w = {(int(u), int(v)): x for u, v, x in zip(rows, indices, got[2].cpu().numpy().view(np.int64))}
    assert all(w[(v, u)] == x for (u, v), x in w.items())


# ------------------------------------------------------------------ Louvain ---
IDENTITY = ["ring", "triangles", "edge", "edgeless", "planted300", "jaccard600_g1", "jaccard600_g2", "k88"]


@pytest.mark.parametrize("name", IDENTITY)
def test_louvain_equals_the_numpy_restatement(cuda, golden, louvain_ref, name):
    (indptr, indices, weight, gamma), want_labels, want_q = louvain_ref[name]
    dev = on(cuda, indptr, indices, weight)
    labels, q, stats = pg.louvain(*dev, resolution=gamma, return_stats=True)
    again, q2 = pg.louvain(*dev, resolution=gamma)
    assert labels.dtype == torch.int32 and torch.equal(labels, again) and q == q2
    lab = labels.cpu().numpy()
    print(f"{name}: {lab.max() + 1 if len(lab) else 0} clusters, Q {q!r} (oracle {want_q!r}), {stats}")
    assert stats["rounds"] <= pc.MAX_ROUNDS * stats["levels"] and stats["levels"] <= 100
    assert pc.same_partition(lab, want_labels)
    assert abs(q - want_q) <= 1e-12
    assert abs(q - pc.modularity_f64(indptr, indices, weight, lab, gamma)) <= 1e-12
    comp = pc.components(indptr, indices)
    assert all(len(set(comp[lab == c].tolist())) == 1 for c in set(lab.tolist()))    # no cluster spans two components
    if name == "ring":
        assert pc.same_partition(lab, np.arange(48) // 6)
    if name == "triangles":
        assert len(set(comp.tolist())) == 2 and pc.same_partition(lab, [0, 0, 0, 1, 1, 1])
    if name == "edgeless":
        assert q == 0.0 and sorted(lab.tolist()) == list(range(len(lab)))
    if name in pc.QUALITY_CASES:
        assert np.array_equal(golden[f"indptr_{name}"], indptr) and np.array_equal(golden[f"weight_{name}"], weight)
        nxq = golden[f"nxq_{name}"]
        bar = nxq.min() - (nxq.max() - nxq.min())
        print(f"{name}: Q {q:.6f} against networkx {nxq.min():.6f} .. {nxq.max():.6f}, bar {bar:.6f}")
        assert q >= bar


def test_blobs_graph_is_disconnected_and_clusters_stay_inside_components(cuda):
    X = np.concatenate([pc.mixture_case(120, 4, 0.0, seed=s, n_types=1) + 1000.0 * s for s in range(3)]).astype(np.float32)
    table = pc.knn_oracle(X, 6)[0]
    indptr, indices, weight = pc.jaccard_oracle(table)
    comp = pc.components(indptr, indices)
    assert len(set(comp.tolist())) >= 3                                # really disconnected
    labels, q = pg.louvain(*on(cuda, indptr, indices, weight), resolution=1.0)
    lab = labels.cpu().numpy()
    assert all(len(set(comp[lab == c].tolist())) == 1 for c in set(lab.tolist()))
    assert abs(q - pc.modularity_f64(indptr, indices, weight, lab, 1.0)) <= 1e-12


# ------------------------------------------------------------------ phenograph / anndata_features ---
@pytest.mark.parametrize("min_size", [-1, 100])
def test_phenograph_relabels_as_the_reference(cuda, golden, min_size):
    X = golden["X_mix16"].astype(np.float64)
    got = pg.phenograph(on(cuda, X)[0], 10, resolution=1.0, min_size=min_size)
    centred = (X - X.mean(axis=0)).astype(np.float32)
    idx = pg.knn_bruteforce(on(cuda, centred)[0], 10)[0].cpu().numpy()
    raw = pc.louvain_oracle(*pc.jaccard_oracle(idx), 1.0)[0]
    want = pc.relabel_oracle(raw, min_size)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    if min_size == 100:
        sizes = np.bincount(pc.relabel_oracle(raw, -1))
        assert set(got.cpu().numpy().tolist()) == {r for r, s in enumerate(sizes) if s > 100} | ({-1} if (sizes <= 100).any() else set())
    assert np.array_equal(pg.relabel_by_size(on(cuda, np.array([5, 5, 2, 2, 9, 9, 9, 7]))[0], 1).cpu().numpy(),
                          np.array([1, 1, 2, 2, 0, 0, 0, -1]))       # tie: the cluster of vertex 0 first; rank 3 filtered


def test_anndata_features_end_to_end(cuda):
    acc = pp.SegmentationAccumulator(4000, cuda)
    for batch in fake_predictions(0):
        acc.update(*batch)
    expr = acc.expression()
    got = ft.anndata_features(expr, 6, 20, 30, cells_clusters_n_neighbors=5, genes_clusters_n_neighbors=3, out_dtype=torch.float64)
    again = ft.anndata_features(expr, 6, 20, 30, cells_clusters_n_neighbors=5, genes_clusters_n_neighbors=3, out_dtype=torch.float64)
    base = ft.expression_features(expr, 6, 20, 30, torch.float64)
    for key, value in base.items():
        assert torch.equal(got[key], value), key
    filtered = got["filtered"]
    assert int(filtered.sum()) >= 5
    cells, genes = got["cell_clusters"], got["gene_clusters"]
    assert cells.dtype == genes.dtype == torch.int64
    assert bool((cells[~filtered] == -1).all()) and genes.numel() == int(got["gene_keep"].sum()) and bool((genes >= 0).all())
    want_cells = pg.phenograph(got["X_pca"][filtered], 5, 2.0, min_size=100)
    assert torch.equal(cells[filtered], want_cells)                    # fewer than 100 cells a cluster here: all -1
    assert torch.equal(genes, pg.phenograph(got["X_corr"], 3, 2.0, min_size=-1))
    with ft.deterministic_sums():                                      # the function's own index_add_ is atomic otherwise
        assert torch.equal(got["cell_cluster_similarities"], ft.cluster_cosine_similarity(got["X_pca"], cells))
        assert torch.equal(got["gene_cluster_similarities"], ft.cluster_cosine_similarity(got["X_corr"], genes))
    for key in ("cell_clusters", "gene_clusters", "cell_cluster_similarities", "gene_cluster_similarities"):
        assert torch.equal(got[key], again[key]), key


# ------------------------------------------------------------------ arguments ---
def test_bad_arguments(cuda):
    X = torch.zeros(10, 4, device=cuda)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        pg.knn_bruteforce(X, 11)
    with pytest.raises(ValueError, match="k = 65"):
        pg.knn_bruteforce(torch.zeros(100, 4, device=cuda), 65)
    with pytest.raises(ValueError, match="d = 257"):
        pg.knn_bruteforce(torch.zeros(10, 257, device=cuda), 2)
    with pytest.raises(ValueError):
        pg.knn_bruteforce(X, 0)
    for call in (lambda: pg.knn_bruteforce(torch.zeros(10, 4), 2), lambda: pg.jaccard_graph(torch.zeros(4, 2, dtype=torch.int32)),
                 lambda: pg.louvain(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)),
                 lambda: pg.phenograph(torch.zeros(10, 4), 2)):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
            call()
