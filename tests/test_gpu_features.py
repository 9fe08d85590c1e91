"""Boundary and gene features on the device (``segger_amd.features``, ``csrc/features.hip``) against the numpy oracle of
tests/features_cases.py and the sklearn golden file tests/golden/features_small.npz.

Tolerances, all derived (EPS = 2^-52):

* ``S`` and ``s``: every term is non-negative, so a float64 sum of ``n`` terms in any order is within ``n EPS`` of the
  entry itself; kernel and BLAS oracle together: ``2 (n_rows + 4) EPS max|S|``.
* ``corr``: 1e-10 absolute -- sums of <= 5 000 terms give <= 1.1e-12, times the cancellation factor of the moment form,
  ``1 + mean^2 / var <= 101`` (tests/test_features_cases.py asserts both conditions on the oracle alone).
* ``sparse_project``: <= 200 products per row, 1e-12 of the largest entry in float64; float32 output adds one rounding,
  2^-24 of the largest entry.
* embeddings against the golden: ``max(1e3 x solver_noise, 1e-12 x scale)`` per component, signs included --
  ``solver_noise`` is what two CPU solvers differ by, 1e3 the amplification ``1 / gap`` of the asserted gap condition;
  at k = 128 through ``X X^T``.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segger_amd import _lib                                            # noqa: E402
from segger_amd import features as ft                                  # noqa: E402
from segger_amd import postprocess as pp                               # noqa: E402

from features_cases import (CASES, EPS, GOLDEN_K, features_oracle, gram_oracle, low_rank_case, relative_gaps,  # noqa: E402
                            to_csr)
from test_postprocess import fake_predictions                          # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features_small.npz")
SLAB = _lib.FEATURES_SLAB_ROWS
N_ROWS = (1, 3, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 5)


def on(cuda, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays)


def expr_of(cuda, dense):
    indptr, indices, values = on(cuda, *to_csr(dense))
    return {"indptr": indptr, "indices": indices, "counts": values,
            "gene_ids": torch.arange(dense.shape[1], dtype=torch.int32, device=cuda)}


def bits(t):
    return t.cpu().view(torch.int64)


def gram_matrix(n, g, seed):
    """counts with empty rows, rows of more than 64 entries (g > 64), one row holding every gene and, for g > 128, a gene
    tile (columns 64 .. 127) that no row but that one touches"""
    rng = np.random.default_rng(seed)
    dense = rng.poisson(0.4, (n, g)) * (rng.random((n, g)) < 0.5)
    dense[rng.random(n) < 0.1] = 0                                     # rows with 0 entries
    if n >= 3:
        dense[1] = rng.integers(1, 5, g)                               # more than 64 entries when g > 64
        dense[2] = 0
    if g > 128:
        dense[:, 64:128] = 0
    every = n // 2
    dense[every] = rng.integers(1, 4, g)                               # a row holding every gene
    if g > 128 and n > 1:
        dense[every, 64:128] = 0                                       # ... and with n > 1 the middle tile stays untouched
    weight = rng.uniform(0.25, 4.0, n)
    weight[rng.random(n) < 0.15] = 0.0
    weight[every] = 1.5
    return dense.astype(np.int64), weight


def check_gram(cuda, dense, weight):
    n, g = dense.shape
    indptr, indices, values = on(cuda, *to_csr(dense))
    S, s = ft.sparse_gram(indptr, indices, values, torch.from_numpy(weight).to(cuda), g)
    torch.cuda.synchronize()
    want_S, want_s = gram_oracle(dense, weight)
    got_S, got_s = S.cpu().numpy(), s.cpu().numpy()
    tol = 2 * (n + 4) * EPS
    err_S, err_s = np.abs(got_S - want_S).max(), np.abs(got_s - want_s).max()
    print(f"gram n={n} g={g}: |dS| {err_S:.3e} (tol {tol * max(np.abs(want_S).max(), 1e-300):.3e}) |ds| {err_s:.3e}")
    assert err_S <= tol * np.abs(want_S).max() and err_s <= tol * np.abs(want_s).max()
    assert torch.equal(bits(S), bits(S.T.contiguous()))                # bit-symmetric
    return S, s


@pytest.mark.parametrize("g", [1, 15, 16, 17, 40, 136, 160])
def test_gram_matches_the_oracle(cuda, g):
    for n in N_ROWS:
        assert _lib.load().segger_features_gram_slabs(n, g) == -(-n // SLAB)
        dense, weight = gram_matrix(n, g, seed=100 * g + n % 97)
        assert g <= 64 or n < 3 or (dense[1] > 0).sum() > 64
        assert g <= 128 or n == 1 or not dense[:, 64:128].any()
        check_gram(cuda, dense, weight)


def test_gram_all_weights_zero_but_one(cuda):
    dense, _ = gram_matrix(SLAB + 7, 70, seed=5)
    weight = np.zeros(dense.shape[0])
    row = SLAB + 2                                                     # in the second slab
    dense[row] = np.arange(70) % 3 + 1
    weight[row] = 0.5
    S, s = check_gram(cuda, dense, weight)
    x = 0.5 * dense[row].astype(np.float64)
    assert np.array_equal(S.cpu().numpy(), np.outer(x, x)) and np.array_equal(s.cpu().numpy(), x)      # one term: exact
    weight[:] = 0.0
    S, s = check_gram(cuda, dense, weight)
    assert not S.any() and not s.any()                                 # every row left out: zeros


def test_gram_bits(cuda):
    dense, weight = gram_matrix(3 * SLAB + 5, 136, seed=6)
    indptr, indices, values = on(cuda, *to_csr(dense))
    w = torch.from_numpy(weight).to(cuda)
    S0, s0 = ft.sparse_gram(indptr, indices, values, w, 136)
    S1, s1 = ft.sparse_gram(indptr, indices, values, w, 136)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        S2, s2 = ft.sparse_gram(indptr, indices, values, w, 136)
    side.synchronize()
    torch.cuda.synchronize()
    assert S0.abs().max() > 0
    for S, s in ((S1, s1), (S2, s2)):
        assert torch.equal(bits(S0), bits(S)) and torch.equal(bits(s0), bits(s))
    assert torch.equal(bits(S0), bits(S0.T.contiguous()))


@pytest.fixture(scope="module")
def project_case():
    rng = np.random.default_rng(21)
    n, g = 300, 200
    dense = rng.poisson(0.3, (n, g)).astype(np.int64)                  # <= 200 products per row
    dense[0] = 0                                                       # an empty row
    dense[1] = rng.integers(1, 6, g)                                   # a full one
    weight = rng.uniform(0.1, 3.0, n)
    weight[5] = 0.0
    V = rng.normal(size=(g, 256))
    offset = rng.normal(size=256)
    return dense, weight, V, offset


@pytest.mark.parametrize("k", [1, 7, 8, 16, 64, 128, 129, 256])
def test_project_matches_the_oracle(cuda, project_case, k):
    dense, weight, V, offset = project_case
    V, offset = np.ascontiguousarray(V[:, :k]), offset[:k]
    indptr, indices, values = on(cuda, *to_csr(dense))
    w, Vd, od = on(cuda, weight, V, offset)
    want = (dense.astype(np.float64) @ V) * weight[:, None] - offset
    scale = np.abs(want).max()
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-12 + 2.0 ** -24)):
        got = ft.sparse_project(indptr, indices, values, w, Vd, od, dtype)
        again = ft.sparse_project(indptr, indices, values, w, Vd, od, dtype)
        torch.cuda.synchronize()
        assert got.dtype == dtype and got.shape == (dense.shape[0], k)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(f"project k={k} {dtype}: err {err:.3e} tol {tol * scale:.3e}")
        assert err <= tol * scale
        assert torch.equal(got, again)                                 # no NaN in it, and the same bits
        minus = torch.from_numpy(-offset).to(dtype)
        assert torch.equal(got[5].cpu(), minus)                        # w = 0: exactly -offset
        assert np.abs(got[0].cpu().numpy().astype(np.float64) + offset).max() <= tol * scale           # an empty row


@pytest.mark.parametrize("name", sorted(CASES))
def test_features_match_the_oracle(cuda, name):
    builder, args = CASES[name]
    dense = builder()
    want = features_oracle(dense, **args)
    got = ft.expression_features(expr_of(cuda, dense), args["k"], args["cells_min_counts"], args["genes_min_counts"], torch.float64)
    assert all(torch.is_tensor(v) and v.is_cuda for v in got.values())
    assert np.array_equal(got["gene_keep"].cpu().numpy(), want["gene_keep"])
    assert np.array_equal(got["n_counts"].cpu().numpy(), want["n_counts"])
    assert np.array_equal(got["filtered"].cpu().numpy(), want["filtered"])
    assert float(got["target_sum"]) == want["target_sum"]
    err = np.abs(got["corr"].cpu().numpy() - want["corr"]).max()
    print(f"{name}: |d corr| {err:.3e}")
    assert err <= 1e-10
    k = args["k"]
    assert got["X_pca"].shape == (dense.shape[0], k) and got["X_corr"].shape == (int(want["gene_keep"].sum()), k)
    ev = np.abs(got["explained_variance"].cpu().numpy() - want["explained_variance"]).max()
    assert ev <= 1e-10 * want["explained_variance"][0] * 101


def test_zero_variance_gene_is_an_exact_zero(cuda):
    dense = low_rank_case(300, 20, 4, seed=31, n_shallow=30)
    dense[:, 7] = 0
    dense[270:, :] = 0
    dense[270:, 7] = 2                                                 # gene 7: 60 counts, all in cells of 2 counts
    got = ft.expression_features(expr_of(cuda, dense), 4, 10, 20, torch.float64)
    keep = got["gene_keep"].cpu().numpy()
    assert keep[7] and not got["filtered"][270:].any() and int(got["filtered"].sum()) > 200
    pos = int(keep[:7].sum())
    corr = got["corr"].cpu().numpy()
    assert not corr[pos].any() and not corr[:, pos].any()              # row, column and diagonal: exactly 0
    live = np.delete(np.arange(corr.shape[0]), pos)
    assert np.abs(np.diag(corr)[live] - 1).max() <= 4 * EPS
    want = features_oracle(dense, 4, 10, 20)
    assert np.abs(corr - want["corr"]).max() <= 1e-10
    assert np.isfinite(got["X_pca"].cpu().numpy()).all() and np.isfinite(got["X_corr"].cpu().numpy()).all()


def test_every_cell_filtered_out(cuda):
    dense = low_rank_case(50, 12, 3, seed=32, depth=4.0)
    with pytest.raises(ValueError, match=r"min\(n_samples, n_features\)=0 with svd_solver='full'"):
        ft.expression_features(expr_of(cuda, dense), 2, cells_min_counts=10_000, genes_min_counts=1)
    with pytest.raises(ValueError, match="svd_solver='full'"):         # more components than kept genes
        ft.expression_features(expr_of(cuda, dense), 13, cells_min_counts=1, genes_min_counts=1)
    indptr, indices, values = on(cuda, *to_csr(dense))
    S, s = ft.sparse_gram(indptr, indices, values, torch.zeros(50, dtype=torch.float64, device=cuda), 12)
    assert not S.any() and not s.any()
    S, s = ft.sparse_gram(indptr[:1], indices[:0], values[:0], torch.zeros(0, dtype=torch.float64, device=cuda), 12)
    assert S.shape == (12, 12) and not S.any() and not s.any()         # no rows at all


def test_features_match_the_golden(cuda):
    g = np.load(GOLDEN)
    small, big = GOLDEN_K
    expr = expr_of(cuda, g["counts"].astype(np.int64))
    args = (int(g["cells_min_counts"]), int(g["genes_min_counts"]))
    got = ft.expression_features(expr, small, *args, out_dtype=torch.float64)
    for key in ("gene_keep", "n_counts", "filtered"):
        assert np.array_equal(got[key].cpu().numpy(), g[key]), key
    assert float(got["target_sum"]) == float(g["target_sum"])
    err = np.abs(got["corr"].cpu().numpy() - g["corr"]).max()
    print(f"golden: |d corr| {err:.3e}")
    assert err <= 1e-10
    for name in ("X_corr", "X_pca"):
        want = g[f"{name}_{small}"]
        noise = float(g[f"solver_noise_{name[2:]}_{small}"])
        tol = max(1e3 * noise, 1e-12 * np.abs(want).max())
        err = np.abs(got[name].cpu().numpy() - want).max()
        print(f"golden k={small} {name}: err {err:.3e} tol {tol:.3e} (solver_noise {noise:.3e})")
        assert err <= tol
    ev = np.abs(got["explained_variance"].cpu().numpy() - g[f"explained_variance_{small}"]).max()
    assert ev <= 1e-10 * 101 * g[f"explained_variance_{small}"][0]
    # float32, the default: one rounding of the same numbers
    f32 = ft.expression_features(expr, small, *args)["X_pca"]
    assert f32.dtype == torch.float32
    assert (f32.double() - got["X_pca"]).abs().max().item() <= 2.0 ** -24 * got["X_pca"].abs().max().item()
    # k = 128: the inner gaps are below the condition, X X^T is what is defined
    got = ft.expression_features(expr, big, *args, out_dtype=torch.float64)
    rows = torch.from_numpy(g["pca128_rows"]).to(cuda)
    for name, mine in (("X_corr", got["X_corr"]), ("X_pca", got["X_pca"][rows])):
        want = g[f"{name}_{big}"]
        want = want @ want.T
        noise = float(g[f"solver_noise_{name[2:]}_{big}"])
        tol = max(1e3 * noise, 1e-12 * np.abs(want).max())
        err = np.abs((mine @ mine.T).cpu().numpy() - want).max()
        print(f"golden k={big} {name} X X^T: err {err:.3e} tol {tol:.3e} (solver_noise {noise:.3e})")
        assert err <= tol


def test_accumulator_to_features_end_to_end(cuda):
    """accumulator -> expression() -> expression_features on a seeded slide (50 cells x 12 genes).  The counts are exact;
    ``corr`` is within 1e-10; the embeddings are compared through X X^T, which the gap at position k defines: the moment
    form is within 1e-10 (relative) of the covariance and Davis-Kahan amplifies that by 1 / gap, so the bound is
    ``1e-10 / gap_k`` of the largest entry, with k the largest of 2 .. 6 whose gap is >= 1e-2 on the oracle."""
    acc = pp.SegmentationAccumulator(4000, cuda)
    for batch in fake_predictions(0):
        acc.update(*batch)
    expr = acc.expression()
    dense = pp.expression_to_scipy(expr)[0].toarray().astype(np.int64)
    probe = features_oracle(dense, 6, 20, 30)
    gaps = [min(relative_gaps(probe["sv_corr"], k)[-1], relative_gaps(probe["sv_cells"], k)[-1]) for k in range(2, 7)]
    k = max(k for k, gap in zip(range(2, 7), gaps) if gap >= 1e-2)
    gap = gaps[k - 2]
    want = features_oracle(dense, k, 20, 30)
    got = ft.expression_features(expr, k, 20, 30, torch.float64)
    for key in ("gene_keep", "n_counts", "filtered"):
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
    assert float(got["target_sum"]) == want["target_sum"]
    assert np.abs(got["corr"].cpu().numpy() - want["corr"]).max() <= 1e-10
    for name in ("X_corr", "X_pca"):
        a, b = got[name].cpu().numpy(), want[name]
        err, scale = np.abs(a @ a.T - b @ b.T).max(), np.abs(b @ b.T).max()
        print(f"end to end k={k} gap {gap:.3e} {name}: err {err:.3e} tol {1e-10 / gap * scale:.3e}")
        assert err <= 1e-10 / gap * scale


def test_cluster_cosine_similarity(cuda):
    rng = np.random.default_rng(41)
    emb = rng.normal(size=(200, 16))
    labels = rng.integers(0, 5, 200)
    labels[:20] = -1                                                   # removed cells: a cluster like any other
    labels[199] = 9                                                    # a cluster of one member
    unit = emb / np.maximum(np.linalg.norm(emb, axis=1, keepdims=True), 1e-8)
    ids = np.unique(labels)
    means = np.stack([unit[labels == c].mean(axis=0) for c in ids])
    want = means @ means.T
    got = ft.cluster_cosine_similarity(*on(cuda, emb, labels))
    assert got.is_cuda and got.shape == (7, 7)
    assert np.abs(got.cpu().numpy() - want).max() <= 200 * EPS         # unit vectors, sums of <= 200 terms
    assert abs(got[6, 6].item() - 1.0) <= 4 * EPS                      # the single member: its own unit vector
    f32 = ft.cluster_cosine_similarity(torch.from_numpy(emb).float().to(cuda), torch.from_numpy(labels).to(cuda))
    assert f32.dtype == torch.float32 and np.abs(f32.cpu().numpy() - want).max() <= 200 * 2.0 ** -23
