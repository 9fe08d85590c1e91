"""Shared by the feature tests: the CPU oracle of ``segger_amd.features`` and the seeded case builders.

The reference computes these numbers in ``setup_anndata`` (``src/segger/data/utils/anndata.py:184-259``) with scanpy,
cuML and sklearn; scanpy and cuML are absent here, so the oracle is an independent dense restatement in float64 of what
those calls do: ``normalize_total`` (divide every row by ``n_counts / target_sum``), ``np.corrcoef`` of the filtered
rows, ``nan_to_num``, and an exact PCA by ``np.linalg.svd`` of the centred matrix with sklearn's sign rule
(``svd_flip(u_based_decision=False)``: the largest-magnitude loading of every component is positive).  The golden file
tests/golden/features_small.npz holds what sklearn itself returns."""
import numpy as np

EPS = 2.0 ** -52


def to_csr(dense):
    """canonical CSR of a dense integer matrix, with the dtypes ``expression_matrix`` returns"""
    dense = np.asarray(dense)
    rows, cols = np.nonzero(dense)                                     # row-major: ascending columns inside a row
    indptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=dense.shape[0]), out=indptr[1:])
    return indptr, cols.astype(np.int32), dense[rows, cols].astype(np.int32)


def gram_oracle(dense, weight):
    """``S = sum_r w_r^2 x_r x_r^T`` and ``s = sum_r w_r x_r`` of the rows of weight != 0, dense float64"""
    w = np.asarray(weight, dtype=np.float64)
    use = w != 0.0
    Xw = np.asarray(dense, dtype=np.float64)[use] * w[use, None]
    return Xw.T @ Xw, Xw.sum(axis=0)


def flip_rows(Vt):
    """sklearn's svd_flip(u_based_decision=False): the sign of every ROW of Vt so that its largest |entry| is positive"""
    top = np.argmax(np.abs(Vt), axis=1)
    sign = np.sign(Vt[np.arange(Vt.shape[0]), top])
    sign[sign == 0] = 1.0
    return sign


def exact_pca(fit, k, transform=None):
    """-> (scores of ``transform`` (default: ``fit``) on the top ``k`` components, all singular values, mean)"""
    mean = fit.mean(axis=0)
    U, sv, Vt = np.linalg.svd(fit - mean, full_matrices=False)
    sign = flip_rows(Vt)
    V = (Vt * sign[:, None])[:k].T
    target = fit if transform is None else transform
    return (target - mean) @ V, sv, mean


def features_oracle(dense, k, cells_min_counts, genes_min_counts):
    """-> dict named like the outputs of ``expression_features`` plus ``norm_filtered`` (the matrix ``corrcoef`` sees) and
    the singular values ``sv_corr`` (of the centred correlation matrix) and ``sv_cells`` (of the centred filtered rows)."""
    dense = np.asarray(dense, dtype=np.int64)
    gene_keep = dense.sum(axis=0) >= genes_min_counts
    X = dense[:, gene_keep]
    n_counts = X.sum(axis=1)
    filtered = n_counts >= cells_min_counts
    target_sum = float(np.median(n_counts[filtered]))
    per_cell = n_counts / target_sum                                   # normalize_total: X / (counts / target_sum),
    per_cell = per_cell + (per_cell == 0)                              # an empty cell is divided by 1
    norm = X / per_cell[:, None]
    F = norm[filtered]
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = np.corrcoef(F.T)
    corr = np.nan_to_num(np.atleast_2d(corr), nan=0.0, posinf=1.0, neginf=1.0)
    X_corr, sv_corr, _ = exact_pca(corr, k)
    X_pca, sv_cells, mean = exact_pca(F, k, norm)
    return {"gene_keep": gene_keep, "n_counts": n_counts, "filtered": filtered, "target_sum": target_sum, "corr": corr,
            "X_corr": X_corr, "X_pca": X_pca, "norm_filtered": F, "sv_corr": sv_corr, "sv_cells": sv_cells, "mean": mean,
            "explained_variance": sv_cells[:k] ** 2 / (F.shape[0] - 1)}


def moment_condition(F):
    """max over the genes of non-zero variance of mean^2 / var: the cancellation factor of the moment form of the
    covariance, ``(S - s s^T / n) / (n - 1)``, is ``1 + mean^2 / var``"""
    mean, var = F.mean(axis=0), F.var(axis=0, ddof=1)
    live = var > 0
    return float(np.max(mean[live] ** 2 / var[live]))


def relative_gaps(sv, k):
    """(sigma_i - sigma_{i+1}) / sigma_1 for the ``k`` compared components i = 0 .. k - 1"""
    sv = np.r_[np.asarray(sv, dtype=np.float64), 0.0]
    return (sv[:k] - sv[1:k + 1]) / sv[0]


def low_rank_case(n_cells, n_genes, rank, seed, depth=60.0, n_shallow=0, n_rare=0, strength=1.0):
    """Poisson counts of a low-rank log-rate model: ``rank`` factors of geometrically falling strength (distinct singular
    values), log-normal depths around ``depth`` counts per cell; the last ``n_shallow`` cells get about 3 counts (they
    fail ``cells_min_counts``) and the last ``n_rare`` genes a rate 200 times lower (they fail ``genes_min_counts``)."""
    rng = np.random.default_rng(seed)
    scale = strength * 0.8 ** np.arange(rank)
    logit = (rng.normal(size=(n_cells, rank)) * scale) @ rng.normal(size=(rank, n_genes)) + 0.6 * rng.normal(size=n_genes)
    if n_rare:
        logit[:, n_genes - n_rare:] -= np.log(200.0)
    rate = np.exp(logit - logit.max(axis=1, keepdims=True))
    rate /= rate.sum(axis=1, keepdims=True)
    cell_depth = rng.lognormal(np.log(depth), 0.4, n_cells)
    if n_shallow:
        cell_depth[n_cells - n_shallow:] = 3.0
    return rng.poisson(rate * cell_depth[:, None]).astype(np.int64)


def hand_case():
    """Four cells x three genes, ``cells_min_counts = 2``, ``genes_min_counts = 1``:

        counts = [[2, 0, 2],      n_counts = 4
                  [0, 4, 0],                 4
                  [1, 1, 2],                 4
                  [1, 0, 0]]                 1 -> not filtered

    Gene totals 4, 5, 4: all kept.  target_sum = median(4, 4, 4) = 4, so the filtered rows keep their values (weight 1) and
    the fourth row is scaled by 4 to [4, 0, 0].  Over the three filtered rows s = [3, 5, 4] and
    S = [[5, 1, 6], [1, 17, 2], [6, 2, 8]], hence cov = (S - s s^T / 3) / 2 =
    [[1, -2, 1], [-2, 13/3, -7/3], [1, -7/3, 4/3]] and
    corr01 = -2 / sqrt(13/3), corr02 = 1 / sqrt(4/3), corr12 = -7 / sqrt(52)."""
    return np.array([[2, 0, 2], [0, 4, 0], [1, 1, 2], [1, 0, 0]], dtype=np.int64)


# name -> (builder, oracle arguments); k is chosen so that the oracle alone meets the gap condition
# (tests/test_features_cases.py asserts it)
CASES = {
    "small": (lambda: low_rank_case(400, 40, 10, seed=11, n_shallow=9, n_rare=3), dict(k=8, cells_min_counts=10, genes_min_counts=20)),
    "medium": (lambda: low_rank_case(3000, 160, 20, seed=12, n_shallow=40, n_rare=6), dict(k=16, cells_min_counts=10, genes_min_counts=100)),
    "hand": (hand_case, dict(k=2, cells_min_counts=2, genes_min_counts=1)),
}
GOLDEN_CASE = (lambda: low_rank_case(1500, 136, 20, seed=19, n_shallow=25, n_rare=6), dict(cells_min_counts=10, genes_min_counts=100))
GOLDEN_K = (16, 128)               # 16: compared per component; 128: through X X^T (129 genes are kept, and the normalised
                                   # rows all sum to target_sum, so sigma_129 is 0 and the gap at position 128 is wide)
