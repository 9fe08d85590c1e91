"""Writes tests/golden/features_small.npz: what the reference's own library calls return for one seeded count matrix
(1 500 cells x 136 genes, tests/features_cases.py GOLDEN_CASE), on the CPU in float64.

``setup_anndata`` (``src/segger/data/utils/anndata.py:184-259``) calls, in this order: scanpy's ``normalize_total`` (absent
here: restated as ``X / (n_counts / target_sum)``), ``np.corrcoef`` + ``np.nan_to_num``,
``sklearn.decomposition.PCA(n_components=k, random_state=0).fit_transform(C)`` (at ``G <= 500`` the auto solver is the
exact one) and cuML's PCA fit on the filtered rows / transform of all rows (absent here: sklearn's
``PCA(svd_solver="full")``, the same exact decomposition with sklearn's sign rule).  Those calls are made literally below.

``solver_noise_*`` is the largest difference between two independent CPU float64 routes to the same embedding -- numpy's
SVD of the centred matrix against scipy's ``eigh`` of its Gram matrix: the floor under any comparison of a third solver.

Run from the repository root:  python tests/golden/make_features_golden.py"""
import os
import sys

import numpy as np
import scipy.linalg
from sklearn.decomposition import PCA

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from features_cases import GOLDEN_CASE, GOLDEN_K, exact_pca, flip_rows  # noqa: E402

PCA128_ROWS = np.arange(0, 1500, 12)               # X_pca at k = 128 is stored for these rows only (the file stays small)


def eigh_route(fit, k, transform=None):
    """the same scores as ``exact_pca`` through scipy's eigh of the Gram matrix of the centred data"""
    mean = fit.mean(axis=0)
    centred = fit - mean
    _, vecs = scipy.linalg.eigh(centred.T @ centred)
    Vt = vecs[:, ::-1].T[:k]
    V = (Vt * flip_rows(Vt)[:, None]).T
    return ((fit if transform is None else transform) - mean) @ V


def main():
    builder, args = GOLDEN_CASE
    dense = builder()
    assert dense.max() < 256
    gene_keep = dense.sum(axis=0) >= args["genes_min_counts"]
    X = dense[:, gene_keep]
    n_counts = X.sum(axis=1)
    filtered = n_counts >= args["cells_min_counts"]
    target_sum = float(np.median(n_counts[filtered]))
    per_cell = n_counts / target_sum
    per_cell = per_cell + (per_cell == 0)
    norm = X / per_cell[:, None]
    F = norm[filtered]
    C = np.corrcoef(np.asarray(F).T)
    C = np.nan_to_num(C, 0, posinf=True, neginf=True)
    out = {"counts": dense.astype(np.uint8), "gene_keep": gene_keep, "n_counts": n_counts.astype(np.int64), "filtered": filtered,
           "target_sum": np.float64(target_sum), "corr": C, "pca128_rows": PCA128_ROWS,
           "cells_min_counts": np.int64(args["cells_min_counts"]), "genes_min_counts": np.int64(args["genes_min_counts"])}
    for k in GOLDEN_K:
        X_corr = PCA(n_components=k, random_state=0).fit_transform(C)
        model = PCA(n_components=k, svd_solver="full").fit(F)
        X_pca = model.transform(norm)
        mine_corr, mine_pca = exact_pca(C, k)[0], exact_pca(F, k, norm)[0]
        other_corr, other_pca = eigh_route(C, k), eigh_route(F, k, norm)
        if k == GOLDEN_K[0]:                                           # per component, signs included
            out[f"X_corr_{k}"], out[f"X_pca_{k}"] = X_corr, X_pca
            out[f"explained_variance_{k}"] = model.explained_variance_
            out[f"solver_noise_corr_{k}"] = np.float64(np.abs(mine_corr - other_corr).max())
            out[f"solver_noise_pca_{k}"] = np.float64(np.abs(mine_pca - other_pca).max())
            assert np.abs(X_corr - mine_corr).max() < 1e-9 and np.abs(X_pca - mine_pca).max() < 1e-9
        else:                                                          # through X X^T: no component is singled out
            rows = PCA128_ROWS
            out[f"X_corr_{k}"], out[f"X_pca_{k}"] = X_corr, X_pca[rows]
            out[f"solver_noise_corr_{k}"] = np.float64(np.abs(mine_corr @ mine_corr.T - other_corr @ other_corr.T).max())
            out[f"solver_noise_pca_{k}"] = np.float64(np.abs(mine_pca[rows] @ mine_pca[rows].T - other_pca[rows] @ other_pca[rows].T).max())
        print(k, {n: float(out[n]) for n in out if n.startswith("solver_noise") and n.endswith(str(k))})
    path = os.path.join(HERE, "features_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
