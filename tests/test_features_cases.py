"""The CPU oracle of the feature tests (tests/features_cases.py) on a case small enough to work out by hand, and the
CONDITIONS the GPU tolerances of tests/test_gpu_features.py rest on, asserted on the oracle alone for every case:

* every kept gene of non-zero variance has ``mean^2 / var <= 100`` over the filtered cells, so the moment form of the
  covariance loses at most a factor 101 to cancellation (the 1e-10 bound on ``corr``);
* the relative gap ``(sigma_i - sigma_{i+1}) / sigma_1`` of every compared component is ``>= 1e-3``, for the correlation
  matrix and for the cells, so a component is defined to ~1e3 x the solvers' own noise.  At ``k = 128`` the inner gaps
  are far smaller: only ``X X^T`` is compared there, under the gap at position ``k`` alone."""
import os

import numpy as np
import pytest

from features_cases import (CASES, GOLDEN_CASE, GOLDEN_K, features_oracle, gram_oracle, hand_case, moment_condition,
                            relative_gaps, to_csr)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features_small.npz")
MAX_MOMENT, MIN_GAP = 100.0, 1e-3


def test_hand_written_four_cells_three_genes():
    o = features_oracle(hand_case(), k=2, cells_min_counts=2, genes_min_counts=1)
    assert o["gene_keep"].tolist() == [True] * 3 and o["n_counts"].tolist() == [4, 4, 4, 1]
    assert o["filtered"].tolist() == [True, True, True, False] and o["target_sum"] == 4.0
    assert o["norm_filtered"].tolist() == [[2, 0, 2], [0, 4, 0], [1, 1, 2]]
    S, s = gram_oracle(hand_case(), [1.0, 1.0, 1.0, 0.0])
    assert S.tolist() == [[5, 1, 6], [1, 17, 2], [6, 2, 8]] and s.tolist() == [3, 5, 4]
    want = np.array([[1.0, -2 / np.sqrt(13 / 3), 1 / np.sqrt(4 / 3)],
                     [-2 / np.sqrt(13 / 3), 1.0, -7 / np.sqrt(52)],
                     [1 / np.sqrt(4 / 3), -7 / np.sqrt(52), 1.0]])
    assert np.abs(o["corr"] - want).max() < 4 * 2.0 ** -52
    # the fourth cell is projected although it took no part in the fit: (4, 0, 0) - mean on the components
    mean = np.array([1.0, 5 / 3, 4 / 3])
    assert np.allclose(np.linalg.norm(o["X_pca"][3]), np.linalg.norm(np.array([4.0, 0, 0]) - mean))    # rank 2: nothing is lost
    assert o["X_pca"].shape == (4, 2) and o["X_corr"].shape == (3, 2)
    indptr, indices, values = to_csr(hand_case())
    assert indptr.tolist() == [0, 2, 3, 6, 7] and indices.tolist() == [0, 2, 1, 0, 1, 2, 0] and values.tolist() == [2, 2, 4, 1, 1, 2, 1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_conditions_of_the_gpu_tolerances(name):
    builder, args = CASES[name]
    o = features_oracle(builder(), **args)
    k = args["k"]
    assert not o["gene_keep"].all() or name == "hand"                 # the seeded cases drop genes and cells
    assert not o["filtered"].all()
    assert k <= min(o["gene_keep"].sum(), o["filtered"].sum())
    assert moment_condition(o["norm_filtered"]) <= MAX_MOMENT
    assert relative_gaps(o["sv_corr"], k).min() >= MIN_GAP
    assert relative_gaps(o["sv_cells"], k).min() >= MIN_GAP
    assert o["filtered"].sum() <= 5000                                # the length of a sum behind the 1e-10 bound


def test_conditions_of_the_golden_case():
    builder, args = GOLDEN_CASE
    small, big = GOLDEN_K
    o = features_oracle(builder(), k=big, **args)
    assert moment_condition(o["norm_filtered"]) <= MAX_MOMENT and o["filtered"].sum() <= 5000
    for sv in (o["sv_corr"], o["sv_cells"]):
        assert relative_gaps(sv, small).min() >= MIN_GAP
        assert relative_gaps(sv, big)[-1] >= MIN_GAP                  # at k = 128 the gap at position k alone
        assert relative_gaps(sv, big).min() < MIN_GAP                 # ... because the inner ones fail it


def test_golden_file_agrees_with_the_oracle():
    g = np.load(GOLDEN)
    builder, args = GOLDEN_CASE
    small, big = GOLDEN_K
    dense = builder()
    assert np.array_equal(g["counts"], dense)                         # the seeded builder still gives the stored matrix
    o = features_oracle(dense, k=small, **args)
    for key in ("gene_keep", "n_counts", "filtered"):
        assert np.array_equal(g[key], o[key]), key
    assert float(g["target_sum"]) == o["target_sum"]
    assert np.abs(g["corr"] - o["corr"]).max() < 1e-14
    assert np.abs(g[f"X_corr_{small}"] - o["X_corr"]).max() <= 1e3 * float(g[f"solver_noise_corr_{small}"])
    assert np.abs(g[f"X_pca_{small}"] - o["X_pca"]).max() <= 1e3 * float(g[f"solver_noise_pca_{small}"])
    assert np.abs(g[f"explained_variance_{small}"] - o["explained_variance"]).max() < 1e-9
    ob = features_oracle(dense, k=big, **args)
    rows = g["pca128_rows"]
    assert np.abs(g[f"X_corr_{big}"] @ g[f"X_corr_{big}"].T - ob["X_corr"] @ ob["X_corr"].T).max() <= 1e3 * float(g[f"solver_noise_corr_{big}"])
    assert np.abs(g[f"X_pca_{big}"] @ g[f"X_pca_{big}"].T - ob["X_pca"][rows] @ ob["X_pca"][rows].T).max() <= 1e3 * float(g[f"solver_noise_pca_{big}"])
    assert os.path.getsize(GOLDEN) < 1 << 20
