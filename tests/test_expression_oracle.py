"""The CPU oracle of the expression matrix (tests/expression_cases.py) against a case small enough to type out, and the
seeded slides the GPU tests use: the oracle alone must give them a non-trivial matrix."""
import numpy as np
import pytest

from segger_amd import postprocess as pp

from expression_cases import expression_oracle
from test_postprocess import fake_predictions

NAN = float("nan")


def test_hand_written_six_rows():
    #        row  0     1     2     3     4     5
    cell = [2, -1, 0, 2, 0, 2]           # row 1: no cell
    gene = [1, 1, 3, 1, 0, 2]            # gene 2 loses its only row (row 5), gene 0 has no threshold (row 4)
    sim = [0.75, 0.9, 0.5, 0.25, 0.9, 0.1]
    thr = [0.25, 0.25, 0.5, 0.25, NAN, 0.5]       # row 2 and row 3: sim == thr, kept
    xy = [[1.0, 2.0], [9.0, 9.0], [4.0, 8.0], [3.0, 6.0], [7.0, 7.0], [5.0, 5.0]]
    o = expression_oracle(cell, gene, sim, thr, xy)
    # kept: rows 0, 2, 3 -> cell 0 owns gene 3 once, cell 2 owns gene 1 twice
    assert o["n_kept"] == 3
    assert o["cell_ids"].tolist() == [0, 2] and o["gene_ids"].tolist() == [1, 3]
    assert o["dense"].tolist() == [[0, 1],
                                   [2, 0]]
    assert o["indptr"].tolist() == [0, 1, 2] and o["indices"].tolist() == [1, 0] and o["counts"].tolist() == [1, 2]
    assert o["mean_similarity"].tolist() == [0.5, 0.5]                 # 0.5; (0.75 + 0.25) / 2
    assert o["cell_count"].tolist() == [1, 2]
    assert o["centroid"].tolist() == [[4.0, 8.0], [2.0, 4.0]]
    assert o["n_max_run"] == 2 and o["n_max_cell"] == 2
    assert all(o[k].dtype == np.int32 for k in ("cell_ids", "gene_ids", "indices", "counts"))
    assert o["indptr"].dtype == np.int64 and o["cell_count"].dtype == np.int64 and o["mean_similarity"].dtype == np.float64


def test_nothing_kept_and_no_rows():
    for o in (expression_oracle([], [], [], [], np.zeros((0, 2))),
              expression_oracle([-1, 3], [0, 0], [0.9, 0.1], [0.5, 0.5], np.ones((2, 2)))):
        assert o["n_kept"] == 0 and o["indptr"].tolist() == [0] and o["cell_ids"].size == 0 and o["gene_ids"].size == 0
        assert o["counts"].size == 0 and o["mean_similarity"].size == 0 and o["centroid"].shape == (0, 2)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_slides_are_not_trivial(seed):
    seg = pp.assign_transcripts_to_cells(fake_predictions(seed))
    o = expression_oracle(seg["cell_encoding"].numpy(), seg["gene"].numpy(), seg["similarity"].numpy(),
                          seg["similarity_threshold"].numpy())
    assert o["counts"].size > 0 and int(o["counts"].max()) > 1
    assert 0 < o["n_kept"] < seg["row_index"].numel()                  # the filter removes something and keeps something
