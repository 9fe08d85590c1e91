"""Expression matrix of a segmentation on the device: ``postprocess.expression_matrix`` (``csrc/expression.hip``) against
the numpy oracle of tests/expression_cases.py on CPU copies of the same columns.  Ids, row pointers, column positions and
counts are exact (``torch.equal``); means and centroids are within the float64 summation-order bound of each case,
``n_max_run * 2^-52 * max|v|`` (``assert_matches_oracle`` derives it).  Shapes: the 4 000-transcript slides of
tests/test_postprocess.py, and run lengths around a wave (63 / 64 / 65), a block (257), one pair that owns all of 70 000
rows (the cooperative path) and 262 401 rows: past the 1024 x 256 threads of one grid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segger_amd import _lib                                            # noqa: E402
from segger_amd import postprocess as pp                               # noqa: E402

from expression_cases import (INT_KEYS, as_result, assert_matches_oracle, case_oracle, expression_oracle, make_case,  # noqa: E402
                              random_case, runs_case)
from test_postprocess import fake_predictions                          # noqa: E402

N_TX = 4000


def run_case(cuda, case):
    xy = None if case["xy"] is None else torch.from_numpy(case["xy"]).to(cuda)
    return pp.expression_matrix(as_result(case, cuda), xy, n_cells=case["n_cells"], n_genes=case["n_genes"])


def check_case(cuda, case):
    got = run_case(cuda, case)
    assert all(got[k].is_cuda for k in INT_KEYS + ("mean_similarity",))
    max_coord = float(np.abs(case["xy"]).max()) if case["xy"] is not None and case["xy"].size else 0.0
    want = case_oracle(case)
    assert_matches_oracle(got, want, max_coord=max_coord)
    return got, want


def bit_equal(a, b):
    """every tensor of two results, float64 included, bit for bit"""
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            x, y = a[k].cpu(), b[k].cpu()
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert x.shape == y.shape and torch.equal(x, y), k
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope="module")
def slide_xy():
    return torch.from_numpy(np.random.default_rng(7).uniform(0.0, 4096.0, (N_TX, 2)).astype(np.float32))


def feed(cuda, batches):
    acc = pp.SegmentationAccumulator(N_TX, cuda)
    for b in batches:
        acc.update(*b)
    return acc


def slide_oracle(seg, xy):
    """the oracle on CPU copies of a segmentation() dict; xy [N_TX, 2] is indexed by row_index"""
    rows = seg["row_index"].cpu().numpy()
    return expression_oracle(seg["cell_encoding"].cpu().numpy(), seg["gene"].cpu().numpy(), seg["similarity"].cpu().numpy(),
                             seg["similarity_threshold"].cpu().numpy(), xy.numpy()[rows])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_slides(cuda, slide_xy, seed):
    acc = feed(cuda, fake_predictions(seed))
    got = acc.expression(slide_xy.to(cuda))
    want = slide_oracle(acc.segmentation(), slide_xy)
    assert want["counts"].size > 0 and int(want["counts"].max()) > 1
    assert_matches_oracle(got, want, max_coord=float(slide_xy.abs().max()))
    assert int(got["counts"].sum()) == got["n_kept"] == int(got["cell_count"].sum())
    if seed == 0:                                                     # the scipy round trip
        X, scores, obs_names, var_ids, X_spatial = pp.expression_to_scipy(got)
        assert np.array_equal(X.toarray(), want["dense"]) and X.has_canonical_format and scores.has_canonical_format
        assert np.array_equal(obs_names, want["cell_ids"]) and np.array_equal(var_ids, want["gene_ids"])
        assert scores.shape == X.shape and np.array_equal(scores.indices, X.indices)
        assert np.array_equal(X_spatial, got["centroid"].cpu().numpy())
        import pandas as pd
        obs = pd.DataFrame({"cell_id": [f"cell-{i}" for i in range(60)], "cell_encoding": np.arange(60)})
        names = pp.expression_to_scipy(got, obs)[2]
        assert list(names) == [f"cell-{i}" for i in want["cell_ids"]]
        no_xy = acc.expression()
        assert "centroid" not in no_xy and pp.expression_to_scipy(no_xy)[4] is None
        assert torch.equal(no_xy["counts"], got["counts"]) and torch.equal(no_xy["cell_count"], got["cell_count"])


def test_no_rows_and_nothing_kept(cuda):
    for case in (make_case([], [], [], [], n_cells=5, n_genes=3),
                 make_case([], [], [], []),                           # the id domains default to one cell, one gene
                 make_case([-1, 2, 3, 0], [0, 1, 2, 0], [0.9, 0.1, np.nan, 0.7], [0.5, 0.5, 0.5, np.nan])):
        got, _ = check_case(cuda, case)
        assert got["n_kept"] == 0 and got["indptr"].tolist() == [0]
        assert got["cell_ids"].numel() == 0 and got["gene_ids"].numel() == 0 and got["counts"].numel() == 0
        assert got["centroid"].shape == (0, 2)


def test_one_row(cuda):
    got, _ = check_case(cuda, make_case([3], [2], [0.5], [0.25]))
    assert got["cell_ids"].tolist() == [3] and got["gene_ids"].tolist() == [2] and got["indptr"].tolist() == [0, 1]
    assert got["indices"].tolist() == [0] and got["counts"].tolist() == [1] and got["mean_similarity"].tolist() == [0.5]


def test_run_lengths_around_a_wave_and_a_block(cuda):
    got, want = check_case(cuda, runs_case([1, 63, 1, 64, 65, 1, 1, 257, 1, 2, 128, 129], seed=3, not_kept=0.3))
    assert sorted(want["counts"].tolist()) == [1, 1, 1, 1, 1, 2, 63, 64, 65, 128, 129, 257]


def test_one_pair_owns_every_row(cuda):
    case = runs_case([70_000], seed=4)
    got, want = check_case(cuda, case)
    assert got["counts"].tolist() == [70_000] and got["cell_count"].tolist() == [70_000] and want["n_max_run"] == 70_000


def test_past_one_grid(cuda):
    got, want = check_case(cuda, random_case(262_401, 50, 30, seed=5))
    assert got["cell_ids"].numel() == 50 and got["gene_ids"].numel() == 29          # one gene has no threshold
    assert want["n_max_run"] > 64 and int(want["counts"].min()) >= 1


def test_sparse_ids(cuda):
    cells = np.array([0, 17, 18, 400, 401, 800, 999])
    rng = np.random.default_rng(6)
    n = 300
    cell = cells[rng.integers(0, 7, n)]
    gene = rng.integers(0, 40, n) * 2                                # even genes only, 0 .. 78
    gene[gene == 30] = 32
    sim = rng.uniform(0.3, 1.0, n).astype(np.float32)
    thr = np.full(n, 0.25)
    # gene 30 is present only in rows that are not kept; the highest cell and the highest gene (79) are present
    cell = np.r_[cell, 17, -1, 999, 999]
    gene = np.r_[gene, 30, 30, 30, 79]
    sim = np.r_[sim, np.float32(0.1), np.float32(0.9), np.float32(np.nan), np.float32(0.6)]
    thr = np.r_[thr, 0.25, 0.25, 0.25, 0.25]
    got, want = check_case(cuda, make_case(cell, gene, sim, thr, n_cells=1000, n_genes=80, seed=6))
    assert got["cell_ids"].tolist() == cells.tolist()
    ids = got["gene_ids"].tolist()
    assert 30 not in ids and ids[-1] == 79 and all(g % 2 == 0 for g in ids[:-1])


def test_filter_edges(cuda):
    t = 0.4375
    below = np.nextafter(np.float32(t), np.float32(-np.inf))
    #       ==thr  just below  NaN sim  NaN thr  no cell  kept
    cell = [0, 0, 1, 1, -1, 2]
    gene = [0, 1, 0, 1, 0, 1]
    sim = [t, below, np.nan, 0.9, 0.9, 0.5]
    thr = [t, t, t, np.nan, t, t]
    got, _ = check_case(cuda, make_case(cell, gene, sim, thr))
    assert got["cell_ids"].tolist() == [0, 2] and got["gene_ids"].tolist() == [0, 1]
    assert got["indptr"].tolist() == [0, 1, 2] and got["indices"].tolist() == [0, 1] and got["counts"].tolist() == [1, 1]
    # a float64 threshold between two float32 values: the comparison is made in float64
    thr64 = float(np.float32(t)) - 1e-12
    got, _ = check_case(cuda, make_case([0, 0], [0, 1], [t, below], [thr64, thr64]))
    assert got["counts"].tolist() == [1] and got["gene_ids"].tolist() == [0]


def test_out_of_range_rows_are_counted_and_never_used(cuda):
    n_cells, n_genes = 4, 3
    clean = make_case([0, 3, 3, 1], [0, 2, 2, 1], [0.9, 0.8, 0.7, 0.6], [0.5] * 4, n_cells=n_cells, n_genes=n_genes)
    before = run_case(cuda, clean)
    bad = make_case([0, 3, 3, 1, 2, n_cells, 2 ** 31 - 1, n_cells, 1], [0, 2, 2, 1, n_genes, 0, 0, 0, -5],
                    [0.9, 0.8, 0.7, 0.6, 0.9, 0.9, 0.9, 0.1, 0.9], [0.5] * 9, n_cells=n_cells, n_genes=n_genes)
    with pytest.raises(_lib.SeggerAmdError, match=r"expression_matrix: 4 segmented"):     # not the row that is not kept
        run_case(cuda, bad)
    after, _ = check_case(cuda, clean)
    bit_equal(before, after)


def test_two_calls_are_bit_identical(cuda):
    case = random_case(30_000, 40, 25, seed=8)
    case["cell"][:9_000] = 7                                          # long runs: the cooperative path as well
    bit_equal(run_case(cuda, case), run_case(cuda, case))


def test_feeding_order_does_not_matter(cuda, slide_xy):
    # (reversing the batches may hand a similarity tie between a cell and "no cell" to the other row -- the accumulator's
    # documented rule -- but only among rows the filter drops: the matrix and its float64 sums keep their bits)
    preds = fake_predictions(0)
    xy = slide_xy.to(cuda)
    in_order = feed(cuda, preds).expression(xy)
    bit_equal(in_order, feed(cuda, preds[::-1]).expression(xy))
    cols = tuple(torch.cat([p[i] for p in preds]).to(cuda) for i in range(4))
    sevens = [tuple(c[o:o + 7] for c in cols) for o in range(0, cols[0].numel(), 7)]
    bit_equal(in_order, feed(cuda, sevens).expression(xy))


def test_side_stream(cuda):
    case = runs_case([1, 70, 3, 64, 200], seed=9, not_kept=0.5)
    want = case_oracle(case)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        got = run_case(cuda, case)
    s.synchronize()
    assert_matches_oracle(got, want, max_coord=float(np.abs(case["xy"]).max()))
