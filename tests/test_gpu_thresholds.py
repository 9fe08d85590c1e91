"""Per-gene similarity thresholds on the device: ``postprocess.gene_thresholds`` / ``thresholds="kernel"``
(``csrc/thresholds.hip``: one keys-only radix sort, Yen + Li per gene) against the float64 numpy oracle
(``oracle/postprocess_oracle.py``, gene by gene through tests/thresholds_cases.py) and against the ``"torch"`` route.

Thresholds are float64 results of float sums taken in different orders: atol 1e-9, the bound of tests/test_postprocess.py;
counts, convergence flags and failed genes are exact.  Every input is certified well-conditioned for the oracle by
tests/test_thresholds_cases.py, so no comparison below can hinge on a last bit.  The references are computed once."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segger_amd import _lib                                            # noqa: E402
from segger_amd import postprocess as pp                               # noqa: E402

import thresholds_cases as tc                                          # noqa: E402
from test_postprocess import fake_predictions                          # noqa: E402

ATOL = 1e-9
ROWS = ("row_index", "cell_encoding", "similarity", "gene")


@pytest.fixture(scope="module")
def cases():
    """name -> (case, oracle reference): computed once, shared, never modified."""
    return {name: (case, tc.reference(case)) for name, case in tc.all_cases().items()}


def run(cuda, case, **kw):
    """gene_thresholds over a case -> numpy arrays."""
    got = pp.gene_thresholds(torch.from_numpy(case["sim"]).to(cuda), torch.from_numpy(case["gene"]).to(cuda),
                             torch.from_numpy(case["cell"]).to(cuda), kw.pop("n_genes", case["n_genes"]),
                             kw.pop("max_iter", case["max_iter"]))
    assert all(got[k].is_cuda for k in ("threshold", "yen", "li", "count", "converged", "failed_genes"))
    assert got["threshold"].dtype == got["yen"].dtype == got["li"].dtype == torch.float64
    assert got["count"].dtype == got["failed_genes"].dtype == torch.int64 and got["converged"].dtype == torch.bool
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}


def close(a, b):
    return np.allclose(a, b, rtol=0.0, atol=ATOL, equal_nan=True)


def assert_matches(got, ref):
    for k in ("yen", "li", "threshold"):                               # printed before the assertion: the figures of a failure
        both = np.isfinite(got[k]) & np.isfinite(ref[k])
        print(k, "max abs difference", float(np.abs(got[k][both] - ref[k][both]).max()) if both.any() else 0.0)
    assert np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["converged"], ref["converged"])
    assert np.array_equal(got["failed_genes"], ref["failed_genes"])
    assert close(got["yen"], ref["yen"])                               # each on its own: a min of two must not hide the larger
    ok = ref["converged"]                                              # the oracle has no Li value for a failed gene
    assert close(got["li"][ok], ref["li"][ok]) and np.isfinite(got["li"][~ok]).all()
    assert close(got["threshold"], ref["threshold"])
    assert close(got["global_threshold"], ref["global_threshold"])


@pytest.mark.parametrize("name", ["slide0", "slide1", "slide2", "slide7_max_iter6", "sizes", "edges", "large", "known"])
def test_gene_thresholds_match_the_oracle(cuda, cases, name):
    case, ref = cases[name]
    assert_matches(run(cuda, case), ref)


@pytest.mark.parametrize("seed,n_genes,max_iter", [(0, 12, 250), (1, 12, 250), (2, 12, 250), (7, 9, 6)])
def test_both_entry_points_match_oracle_and_torch_route(cuda, po, seed, n_genes, max_iter):
    preds = fake_predictions(seed, n_genes=n_genes)
    ref = po.assign_transcripts_to_cells([[t.numpy() for t in p] for p in preds], max_iter)
    torch_route = pp.assign_transcripts_to_cells(preds, device=cuda, max_iter=max_iter)
    acc = pp.SegmentationAccumulator(4000, cuda)
    for p in preds:
        acc.update(*p)
    for got in (pp.assign_transcripts_to_cells(preds, device=cuda, max_iter=max_iter, thresholds="kernel"),
                acc.segmentation(max_iter=max_iter, thresholds="kernel")):
        assert set(got) == set(torch_route)
        for k in ROWS:                                                 # the other columns: bit-equal
            assert got[k].dtype == torch_route[k].dtype and torch.equal(got[k], torch_route[k]), k
            assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
        thr = got["similarity_threshold"]
        assert thr.dtype == torch.float64 and thr.is_cuda and isinstance(got["global_threshold"], float)
        assert got["failed_genes"].dtype == torch_route["failed_genes"].dtype == torch.int64
        assert close(thr.cpu().numpy(), ref["similarity_threshold"])
        assert close(thr.cpu().numpy(), torch_route["similarity_threshold"].cpu().numpy())
        assert close(got["global_threshold"], ref["global_threshold"])
        assert close(got["global_threshold"], torch_route["global_threshold"])
        assert np.array_equal(got["failed_genes"].cpu().numpy(), ref["failed_genes"])
        assert torch.equal(got["failed_genes"], torch_route["failed_genes"])
    if max_iter == 6:
        assert 0 < len(ref["failed_genes"]) < n_genes                  # failed genes and a median to back-fill them with
    expr = acc.expression(max_iter=max_iter, thresholds="kernel")      # the keyword goes through
    assert expr["n_kept"] == int((got["similarity"] >= got["similarity_threshold"]).logical_and(got["cell_encoding"] >= 0).sum())


@pytest.fixture(scope="module")
def po():
    import postprocess_oracle
    return postprocess_oracle


def test_known_answers(cuda, cases):
    got = run(cuda, cases["known"][0])
    assert abs(got["li"][0] - 0.5) < 1e-12 and abs(got["yen"][0] - (0.25 + 0.5 / 512)) < 1e-12
    assert abs(got["threshold"][0] - (0.25 + 0.5 / 512)) < 1e-12
    flat = float(np.float32(0.4))
    assert got["li"][1] == flat and abs(got["yen"][1] - (flat - 0.5 + 0.5 / 256)) < 1e-12 and got["threshold"][1] == got["yen"][1]
    assert got["converged"].all() and got["count"].tolist() == [20, 5]
    assert abs(got["global_threshold"] - np.median(got["threshold"])) < 1e-12


def test_absent_genes_and_a_wider_domain(cuda, cases):
    case, ref = cases["edges"]
    got = run(cuda, case)
    absent = [1, 4, 7, 8, 11, 12, 13, 14]
    assert np.isnan(got["threshold"][absent]).all() and np.isnan(got["yen"][absent]).all() and np.isnan(got["li"][absent]).all()
    assert got["converged"][absent].all() and (got["count"][absent] == 0).all()
    wide = run(cuda, case, n_genes=1000)                                # n_genes far above every id present
    assert np.isnan(wide["threshold"][15:]).all() and (wide["count"][15:] == 0).all()
    for k in ("threshold", "yen", "li"):
        assert np.array_equal(wide[k][:15].view(np.int64), got[k].view(np.int64)), k


def test_empty_inputs(cuda):
    n_genes = 7
    none = {"sim": np.linspace(0, 1, 50, dtype=np.float32), "gene": (np.arange(50) % n_genes).astype(np.int32),
            "cell": np.full(50, -1, dtype=np.int32), "n_genes": n_genes, "max_iter": 250}
    empty = {k: v[:0] if isinstance(v, np.ndarray) else v for k, v in none.items()}
    for case in (none, empty):
        got = run(cuda, case)
        for k in ("threshold", "yen", "li"):
            assert got[k].shape == (n_genes,) and np.isnan(got[k]).all(), k
        assert got["converged"].all() and not got["count"].any() and got["failed_genes"].size == 0
        assert np.isnan(got["global_threshold"])
    # the C entry with n_rows == 0: no row pointer, no workspace; the outputs are filled and the counters zeroed
    thr = torch.zeros(3, n_genes, dtype=torch.float64, device=cuda)
    count = torch.full((n_genes,), 9, dtype=torch.int64, device=cuda)
    conv = torch.zeros(n_genes, dtype=torch.uint8, device=cuda)
    counters = torch.full((4,), 9, dtype=torch.int64, device=cuda)
    with _lib.on_device(cuda):
        rc = _lib.load().segger_thresholds_build(None, None, None, 0, n_genes, 250, thr[0].data_ptr(), thr[1].data_ptr(),
                                                 thr[2].data_ptr(), count.data_ptr(), conv.data_ptr(), counters.data_ptr(),
                                                 None, 0, _lib.stream_ptr(cuda))
    _lib.check(rc, "segger_thresholds_build")
    assert bool(thr.isnan().all()) and count.tolist() == [0] * n_genes and conv.tolist() == [1] * n_genes
    assert counters.tolist() == [0, 0, 0, 0]
    preds = [(torch.arange(50), torch.from_numpy(none["cell"]), torch.from_numpy(none["sim"]), torch.from_numpy(none["gene"]))]
    seg = pp.assign_transcripts_to_cells(preds, device=cuda, thresholds="kernel")
    assert bool(seg["similarity_threshold"].isnan().all()) and np.isnan(seg["global_threshold"])


def guarded_build(cuda, sim, gene, cell, n_genes, guard=8):
    """segger_thresholds_build with every [n_genes] output between two walls of guard elements -> (outputs, walls, counters)."""
    lib = _lib.load()
    fills = {"threshold": (torch.float64, 12345.0), "yen": (torch.float64, 12345.0), "li": (torch.float64, 12345.0),
             "count": (torch.int64, 0x5A5A5A5A5A5A5A5A), "converged": (torch.uint8, 0x5A)}
    big = {k: torch.full((n_genes + 2 * guard,), fill, dtype=dt, device=cuda) for k, (dt, fill) in fills.items()}
    out = {k: v[guard:guard + n_genes] for k, v in big.items()}
    counters = torch.zeros(4, dtype=torch.int64, device=cuda)
    n = sim.numel()
    ws_bytes = lib.segger_thresholds_workspace_bytes(n, n_genes)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
    with _lib.on_device(cuda):
        rc = lib.segger_thresholds_build(sim.data_ptr(), gene.data_ptr(), cell.data_ptr(), n, n_genes, 250,
                                         out["threshold"].data_ptr(), out["yen"].data_ptr(), out["li"].data_ptr(),
                                         out["count"].data_ptr(), out["converged"].data_ptr(), counters.data_ptr(),
                                         ws.data_ptr(), ws_bytes, _lib.stream_ptr(cuda))
    _lib.check(rc, "segger_thresholds_build")
    torch.cuda.synchronize()
    walls_ok = all(bool((v[:guard] == fills[k][1]).all()) and bool((v[guard + n_genes:] == fills[k][1]).all())
                   for k, v in big.items())
    return out, walls_ok, counters.tolist()


def test_bad_rows_are_counted_never_written_and_raise(cuda, cases):
    case, ref = cases["slide0"]
    n_genes = case["n_genes"]
    sim = torch.from_numpy(np.concatenate([case["sim"], np.float32([0.9, 0.9, 0.9, np.nan, np.nan])])).to(cuda)
    # assigned rows with gene n_genes, -1 and 2^31 - 1, an assigned NaN; an unassigned NaN is no offence
    gene = torch.from_numpy(np.concatenate([case["gene"], np.int32([n_genes, -1, 2 ** 31 - 1, 3, 3])])).to(cuda)
    cell = torch.from_numpy(np.concatenate([case["cell"], np.int32([1, 1, 1, 1, -1])])).to(cuda)
    out, walls_ok, counters = guarded_build(cuda, sim, gene, cell, n_genes)
    assert walls_ok
    assert counters == [int(ref["count"].sum()), int((ref["count"] > 0).sum()), 3, 1]
    assert np.array_equal(out["count"].cpu().numpy(), ref["count"])    # the rejected rows took part in nothing
    assert ref["converged"].all() and close(out["threshold"].cpu().numpy(), ref["threshold"])
    with pytest.raises(_lib.SeggerAmdError, match="outside"):
        pp.gene_thresholds(sim[:-2], gene[:-2], cell[:-2], n_genes)
    with pytest.raises(_lib.SeggerAmdError, match="NaN"):
        pp.gene_thresholds(sim[-2:], gene[-2:], cell[-2:], n_genes)
    ok = pp.gene_thresholds(sim[-1:], gene[-1:], cell[-1:], n_genes)    # the unassigned NaN alone
    assert bool(ok["threshold"].isnan().all())


def bits(got):
    return [got[k].view(np.int64) for k in ("threshold", "yen", "li")]


@pytest.mark.parametrize("name", ["slide1", "sizes", "large"])
def test_same_bits_from_run_to_run_and_for_any_row_order(cuda, cases, name):
    case, _ = cases[name]
    first = run(cuda, case)
    again = run(cuda, case)
    order = np.random.default_rng(5).permutation(case["sim"].size)
    shuffled = run(cuda, {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in case.items()})
    for a, b, c in zip(bits(first), bits(again), bits(shuffled)):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(first["count"], shuffled["count"]) and np.array_equal(first["converged"], shuffled["converged"])


def test_runs_on_the_current_stream(cuda, cases):
    case, ref = cases["slide2"]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):                                      # the default stream stays idle
        got = run(cuda, case)
    side.synchronize()
    assert_matches(got, ref)
