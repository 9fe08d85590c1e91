"""segger_amd.fragments without a GPU: the oracle of tests/fragment_cases.py on hand-worked graphs, every refusal of the
Python side, the CPU joints (unassigned_mask, merge_fragments), and -- for every seeded case tests/test_gpu_fragments.py
runs through the device cosine -- the assertion that no live edge's float64 similarity lies within the derived error bound
of ``min_similarity``, which is what keeps the GPU comparison exact."""
import numpy as np
import pytest
import torch

import fragment_cases as fc
from segger_amd import _lib
from segger_amd import fragments as F


# ------------------------------------------------------------------------------------------------ the oracle ---
def test_oracle_on_hand_worked_graphs():
    # a triangle, a pair, a singleton; transcript 4 is assigned and sits between 3 and 5
    un = [True, True, True, True, False, True, True, True]
    c = fc.graph_case(8, [(2, 1), (1, 0), (0, 2), (3, 4), (4, 5), (6, 5)], un, min_size=2, first_id=10)
    o = fc.oracle(c)
    assert o["fragment"].tolist() == [10, 10, 10, -1, -1, 11, 11, -1]
    assert o["root"].tolist() == [0, 5] and o["size"].tolist() == [3, 2]
    assert o["parent"].tolist() == [0, 0, 0, 3, 4, 5, 5, 7]
    assert (o["n_edges"], o["n_live_edges"], o["n_kept_edges"], o["n_bad"]) == (6, 4, 4, 0)
    assert (o["n_candidates"], o["n_components"], o["n_fragments"]) == (7, 4, 2)
    # min_size 3 drops the pair, 4 drops everything; self loops and duplicates change nothing
    assert fc.oracle(c._replace(min_size=3))["fragment"].tolist() == [10, 10, 10, -1, -1, -1, -1, -1]
    assert fc.oracle(c._replace(min_size=4))["n_fragments"] == 0
    d = fc.oracle(fc.graph_case(8, [(2, 1), (1, 0), (0, 2), (3, 4), (4, 5), (6, 5), (6, 6), (2, 1), (1, 2)], un, min_size=2, first_id=10))
    assert d["fragment"].tolist() == o["fragment"].tolist() and d["n_live_edges"] == 6      # the loop is not live, the copies are


def test_oracle_mask_tx_index_and_bad_rows():
    z = fc.ones_z(4)
    tx = torch.tensor([5, 6, 7, 99])
    mask = torch.tensor([True, False, True, True])
    b = fc.Batch(z, fc.edges([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0), (0, 4), (1, 3)]), tx, mask)
    o = fc.oracle(fc.Case(10, torch.ones(10, dtype=torch.bool), [b], 0.5, 1, 0))
    # (1, 2) and (1, 3): the source is masked out, so not even its bad tx_index counts; (2, 3), (3, 0): tx 99; (0, 4): no node 4
    assert (o["n_live_edges"], o["n_kept_edges"], o["n_bad"]) == (2, 2, 3)
    assert o["parent"].tolist() == [0, 1, 2, 3, 4, 5, 5, 5, 8, 9]


def test_oracle_exact_threshold_and_similarity_route():
    for dt in fc.DTYPES:
        c = fc.exact_threshold_case(dt)
        z = c.batches[0].z.double()
        assert set(z.unique().tolist()) == {0.0, 1.0} and (z.sum(1) == 4).all()       # small integers: fp32 is exact on them
        cos = (z[0] * z[1:]).sum(1) / 4
        assert cos.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
        o = fc.oracle(c)
        assert o["parent"].tolist() == [0, 1, 2, 0, 0, 0] and o["n_kept_edges"] == 6 and o["margin"] == 0.0
    o = fc.oracle(fc.similarity_case())
    assert o["parent"].tolist() == [0, 0, 2, 3, 4, 4, 6, 6, 8, 9] and o["n_kept_edges"] == 3


def test_tiles_restate_the_scene():
    xy, base = fc.scene(**fc.RANDOM)
    whole, tiles = fc.oracle(base), fc.oracle(fc.tiled(xy, base))
    for k in ("fragment", "root", "size", "parent"):
        assert np.array_equal(whole[k], tiles[k]), k
    assert (whole["n_live_edges"], whole["n_kept_edges"]) == (tiles["n_live_edges"], tiles["n_kept_edges"])
    assert tiles["n_edges"] > whole["n_edges"] and whole["n_fragments"] > 100 and whole["n_kept_edges"] < whole["n_live_edges"]


@pytest.mark.parametrize("name", sorted(fc.z_cases()))
def test_no_live_edge_of_a_gpu_case_is_within_the_error_bound_of_the_threshold(name):
    case = fc.z_cases()[name]
    o = fc.oracle(case)
    for b in case.batches:
        bound = F.similarity_error_bound(b.z.shape[1], b.z.dtype) + b.z.shape[1] * 2.0 ** -50      # + the oracle's own float64 sums
        assert o["margin"] > 100 * bound, (name, o["margin"], bound)
    assert o["n_live_edges"] > 0 and o["n_bad"] == 0


def test_similarity_error_bound():
    assert F.similarity_error_bound(64) == 134 * 2.0 ** -24 and F.similarity_error_bound(64, torch.bfloat16) == 132 * 2.0 ** -24
    assert F.similarity_error_bound(1024, torch.float16) < 1.3e-4
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="channels"):
            F.similarity_error_bound(bad)
    with pytest.raises(ValueError, match="dtype"):
        F.similarity_error_bound(8, torch.float64)
    # the bound against fp32 arithmetic emulated on the CPU in the kernel's shape (fused multiply-adds are at least as exact)
    rng = np.random.default_rng(0)
    for C in (3, 64, 1024):
        a, b = rng.standard_normal((2, 200, C)).astype(np.float32)
        dot, aa, bb = ((x * y).astype(np.float32).sum(1, dtype=np.float32) for x, y in ((a, b), (a, a), (b, b)))
        sim = dot / (np.sqrt(aa) * np.sqrt(bb))
        ad, bd = a.astype(np.float64), b.astype(np.float64)
        exact = (ad * bd).sum(1) / np.sqrt((ad * ad).sum(1) * (bd * bd).sum(1))
        assert np.abs(sim - exact).max() <= F.similarity_error_bound(C)


# ------------------------------------------------------------------------------------------------ refusals ---
def test_every_python_side_refusal():
    n = 6
    un = torch.ones(n, dtype=torch.bool)
    ei = fc.edges([(0, 1), (1, 2), (3, 4)])
    z = fc.ones_z(n)
    A, fcells, cc = F.FragmentAccumulator, F.fragment_cells, F.connected_components
    for bad in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="n_transcripts must be in"):
            A(bad, un)
        with pytest.raises(ValueError, match="n_transcripts must be in"):
            cc(ei, bad)
    for bad in (un.float(), un.view(2, 3), un.numpy(), None):
        with pytest.raises(ValueError, match="unassigned is a 1-D bool tensor"):
            A(n, bad)
        with pytest.raises(ValueError, match="unassigned is a 1-D bool tensor"):
            fcells(ei, bad, z=z)
    with pytest.raises(ValueError, match="unassigned has 6 entries, n_transcripts is 7"):
        A(7, un)
    with pytest.raises(ValueError, match="min_similarity is NaN"):
        A(n, un, float("nan"))
    with pytest.raises(ValueError, match="min_similarity is NaN"):
        fcells(ei, un, z=z, min_similarity=float("nan"))
    for kw in (dict(), dict(z=z, similarity=torch.zeros(3))):
        with pytest.raises(ValueError, match="exactly one of z and similarity"):
            fcells(ei, un, **kw)
    for bad in (ei.float(), ei[0], ei.T.contiguous(), ei.numpy()):
        with pytest.raises(ValueError, match="edge_index"):
            fcells(bad, un, z=z)
        with pytest.raises(ValueError, match="edge_index"):
            cc(bad, n)
    for bad in (z.double(), z[0], z.long(), torch.ones(n, 0), torch.ones(n, 1025)):
        with pytest.raises(ValueError, match="z "):
            fcells(ei, un, z=bad)
    for bad in (torch.zeros(2), torch.zeros(3, dtype=torch.float64), torch.zeros(3, 1), [0.5, 0.5, 0.5]):
        with pytest.raises(ValueError, match="similarity is a 1-D fp32 tensor"):
            fcells(ei, un, similarity=bad)
    for bad in (torch.ones(2, dtype=torch.bool), torch.ones(3), [True, False, True]):
        with pytest.raises(ValueError, match="keep is a 1-D bool tensor"):
            cc(ei, n, keep=bad)
    for bad in (torch.zeros(n), torch.zeros(n, 1, dtype=torch.int64), list(range(n))):
        with pytest.raises(ValueError, match="tx_index is a 1-D int64"):
            fcells(ei, un, z=z, tx_index=bad)
    for bad in (torch.ones(n), torch.ones(n, 1, dtype=torch.bool), [True] * n):
        with pytest.raises(ValueError, match="mask is a 1-D bool tensor"):
            fcells(ei, un, z=z, mask=bad)
    with pytest.raises(ValueError, match="disagree on the number of nodes"):
        fcells(ei, un, z=z, tx_index=torch.arange(n + 1))
    with pytest.raises(ValueError, match="disagree on the number of nodes"):
        fcells(ei, un, z=z, mask=torch.ones(n - 1, dtype=torch.bool))
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="min_size must be an integer >= 1"):
            fcells(ei, un, z=z, min_size=bad)
    for bad in (-1, 1.0, 1 << 62, None):
        with pytest.raises(ValueError, match="first_id must be an integer in"):
            fcells(ei, un, z=z, first_id=bad)
    # everything in order, but on the CPU: there is no CPU path, and the oracle is named
    for fn in (lambda: A(n, un, device="cpu"), lambda: fcells(ei, un, z=z),
               lambda: fcells(ei, un, similarity=torch.zeros(3)), lambda: cc(ei, n)):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only.*fragment_cases"):
            fn()


# ------------------------------------------------------------------------------------------------ the joints ---
def _segmentation():
    return {"row_index": torch.tensor([0, 1, 2, 4, 5, 7]), "cell_encoding": torch.tensor([3, -1, 2, 1, -1, 0]),
            "similarity": torch.tensor([0.9, 0.8, 0.2, float("nan"), float("nan"), 0.5]),
            "gene": torch.tensor([1, 1, 2, 2, 3, 3]),
            "similarity_threshold": torch.tensor([0.5, 0.5, 0.4, 0.4, 0.1, 0.5], dtype=torch.float64),
            "global_threshold": 0.45, "failed_genes": torch.zeros(0, dtype=torch.int64)}


def test_unassigned_mask():
    seg = _segmentation()
    # counted: rows 0 (0.9 >= 0.5) and 7 (0.5 >= 0.5); 2 is below its threshold, 4's similarity is NaN; 3 and 6 have no row
    assert F.unassigned_mask(seg, 8).tolist() == [False, True, True, True, True, True, True, False]
    assert F.unassigned_mask(seg, 9).tolist()[8] is True
    with pytest.raises(ValueError, match="n_transcripts"):
        F.unassigned_mask(seg, 0)
    with pytest.raises(ValueError, match="segmentation is the dict"):
        F.unassigned_mask({"row_index": seg["row_index"]}, 8)
    with pytest.raises(ValueError, match="different lengths"):
        F.unassigned_mask(dict(seg, similarity=seg["similarity"][:3]), 8)


def test_merge_fragments():
    seg = _segmentation()
    frag = {"fragment": torch.tensor([-1, 7, 7, 7, -1, 8, 8, -1]), "first_id": 7, "n_fragments": 2}
    out = F.merge_fragments(seg, frag, 10)
    assert out["cell_encoding"].tolist() == [3, 10, 10, 1, 11, 0] and out["cell_encoding"].dtype == seg["cell_encoding"].dtype
    assert out["similarity_threshold"].tolist() == [0.5, float("-inf"), float("-inf"), 0.4, float("-inf"), 0.5]
    sim = out["similarity"].tolist()
    assert sim[:3] == seg["similarity"].tolist()[:3] and np.isnan(sim[3]) and sim[4] == 0.0     # a member's NaN becomes 0
    counted = (out["cell_encoding"] >= 0) & (out["similarity"].double() >= out["similarity_threshold"])
    assert counted.tolist() == [True, True, True, False, True, True]
    for k in ("row_index", "gene", "global_threshold", "failed_genes"):
        assert out[k] is seg[k]
    assert seg["cell_encoding"].tolist() == [3, -1, 2, 1, -1, 0]                                # the input is not touched
    for bad in (-1, 1.0, True):
        with pytest.raises(ValueError, match="n_cells"):
            F.merge_fragments(seg, frag, bad)
    with pytest.raises(ValueError, match="fragments is the dict"):
        F.merge_fragments(seg, {"fragment": frag["fragment"]}, 10)
    with pytest.raises(ValueError, match="2\\^31"):
        F.merge_fragments(seg, frag, (1 << 31) - 2)
