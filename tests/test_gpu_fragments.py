"""segger_amd.fragments on the device against the sequential oracle of tests/fragment_cases.py (unpinned by any reference:
the contract is this project's own).  Every returned tensor and every counter must be EQUAL to the oracle's; the seeded
cases that go through the device cosine are those whose margin from the threshold tests/test_host_fragments.py asserts."""
import numpy as np
import pytest
import torch

import fragment_cases as fc

pytestmark = pytest.mark.gpu
COUNTERS = ("n_edges", "n_live_edges", "n_kept_edges", "n_bad", "n_candidates", "n_components", "n_fragments")


def dev():
    return torch.device("cuda:0")


def up(t):
    return None if t is None else t.to(dev())


def feed(acc, case):
    for b in case.batches:
        acc._feed("test", up(b.z), up(b.edge_index), up(b.tx_index), up(b.mask), up(b.similarity), up(b.keep))


def run(case, return_acc=False):
    from segger_amd import FragmentAccumulator
    acc = FragmentAccumulator(case.n, up(case.unassigned), case.min_similarity, dev())
    feed(acc, case)
    out = acc.result(case.min_size, case.first_id)
    return (out, acc) if return_acc else out


def assert_equal(got, want, what):
    for k in COUNTERS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("fragment", "root", "size"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.int64 and np.array_equal(g, want[k]), (what, k, g[:16], want[k][:16])


def check(case, what):
    out, acc = run(case, return_acc=True)
    want = fc.oracle(case)
    assert_equal(out, want, what)
    assert np.array_equal(acc.parent.cpu().numpy(), want["parent"]), (what, "parent")       # flattened: the smallest member
    return out


@pytest.fixture(scope="module")
def random_scene():
    """the 20 000-point scene with its oracle result -- computed once, never changed"""
    xy, case = fc.scene(**fc.RANDOM)
    return xy, case, fc.oracle(case)


# ------------------------------------------------------------------------------------------------ trivial ---
def test_trivial_graphs():
    check(fc.graph_case(1, np.zeros((0, 2), np.int64)), "N = 1, E = 0")
    check(fc.graph_case(2, [(1, 0)]), "one edge")
    check(fc.graph_case(3, [(0, 0), (1, 1), (2, 2)]), "self loops")
    check(fc.graph_case(4, [(0, 1), (0, 1), (1, 0), (0, 1), (3, 2), (3, 2)]), "duplicate edges")
    out = check(fc.similarity_case(), "one pair, one direction passing; the threshold and its neighbours")
    assert out["fragment"].tolist() == [0, 0, 1, 2, 3, 3, 4, 4, 5, 6]


# ------------------------------------------------------------------------------------------------ wave boundaries ---
@pytest.mark.parametrize("E", [63, 64, 65, 4095, 4097])
def test_wave_and_compaction_boundaries(E):
    pairs = fc.disjoint_pairs(E)
    check(fc.graph_case(2 * E, pairs), f"E = {E}, every edge live")
    check(fc.graph_case(2 * E, pairs, np.zeros(2 * E, bool)), f"E = {E}, no edge live")
    one = np.zeros(2 * E, bool)
    live = np.arange(E)[np.arange(E) % 64 == 17 % min(E, 64)]
    one[2 * live] = one[2 * live + 1] = True
    out = check(fc.graph_case(2 * E, pairs, one), f"E = {E}, one live edge per wave")
    assert out["n_live_edges"] == live.size == (E + 63 - 17) // 64
    for C, dt in ((4, torch.float32), (24, torch.float16), (5, torch.bfloat16)):        # group widths 1, 4 and 8 lanes
        check(fc.graph_case(2 * E, pairs, C=C, dtype=dt), f"E = {E}, C = {C}")


# ------------------------------------------------------------------------------------------------ deep trees ---
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("splits", [1, 3])
def test_a_path_of_4097_nodes(order, splits):
    out = check(fc.graph_case(4097, fc.path_pairs(4097, order), splits=splits), f"path {order} in {splits} updates")
    assert out["n_fragments"] == 1 and out["size"].tolist() == [4097] and out["root"].tolist() == [0]


# ------------------------------------------------------------------------------------------------ contention ---
def test_complete_graph_and_star():
    k64 = [(i, j) for i in range(64) for j in range(64) if i != j]
    out = check(fc.graph_case(64, k64), "K64 in one launch")
    assert out["n_kept_edges"] == 4032 and out["size"].tolist() == [64]
    star = [(1000, i) for i in range(1000)]
    out = check(fc.graph_case(1001, star), "a star whose hub has the largest id")
    assert out["size"].tolist() == [1001] and out["root"].tolist() == [0]
    check(fc.graph_case(1001, [(i, 1000) for i in range(1000)][::-1]), "the star, leaves as sources")


# ------------------------------------------------------------------------------------------------ semantics ---
def test_semantics():
    un = np.ones(11, bool)
    un[5] = False                                               # 0-1-2-3-4 and 6-7-8-9-10 meet only in the assigned 5
    two = [(i, i + 1) for i in range(10)]
    out = check(fc.graph_case(11, two, un, min_size=5), "two groups joined only through an assigned transcript")
    assert out["fragment"].tolist() == [0] * 5 + [-1] + [1] * 5
    out = check(fc.graph_case(11, two[:4] + two[6:9], un, min_size=5), "min_size kept, min_size - 1 dropped")
    assert out["fragment"].tolist() == [0] * 5 + [-1] * 6 and out["n_components"] == 3
    out = check(fc.graph_case(11, two, un, min_size=5, first_id=1 << 40), "first_id")
    assert out["fragment"].tolist() == [1 << 40] * 5 + [-1] + [(1 << 40) + 1] * 5
    mask = torch.ones(11, dtype=torch.bool)
    mask[2] = False                                             # (2, 3) is the only edge between {0, 1, 2} and {3, 4}
    out = check(fc.graph_case(11, two, un, mask=mask), "mask excludes a source")
    assert out["fragment"].tolist() == [0, 0, 0, 1, 1, -1, 2, 2, 2, 2, 2]


# ------------------------------------------------------------------------------------------------ exact threshold ---
@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_exact_threshold(dtype):
    out = check(fc.exact_threshold_case(dtype), f"cosines k / 4 in {dtype}")
    assert out["n_kept_edges"] == 6                             # k = 2, 3, 4 in both directions; k = 1 is not kept
    assert out["fragment"].tolist() == [0, 1, 2, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ widths and dtypes ---
@pytest.mark.parametrize("dtype", fc.DTYPES)
@pytest.mark.parametrize("C", fc.WIDTHS)
def test_widths_and_dtypes(C, dtype):
    check(fc.width_case(C, dtype), f"C = {C}, {dtype}")


def test_strided_rows():
    """rows of a wider tensor: 16-byte pieces when the stride allows, an element a lane when it does not"""
    case = fc.width_case(64, torch.float32)
    b = case.batches[0]
    want = fc.oracle(case)
    from segger_amd import FragmentAccumulator
    for pad in (4, 3):
        wide = torch.zeros(b.z.shape[0], 64 + pad, device=dev())
        wide[:, :64] = up(b.z)
        acc = FragmentAccumulator(case.n, up(case.unassigned), 0.5, dev())
        acc.update(wide[:, :64], up(b.edge_index))
        assert_equal(acc.result(case.min_size), want, f"row stride {64 + pad}")


# ------------------------------------------------------------------------------------------------ random, invariance ---
def test_random_scene(random_scene):
    _, case, want = random_scene
    assert_equal(run(case), want, "20 000 points, k = 5, 40 % unassigned")


def test_invariance(random_scene):
    xy, case, want = random_scene
    runs = {"permuted": fc.permuted(case), "tiles": fc.tiled(xy, case), "tiles, other order": fc.tiled(xy, case, order=(2, 0, 1)),
            "again": case}
    first = run(case)
    for what, c in runs.items():
        got = run(c)
        for k in ("fragment", "root", "size"):
            assert torch.equal(got[k], first[k]), (what, k)
        for k in COUNTERS[1:]:
            assert got[k] == first[k], (what, k)
    assert_equal(first, want, "the scene itself")


def test_one_shot_forms(random_scene):
    from segger_amd import connected_components, fragment_cells
    _, case, want = random_scene
    b = case.batches[0]
    assert_equal(fragment_cells(up(b.edge_index), up(case.unassigned), z=up(b.z)), want, "fragment_cells(z=)")
    s, d = b.edge_index
    zz = b.z.double()
    sim = ((zz[s] * zz[d]).sum(1)).float()                     # unit rows: the margin is far above this rounding
    assert_equal(fragment_cells(up(b.edge_index), up(case.unassigned), similarity=up(sim)), want, "fragment_cells(similarity=)")
    keep = case.unassigned[s] & case.unassigned[d] & (sim >= 0.5)
    labels = connected_components(up(b.edge_index), case.n, keep=up(keep))
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), want["parent"])
    everything = fc.oracle(fc.Case(case.n, torch.ones(case.n, dtype=torch.bool), [fc.Batch(None, b.edge_index)], 0.0, 1, 0))
    assert np.array_equal(connected_components(up(b.edge_index), case.n).cpu().numpy(), everything["parent"])


# ------------------------------------------------------------------------------------------------ bad input ---
def test_bad_rows_are_counted_and_never_followed():
    from segger_amd import FragmentAccumulator, _lib
    z = fc.ones_z(6)
    tx = torch.tensor([0, 1, 2, 50, -1, 5])                      # rows 3 and 4 are outside [0, 8)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 4), (0, 6), (-1, 2), (1 << 40, 0), (5, 0)]
    case = fc.Case(8, torch.ones(8, dtype=torch.bool), [fc.Batch(z, fc.edges(pairs), tx)], 0.5, 1, 0)
    want = fc.oracle(case)
    assert want["n_bad"] == 7 and want["parent"].tolist() == [0, 0, 0, 3, 4, 0, 6, 7]
    acc = FragmentAccumulator(8, up(case.unassigned), 0.5, dev())
    feed(acc, case)
    with pytest.raises(_lib.SeggerAmdError, match="7 of 10 edges had a local id or a tx_index outside its range"):
        acc.result(1)
    assert acc.parent.tolist() == want["parent"].tolist()        # the good edges took part; nothing else was written
    assert acc.counters.tolist()[:4] == [10, 3, 3, 7]
    acc.reset()
    good = case._replace(batches=[fc.Batch(z, fc.edges(pairs[:2] + pairs[-1:]), tx)])
    feed(acc, good)
    assert_equal(acc.result(1), fc.oracle(good), "after reset")


# ------------------------------------------------------------------------------------------------ the chain ---
def test_chain_to_expression_and_boundaries():
    from segger_amd import (FragmentAccumulator, expression_matrix, merge_fragments, segmentation_boundaries, unassigned_mask)
    rng = np.random.default_rng(5)
    # two blobs of 12 unassigned transcripts, 6 assigned ones in cell 0 and cell 2, 3 stragglers
    blob = lambda cx, cy, m: np.stack([cx + rng.random(m), cy + rng.random(m)], 1)       # noqa: E731
    xy = np.concatenate([blob(0, 0, 12), blob(10, 0, 12), blob(0, 10, 6), blob(20, 20, 3)])
    n = xy.shape[0]
    cell = np.full(n, -1)
    cell[24:27], cell[27:30] = 0, 2
    seg = {"row_index": torch.arange(n), "cell_encoding": torch.tensor(cell), "similarity": torch.full((n,), 0.9),
           "gene": torch.tensor(np.arange(n) % 4), "similarity_threshold": torch.full((n,), 0.5, dtype=torch.float64)}
    seg = {k: up(v) for k, v in seg.items()}
    un = unassigned_mask(seg, n)
    assert un.tolist() == [True] * 24 + [False] * 6 + [True] * 3
    pairs = fc.knn_pairs(xy, 4)
    z = torch.zeros(n, 8)
    z[:12, 0], z[12:24, 1], z[24:30, 2], z[30:, 3:6] = 1, 1, 1, torch.eye(3)
    acc = FragmentAccumulator(n, un, 0.5, dev())
    acc.update(up(z), up(fc.edges(pairs)))
    frag = acc.result(min_size=5, first_id=100)
    assert frag["n_fragments"] == 2 and frag["size"].tolist() == [12, 12] and frag["root"].tolist() == [0, 12]
    merged = merge_fragments(seg, frag, 3)
    expr = expression_matrix(merged, up(torch.tensor(xy)))
    assert expr["cell_ids"].tolist() == [0, 2, 3, 4] and expr["cell_count"].tolist() == [3, 3, 12, 12]
    assert expr["n_kept"] == 30 and int(expr["counts"].sum()) == 30
    rings = segmentation_boundaries(merged, up(torch.tensor(xy)))
    assert rings["cell_ids"].tolist() == [0, 2, 3, 4] and rings["n_transcripts"].tolist() == [3, 3, 12, 12]
    assert rings["ring_offsets"].numel() == 5 and bool((rings["ring_offsets"][1:] - rings["ring_offsets"][:-1] >= 3).all())


def test_update_from_batch_reads_the_prediction_batch():
    """the model's unit-norm tx embeddings, the tx-neighbors-tx edges, tx.index and tx.predict_mask: equal, bit for bit, to
    ``update`` on those four (the forward is deterministic in eval mode)"""
    from segger_amd import FragmentAccumulator, LitISTEncoder
    from segger_amd.hetero import TX_TX
    from segger_amd.synthetic import C1, make_graph
    b = make_graph(C1)
    torch.manual_seed(0)
    m = LitISTEncoder(n_genes=C1.n_genes, in_channels=128)
    m.model._materialize_bd(C1.bd_dim, "cpu")
    m = m.to(dev()).eval()
    bg = b.to(dev())
    index, mask = bg["tx"]["index"], bg["tx"]["predict_mask"]
    n = int(index.max()) + 1
    un = torch.rand(n, generator=torch.Generator().manual_seed(3)) < 0.6
    with torch.no_grad():
        z = m(bg)["tx"]
    thr = float(torch.cosine_similarity(z[bg[TX_TX].edge_index[0]], z[bg[TX_TX].edge_index[1]]).median())   # about half are kept
    got, want = FragmentAccumulator(n, up(un), thr, dev()), FragmentAccumulator(n, up(un), thr, dev())
    got.update_from_batch(m, bg)
    want.update(z, bg[TX_TX].edge_index, index, mask)
    a, b_ = got.result(2), want.result(2)
    for k in ("fragment", "root", "size"):
        assert torch.equal(a[k], b_[k]), k
    for k in COUNTERS:
        assert a[k] == b_[k], k
    assert 0 < a["n_kept_edges"] < a["n_live_edges"] and a["n_fragments"] > 0
