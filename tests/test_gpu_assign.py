"""Streaming transcript -> cell assignment on the device: ``postprocess.SegmentationAccumulator`` (``csrc/assign.hip``:
one 64-bit atomic max per row over a packed (similarity, arrival order) key) against ``postprocess.best_assignment`` /
``assign_transcripts_to_cells`` on CPU copies of the same tuples.  The arg-max is exact, so every comparison is
``torch.equal`` (NaN == NaN for similarities).  Shapes: the 4 000-transcript slides of tests/test_postprocess.py, and row
counts around a wave (63 / 64 / 65), a block (257) and the grid-stride bound (70 000 rows on one transcript: maximum
contention; 262 401 rows: past the 1024 x 256 threads of one grid)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segger_amd import _lib                                            # noqa: E402
from segger_amd import postprocess as pp                               # noqa: E402

from assign_cases import assign_keys, key_test_similarities, same     # noqa: E402
from test_postprocess import fake_predictions                          # noqa: E402

N_TX = 4000
KEYS = ("row_index", "cell_encoding", "similarity", "gene")


@pytest.fixture(scope="module")
def slides():
    """seed -> (CPU tuples, best_assignment of them): computed once, shared, never modified."""
    out = {}
    for seed in (0, 1, 2):
        preds = fake_predictions(seed)
        out[seed] = (preds, pp.best_assignment(preds))
    return out


def feed(cuda, batches, n_tx=N_TX):
    acc = pp.SegmentationAccumulator(n_tx, cuda)
    for b in batches:
        acc.update(*b)
    return acc


def assert_result(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and same(got[k], want[k]), k


def state(acc):
    torch.cuda.synchronize()
    return acc.best_key.cpu(), acc.cell.cpu(), acc.gene.cpu()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_slides_equal_best_assignment_and_segmentation(cuda, slides, seed):
    preds, want = slides[seed]
    acc = feed(cuda, preds)
    got = acc.result()
    assert all(got[k].is_cuda for k in KEYS)
    assert_result(got, want)
    assert acc.rows_fed == sum(p[0].numel() for p in preds) and acc.counters.tolist() == [acc.rows_fed, 0]
    # the same thresholds-and-join tail on the same device: bit-equal thresholds
    seg, ref = acc.segmentation(), pp.assign_transcripts_to_cells(preds, device=cuda)
    assert_result(seg, ref)
    assert same(seg["similarity_threshold"], ref["similarity_threshold"]) and same(seg["failed_genes"], ref["failed_genes"])
    assert seg["global_threshold"] == ref["global_threshold"] or (np.isnan(seg["global_threshold"]) and np.isnan(ref["global_threshold"]))
    few = acc.segmentation(max_iter=6), pp.assign_transcripts_to_cells(preds, device=cuda, max_iter=6)
    assert same(few[0]["similarity_threshold"], few[1]["similarity_threshold"])
    acc.reset()
    assert acc.rows_fed == 0 and acc.result()["row_index"].numel() == 0
    acc.update(*preds[1])
    assert_result(acc.result(), pp.best_assignment(preds[1:2]))


def test_chunking_invariance(cuda, slides):
    preds, want = slides[0]
    cols = tuple(torch.cat([p[i] for p in preds]).to(cuda) for i in range(4))
    n = cols[0].numel()
    one = state(feed(cuda, [cols]))
    five = state(feed(cuda, preds))
    sevens = feed(cuda, [tuple(c[o:o + 7] for c in cols) for o in range(0, n, 7)])
    assert_result(sevens.result(), want)
    sevens = state(sevens)
    for a, b, c in zip(one, five, sevens):
        assert torch.equal(a, b) and torch.equal(a, c)                # best_key bitwise, cell, gene


def rows_case(n, n_tx, one_transcript, seed):
    g = torch.Generator().manual_seed(seed)
    tx = torch.full((n,), n_tx - 1) if one_transcript else torch.randint(0, n_tx, (n,), generator=g)
    sim = torch.randint(-8, 9, (n,), generator=g).float() / 8          # 17 values: the maximum is shared by many rows
    return tx, torch.arange(n), sim, torch.randint(0, 100, (n,), generator=g, dtype=torch.int32)


@pytest.mark.parametrize("n_tx", [1, 5])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 70_000, 262_401])
def test_row_counts(cuda, n, n_tx):
    batch = rows_case(n, n_tx, one_transcript=(n == 70_000), seed=n + n_tx)
    got = feed(cuda, [batch], n_tx).result()
    assert_result(got, pp.best_assignment([batch]))
    if n == 70_000:                                                   # seg = row number: the first row of highest similarity
        assert got["row_index"].tolist() == [n_tx - 1]
        assert got["cell_encoding"].item() == int((batch[2] == batch[2].max()).nonzero()[0])


def bits(*words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


def test_special_similarities(cuda):
    nan, inf = float("nan"), float("inf")
    rows = [  # (tx, seg, sim)
        (0, 10, 0.9), (0, 11, nan), (0, 12, inf),                     # NaN wins, above +inf
        (1, 20, 0.0), (1, 21, -0.0),                                  # +-0 tie: the first row
        (2, 30, -0.0), (2, 31, 0.0), (2, 32, -1e-45),                 # ... whichever sign comes first; a denormal loses
        (3, 40, 1.0), (3, 41, inf), (3, 42, inf),                     # +inf, first of two
        (4, 50, -inf), (4, 51, -inf),                                 # only -inf rows
        (5, -1, 0.5), (5, 60, 0.25),                                  # an unassigned row (seg = -1) wins
        (7, 70, nan), (7, 71, nan),                                   # NaN tie: the first row
        (8, -1, 0.0),
    ]                                                                 # transcripts 6 and 9 are never seen
    tx = torch.tensor([r[0] for r in rows])
    seg = torch.tensor([r[1] for r in rows])
    sim = torch.tensor([r[2] for r in rows], dtype=torch.float32)
    tx = torch.cat([tx, torch.tensor([7, 7, 1])])                     # -NaN and a payload NaN behind the first NaN; a late tie
    seg = torch.cat([seg, torch.tensor([72, 73, 22])])
    sim = torch.cat([sim, bits(0xFFC00000, 0x7F800001), torch.tensor([0.0])])
    gene = (seg % 7).int()
    want = pp.best_assignment([(tx, seg, sim, gene)])
    assert want["row_index"].tolist() == [0, 1, 2, 3, 4, 5, 7, 8] and want["cell_encoding"].tolist() == [11, 20, 30, 41, 50, -1, 70, -1]
    for split in (len(rows), 5, 1):                                   # one batch, two batches, row by row
        batches = [tuple(c[o:o + split] for c in (tx, seg, sim, gene)) for o in range(0, tx.numel(), split)]
        got = feed(cuda, batches, 10).result()
        assert_result(got, want)
        s = got["similarity"].cpu()
        assert torch.equal(s.view(torch.int32)[[0, 6]], torch.full((2,), 0x7FC00000, dtype=torch.int32))    # canonical NaN
        assert not torch.signbit(s[2])                                # a winning -0.0 comes back as +0.0


def test_device_keys_equal_numpy_keys(cuda):
    sim = key_test_similarities()
    n = sim.size
    tx = torch.from_numpy(np.random.default_rng(2).permutation(n))    # one row per transcript: every key survives
    cols = (tx, torch.arange(n), torch.from_numpy(sim), torch.zeros(n, dtype=torch.int32))
    half = n // 2 + 1
    acc = feed(cuda, [tuple(c[:half] for c in cols), tuple(c[half:] for c in cols)], n)
    key = state(acc)[0].numpy().view(np.uint64)
    assert np.array_equal(key[tx.numpy()], assign_keys(sim, np.arange(n)))
    assert torch.equal(acc.cell.cpu()[tx].long(), cols[1])


def test_mask_equals_prefiltered_rows(cuda, slides):
    preds, _ = slides[1]
    g = torch.Generator().manual_seed(11)
    masks = [torch.rand(p[0].numel(), generator=g) < 0.6 for p in preds]
    masks[2] = torch.zeros_like(masks[2])                             # a batch that is masked out entirely
    acc = pp.SegmentationAccumulator(N_TX, cuda)
    for p, m in zip(preds, masks):
        acc.update(*p, mask=m.to(cuda) if m.numel() % 2 else m)       # device and CPU masks
    filtered = [tuple(c[m] for c in p) for p, m in zip(preds, masks)]
    got = acc.result()
    assert_result(got, feed(cuda, filtered).result())
    assert_result(got, pp.best_assignment(filtered))


def test_out_of_range_rows_are_counted_and_never_written(cuda):
    n_tx, guard = 50, 8
    acc = pp.SegmentationAccumulator(n_tx, cuda)
    walls = {}
    for name, fill in (("best_key", 0x5A5A5A5A5A5A5A5A), ("cell", 0x5A5A5A5A), ("gene", 0x5A5A5A5A)):
        old = getattr(acc, name)
        big = torch.full((n_tx + 2 * guard,), fill, dtype=old.dtype, device=cuda)
        big[guard:guard + n_tx] = 0
        setattr(acc, name, big[guard:guard + n_tx])                   # the state, between two walls of guard elements
        walls[name] = (big, fill)
    tx = torch.tensor([3, -1, n_tx, 7, 3, n_tx - 1, 0, -(2 ** 40), 2 ** 40])
    seg = torch.arange(100, 100 + tx.numel())
    sim = torch.tensor([0.1, 9.0, 9.0, 0.2, 0.3, 0.4, 0.5, 9.0, 9.0])
    gene = torch.arange(tx.numel(), dtype=torch.int32)
    acc.update(tx, seg, sim, gene)
    torch.cuda.synchronize()
    for name, (big, fill) in walls.items():
        assert bool((big[:guard] == fill).all()) and bool((big[guard + n_tx:] == fill).all()), name
    assert acc.counters.tolist() == [9, 4]                            # the rows are counted ...
    ok = (tx >= 0) & (tx < n_tx)
    want = pp.best_assignment([tuple(c[ok] for c in (tx, seg, sim, gene))])
    seen = (acc.best_key != 0).nonzero().squeeze(1)
    assert torch.equal(seen.cpu(), want["row_index"]) and torch.equal(acc.cell[seen].cpu().long(), want["cell_encoding"])
    with pytest.raises(_lib.SeggerAmdError, match="dropped"):         # ... and result() refuses
        acc.result()


def test_update_captured_in_a_graph_replays_correctly(cuda, slides):
    preds, _ = slides[2]
    n = min(p[0].numel() for p in preds[:3])
    batches = [tuple(c[:n] for c in p) + (torch.arange(n) % 5 != b,) for b, p in enumerate(preds[:3])]
    eager = pp.SegmentationAccumulator(N_TX, cuda)
    for b in batches:
        eager.update(*b[:4], mask=b[4])
    dtypes = (torch.int64, torch.int64, torch.float32, torch.int32, torch.bool)
    static = [torch.zeros(n, dtype=d, device=cuda) for d in dtypes]
    acc = pp.SegmentationAccumulator(N_TX, cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # one stream; nothing runs during capture
        acc.update(*static[:4], mask=static[4])
    for b in batches:
        for s, c in zip(static, b):
            s.copy_(c)
        graph.replay()
    for a, b in zip(state(acc), state(eager)):                        # the base sequence number advanced on the device
        assert torch.equal(a, b)
    assert acc.counters.tolist() == [3 * n, 0]
    assert_result(acc.result(), pp.best_assignment([tuple(c[b[4]] for c in b[:4]) for b in batches]))


def test_two_runs_are_bitwise_identical(cuda, slides):
    preds, _ = slides[0]
    for a, b in zip(state(feed(cuda, preds)), state(feed(cuda, preds))):
        assert torch.equal(a, b)


def test_predict_into_equals_best_assignment_over_predict(cuda):
    """Three overlapping prediction tiles (different predict masks over one small graph) through the hipGraph predictor:
    rows fed straight from the static output buffers == best_assignment over predict() of the same tiles."""
    from segger_amd.inference import GraphedPredictor, GraphedPredictorPool, bucket_sizes
    from test_gpu_golden import golden_model, load_encoder_golden
    _, sd, b = load_encoder_golden()
    m = golden_model(sd, cuda, torch.float32).eval()
    bg = b.to(cuda)
    n_tx = int(b["tx"]["index"].max()) + 1
    bd_dim = int(b["bd"]["x"].shape[1])
    g = torch.Generator().manual_seed(5)
    masks = [(torch.rand(b["tx"].num_nodes, generator=g) < 0.6).to(cuda) for _ in range(3)]
    for predictor in (GraphedPredictor(m, bucket_sizes(bg, floor=256), bd_dim), GraphedPredictorPool(m, bd_dim)):
        acc = pp.SegmentationAccumulator(n_tx, cuda)
        outs = []
        for mask in masks:
            bg["tx"]["predict_mask"] = mask
            predictor.predict_into(bg, acc)
            outs.append(predictor.predict(bg))
        assert sum(o[0].numel() for o in outs) > int(torch.stack(masks).any(0).sum()) > 0      # the tiles overlap
        assert acc.rows_fed == 3 * b["tx"].num_nodes
        assert_result(acc.result(), pp.best_assignment(outs))
        seg, ref = acc.segmentation(), pp.assign_transcripts_to_cells(outs, device=cuda)
        assert same(seg["similarity_threshold"], ref["similarity_threshold"])
