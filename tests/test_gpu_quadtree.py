"""Adaptive quadtree tiling on the device: ``csrc/quadtree.hip`` (key, radix sort, leaf work list, label) against the
torch path of ``QuadTreeTiling`` on the same float32 inputs.  The tree is exact integer arithmetic, so every comparison
is ``torch.equal``.  Shapes: the point sets (A)-(G) of tests/test_quadtree.py plus N = 255 / 257 (a block's edge) -- the
smallest at which key packing, the sort, the prefix searches, the capacity bound or the label pass can go wrong."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from segger_amd.hetero import TX_BD, TX_NB_BD, TX_TX, collate          # noqa: E402
from segger_amd import tiles as T                                      # noqa: E402

from quadtree_cases import block_edge_cases, cases, foreign_points, skewed_graph      # noqa: E402

CASES = {**cases(), **block_edge_cases()}
ETS = (TX_TX, TX_BD, TX_NB_BD)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_tree_equals_torch_tree(cuda, name):
    pos, max_size = CASES[name]
    host = T.QuadTreeTiling(pos, max_size)
    dev = T.QuadTreeTiling(pos.to(cuda), max_size)
    assert (dev.x0, dev.y0, dev.x1, dev.y1, dev.depth, dev.cell) == (host.x0, host.y0, host.x1, host.y1, host.depth, host.cell)
    assert len(dev) == len(host) <= dev.leaf_capacity(len(pos))
    for a in ("tiles", "levels", "keys", "counts"):
        assert torch.equal(getattr(dev, a), getattr(host, a)), a
    assert dev.labels.is_cuda and dev.labels.dtype == torch.int32 and torch.equal(dev.labels.cpu(), host.labels)
    assert torch.equal(dev.label(pos.to(cuda)).cpu(), host.label(pos))
    far = foreign_points(pos)
    got = dev.label(far.to(cuda))
    assert got.is_cuda and got.dtype == torch.long and torch.equal(got.cpu(), host.label(far))
    assert torch.equal(host.label(far.to(cuda)).cpu(), host.label(far))      # a host-built tree labels device points too
    assert torch.equal(dev.mask(far.to(cuda), 2.0).cpu(), host.mask(far, 2.0))


@pytest.fixture(scope="module")
def graphs(cuda):
    g = skewed_graph()
    return g, g.to(cuda)


def all_pos(g):
    return torch.cat([g["tx"].pos, g["bd"].pos])


def test_partition_by_device_quadtree_equals_host_partition(graphs):
    host, dev = graphs
    tiling, h_tiling = T.QuadTreeTiling(all_pos(dev), 200), T.QuadTreeTiling(all_pos(host), 200)
    part = T.partition_by_tiling(dev, tiling, margin=3.0)
    assert part.data["tx"]["pos"].is_cuda and part.data[TX_TX].edge_index.is_cuda
    labels = {nt: h_tiling.label(host[nt].pos) for nt in ("tx", "bd")}
    n_t = len(tiling)
    assert n_t == len(h_tiling) and sum(part.node_sizes["tx"].tolist()) == 3000
    for t in range(n_t):
        tile = part.tile(t)
        for nt in ("tx", "bd"):
            ids = (labels[nt] == t).nonzero().squeeze(1)                     # stable order inside a tile
            assert torch.equal(tile[nt].index.long().cpu(), host[nt].index[ids].long())
            assert torch.equal(tile[nt].pos.cpu(), host[nt].pos[ids])
            assert torch.equal(tile[nt]["mask"].cpu(), h_tiling.mask(host[nt].pos[ids], 3.0))
            assert bool((tile[nt]["batch"] == 0).all())
        for et in ETS:
            s, _, d = et
            ei = host[et].edge_index
            keep = (labels[s][ei[0]] == t) & (labels[d][ei[1]] == t)         # intra-tile edges only, original order
            want = torch.stack([host[s].index[ei[0, keep]].long(), host[d].index[ei[1, keep]].long()])
            got_ei = tile[et].edge_index.cpu()
            got = torch.stack([tile[s].index.long().cpu()[got_ei[0]], tile[d].index.long().cpu()[got_ei[1]]])
            assert torch.equal(got, want), (t, et)
    # a batch assembled on the device partition == collation of the individual tiles of the HOST partition
    h_part = T.partition_by_tiling(host, h_tiling, margin=3.0)
    ids = [3, 0, n_t - 1]
    b1, b2 = part.batch(ids), collate([h_part.tile(i) for i in ids])
    assert b1.num_graphs == 3
    for nt in ("tx", "bd"):
        for a in ("x", "pos", "index", "mask", "cluster", "batch"):
            assert torch.equal(b1[nt][a].cpu(), b2[nt][a]), (nt, a)
    for et in ETS:
        assert torch.equal(b1[et].edge_index.cpu(), b2[et].edge_index)


@pytest.mark.parametrize("margin", [0.0, 2.0, 40.0])
def test_predict_quadtree_index_on_device_equals_host_predict_tiles(graphs, margin):
    host, dev = graphs
    tiling = T.QuadTreeTiling(all_pos(dev), 200)
    slow = T.PredictTiles(host, T.QuadTreeTiling(all_pos(host), 200).tiles, margin=margin)      # host, whole-slide scan
    fast = T.PredictQuadTreeIndex(dev, tiling, margin=margin)                                   # device, binned by leaf
    assert len(fast) == len(slow)
    for i in range(len(slow)):
        a, b = slow[i], fast[i]
        for nt in ("tx", "bd"):
            assert set(a[nt].keys()) == set(b[nt].keys())
            for k, v in a[nt].items():
                if isinstance(v, torch.Tensor):
                    assert b[nt][k].is_cuda and torch.equal(v, b[nt][k].cpu()), (i, nt, k)
        for et in a.edge_types:
            assert torch.equal(a[et].edge_index, b[et].edge_index.cpu()), (i, et)
    assert all(bool((v == -1).all()) for v in fast._new_id.values())       # scratch map restored
