"""A small slide with HOLES for the tile batcher's tests (tests/test_tiles.py on the host, tests/test_gpu_tiles.py on the
device): about 300 transcripts and 30 boundaries on a 3 x 3 square tiling (tile id = 3 ix + iy, side 10) where

* tile 4 (the centre) is empty of everything,
* tile 1 has transcripts but no boundary (hence no edge into a boundary),
* tile 7 has both node types but no ``tx-belongs-bd`` edge,

plus the brute-force restatement of a batch: nodes by label in their original order, intra-tile edges in their original
order with tile-local ids, collated the way PyG does (``hetero.collate``)."""
import torch

from segger_amd.hetero import TX_BD, TX_NB_BD, TX_TX, HeteroBatch, collate

SIDE, MARGIN = 10.0, 1.0
EMPTY_TILE, NO_BD_TILE, NO_BELONGS_TILE = 4, 1, 7
ETS = (TX_TX, TX_BD, TX_NB_BD)
NODE_ATTRS = ("x", "pos", "index", "cluster", "mask")


def holed_graph(seed: int = 7) -> HeteroBatch:
    g = torch.Generator().manual_seed(seed)
    tx_pos, tx_tile, bd_pos, bd_tile = [], [], [], []
    for t in range(9):
        if t == EMPTY_TILE:
            continue
        lo = torch.tensor([SIDE * (t // 3), SIDE * (t % 3)])
        n_tx = 30 + int(torch.randint(0, 15, (1,), generator=g))
        tx_pos.append(lo + 0.5 + (SIDE - 1.0) * torch.rand(n_tx, 2, generator=g))
        tx_tile += [t] * n_tx
        n_bd = 0 if t == NO_BD_TILE else 3 + int(torch.randint(0, 3, (1,), generator=g))
        bd_pos.append(lo + 0.5 + (SIDE - 1.0) * torch.rand(n_bd, 2, generator=g))
        bd_tile += [t] * n_bd
    # the corners of the extent, so that the tiling is exactly 3 x 3 tiles of side 10
    tx_pos.append(torch.tensor([[0.0, 0.0], [3 * SIDE, 3 * SIDE]]))
    tx_tile += [0, 8]
    tx_pos, bd_pos = torch.cat(tx_pos), torch.cat(bd_pos)
    tx_tile, bd_tile = torch.tensor(tx_tile), torch.tensor(bd_tile)
    # original node order is unrelated to the tiles
    p_tx, p_bd = torch.randperm(tx_pos.shape[0], generator=g), torch.randperm(bd_pos.shape[0], generator=g)
    tx_pos, tx_tile, bd_pos, bd_tile = tx_pos[p_tx], tx_tile[p_tx], bd_pos[p_bd], bd_tile[p_bd]
    n_tx, n_bd = tx_pos.shape[0], bd_pos.shape[0]
    out = HeteroBatch(num_graphs=1)
    out["tx"]["x"] = torch.randint(0, 16, (n_tx,), generator=g)
    out["tx"]["pos"] = tx_pos
    out["tx"]["index"] = torch.arange(n_tx)
    out["tx"]["cluster"] = torch.randint(0, 4, (n_tx,), generator=g)
    out["bd"]["x"] = torch.randn(n_bd, 5, generator=g)
    out["bd"]["pos"] = bd_pos
    out["bd"]["index"] = torch.arange(n_bd, dtype=torch.int32)
    out["bd"]["cluster"] = torch.randint(0, 4, (n_bd,), generator=g)

    def pick(src_tile, dst_tile, per_src, same_tile_share):
        """``per_src`` edges from every source: into a random node of its own tile (where there is one) with the given
        probability, else into a random node anywhere (mostly another tile: the partition drops those)."""
        src, dst = [], []
        for i in range(src_tile.numel()):
            own = (dst_tile == src_tile[i]).nonzero().squeeze(1)
            for _ in range(per_src):
                if own.numel() and float(torch.rand(1, generator=g)) < same_tile_share:
                    j = int(own[int(torch.randint(0, own.numel(), (1,), generator=g))])
                else:
                    j = int(torch.randint(0, dst_tile.numel(), (1,), generator=g))
                src.append(i); dst.append(j)
        return torch.tensor([src, dst], dtype=torch.long)
    out[TX_TX]["edge_index"] = pick(tx_tile, tx_tile, 3, 0.7)
    belongs = pick(tx_tile, bd_tile, 1, 0.8)
    out[TX_BD]["edge_index"] = belongs[:, tx_tile[belongs[0]] != NO_BELONGS_TILE]
    out[TX_NB_BD]["edge_index"] = pick(tx_tile, bd_tile, 2, 0.6)
    return out


def naive_tile(graph: HeteroBatch, tiling, labels, t: int) -> HeteroBatch:
    out = HeteroBatch(num_graphs=1)
    local = {}
    for nt in ("tx", "bd"):
        ids = (labels[nt] == t).nonzero().squeeze(1)                         # stable order inside a tile
        for a in ("x", "pos", "index", "cluster"):
            out[nt][a] = graph[nt][a][ids]
        out[nt]["mask"] = tiling.mask(graph[nt]["pos"][ids], MARGIN)
        loc = torch.full((labels[nt].numel(),), -1, dtype=torch.long)
        loc[ids] = torch.arange(ids.numel())
        local[nt] = loc
    for et in ETS:
        s, _, d = et
        ei = graph[et].edge_index
        keep = (labels[s][ei[0]] == t) & (labels[d][ei[1]] == t)             # intra-tile edges only, original order
        out[et]["edge_index"] = torch.stack([local[s][ei[0, keep]], local[d][ei[1, keep]]])
    return out


def assert_batch_equals_naive(batch: HeteroBatch, graph: HeteroBatch, tiling, labels, ids) -> None:
    """``batch`` (host or device) against the collation of the brute-force tiles ``ids`` of the HOST ``graph``."""
    assert batch.num_graphs == len(ids)
    if not ids:
        for nt in ("tx", "bd"):
            for a in NODE_ATTRS[:4]:
                assert batch[nt][a].shape == (0,) + graph[nt][a].shape[1:] and batch[nt][a].dtype == graph[nt][a].dtype
            assert batch[nt]["mask"].shape == (0,) and batch[nt]["batch"].shape == (0,)
            assert batch[nt]["batch"].dtype == torch.long
        for et in ETS:
            assert batch[et].edge_index.shape == (2, 0) and batch[et].edge_index.dtype == torch.long
        return
    want = collate([naive_tile(graph, tiling, labels, t) for t in ids])
    for nt in ("tx", "bd"):
        assert set(batch[nt].keys()) == set(NODE_ATTRS) | {"batch"}
        for a in NODE_ATTRS + ("batch",):
            got = batch[nt][a].cpu()
            assert got.dtype == want[nt][a].dtype and torch.equal(got, want[nt][a]), (ids, nt, a)
    for et in ETS:
        got = batch[et].edge_index.cpu()
        assert got.dtype == torch.long and torch.equal(got, want[et].edge_index), (ids, et)
