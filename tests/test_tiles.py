"""Tile batcher (host / torch logic; CPU): partition, O(1) tile slicing, collation, bin packing, predict tiles."""
import random

import pytest
import torch

from segger_amd.hetero import TX_BD, TX_NB_BD, TX_TX, collate
from segger_amd.synthetic import SyntheticSpec, make_graph
from segger_amd import tiles as T


@pytest.fixture(scope="module")
def graph():
    g = make_graph(SyntheticSpec(n_tx=3000, n_bd=90, k_tx=6, seed=4))
    for nt in ("tx", "bd"):
        del g[nt]["mask"]                       # the fit mask is what the tile partition adds
    return g


def all_pos(g):
    return torch.cat([g["tx"].pos, g["bd"].pos])


def test_square_tiling_label_and_mask():
    pos = torch.tensor([[0.0, 0.0], [10.0, 10.0], [4.9, 5.1], [5.0, 5.0], [9.99, 0.01], [2.5, 2.5]])
    t = T.SquareTiling(pos, 5.0)
    assert len(t) == 4 and t.tiles.shape == (4, 4)
    lab = t.label(pos)
    assert lab.tolist() == [0, 3, 1, 3, 2, 0]                 # id = ix * ny + iy; shared edges go to the upper tile
    assert t.label(torch.tensor([[-1.0, 0.0], [11.0, 3.0]])).tolist() == [-1, -1]
    m = t.mask(pos, 1.0)
    assert m.tolist() == [False, False, False, False, False, True]
    assert t.mask(pos, 0.0).tolist() == [False, False, True, False, True, True]     # strict interior
    with pytest.raises(ValueError):
        t.mask(pos, -1.0)
    assert t.mask(pos, 100.0).dtype == torch.bool              # oversize margin is halved until tiles survive
    with pytest.raises(ValueError):
        T.SquareTiling(pos, 0.0)


def test_partition_matches_naive_and_collate(graph):
    tiling = T.SquareTiling(all_pos(graph), 40.0)
    part = T.partition_by_tiling(graph, tiling, margin=3.0)
    labels = {nt: tiling.label(graph[nt].pos) for nt in ("tx", "bd")}
    n_t = len(tiling)
    assert len(part) == n_t and sum(part.node_sizes["tx"].tolist()) == 3000
    total_edges = {et: 0 for et in (TX_TX, TX_BD, TX_NB_BD)}
    for t in range(n_t):
        tile = part.tile(t)
        for nt in ("tx", "bd"):
            ids = (labels[nt] == t).nonzero().squeeze(1)                     # stable order inside a tile
            assert torch.equal(tile[nt].index if nt == "tx" else tile[nt].index.long(), graph[nt].index[ids].long())
            assert torch.equal(tile[nt].pos, graph[nt].pos[ids])
            assert torch.equal(tile[nt]["mask"], tiling.mask(graph[nt].pos[ids], 3.0))
            assert (tile[nt]["batch"] == 0).all()
        for et in (TX_TX, TX_BD, TX_NB_BD):
            s, _, d = et
            ei = graph[et].edge_index
            keep = (labels[s][ei[0]] == t) & (labels[d][ei[1]] == t)         # intra-tile edges only
            want = {(int(graph[s].index[a]), int(graph[d].index[b])) for a, b in ei[:, keep].t().tolist()}
            got_ei = tile[et].edge_index
            got = {(int(tile[s].index[a]), int(tile[d].index[b])) for a, b in got_ei.t().tolist()}
            assert got == want and got_ei.shape[1] == int(keep.sum())
            total_edges[et] += got_ei.shape[1]
    assert total_edges[TX_TX] < graph[TX_TX].edge_index.shape[1]             # inter-tile edges were dropped
    # a batch assembled on the partition == PyG-style collation of the individual tiles
    ids = [3, 0, n_t - 1]
    b1, b2 = part.batch(ids), collate([part.tile(i) for i in ids])
    assert b1.num_graphs == 3
    for nt in ("tx", "bd"):
        for a in ("x", "pos", "index", "mask", "cluster", "batch"):
            assert torch.equal(b1[nt][a], b2[nt][a]), (nt, a)
    for et in (TX_TX, TX_BD, TX_NB_BD):
        assert torch.equal(b1[et].edge_index, b2[et].edge_index)
    assert part.batch([-1])["tx"].num_nodes == part.tile(n_t - 1)["tx"].num_nodes
    with pytest.raises(IndexError):
        part.batch([n_t])
    with pytest.raises(ValueError):
        T.TilePartition(graph, {"tx": labels["tx"] - 1, "bd": labels["bd"]}, n_t)


def check_bins(bins, items, cap):
    flat = sorted(i for b in bins for i in b)
    assert flat == list(range(len(items)))
    assert all(sum(items[i] for i in b) <= cap + 1e-9 for b in bins)


def test_bin_packing_algorithms():
    items = [7, 5, 5, 4, 4, 3, 2, 2, 1, 1]
    bfd = T.best_fit_decreasing(items, 10)
    check_bins(bfd, items, 10)
    assert len(bfd) == 4 and bfd[0] == [0, 5]                               # 7 + 3 fills the first bin exactly
    hk = T.harmonic_k([6, 6, 4, 4, 4, 3, 1, 1], 10, k=3)
    # classes: 0.6 -> j=1 (own bin each); 0.4 -> j=2 (pairs); 0.3, 0.1 -> small items, first-fit together
    assert hk == [[0], [1], [2, 3], [4], [5, 6, 7]]
    rng = random.Random(0)
    ffd = T.first_fit_decreasing_bucketed(items, 10, n_buckets=None)
    check_bins(ffd, items, 10)
    assert ffd[0] == [0, 5]
    check_bins(T.first_fit_decreasing_bucketed(items, 10, n_buckets=1, rng=rng), items, 10)
    check_bins(T.first_fit_decreasing_bucketed(items, 10, n_buckets=3, rng=rng), items, 10)
    with pytest.raises(ValueError):
        T.best_fit_decreasing([11], 10)
    assert T.best_fit_decreasing([11, 0, 3], 10, skip_too_big=True) == [[2]]
    with pytest.raises(ValueError):
        T.harmonic_k([1], 10, k=1)
    assert T.first_fit_decreasing_bucketed([], 10) == []


def test_tile_batch_sampler(graph):
    part = T.partition_by_tiling(graph, T.SquareTiling(all_pos(graph), 25.0), margin=2.0)
    w = part.weights("edge")
    cap = max(w) * 3
    s = T.TileBatchSampler(part, cap, mode="edge", skip_too_big=True)
    batches = list(s)
    used = sorted(i for b in batches for i in b)
    assert used == [i for i, v in enumerate(w) if v > 0] and len(s) == len(batches)
    assert all(sum(w[i] for i in b) <= cap for b in batches)
    assert list(s) == batches                                                # deterministic without shuffle
    sh = T.TileBatchSampler(part, cap, shuffle=True, skip_too_big=True, seed=1)
    e1, e2 = list(sh), list(sh)
    assert sorted(i for b in e1 for i in b) == used and e1 != e2             # re-packed every epoch
    assert T.TileBatchSampler(part, max(part.weights("node")) * 2, mode="node", skip_too_big=True)
    with pytest.raises(ValueError):
        T.TileBatchSampler(part, 1, skip_too_big=False)


def test_predict_tiles_subgraph(graph):
    tiling = T.SquareTiling(all_pos(graph), 30.0)
    ds = T.PredictTiles(graph, tiling.tiles, margin=4.0)
    assert len(ds) == len(tiling)
    seen = torch.zeros(3000, dtype=torch.long)
    for i in range(len(ds)):
        x0, y0, x1, y1 = ds.tiles[i].tolist()
        t = ds[i]
        pos = graph["tx"].pos
        outer = (pos[:, 0] >= x0 - 4) & (pos[:, 0] < x1 + 4) & (pos[:, 1] >= y0 - 4) & (pos[:, 1] < y1 + 4)
        assert torch.equal(t["tx"].index, graph["tx"].index[outer])
        inner = (t["tx"].pos[:, 0] >= x0) & (t["tx"].pos[:, 0] <= x1) & (t["tx"].pos[:, 1] >= y0) & (t["tx"].pos[:, 1] <= y1)
        assert torch.equal(t["tx"].predict_mask, inner)
        seen[t["tx"].index[t["tx"].predict_mask]] += 1
        ei = t[TX_NB_BD].edge_index
        g_ei = graph[TX_NB_BD].edge_index
        bd_outer = ((graph["bd"].pos[:, 0] >= x0 - 4) & (graph["bd"].pos[:, 0] < x1 + 4) &
                    (graph["bd"].pos[:, 1] >= y0 - 4) & (graph["bd"].pos[:, 1] < y1 + 4))
        want = {(a, b) for a, b in g_ei[:, outer[g_ei[0]] & bd_outer[g_ei[1]]].t().tolist()}
        got = {(int(t["tx"].index[a]), int(t["bd"].index[b])) for a, b in ei.t().tolist()}
        assert got == want
    assert (seen >= 1).all()                    # every transcript is predicted by at least one tile
    with pytest.raises(IndexError):
        ds[len(ds)]


@pytest.mark.parametrize("side,margin", [(30.0, 4.0), (17.0, 17.0), (1000.0, 5.0), (20.0, 10.0), (25.0, 9.9), (12.0, 0.0)])
def test_predict_tile_index_equals_predict_tiles(graph, side, margin):
    """The binned index (border strips for margins up to half a tile, whole 3 x 3 neighbourhoods beyond) returns
    exactly the whole-slide subgraph of PredictTiles."""
    tiling = T.SquareTiling(all_pos(graph), side)
    slow = T.PredictTiles(graph, tiling.tiles, margin=margin)
    fast = T.PredictTileIndex(graph, tiling, margin=margin)
    assert len(fast) == len(slow)
    for i in range(len(slow)):
        a, b = slow[i], fast[i]
        for nt in ("tx", "bd"):
            assert set(a[nt].keys()) == set(b[nt].keys())
            for k, v in a[nt].items():
                if isinstance(v, torch.Tensor):
                    assert torch.equal(v, b[nt][k]), (i, nt, k)
        for et in a.edge_types:
            assert torch.equal(a[et].edge_index, b[et].edge_index), (i, et)
    assert all(bool((v == -1).all()) for v in fast._new_id.values())       # scratch map restored
    with pytest.raises(ValueError):
        T.PredictTileIndex(graph, tiling, margin=side * 1.5)


def test_bin_packers_reproduce_reference_vectors():
    """N2 pin: ``tests/golden/bin_packing.npz`` holds outputs of the reference's own ``partition/sampler.py``
    (``best_fit_decreasing`` :11-82, ``harmonic_k`` :85-183, ``first_fit_decreasing_bucketed`` :186-289; generated by
    tests/golden/make_bin_packing_golden.py).  The product's packers must return the very same bins -- same item
    indices, same order inside a bin, same bin order -- including the randomised variants given the same
    ``random.Random`` and the error raised for oversize items."""
    import json
    import os
    import random
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "bin_packing.npz"))
    blob = json.loads(bytes(z["json"]).decode())
    assert len(blob["cases"]) >= 12
    for rec in blob["cases"]:
        items, cap, skip = rec["items"], rec["capacity"], rec["skip_too_big"]
        assert T.best_fit_decreasing(items, cap, skip_too_big=skip) == rec["best_fit_decreasing"]
        assert T.first_fit_decreasing_bucketed(items, cap, skip_too_big=skip, n_buckets=None) == rec["first_fit_decreasing"]
        for k in (2, 3, 6, 10):
            assert T.harmonic_k(items, cap, k=k, skip_too_big=skip) == rec[f"harmonic_{k}"], k
        for nb in (1, 3):
            got = T.first_fit_decreasing_bucketed(items, cap, skip_too_big=skip, n_buckets=nb, rng=random.Random(7))
            assert got == rec[f"ffd_buckets_{nb}_seed7"], nb
    err = blob["errors"]
    for name, fn in (("best_fit_decreasing", T.best_fit_decreasing), ("harmonic_k", T.harmonic_k),
                     ("first_fit_decreasing_bucketed", T.first_fit_decreasing_bucketed)):
        with pytest.raises(ValueError) as e:
            fn([3.0, 11.0], 10.0)
        assert [type(e.value).__name__, str(e.value)] == err[name]
    with pytest.raises(ValueError) as e:
        T.harmonic_k([1.0], 10.0, k=1)
    assert str(e.value) == err["harmonic_k_k1"][1]


def test_persistent_store_is_bounded(graph):
    """The per-tile-set store behind ``batch_cache(batch)['persistent']`` is an LRU: a shuffling sampler makes new tile
    tuples every epoch (reference data_module.py:344) and must not grow it without bound (round-2 advice)."""
    from segger_amd.graph import batch_cache
    part = T.partition_by_tiling(graph, T.SquareTiling(all_pos(graph), 25.0), margin=2.0)
    part.persist_max = 4
    first = batch_cache(part.batch([0]))["persistent"]
    first["marker"] = 1
    assert batch_cache(part.batch([0]))["persistent"] is first               # same tile set -> same entry
    for i in range(1, 4):
        batch_cache(part.batch([i]))["persistent"]["marker"] = i
    assert batch_cache(part.batch([0]))["persistent"] is first               # still there (4 entries) and now most recent
    batch_cache(part.batch([0, 1]))                                          # 5th entry evicts the least recently used: [1]
    assert len(part._persist) == 4 and (1,) not in part._persist and (0,) in part._persist
    assert "marker" not in batch_cache(part.batch([1]))["persistent"]


def test_shard_keeps_only_its_tiles_and_batches_match(graph):
    """``TilePartition.shard``: a data-parallel rank's resident subset.  Batches assembled on the shard are identical to
    the same batches assembled on the full partition; two complementary shards hold every node and edge exactly once
    and about half the bytes each."""
    part = T.partition_by_tiling(graph, T.SquareTiling(all_pos(graph), 25.0), margin=2.0)
    n_t = len(part)
    mine, theirs = list(range(0, n_t, 2)), list(range(1, n_t, 2))
    a, b = part.shard(mine), part.shard(theirs)
    assert len(a) == len(mine) and len(b) == len(theirs)
    for nt in ("tx", "bd"):
        assert int(a.node_sizes[nt].sum()) + int(b.node_sizes[nt].sum()) == int(part.node_sizes[nt].sum())
        assert sorted(torch.cat([a.node_perm[nt], b.node_perm[nt]]).tolist()) == sorted(part.node_perm[nt].tolist())
    for et in (TX_TX, TX_BD, TX_NB_BD):
        assert int(a.edge_sizes[et].sum()) + int(b.edge_sizes[et].sum()) == int(part.edge_sizes[et].sum())
    assert 0.3 * part.resident_bytes() < a.resident_bytes() < 0.7 * part.resident_bytes()
    for local, glob in (([0], [mine[0]]), ([2, 0, 1], [mine[2], mine[0], mine[1]]), (list(range(len(mine))), mine)):
        x, y = a.batch(local), part.batch(glob)
        assert x.num_graphs == y.num_graphs
        for nt in ("tx", "bd"):
            for k in ("x", "pos", "index", "mask", "cluster", "batch"):
                assert torch.equal(x[nt][k], y[nt][k]), (nt, k)
        for et in (TX_TX, TX_BD, TX_NB_BD):
            assert torch.equal(x[et].edge_index, y[et].edge_index), et
    assert part.shard([]).num_tiles == 0
    with pytest.raises(IndexError):
        part.shard([0, 0])


def test_single_tile_batches_are_read_only_views_and_the_checksum_sees_a_write(graph):
    """A single-tile batch hands out VIEWS of the slide-level stores (no copy per batch): `TilePartition.checksum()` is
    unchanged by an epoch of batches and changes when a consumer edits an edge list in place (the contract is
    documented on `TilePartition.batch`; this is the cheap regression check)."""
    part = T.partition_by_tiling(graph, T.SquareTiling(all_pos(graph), 25.0), margin=2.0)
    before = part.checksum()
    for t in range(len(part)):
        b = part.tile(t)
        ei = b[("tx", "neighbors", "tx")].edge_index
        if ei.numel():
            assert ei.data_ptr() >= part.data[("tx", "neighbors", "tx")].edge_index.data_ptr()     # a view, not a copy
    assert part.checksum() == before
    t = next(t for t in range(len(part)) if part.tile(t)[("tx", "neighbors", "tx")].edge_index.numel())
    part.tile(t)[("tx", "neighbors", "tx")].edge_index.add_(1)           # what a consumer must NOT do
    assert part.checksum() != before


def test_fov_graph_subset_is_the_induced_subgraph():
    """``synthetic.fov_graph`` with node subsets (what a data-parallel rank assembles from its own tiles' nodes and edges,
    ``fov.build_fov_shard``): node attributes are the selected rows, ``index`` keeps the GLOBAL ids, and edges given in
    global ids come back in the subset's numbering -- the induced subgraph of the full graph."""
    from segger_amd.hetero import TX_BD, TX_NB_BD, TX_TX
    from segger_amd.synthetic import fov_graph
    g = torch.Generator().manual_seed(4)
    nt, nb, G = 200, 30, 16
    nodes = dict(centres=torch.rand(nb, 2, generator=g), bd_type=torch.randint(0, 4, (nb,), generator=g),
                 bd_x=torch.randn(nb, 8, generator=g), cell=torch.randint(0, nb, (nt,), generator=g),
                 pos=torch.rand(nt, 2, generator=g), gene=torch.randint(0, G, (nt,), generator=g),
                 gene_cluster=torch.randint(0, 4, (G,), generator=g), aux={})
    tx_ids = torch.arange(nt)[torch.rand(nt, generator=g) < 0.4]
    bd_ids = torch.arange(nb)[torch.rand(nb, generator=g) < 0.5]
    keep_t, keep_b = torch.zeros(nt, dtype=torch.bool), torch.zeros(nb, dtype=torch.bool)
    keep_t[tx_ids] = True; keep_b[bd_ids] = True
    ett = torch.randint(0, nt, (2, 900), generator=g)
    etb = torch.stack([torch.randint(0, nt, (300,), generator=g), torch.randint(0, nb, (300,), generator=g)])
    ep = torch.stack([torch.randint(0, nt, (400,), generator=g), torch.randint(0, nb, (400,), generator=g)])
    full = fov_graph(nodes, (ett, etb, ep))
    sub_edges = (ett[:, keep_t[ett[0]] & keep_t[ett[1]]], etb[:, keep_t[etb[0]] & keep_b[etb[1]]], ep[:, keep_t[ep[0]] & keep_b[ep[1]]])
    sub = fov_graph(nodes, sub_edges, tx_ids, bd_ids)
    assert torch.equal(full["tx"]["index"], torch.arange(nt)) and torch.equal(sub["tx"]["index"], tx_ids)
    assert torch.equal(sub["bd"]["index"].long(), bd_ids)
    for a in ("x", "pos", "cluster", "cell"):
        assert torch.equal(sub["tx"][a], full["tx"][a][tx_ids]), a
    for a in ("x", "pos", "cluster"):
        assert torch.equal(sub["bd"][a], full["bd"][a][bd_ids]), a
    for et, e_glob, (ids_s, ids_d) in ((TX_TX, sub_edges[0], (tx_ids, tx_ids)), (TX_BD, sub_edges[1], (tx_ids, bd_ids)),
                                      (TX_NB_BD, sub_edges[2], (tx_ids, bd_ids))):
        loc = sub[et].edge_index
        assert loc.shape == e_glob.shape
        assert torch.equal(ids_s[loc[0]], e_glob[0]) and torch.equal(ids_d[loc[1]], e_glob[1])


# ---------------------------------------------------------------------------------------- segments
def test_segments_group_slice_and_lay_out():
    """``Segments`` on its own: segments 1 and 3 of four are empty."""
    seg = T.Segments.from_labels(torch.tensor([2, 0, 2, 2, 0]), 4)
    assert seg.perm.tolist() == [1, 4, 0, 2, 3]                            # the stable order
    assert seg.sizes.tolist() == [2, 0, 3, 0] and seg.indptr.tolist() == [0, 2, 2, 5, 5] == seg.ptr
    assert [seg.size(t) for t in range(4)] == [2, 0, 3, 0] and seg.span(2) == (2, 5) and seg.span(3) == (5, 5)
    v = torch.arange(15.0).reshape(5, 3)[seg.perm]
    e = torch.arange(10).reshape(2, 5)[:, seg.perm]
    for t in (1, 3):                                                        # empty views with the right trailing shape
        assert seg.view(v, t).shape == (0, 3) and seg.view(v, t).dtype == v.dtype
        assert seg.view(e, t, dim=1).shape == (2, 0) and seg.view(e, t, dim=1).dtype == e.dtype
    assert seg.view(v, 2)[:, 0].tolist() == [0.0, 6.0, 9.0] and seg.view(e, 0, dim=1).tolist() == [[1, 4], [6, 9]]
    assert seg.take(v, []).shape == (0, 3) and seg.take(e, [], dim=1).shape == (2, 0)
    assert seg.take(v, [3]).shape == (0, 3)
    assert seg.take(v, [2, 0])[:, 0].tolist() == [0.0, 6.0, 9.0, 3.0, 12.0]
    assert seg.take(e, [2, 0], dim=1).tolist() == [[0, 2, 3, 1, 4], [5, 7, 8, 6, 9]]
    for t in (0, 2):                                                        # one id: the view itself, no copy
        assert seg.take(v, [t]).data_ptr() == seg.view(v, t).data_ptr() == v.data_ptr() + seg.ptr[t] * 3 * v.element_size()
        assert seg.take(e, [t], dim=1).data_ptr() == e.data_ptr() + seg.ptr[t] * e.element_size()
    assert seg.layout([]) == ([], [], 0) and seg.layout([2]) == ([3], [0], 3)
    assert seg.layout([2, 1, 0, 3]) == ([3, 0, 2, 0], [0, 3, 3, 5], 5)
    ends = seg.with_ends()                                                  # a store with one more entry behind every segment
    assert type(ends) is T.Segments
    assert [ends.span(t) for t in range(4)] == [(seg.ptr[t] + t, seg.ptr[t + 1] + t + 1) for t in range(4)]
    assert ends.view(torch.arange(9), 2).tolist() == [4, 5, 6, 7] and ends.view(torch.arange(9), 3).tolist() == [8]
    given = T.Segments(torch.tensor([3, 0, 2]))                             # from sizes: no permutation
    assert given.perm is None and given.ptr == [0, 3, 3, 5]
    for bad in ([0, -1], [0, 4]):
        with pytest.raises(ValueError, match=r"tile labels must lie in \[0, 4\)"):
            T.Segments.from_labels(torch.tensor(bad), 4)
    with pytest.raises(ValueError, match=r"node type 'tx': tile labels must lie in \[0, 4\)"):
        T.Segments.from_labels(torch.tensor([4]), 4, "node type 'tx'")


# ------------------------------------------------------------------------- a partition with holes
@pytest.fixture(scope="module")
def holed():
    from tile_cases import MARGIN, SIDE, holed_graph
    g = holed_graph()
    tiling = T.SquareTiling(torch.cat([g["tx"].pos, g["bd"].pos]), SIDE)
    labels = {nt: tiling.label(g[nt].pos) for nt in ("tx", "bd")}
    return g, tiling, labels, T.partition_by_tiling(g, tiling, margin=MARGIN)


def test_holed_partition_has_the_holes(holed):
    from tile_cases import EMPTY_TILE, NO_BD_TILE, NO_BELONGS_TILE
    g, tiling, labels, part = holed
    assert len(tiling) == 9 and 250 <= g["tx"].num_nodes <= 400 and 20 <= g["bd"].num_nodes <= 40
    assert part.node_sizes["tx"][EMPTY_TILE] == 0 and part.node_sizes["bd"][EMPTY_TILE] == 0
    assert all(int(v[EMPTY_TILE]) == 0 for v in part.edge_sizes.values())
    assert part.node_sizes["tx"][NO_BD_TILE] > 0 and part.node_sizes["bd"][NO_BD_TILE] == 0
    assert part.node_sizes["bd"][NO_BELONGS_TILE] > 0 and part.edge_sizes[TX_BD][NO_BELONGS_TILE] == 0
    assert part.edge_sizes[TX_TX][NO_BELONGS_TILE] > 0 and part.edge_sizes[TX_NB_BD][NO_BELONGS_TILE] > 0
    for et in (TX_TX, TX_BD, TX_NB_BD):                                     # some edges cross tiles and were dropped
        assert 0 < int(part.edge_sizes[et].sum()) < g[et].edge_index.shape[1]


def test_holed_partition_batches_equal_brute_force_collate(holed):
    from tile_cases import EMPTY_TILE, NO_BD_TILE, assert_batch_equals_naive
    g, tiling, labels, part = holed
    cases = [[]] + [[t] for t in range(9)] + [[EMPTY_TILE, 2], [NO_BD_TILE, EMPTY_TILE], [7, 1], list(range(8, -1, -1))]
    for ids in cases:
        assert_batch_equals_naive(part.batch(ids), g, tiling, labels, ids)
    assert_batch_equals_naive(part.batch([-1]), g, tiling, labels, [8])
    assert_batch_equals_naive(part.batch([-9, -5]), g, tiling, labels, [0, 4])
    for t in range(9):                                                      # one tile: views of the slide stores
        b = part.batch([t])
        for nt in ("tx", "bd"):
            for a in ("x", "pos", "index", "cluster", "mask"):
                assert b[nt][a].untyped_storage().data_ptr() == part.data[nt][a].untyped_storage().data_ptr()
        for et in (TX_TX, TX_BD, TX_NB_BD):
            assert b[et].edge_index.untyped_storage().data_ptr() == part.data[et].edge_index.untyped_storage().data_ptr()


def _same_batch(x, y):
    assert x.num_graphs == y.num_graphs
    for nt in ("tx", "bd"):
        assert set(x[nt].keys()) == set(y[nt].keys())
        for k, v in y[nt].items():
            assert x[nt][k].dtype == v.dtype and torch.equal(x[nt][k], v), (nt, k)
    for et in (TX_TX, TX_BD, TX_NB_BD):
        assert torch.equal(x[et].edge_index, y[et].edge_index), et


def _storages(part):
    ts = [v for st in list(part.data._nodes.values()) + list(part.data._edges.values()) for v in st.values()]
    for d in (part.node_perm, part.node_indptr, part.node_sizes, part.edge_indptr, part.edge_sizes):
        ts += list(d.values())
    return {t.untyped_storage().data_ptr() for t in ts if isinstance(t, torch.Tensor) and t.numel()}


def test_holed_partition_shards_equal_the_parent_batch_by_batch(holed):
    g, tiling, labels, part = holed
    ids = [5, 0, 4, 7, 1]                                                   # permuted, with the empty tile
    sh = part.shard(ids)
    assert len(sh) == 5
    for nt in ("tx", "bd"):
        assert sh.node_sizes[nt].tolist() == part.node_sizes[nt][ids].tolist()
        assert sh.node_indptr[nt].tolist() == [0] + part.node_sizes[nt][ids].cumsum(0).tolist()
    for loc in ([], [0], [1], [2], [3], [4], [3, 1], [2, 4], [4, 3, 2, 1, 0]):
        _same_batch(sh.batch(loc), part.batch([ids[i] for i in loc]))
    sub = sh.shard([3, 2, 0])                                               # a shard of a shard
    for loc in ([0], [1], [2], [2, 1, 0]):
        _same_batch(sub.batch(loc), part.batch([[7, 4, 5][i] for i in loc]))
    none = part.shard([])
    assert len(none) == 0 and none.batch([]).num_graphs == 0 and none.resident_bytes() == part.shard([]).resident_bytes()
    _same_batch(none.batch([]), part.batch([]))
    # the resident_bytes contract: a shard owns what it keeps
    assert not (_storages(sh) & _storages(part)) and not (_storages(sub) & _storages(sh))
    assert sub.resident_bytes() < sh.resident_bytes() < part.resident_bytes()
    assert part.checksum() == T.partition_by_tiling(g, tiling, margin=1.0).checksum()


def test_shard_carries_the_settings_and_starts_with_an_empty_store(holed):
    g, tiling, labels, _ = holed
    part = T.partition_by_tiling(g, tiling, margin=1.0)
    default = T.TilePartition.csr_sort_max_edges
    assert part.persist_max is None and part.csr_max_tiles == 1 and part._csr is None and part.csr_sort_max_edges == default
    plain = part.shard([2, 3])
    assert plain.persist_max is None and plain.csr_max_tiles == 1 and plain.csr_sort_max_edges == default
    part.persist_max, part.csr_sort_max_edges, part.csr_max_tiles = 5, 123, 7
    part.batch([0]); part.batch([1, 2])
    assert len(part._persist) == 2
    sh = part.shard([2, 3])
    assert (sh.persist_max, sh.csr_sort_max_edges, sh.csr_max_tiles) == (5, 123, 7)
    assert len(sh._persist) == 0 and sh._csr is None and sh._src_unique == {}
    assert sh.shard([1]).csr_sort_max_edges == 123                          # ... and so do its own shards
    assert T.TilePartition.csr_sort_max_edges == default                    # the override stayed on the instance


def test_a_shard_has_every_attribute_a_fresh_partition_has(holed):
    """A shard goes through the initialiser of a fresh partition: no attribute can be missing from it."""
    g, tiling, labels, _ = holed
    part = T.partition_by_tiling(g, tiling, margin=1.0)
    fresh = set(vars(part))
    assert {"persist_max", "csr_max_tiles", "_csr", "_src_unique", "_persist", "_zero_vec", "node_perm", "node_indptr",
            "node_sizes", "edge_indptr", "edge_sizes", "data", "num_tiles"} <= fresh
    assert set(vars(part.shard([3, 1]))) == fresh and set(vars(part.shard([]))) == fresh
    part.batch([0]); part.batch([0, 1])                                     # using a partition adds no attribute either
    assert set(vars(part)) == fresh
    assert set(vars(part.shard([0]).shard([0]))) == fresh


# (the parent commit's single module segger_amd/tiles.py: what it defined, and the project types it re-exported;
#  names of the standard library, typing and torch that it merely imported are not part of the surface)
TILES_NAMES = ("EdgeType", "HeteroBatch", "NODE_SKIP", "PredictQuadTreeIndex", "PredictTileIndex", "PredictTiles",
               "QuadTreeTiling", "SquareTiling", "TileBatchSampler", "TilePartition", "_BinnedPredictTiles", "_indexed",
               "best_fit_decreasing", "first_fit_decreasing_bucketed", "harmonic_k", "partition_by_tiling")


def test_tiles_package_keeps_the_import_surface_of_the_module():
    import importlib
    mod = importlib.import_module("segger_amd.tiles")
    for name in TILES_NAMES:
        assert hasattr(mod, name), name
        assert getattr(__import__("segger_amd.tiles", fromlist=[name]), name) is getattr(mod, name)
    from segger_amd.tiles import (PredictQuadTreeIndex, PredictTileIndex, PredictTiles, QuadTreeTiling,  # noqa: F401
                                  SquareTiling, TileBatchSampler, TilePartition, partition_by_tiling)
    assert issubclass(PredictTileIndex, PredictTiles) and issubclass(PredictQuadTreeIndex, PredictTiles)
