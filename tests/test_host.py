"""Host-side logic on the CPU: C-ABI surface, data contract, synthetic generator, module tree,
metric-loss sampling, loud failure without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def header_functions():
    src = open(os.path.join(ROOT, "include", "segger_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(segger_[a-z0-9_]+)\s*\(", src)))


def header_abi_version():
    src = open(os.path.join(ROOT, "include", "segger_amd.h")).read()
    return int(re.search(r"#define\s+SEGGER_ABI_VERSION\s+(\d+)", src).group(1))


def test_library_exports_only_the_c_entry_points():
    """The dynamic symbol table of the built library is exactly the header's declarations: no C++ launcher
    (``_ZN6segger...``), no kernel handle, no rocPRIM template (csrc/exports.map + -fvisibility=hidden)."""
    import shutil
    import subprocess
    from segger_amd import _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert syms == header_functions(), [s_ for s_ in syms if s_ not in header_functions()][:5]
    assert not any("_ZN6segger" in s_ for s_ in syms)


def test_library_exports_every_declared_symbol():
    from segger_amd import _lib
    lib = _lib.load()                      # loads without a GPU; no compute call is made
    names = header_functions()
    assert len(names) >= 12
    assert sorted(_lib.EXPORTS) == names, "ctypes binding and header disagree"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/segger_amd.h but not exported"
    assert lib.segger_abi_version() == _lib.ABI_VERSION == header_abi_version()
    assert lib.segger_csr_from_coo_workspace_bytes(0, 10) > 0
    assert lib.segger_gatv2_bwd_workspace_bytes(1000, 2, 64) >= 1000 // 32 * 2 * 128 * 4
    assert lib.segger_triplet_workspace_bytes(1000) >= 16 * 4


def test_argument_errors_are_reported_not_thrown():
    from segger_amd import _lib
    lib = _lib.load()
    a = _lib.GatFwdArgs()
    a.heads, a.channels = 2, 64
    rc = lib.segger_gatv2_fwd(ctypes.byref(a), None)       # NULL indptr: rejected on the host, nothing launched
    assert rc == -1 and b"indptr" in lib.segger_last_error()
    assert lib.segger_gatv2_fwd(None, None) == -1
    t = _lib.TripletArgs(); t.n_edges, t.channels = -1, 64
    assert lib.segger_triplet_fwd(ctypes.byref(t), None) == -1


def test_product_fails_loudly_on_cpu_tensors():
    from segger_amd import LitISTEncoder, _lib
    from segger_amd.synthetic import C1, make_graph
    b = make_graph(C1)
    m = LitISTEncoder(n_genes=C1.n_genes, in_channels=32)
    with pytest.raises(_lib.SeggerAmdError, match="no CPU fallback"):
        m(b)


def test_missing_library_raises(monkeypatch, tmp_path):
    from segger_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libsegger_amd.so"))
    with pytest.raises(_lib.SeggerAmdError, match="not built"):
        _lib.load()


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "segger_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "segger_oracle" not in src and "import oracle" not in src, f


def test_state_dict_keys_follow_the_reference():
    from segger_amd import LitISTEncoder
    m = LitISTEncoder(n_genes=10, in_channels=16, hidden_channels=8, out_channels=8, n_mid_layers=2, n_heads=2)
    m.model._materialize_bd(5, "cpu")
    keys = set(m.state_dict())
    want = {"model.lin_first.tx.weight", "model.lin_first.bd.weight", "model.lin_first.bd.bias",
            "model.pos_emb.mlp.0.weight", "model.pos_emb.mlp.2.bias",
            "model.conv_layers.0.conv.convs.<tx___neighbors___tx>.lin_l.weight",
            "model.conv_layers.3.conv.convs.<tx___belongs___bd>.att",
            "model.conv_layers.2.conv.convs.<tx___belongs___bd>.lin_r.bias",
            "model.conv_layers.1.conv.convs.<tx___neighbors___tx>.bias",
            "model.lin_last.lins.tx.weight", "model.lin_last.lins.bd.bias"}
    assert want <= keys
    sd = m.state_dict()
    assert sd["model.conv_layers.0.conv.convs.<tx___neighbors___tx>.lin_l.weight"].shape == (16, 32)   # [H*C, 2*in]
    assert sd["model.conv_layers.1.conv.convs.<tx___belongs___bd>.att"].shape == (1, 2, 8)
    assert sd["model.lin_last.lins.tx.weight"].shape == (8, 16)
    assert len(m.model.conv_layers) == 4
    import inspect
    sig = inspect.signature(LitISTEncoder.__init__)
    assert list(sig.parameters)[1:] == [
        "n_genes", "in_channels", "hidden_channels", "out_channels", "n_mid_layers", "n_heads", "learning_rate",
        "sg_loss_type", "tx_margin", "sg_margin", "tx_weight_start", "tx_weight_end", "bd_weight_start",
        "bd_weight_end", "sg_weight_start", "sg_weight_end", "update_gene_embedding",
        "use_positional_embeddings", "normalize_embeddings"]
    assert sig.parameters["sg_margin"].default == 0.4 and sig.parameters["n_heads"].default == 2
    with pytest.raises(ValueError, match="Unrecognized segmentation loss"):
        LitISTEncoder(n_genes=3, in_channels=8, sg_loss_type="hinge")
    assert isinstance(m.configure_optimizers(), torch.optim.Adam)


def test_reference_checkpoint_loads_strictly():
    """A reference-shaped state dict (trained ``lin_first.bd`` of the reference's lazy Linear + the never-initialised
    ``<bd___contains___tx>`` placeholders) loads with strict=True into a fresh module and keeps the
    boundary projection's trained values (no random re-materialisation on the first forward)."""
    from segger_amd import LitISTEncoder
    kw = dict(n_genes=10, in_channels=16, hidden_channels=8, out_channels=8, n_mid_layers=2, n_heads=2)
    src = LitISTEncoder(**kw)
    src.model._materialize_bd(5, "cpu")
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    for li in range(4):                                     # what PyG saves for an uninitialised lazy conv
        p = f"model.conv_layers.{li}.conv.convs.<bd___contains___tx>."
        for name in ("lin_l.weight", "lin_r.weight", "att", "bias", "lin_l.bias", "lin_r.bias"):
            sd[p + name] = torch.empty(0)
    m = LitISTEncoder(**kw)
    assert "bd" not in m.model.lin_first
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.model.lin_first["bd"].weight, src.model.lin_first["bd"].weight)
    assert m.model.lin_first["bd"].in_features == 5
    m.model._materialize_bd(5, "cpu")                        # what the first forward calls: must keep the loaded weights
    assert torch.equal(m.model.lin_first["bd"].bias, src.model.lin_first["bd"].bias)
    assert set(m.state_dict()) == set(src.state_dict())
    with pytest.raises(RuntimeError):                        # a genuinely foreign key is still an error
        LitISTEncoder(**kw).load_state_dict({**sd, "model.foo.weight": torch.zeros(1)}, strict=True)


def test_setup_requires_datamodule_similarities():
    from segger_amd import LitISTEncoder

    class T:  # noqa: D401
        max_epochs = 20
        datamodule = object()
    m = LitISTEncoder(n_genes=3, in_channels=8)
    m.trainer = T()
    with pytest.raises(TypeError, match="ISTDataModule"):
        m.setup("fit")

    class DM:
        tx_similarity = torch.eye(3)
        bd_similarity = torch.eye(3)
    T.datamodule = DM()
    m.setup("fit")
    assert m.loss_tx is not None and m.loss_bd is not None


def test_scheduled_weights_match_oracle(oracle):
    from segger_amd import LitISTEncoder
    m = LitISTEncoder(n_genes=3, in_channels=8)
    m._max_epochs_override = 20
    for epoch in (0, 5, 19, 40):
        m.current_epoch = epoch
        w = m._scheduled_weights(m._w_start, m._w_end)
        assert torch.allclose(w, oracle.scheduled_weights(m._w_start, m._w_end, epoch, 20), atol=1e-7)


def test_scheduled_weights_match_reference_outputs():
    """The product's ``_scheduled_weights`` against the table the reference's own method produced
    (tests/golden/reference_heads.npz, lightning_model.py:136-149)."""
    from segger_amd import LitISTEncoder
    z = np.load(os.path.join(GOLD, "reference_heads.npz"))
    m = LitISTEncoder(n_genes=3, in_channels=8)
    ws, we = torch.from_numpy(z["sched::w_start"]), torch.from_numpy(z["sched::w_end"])
    for row in z["sched::table"]:
        m._max_epochs_override, m.current_epoch = int(row[0]), int(row[1])
        assert np.allclose(m._scheduled_weights(ws, we).numpy(), row[2:5], atol=1e-6)
        assert np.allclose(m._scheduled_weights(ws, we, normalize=False).numpy(), row[5:8], atol=1e-6)


def test_hetero_batch_contract_and_collate():
    from segger_amd.hetero import TX_BD, TX_NB_BD, TX_TX, collate
    from segger_amd.synthetic import SyntheticSpec, make_graph
    tiles = [make_graph(SyntheticSpec(n_tx=50 + 10 * i, n_bd=6 + i, k_tx=3, seed=i)) for i in range(3)]
    b = collate(tiles)
    assert b.num_graphs == 3 and b["tx"].num_nodes == 50 + 60 + 70 and b["bd"].num_nodes == 6 + 7 + 8
    assert set(b.edge_index_dict) == {TX_TX, TX_BD, TX_NB_BD}
    assert b.batch_dict["tx"].bincount().tolist() == [50, 60, 70]
    e2 = tiles[2][TX_BD].edge_index
    got = b[TX_BD].edge_index[:, -e2.shape[1]:]
    assert torch.equal(got[0], e2[0] + 110) and torch.equal(got[1], e2[1] + 13)
    assert b.x_dict["tx"].dtype == torch.int32 and b.pos_dict["bd"].shape == (21, 2)
    assert b["tx"]["mask"].all() and b["tx"].predict_mask.dtype == torch.bool


def test_synthetic_graph_invariants():
    from segger_amd.hetero import TX_BD, TX_NB_BD, TX_TX
    from segger_amd.synthetic import SyntheticSpec, make_graph
    spec = SyntheticSpec(n_tx=2000, n_bd=64, k_tx=7, n_graphs=4, seed=9)
    b, aux = make_graph(spec, return_aux=True)
    b2 = make_graph(spec)
    assert torch.equal(b[TX_TX].edge_index, b2[TX_TX].edge_index) and torch.equal(b["tx"].pos, b2["tx"].pos)
    ett = b[TX_TX].edge_index
    assert ett.shape == (2, 2000 * 7)
    assert torch.equal(ett[0], torch.arange(2000).repeat_interleave(7))        # source = query point, out-degree k
    assert ((ett[0] == ett[1]).view(2000, 7).sum(1) == 1).all()                # kNN includes self
    etb = b[TX_BD].edge_index
    assert torch.equal(aux["cell"][etb[0]], etb[1]) and 0.25 < etb.shape[1] / 2000 < 0.55
    ep = b[TX_NB_BD].edge_index
    assert ep[0].bincount(minlength=2000).max() <= 3 and 0.3 < aux["label"].float().mean() < 0.9
    assert b.batch_dict["tx"].max() == 3 and b["tx"].x.max() < spec.n_genes
    assert torch.allclose(aux["tx_similarity"].diagonal(), torch.ones(8), atol=1e-5)


def test_product_selector_matches_reference_vectors():
    """segger_amd.triplet_loss (device-agnostic torch code) against vectors produced by the reference file."""
    from segger_amd.triplet_loss import FastTripletSelector, MetricLoss, TripletLoss
    z = np.load(os.path.join(GOLD, "triplet_selector.npz"))
    sim, labels = torch.from_numpy(z["similarity"]), torch.from_numpy(z["labels"])
    emb = torch.from_numpy(z["embeddings"])
    torch.manual_seed(int(z["seed"]))
    pos, neg, dp, dn = FastTripletSelector(sim).sample_triplets(labels)
    assert np.array_equal(pos.numpy(), z["positives"]) and np.array_equal(neg.numpy(), z["negatives"])
    assert np.allclose(dp.numpy(), z["dists_pos"]) and np.allclose(dn.numpy(), z["dists_neg"])
    torch.manual_seed(int(z["seed"]))
    assert abs(float(TripletLoss(sim, margin=float(z["margin"])).forward(emb, labels)) - float(z["triplet_loss"])) < 1e-6
    torch.manual_seed(int(z["seed"]))
    assert abs(float(MetricLoss(sim).forward(emb, labels)) - float(z["metric_loss"])) < 1e-6
    assert TripletLoss(sim).forward(emb[:0], labels[:0]) == 0.0


def test_assign_tiles_balances_load():
    from segger_amd.dp import assign_tiles
    w = [9, 7, 6, 5, 5, 4, 3, 1]
    parts = assign_tiles(w, 3)
    assert sorted(i for p in parts for i in p) == list(range(8))
    loads = [sum(w[i] for i in p) for p in parts]
    assert max(loads) - min(loads) <= 2
    assert assign_tiles(w, 3) == parts and assign_tiles([], 2) == [[], []]


def _emulate_stage(segments):
    """CPU restatement of segger_stage (include/segger_amd.h) for the host-logic tests: copy the source to the front
    of the destination, fill the rest by the segment's formula."""
    for dst, src, fill, a, b, c in segments:
        n_copy = 0 if src is None else src.numel()
        flat = dst.view(-1)
        if n_copy:
            flat[:n_copy] = src.reshape(-1).to(flat.dtype)
        k = torch.arange(flat.numel() - n_copy)
        if fill == "const":
            flat[n_copy:] = a
        elif fill == "tile":
            flat[n_copy:] = src.reshape(-1)[k % a].to(flat.dtype)
        elif fill == "div":
            flat[n_copy:] = (a + k // b).to(flat.dtype)
        elif fill == "mod":
            flat[n_copy:] = (a + k % b).to(flat.dtype)
        elif fill == "ramp":
            flat[n_copy:] = (a + torch.clamp((k + 1) * b, max=c)).to(flat.dtype)
        else:
            raise AssertionError(fill)


@pytest.mark.parametrize("pad_cols", [None, "mod"])
@pytest.mark.parametrize("n_real,n_rows,e_pad_extra", [(7, 9, 5), (7, 8, 40), (1, 4, 0), (20, 33, 13)])
def test_padded_view_segments_build_a_valid_csr_without_sorting(n_real, n_rows, e_pad_extra, pad_cols):
    """graph.padded_view_segments (how a batch's CSR view is written into the static buffers of a captured step):
    the padded view must be a CSR of the real edges plus padding edges that touch dummy rows / columns only, slots in
    row order, edge ids a permutation of 0..E_pad-1 with the real ones unchanged."""
    from segger_amd.graph import EdgeCSR, padded_view_segments
    g = torch.Generator().manual_seed(n_real + e_pad_extra)
    n_cols_real, n_cols = 11, 15
    deg = torch.randint(0, 5, (n_real,), generator=g)
    e = int(deg.sum())
    src = EdgeCSR(torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]),
                  torch.randint(0, n_real if pad_cols is None else n_cols_real, (e,), generator=g).int(),
                  torch.randperm(e, generator=g).int(), n_real, n_real if pad_cols is None else n_cols_real)
    e_pad = e + e_pad_extra
    dst = EdgeCSR(torch.full((n_rows + 1,), -1, dtype=torch.long), torch.full((e_pad,), -1, dtype=torch.int32),
                  torch.full((e_pad,), -1, dtype=torch.int32), n_rows, n_rows if pad_cols is None else n_cols)
    fill = None if pad_cols is None else ("mod", n_cols_real, n_cols - n_cols_real)
    _emulate_stage(padded_view_segments(dst, src, n_real, fill))
    ip = dst.indptr
    assert ip[0] == 0 and ip[-1] == e_pad and bool((ip[1:] >= ip[:-1]).all())
    assert torch.equal(ip[: n_real + 1], src.indptr) and torch.equal(dst.col[:e], src.col) and torch.equal(dst.eid[:e], src.eid)
    assert torch.equal(torch.sort(dst.eid.long()).values, torch.arange(e_pad))
    rows = torch.repeat_interleave(torch.arange(n_rows), ip[1:] - ip[:-1])
    assert bool((rows[e:] >= n_real).all())                               # padding edges hang on dummy rows ...
    if pad_cols is None:
        assert torch.equal(dst.col[e:].long(), rows[e:])                  # ... as self-loops
    else:
        assert bool(((dst.col[e:] >= n_cols_real) & (dst.col[e:] < n_cols)).all())    # ... or point at dummy columns
    with pytest.raises(ValueError):
        padded_view_segments(EdgeCSR(ip[: n_real + 1].clone(), dst.col[:e], dst.eid[:e], n_real, n_real), src, n_real)


def test_step_bucket_sizes_leave_a_dummy_of_every_kind():
    from segger_amd.hetero import HeteroBatch, TX_BD, TX_TX
    from segger_amd.train_step_graph import step_bucket
    b = HeteroBatch(num_graphs=3)
    b["tx"]["x"] = torch.zeros(50_000, dtype=torch.long)
    b["bd"]["x"] = torch.zeros(512, 4)
    b[TX_TX]["edge_index"] = torch.zeros(2, 730_000, dtype=torch.long)
    b[TX_BD]["edge_index"] = torch.zeros(2, 19_000, dtype=torch.long)
    s = step_bucket(b, granularity=1.06)
    assert s["tx"] > 50_000 and s["bd"] > 512 and s["e_tt"] >= 730_000 and s["e_tb"] >= 19_000 and s["graphs"] >= 3
    assert s["tx"] <= 50_000 * 1.07 and s["e_tt"] <= 730_000 * 1.07          # one granule at most on the transcript side
    assert step_bucket(b, granularity=1.06) == s


def test_edge_csr_struct_cache_follows_the_storage_not_the_object_id():
    """EdgeCSR.c_struct() caches the ctypes struct per view; the cache must notice a tensor whose storage moved
    (``set_`` keeps the Python object) and a replaced field (a freed tensor's id() can be reused)."""
    from segger_amd.graph import EdgeCSR
    indptr = torch.tensor([0, 1, 2], dtype=torch.int64)
    col = torch.tensor([1, 0], dtype=torch.int32)
    eid = torch.tensor([0, 1], dtype=torch.int32)
    g = EdgeCSR(indptr, col, eid, 2, 2)
    c0 = g.c_struct()
    assert g.c_struct() is c0                               # cached
    assert c0.col == col.data_ptr()
    other = torch.tensor([0, 1], dtype=torch.int32)
    col.set_(other)                                         # same object, new storage
    c1 = g.c_struct()
    assert c1 is not c0 and c1.col == other.data_ptr()
    g.eid = torch.tensor([1, 0], dtype=torch.int32)         # replaced field
    c2 = g.c_struct()
    assert c2 is not c1 and c2.eid == g.eid.data_ptr()


def test_embedder_pair_route_declines_what_it_does_not_cover():
    """ist_encoder._pair_node (both node types' positional embeddings behind one autograd node) applies to the fused 16-bit
    embedder on the GPU with batch vectors and a graph count; anywhere else it returns None and the caller embeds each type
    by its own call -- no CPU route, no silent fp32 substitute."""
    import torch
    import segger_amd.ist_encoder as ie
    emb = ie.Positional2dEmbedder(128)
    pos_a, pos_b = torch.rand(10, 2), torch.rand(4, 2)
    ba, bb = torch.zeros(10, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    assert ie._pair_node(emb, pos_a, ba, pos_b, bb, 1, torch.bfloat16) is None          # CPU tensors
    from segger_amd import ops
    assert ops.POS_PAIR_NODE is True
    l0, l2 = emb.mlp[0], emb.mlp[2]
    assert not ops.posmlp_pair_supported(l0.weight, l0.bias, l2.weight, l2.bias, torch.float32)
    with torch.no_grad():
        assert not ops.posmlp_pair_supported(l0.weight, l0.bias, l2.weight, l2.bias, torch.bfloat16)


def test_front_plan_truth_table(monkeypatch):
    """``ISTEncoder.front_plan``: the input stage's route from shapes, dtypes, grad mode and the ``ops`` switches alone (no
    launch, no GPU).  Expected values: the conditions of the encoder as it stood before the plan existed -- table: width a
    multiple of 32 and an fp32 embedding; split: table, on the GPU, rows >= 200 000 (fp32: 4 096), widths covered; join:
    table and FRONT_JOIN; merged: staged positions, or MERGED_POS_EMBED and not split and batch vectors + graph count;
    pair_node: split and join and not merged and the fused 16-bit embedder with something to differentiate."""
    import torch
    from segger_amd import ops
    from segger_amd.ist_encoder import FrontPlan, ISTEncoder

    def enc(dtype, **kw):
        kw.setdefault("in_channels", 128)
        return ISTEncoder(256, hidden_channels=64, out_channels=64, n_heads=2, bd_in_channels=128, compute_dtype=dtype, **kw)

    def plan(e, n_tx, on_gpu=True, batched=True, **kw):
        return e.front_plan(n_tx, on_gpu=on_gpu, batched=batched, **kw)

    P = lambda **kw: FrontPlan(positional=True, **kw)
    bf, f32 = enc(torch.bfloat16), enc(torch.float32)
    big = P(table=True, split=True, join=True, pair_node=True)
    small = P(table=True, join=True, merged=True)
    assert plan(bf, 1_000_000) == big
    assert plan(bf, 200_000) == big and plan(bf, 199_999) == small
    assert plan(bf, 9_000) == small
    assert plan(f32, 9_000) == P(table=True, split=True, join=True)                # fp32 threshold: 4 096 rows
    assert plan(f32, 4_096).split and not plan(f32, 4_095).split
    assert plan(f32, 1_000) == small
    assert plan(f32, 1_000_000) == P(table=True, split=True, join=True)            # (the one-node pair is 16-bit)
    for n in (9_000, 1_000_000):
        assert plan(enc(torch.bfloat16, in_channels=48), n) == P(merged=True)      # no table, no join, nothing to split
        assert plan(enc(torch.bfloat16, use_positional_embeddings=False), n) == FrontPlan()
        # no batch vector for a node type, or no graph count: one call per type, each its own node
        assert plan(bf, n, batched=False) == (big if n > 9_000 else small)._replace(merged=False, pair_node=False)
        # a captured step concatenated the positions itself: one call, split or not
        assert plan(bf, n, staged_pos=True) == (big if n > 9_000 else small)._replace(merged=True, pair_node=False)
    assert plan(bf, 1_000_000, on_gpu=False) == P(table=True, join=True, merged=True)    # the table GEMMs are GPU kernels
    with torch.no_grad():
        assert plan(bf, 1_000_000) == big._replace(pair_node=False)                # nothing to differentiate
        assert plan(bf, 9_000) == small
    # each switch off in turn: its field off, and what hangs on that field with it
    off = {"FUSED_POSMLP": (big._replace(pair_node=False), small),
           "MERGED_POS_EMBED": (big, small._replace(merged=False)),
           "FRONT_JOIN": (big._replace(join=False, pair_node=False), small._replace(join=False)),
           "POS_PAIR_NODE": (big._replace(pair_node=False), small),
           "SPLIT_FIRST_LAYER": (small, small)}
    for name, (at_big, at_small) in off.items():
        with monkeypatch.context() as mp:
            mp.setattr(ops, name, False)
            assert plan(bf, 1_000_000) == at_big, name
            assert plan(bf, 9_000) == at_small, name
    with monkeypatch.context() as mp:
        mp.setattr(ops, "SPLIT_FIRST_LAYER_MIN_ROWS", 0)
        assert plan(bf, 9_000) == big and plan(f32, 1_000) == small
        mp.setattr(ops, "SPLIT_FIRST_LAYER_MIN_ROWS_F32", 0)
        assert plan(f32, 1_000) == P(table=True, split=True, join=True)
    assert plan(bf, 1_000_000) == big


def test_embedder_route_truth_table(monkeypatch):
    """``Positional2dEmbedder.route``: where an embedder call's sinusoid features come from and which form of the MLP runs,
    from shapes, dtypes and the ``ops`` switches alone (no tensor, no launch, no GPU).  Expected values: the conditions of
    ``_embed`` as it stood before the route existed -- device features (per-graph min / max kernels) with a batch vector or on
    the GPU when the width is a multiple of 16, else torch; the one-kernel embedder: FUSED_POSMLP, GPU, biases, 16-bit, 256 ->
    64; else, at fp32 storage on the GPU with F32_GATE_EPILOGUE, biases and at least one row, one autograd node: the polynomial
    first layer (POS_POLY_F32, positions without a gradient) or segger_posfreq + the one-node MLP; else composed ops.  The
    pair node: that one-kernel embedder, batch vectors + graph count, POS_PAIR_NODE, FUSED_POSMLP_BWD, something to
    differentiate."""
    import torch
    from torch.nn import Linear
    from segger_amd import _lib, ops
    import segger_amd.ist_encoder as ie
    R = ie.EmbedRoute
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    emb = ie.Positional2dEmbedder(128)                       # 256 -> 64 -> 64, as the encoder builds it
    odd = ie.Positional2dEmbedder(128, frequency_embedding_size=250)
    nobias = ie.Positional2dEmbedder(128)
    nobias.mlp[2] = Linear(64, 64, bias=False)

    def route(e, dtype, on_gpu=True, batched=True, rows=1000, **kw):
        return e.route(on_gpu=on_gpu, batched=batched, dtype=dtype, rows=rows, **kw)

    def table():
        return {(name, str(dt)[6:]): route(e, dt) for name, e in (("emb", emb), ("odd", odd), ("nobias", nobias))
                for dt in (bf, f16, f32)}

    fused, poly, composed = R("none", "fused16"), R("none", "poly_f32"), R("posfreq", "composed")
    base = {("emb", "bfloat16"): fused, ("emb", "float16"): fused, ("emb", "float32"): poly,
            ("odd", "bfloat16"): R("torch", "composed"), ("odd", "float16"): R("torch", "composed"),
            ("odd", "float32"): R("torch", "composed"),
            ("nobias", "bfloat16"): composed, ("nobias", "float16"): composed, ("nobias", "float32"): composed}
    assert table() == base
    for dt, want in ((bf, fused), (f16, fused), (f32, poly)):
        assert route(emb, dt, batched=False) == want                       # no batch vector on the GPU: one graph
        assert route(emb, dt, on_gpu=False, batched=False) == R("torch", "composed")
        # a batch vector on the CPU still asks for the device's min / max: refused there, as before (no CPU route)
        assert route(emb, dt, on_gpu=False) == composed
        assert route(odd, dt, on_gpu=False) == R("torch", "composed")
    for batch in (torch.zeros(5, dtype=torch.int64), None):               # (and ops.linear has none either)
        with pytest.raises(_lib.SeggerAmdError, match="no CPU fallback"):
            emb(torch.rand(5, 2), batch, num_graphs=1)
    # the fp32 nodes want at least one row; the polynomial one also positions that are constants (segger_posfreq's features
    # are constants whatever the positions require, so the one-node MLP takes those)
    assert route(emb, f32, rows=0) == composed and route(emb, f32, rows=1) == poly
    assert route(emb, f32, pos_grad=True) == R("posfreq", "mlp_f32")
    assert route(emb, bf, rows=0) == fused and route(emb, f16, pos_grad=True) == fused
    # each switch off in turn
    off = {"FUSED_POSMLP": {("emb", "bfloat16"): composed, ("emb", "float16"): composed},
           "POS_POLY_F32": {("emb", "float32"): R("posfreq", "mlp_f32")},
           "F32_GATE_EPILOGUE": {("emb", "float32"): composed},
           "FUSED_POSMLP_BWD": {}, "POS_PAIR_NODE": {}}
    for name, changed in off.items():
        with monkeypatch.context() as mp:
            mp.setattr(ops, name, False)
            assert table() == {**base, **changed}, name
            if name == "POS_POLY_F32":
                assert route(emb, f32, rows=0) == composed and route(emb, f32, pos_grad=True) == R("posfreq", "mlp_f32")
                mp.setattr(ops, "F32_GATE_EPILOGUE", False)
                assert route(emb, f32) == composed
    assert table() == base
    # the pair node (ops.posmlp_pair) asks the same function
    pair = lambda e, dt, on_gpu=True, batched=True: ie._pair_node_applies(e, on_gpu, batched, dt)
    assert pair(emb, bf) and pair(emb, f16)
    assert not pair(emb, f32) and not pair(emb, bf, on_gpu=False) and not pair(emb, bf, batched=False)
    assert not pair(odd, bf) and not pair(nobias, bf)
    with torch.no_grad():
        assert not pair(emb, bf) and not pair(emb, f16)                    # nothing to differentiate
    for name in ("POS_PAIR_NODE", "FUSED_POSMLP", "FUSED_POSMLP_BWD"):
        with monkeypatch.context() as mp:
            mp.setattr(ops, name, False)
            assert not pair(emb, bf) and not pair(emb, f16), name
    assert pair(emb, bf)


def test_projection_backward_plan_truth_table(monkeypatch):
    """``ops.linear.backward_plan`` / ``backward_pair_plan``: the kernels of a projection backward from shapes, needs, dtype
    and the ``ops`` switches alone (no tensor, no launch, no GPU).  Expected values: the conditions of the four autograd nodes
    as they stood before the plan existed -- one pass (dX, dW, db from one read of dY): FUSED_WGRAD_DX, the input and a
    parameter want gradients, rows > 0, 16-bit and a covered (M, K); else dX by the fp32 gate epilogue (first layer, fp32,
    ``pre`` wants the gradient, aligned rows), the fp32 split (fp32, aligned rows, covered), the MFMA forward kernel on W^T, or
    -- generic site only -- the vendor GEMM; dW / db by the MFMA weight-gradient kernel (generic site: rows > 0 and covered,
    else vendor GEMM + colsum).  (M, K) = (192, 96) is covered by nothing, K = 256 not by the one-pass kernel."""
    import importlib
    from segger_amd import ops
    lin = importlib.import_module("segger_amd.ops.linear")
    P, bf, f32 = lin.BackwardPlan, torch.bfloat16, torch.float32
    covered = ((384, 128), (128, 128), (64, 128))
    # what the hand-written expectations below rest on
    for m, k in covered:
        assert ops.linear_wgrad_dx_supported(m, k, bf) and not ops.linear_wgrad_dx_supported(m, k, f32)
        assert ops.linear_f32_gate_supported(m, k) and ops.linear_supported(m, k, f32) and ops.linear_wgrad_supported(m, k, f32)
    assert [ops.linear_wgrad_dx_gate_supported(m, k, bf) for m, k in covered] == [True, True, False]
    assert [ops.linear_f32_split_supported(m, k) for m, k in covered] == [True, True, False]
    for dt in (bf, f32):
        assert not ops.linear_wgrad_dx_supported(384, 256, dt) and ops.linear_supported(384, 256, dt)
        assert ops.linear_wgrad_supported(384, 256, dt) and not ops.linear_supported(192, 96, dt)
        assert not ops.linear_wgrad_supported(192, 96, dt) and not ops.linear_wgrad_dx_supported(192, 96, dt)
    assert not ops.linear_f32_split_supported(384, 256) and not ops.linear_f32_gate_supported(384, 256)

    def plan(site, mk, dt, need_x=True, want_w=True, want_b=None, n=1000, pre=False, pre_grad=None, aligned=True, **kw):
        want_b = (site == "generic") if want_b is None else want_b          # (the first layer's nodes have no bias of their own)
        return lin.backward_plan(mk[0], mk[1], n, dt, need_x, want_w, want_b, pre, pre if pre_grad is None else pre_grad,
                                 aligned, site=site, **kw)

    def table():
        """{case: (the plan at the current switches, the plan expected at the default switches)}"""
        t = {}
        for mk in covered:
            split = "f32_split" if mk != (64, 128) else "mfma"
            gate = mk != (64, 128)
            # generic site, 16-bit: one pass whenever the input and a parameter want gradients
            t["g16 all", mk] = plan("generic", mk, bf), P("one_pass", "one_pass", False, True, True)
            t["g16 x+w", mk] = plan("generic", mk, bf, want_b=False), P("one_pass", "one_pass", False, True, False)
            t["g16 x+b", mk] = plan("generic", mk, bf, want_w=False), P("one_pass", "one_pass", False, False, True)
            t["g16 x", mk] = plan("generic", mk, bf, want_w=False, want_b=False), P("mfma", None)
            t["g16 w", mk] = plan("generic", mk, bf, need_x=False, want_b=False), P(None, "mfma", False, True, False)
            t["g16 b", mk] = plan("generic", mk, bf, need_x=False, want_w=False), P(None, "mfma", False, False, True)
            t["g16 none", mk] = plan("generic", mk, bf, need_x=False, want_w=False, want_b=False), P()
            t["g16 n=0", mk] = plan("generic", mk, bf, n=0), P("mfma", "vendor", False, True, True)
            t["g16 paired", mk] = plan("generic", mk, bf, need_x=False, have_dw=True), P(None, None, False, True, True)
            # generic site, fp32: no one-pass kernel; the split where it covers the shape and dY's rows are aligned
            t["g32 all", mk] = plan("generic", mk, f32), P(split, "mfma", False, True, True)
            t["g32 unaligned", mk] = plan("generic", mk, f32, aligned=False), P("mfma", "mfma", False, True, True)
            t["g32 x", mk] = plan("generic", mk, f32, want_w=False, want_b=False), P(split, None)
            t["g32 n=0", mk] = plan("generic", mk, f32, n=0), P(split, "vendor", False, True, True)
            for site in ("first", "row_bias"):
                # 16-bit: one pass, gelu'(pre) inside it where the gated kernel covers the shape
                t[site, "16 pre", mk] = plan(site, mk, bf, pre=True), P("one_pass", "one_pass", gate, True, False)
                t[site, "16", mk] = plan(site, mk, bf), P("one_pass", "one_pass", False, True, False)
                t[site, "16 x", mk] = plan(site, mk, bf, want_w=False, pre=True), P("mfma", None)
                t[site, "16 w", mk] = plan(site, mk, bf, need_x=False, pre=True), P(None, "mfma", False, True, False)
                t[site, "16 n=0", mk] = plan(site, mk, bf, n=0, pre=True), P("mfma", "mfma", False, True, False)
            # fp32: the first-layer node has the gate epilogue and the split, the row-bias node neither
            t["first 32 pre", mk] = plan("first", mk, f32, pre=True), P("f32_gate", "mfma", True, True, False)
            t["first 32 pre const", mk] = plan("first", mk, f32, pre=True, pre_grad=False), P(split, "mfma", False, True, False)
            t["first 32", mk] = plan("first", mk, f32), P(split, "mfma", False, True, False)
            t["first 32 unaligned", mk] = plan("first", mk, f32, pre=True, aligned=False), P("mfma", "mfma", False, True, False)
            t["first 32 n=0", mk] = plan("first", mk, f32, pre=True, n=0), P("f32_gate", "mfma", True, True, False)
            t["row_bias 32 pre", mk] = plan("row_bias", mk, f32, pre=True), P("mfma", "mfma", False, True, False)
            t["row_bias 32", mk] = plan("row_bias", mk, f32), P("mfma", "mfma", False, True, False)
        for dt in (bf, f32):
            for n in (0, 1000):
                # K = 256: the MFMA kernels, one per output; (192, 96): the generic site's vendor routes
                t["g K256", dt, n] = plan("generic", (384, 256), dt, n=n), P("mfma", "mfma" if n else "vendor", False, True, True)
                t["g 192x96", dt, n] = plan("generic", (192, 96), dt, n=n), P("vendor", "vendor", False, True, True)
                for site in ("first", "row_bias"):        # (no vendor route: entered through embed_linear_supported only)
                    for mk in ((384, 256), (192, 96)):
                        t[site, mk, dt, n] = plan(site, mk, dt, n=n, pre=True), P("mfma", "mfma", False, True, False)
            t["g 192x96 b", dt] = plan("generic", (192, 96), dt, need_x=False, want_w=False), P(None, "vendor", False, False, True)
            t["g 192x96 x", dt] = plan("generic", (192, 96), dt, want_w=False, want_b=False), P("vendor", None)
        return t

    def plans():
        return {case: got for case, (got, _) in table().items()}

    for case, (got, want) in table().items():
        assert got == want, case
    base = plans()

    def changed(name, edit):
        """With switch ``name`` off every plan equals ``edit(case, default plan)`` (None: unchanged) -- and at least one differs."""
        with monkeypatch.context() as mp:
            mp.setattr(ops, name, False)
            now = plans()
        n_changed = 0
        for case, was in base.items():
            want = edit(case, was) or was
            assert now[case] == want, (name, case)
            n_changed += want != was
        assert n_changed, name

    # FUSED_WGRAD_DX: every one-pass plan becomes the MFMA forward kernel on W^T + the MFMA weight-gradient kernel, ungated
    changed("FUSED_WGRAD_DX", lambda c, p: p._replace(dx="mfma", dw="mfma", gate=False) if p.dx == "one_pass" else None)
    # FUSED_GELU_GATE: only the gate of a one-pass plan
    changed("FUSED_GELU_GATE", lambda c, p: p._replace(gate=False) if p.dx == "one_pass" else None)
    # F32_SPLIT: the split data gradients go to the exact kernel; the gate epilogue keeps only the exact kernel's shapes (its
    # x operand [n, 384] is not one of them)
    changed("F32_SPLIT", lambda c, p: p._replace(dx="mfma", gate=False)
            if p.dx == "f32_split" or (p.dx == "f32_gate" and c[-1] == (384, 128)) else None)
    # F32_GATE_EPILOGUE: the gated data gradient falls to the split (or, uncovered, to the exact kernel), ungated
    changed("F32_GATE_EPILOGUE", lambda c, p: p._replace(dx="mfma" if c[-1] == (64, 128) else "f32_split", gate=False)
            if p.dx == "f32_gate" else None)

    # ---- the pair: (K, (Ma, Mb)) with rows (257, 7)
    def pair(k, ms=(384, 128), dt=bf, ns=(257, 7), need_xs=(True, True), wants=(True, True), have_grads=True):
        return lin.backward_pair_plan(k, ms, ns, dt, need_xs, wants, have_grads)

    def pair_table():
        return [pair(128), pair(256), pair(128, need_xs=(True, False)), pair(256, need_xs=(False, False)),
                pair(128, dt=f32), pair(256, dt=f32), pair(128, wants=(True, False)), pair(128, wants=(False, True)),
                pair(128, ns=(257, 0)), pair(128, have_grads=False), pair(96, ms=(192, 192)), pair(128, dt=torch.float16)]

    default = ["one_pass", "wgrad+dx", "wgrad", "wgrad", None, None, None, None, None, None, None, "one_pass"]
    assert pair_table() == default
    with monkeypatch.context() as mp:
        mp.setattr(ops, "WGRAD_PAIR", False)
        assert pair_table() == [None] * len(default)
        assert plans() == base                                # (the per-side plans do not read it)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "FUSED_WGRAD_DX", False)
        assert pair_table() == ["wgrad+dx" if p == "one_pass" else p for p in default]
    for name in ("FUSED_GELU_GATE", "F32_SPLIT", "F32_GATE_EPILOGUE"):
        with monkeypatch.context() as mp:
            mp.setattr(ops, name, False)
            assert pair_table() == default, name
    assert pair_table() == default and plans() == base


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("segger_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_contract_line_is_compact_and_complete():
    """Round 5's driver record was lost because bench.py printed ONE 20 890-byte stdout line.  The contract line is now a
    compact summary (diagnostics go to bench_details.json + stderr): round 5's own full record through the formatter gives
    valid JSON of at most 8 KB with every contract key, `roofline` and `cpu_baseline`."""
    import json
    bench = _load_bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line.json")))
    assert len(json.dumps(full)) > 16384                     # the record that broke the driver's parser
    line = bench.contract_line(full)
    assert "\n" not in line and len(line) <= bench.CONTRACT_LINE_MAX == 8192
    c = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in c, k
    assert c["config"]["workload"].startswith("C2") and "model" not in c["config"]
    assert abs(c["value"] - full["value"]) <= 1e-6 * full["value"] and abs(c["ms_per_step"] - full["ms_per_step"]) < 1e-6
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "algorithmic_bytes_per_launch", "ms_per_launch"):
        assert k in c["roofline"], k
    assert abs(c["roofline"]["frac"] - c["roofline"]["achieved"] / c["roofline"]["peak"]) < 1e-4
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c["cpu_baseline"], k
    assert c["cpu_baseline"]["kind"] == "port" and c["cpu_baseline"]["host"]["threads_used"] == c["cpu_baseline"]["cores"]
    # scalar summaries only: no nested record deeper than two levels below a top-level key, no lists of dicts
    def depth(o):
        return 0 if not isinstance(o, dict) else 1 + max([depth(v) for v in o.values()] or [0])
    assert depth(c) <= 4
    assert c["auroc"]["met"] is True and set(c["auroc"]["max_abs_delta"]) == {"f32", "bf16", "f16"}
    assert all(isinstance(v, float) for v in c["roofline_other"].values())
    assert c["strong"]["graphed"]["ms_per_step"] == pytest.approx(full["strong"]["graphed"]["ms_per_step"], rel=1e-5)


def test_bench_contract_line_survives_oversized_and_failed_records():
    """A secondary record that failed (error strings) or grew (a future diagnostic) never costs the contract keys: the
    formatter truncates / drops summaries, largest first, and still asserts the bound."""
    import json
    bench = _load_bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line.json")))
    full["f32"] = {"error": "RuntimeError: " + "x" * 5000}
    full["auroc"] = {"error": "boom " * 1000}
    full["roofline_other"] = {f"kernel_class_{i:04d}_with_a_long_name": {"frac": 0.5} for i in range(400)}
    full["roofline"]["dominant"] = {"kernel": "gatv2_bwd_dst_kernel<bf16,H=2,C=64>", "achieved": 5400.0, "frac": 0.675,
                                    "traffic": 1890440434, "algorithmic_bytes_per_launch": 4700000000, "ms_per_launch": 0.87,
                                    "note": "n" * 3000}
    line = bench.contract_line(full)
    assert len(line) <= 8192
    c = json.loads(line)
    assert c["roofline"]["dominant"]["frac"] == 0.675 and "note" not in c["roofline"]["dominant"]
    assert c["cpu_baseline"]["value"] and c["value"] == pytest.approx(full["value"])
    assert isinstance(c["roofline_other"], str) and "dropped" in c["roofline_other"]
    assert len(c["f32"]["error"]) <= 120


def test_bench_dump_outputs_writes_loss_and_weights(tmp_path):
    """`bench.py --dump-outputs DIR`: the loss and every parameter as float32 .npy under file names that keep the
    parameter name (characters outside [A-Za-z0-9_.-] -> '_')."""
    bench = _load_bench()
    torch.manual_seed(0)
    m = torch.nn.ModuleDict({"<tx___neighbors___tx>": torch.nn.Linear(3, 2)})
    loss = m["<tx___neighbors___tx>"](torch.randn(4, 3)).square().sum()
    loss.backward()
    bench.dump_outputs(str(tmp_path / "out"), m, loss)
    got = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(got) == {"loss.npy", "param._tx___neighbors___tx_.weight.npy", "param._tx___neighbors___tx_.bias.npy"}
    assert all(a.dtype == np.float32 for a in got.values())
    lin = m["<tx___neighbors___tx>"]
    assert got["loss.npy"].shape == () and got["loss.npy"] == np.float32(loss.item())
    assert np.array_equal(got["param._tx___neighbors___tx_.weight.npy"], lin.weight.detach().numpy())
    assert np.array_equal(got["param._tx___neighbors___tx_.bias.npy"], lin.bias.detach().numpy())


def test_cli_default_widths_never_leave_the_hand_written_gemms():
    """Every projection of the encoder at segger's CLI defaults (in 128, hidden 64 x 2 heads, out 64; ist_encoder.py:219-287)
    -- forward, data gradient (K and M swapped) and weight gradient, in fp32 / bf16 / f16 -- is covered by the MFMA kernels,
    so ``ops.vendor_gemm_calls`` stays empty there; an uncovered width is counted and announced once (RuntimeWarning), not
    served silently."""
    import warnings
    from segger_amd import ops
    fwd = [(128, 128),              # lin_first.bd (PCA 128 -> in 128)
           (256, 64), (64, 64),     # positional MLP
           (256, 384), (256, 128),  # conv 0: stacked lin_l | lin_r | lin_l over gelu(cat(E[g], pe)); lin_r(bd)
           (128, 384), (128, 128),  # conv 1..3
           (128, 64)]               # lin_last
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for k, m in fwd:
            assert ops.linear_supported(k, m, dt), ("forward", k, m, dt)
            assert ops.linear_wgrad_supported(m, k, dt), ("weight gradient", m, k, dt)
            if k != 256:            # (the first layer's input needs no data gradient beyond the positional half: K = 128)
                assert ops.linear_supported(m, k, dt), ("data gradient", m, k, dt)
    ops.vendor_gemm_calls.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ops._vendor_gemm("projection y = x W^T", 96, 192, torch.bfloat16)
        ops._vendor_gemm("projection y = x W^T", 96, 192, torch.bfloat16)
    assert len(w) == 1 and "K=96 -> M=192" in str(w[0].message) and issubclass(w[0].category, RuntimeWarning)
    assert ops.vendor_gemm_calls == {("projection y = x W^T", 96, 192, "bfloat16"): 2}
    assert not ops.linear_supported(96, 192, torch.bfloat16)
    ops.vendor_gemm_calls.clear()


OPS_SWITCHES = ("_FWD_PAIR", "_BWD_PAIR", "_CONTRIB_MIN_EDGES", "ONE_LAUNCH_LOSS_HEAD", "LOSS_HEAD_ONE_LAUNCH_MAX_ROWS",
                "USE_ANCHOR_ROWS", "POS_POLY_F32", "FUSED_WGRAD_DX", "FUSED_GELU_GATE", "F32_SPLIT", "F32_GATE_EPILOGUE",
                "F32_SPLIT_WGRAD", "LINEAR_PAIR", "WGRAD_PAIR", "FUSED_POSMLP_BWD", "EMBED_LINEAR_ONE_NODE",
                "EMBED_LINEAR_MAX_GENES", "FUSED_POSMLP", "MERGED_POS_EMBED", "FRONT_JOIN", "POS_PAIR_NODE",
                "SPLIT_FIRST_LAYER", "SPLIT_FIRST_LAYER_MIN_ROWS", "SPLIT_FIRST_LAYER_MIN_ROWS_F32")


def test_ops_route_switches_live_in_the_package_only():
    """The route switches are attributes of the package segger_amd.ops and no submodule binds one of them: the submodules
    read ``ops.NAME`` when called, so ``ops.NAME = value`` (a test's monkeypatch, a tool's A/B flag) reaches every route
    instead of silently leaving a copy in force.  Every ``ops.NAME`` that bench.py and __graft_entry__.py use resolves, to
    an operator and not to a submodule of the same name, and the shared mutable state is one object."""
    import importlib
    import pkgutil
    from segger_amd import ops
    subs = [importlib.import_module(f"segger_amd.ops.{m.name}") for m in pkgutil.iter_modules(ops.__path__)]
    assert len(subs) >= 2
    readers = subs + [importlib.import_module("segger_amd.ist_encoder")]
    for name in OPS_SWITCHES:
        assert hasattr(ops, name), name
        for mod in readers:
            assert name not in vars(mod), f"{mod.__name__} binds its own {name}"
    for fn in ("bench.py", "__graft_entry__.py"):
        src = open(os.path.join(ROOT, fn)).read()
        for name in sorted(set(re.findall(r"(?<![\w.])ops\.([A-Za-z_]\w*)", src))):      # (not torch.ops.*)
            assert hasattr(ops, name), f"{fn} uses ops.{name}"
            assert getattr(ops, name) not in subs, f"{fn}: ops.{name} is a submodule, not the operator"
    assert ops.vendor_gemm_calls is vars(ops._common)["vendor_gemm_calls"]
    assert ops._PACKS is vars(ops.packs)["_PACKS"] and ops._TICKETS is vars(ops.heads)["_TICKETS"]


def test_loss_head_spec_reads_plain_tuples_as_named_fields():
    """``LossHeadSpec`` takes plain tuples (``sg`` of 6 or 7 items, or None) or the named forms, and is read by name from
    then on; ``anchors_unique`` defaults to False and stays as given (a callable is not asked at construction);
    ``defer_finish`` is a constructor keyword, default False, and an ordinary attribute."""
    from segger_amd import ops
    from segger_amd.ops.heads import BdMetric, SgTriplets, TxTriplets
    anchors, pos, neg = torch.arange(5), torch.tensor([1, 2, -1, 0, 3]), torch.tensor([4, 3, 2, 1, 0])
    bpos, bneg = torch.tensor([1, 0, 2]), torch.tensor([2, 2, 0])
    dp, dn, w = torch.rand(3), torch.rand(3), torch.full((3,), 1.0 / 3)
    src, spos, sneg, groups = torch.tensor([0, 2, 4]), torch.tensor([0, 1, 1]), torch.tensor([1, 0, 2]), object()
    tx, bd = (anchors, pos, neg, 0.3, 1e-6), (bpos, bneg, dp, dn, w, 1e-8)
    asked = []
    uniq = lambda: asked.append(1) or True

    def check_common(spec):
        assert isinstance(spec.tx, TxTriplets) and isinstance(spec.bd, BdMetric)
        assert spec.tx.anchors is anchors and spec.tx.pos is pos and spec.tx.neg is neg
        assert (spec.tx.margin, spec.tx.eps) == (0.3, 1e-6)
        assert spec.bd.pos is bpos and spec.bd.neg is bneg and spec.bd.d_pos is dp and spec.bd.d_neg is dn
        assert spec.bd.weight is w and spec.bd.eps == 1e-8
        assert spec.tx_anchors_are_rows is False and spec.sg_of_tx is None and spec.tx_state is None
        assert spec.grad_out_hint is None

    s6 = ops.LossHeadSpec(tx, bd, (src, spos, sneg, 0.4, 1e-6, groups))
    check_common(s6)
    assert isinstance(s6.sg, SgTriplets) and s6.sg.src is src and s6.sg.pos is spos and s6.sg.neg is sneg
    assert (s6.sg.margin, s6.sg.eps) == (0.4, 1e-6) and s6.sg.pos_groups is groups and s6.sg.anchors_unique is False
    assert s6.sg_kind == "triplet" and s6.defer_finish is False
    s6n = ops.LossHeadSpec(tx, bd, (src, spos, sneg, 0.4, 1e-6, None))
    assert s6n.sg.pos_groups is None and s6n.sg.anchors_unique is False
    s7 = ops.LossHeadSpec(tx, bd, (src, spos, sneg, 0.4, 1e-6, groups, uniq), defer_finish=True)
    check_common(s7)
    assert s7.sg.pos_groups is groups and s7.sg.anchors_unique is uniq and not asked
    assert s7.defer_finish is True
    s7.defer_finish = False
    assert s7.defer_finish is False
    s7t = ops.LossHeadSpec(tx, bd, (src, spos, sneg, 0.4, 1e-6, groups, True), tx_anchors_are_rows=True)
    assert s7t.sg.anchors_unique is True and s7t.tx_anchors_are_rows is True
    s0 = ops.LossHeadSpec(tx, bd, None)
    check_common(s0)
    assert s0.sg is None and s0.defer_finish is False
    sb = ops.LossHeadSpec(tx, bd, (src, spos, sneg, 0.0, 0.0, groups, True), sg_kind="bce", defer_finish=True)
    check_common(sb)
    assert sb.sg_kind == "bce" and sb.sg.pos_groups is groups and sb.defer_finish is True
    named = ops.LossHeadSpec(TxTriplets(*tx), BdMetric(*bd), SgTriplets(src, spos, sneg, 0.4, 1e-6, pos_groups=groups))
    check_common(named)
    assert named.sg == s6.sg
