"""MI355X-native ``ISTEncoder``: same module tree, parameter names and forward
contract as reference ``src/segger/models/ist_encoder.py`` (so reference
state dicts load), with the PyG ``HeteroConv``/``GATv2Conv`` message passing
replaced by the fused HIP kernels of ``libsegger_amd.so``.

Reference map
-------------
``sinusoidal_embedding``      ist_encoder.py:22-31
``Positional2dEmbedder``      ist_encoder.py:33-79
``SkipGAT``                   ist_encoder.py:82-211   (HeteroConv of GATv2Conv, dropout 0.2)
``ISTEncoder``                ist_encoder.py:214-333

Differences that are deliberate: the never-used
``('bd','contains','tx')`` conv is not built (it has no edges in segger's data
and its lazy parameters are never materialised); the per-graph min/max loop of
the positional embedder (one host sync per graph, ``:69-73``) is a single
segmented reduction.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import Tensor
from torch.nn import Embedding, Linear, Module, ModuleDict, ModuleList, Parameter, Sequential, SiLU
from torch.nn import functional as F

from . import ops
from .graph import EdgeCSR, EdgeGraph, edge_graph
from .hetero import TX_BD, TX_TX, EdgeType

GAT_DROPOUT = 0.2          # ist_encoder.py:116,123
NEGATIVE_SLOPE = 0.2       # GATv2Conv default


def _layer_seed(seed, which: int):
    """(2*layer + edge-type slot) with the optional device counter carried along; a third entry is a constant added to the
    seed (a captured step reads the counter BEFORE its end-of-step advance: offset = the advance)."""
    if isinstance(seed, tuple):
        return (2 * int(seed[0]) + which + (int(seed[2]) if len(seed) > 2 else 0), seed[1])
    return 2 * int(seed) + which


def pyg_key(edge_type: EdgeType) -> str:
    """torch_geometric's ModuleDict key for a tuple (state-dict compatibility)."""
    return "<" + "___".join(edge_type) + ">"


def sinusoidal_embedding(x: Tensor, dim: int, max_period: float = 1000) -> Tensor:
    """cos|sin features of a flat tensor (ist_encoder.py:22-31); fp32 like the reference."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32, device=x.device) / half)
    args = x[:, None].float() * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


class PosEmbedding(NamedTuple):
    """The embedder's result.  ``pre``: the value before the GELU where ``out`` = gelu(pre) is a constant for autograd and the
    gradient arrives for ``pre`` (as ``ops.posmlp(return_pre=True)``: the consumer, ``ops.embed_linear``, applies gelu')."""
    out: Tensor
    pre: Optional[Tensor]
    gelu_applied: bool


class EmbedRoute(NamedTuple):
    """The route of one embedder call, decided by :meth:`Positional2dEmbedder.route` before anything is launched."""
    features: str    # the sinusoid features: "none" (never materialised) | "posfreq" (segger_posfreq) | "torch"
    mlp: str         # "fused16" (ops.posmlp) | "poly_f32" (ops.pos_poly_mlp_f32) | "mlp_f32" (ops.mlp_silu_f32) | "composed"


class Positional2dEmbedder(Module):
    """Per-graph min-max normalised (x, y) -> 2 x sinusoid(256) -> shared MLP -> concat."""

    def __init__(self, hidden_size: int, frequency_embedding_size: int = 256):
        super().__init__()
        self.dim = hidden_size // 2
        self.mlp = Sequential(
            Linear(frequency_embedding_size, self.dim, bias=True),
            SiLU(),
            Linear(self.dim, self.dim, bias=True),
        )
        self.frequency_embedding_size = frequency_embedding_size

    @staticmethod
    def normalize(pos: Tensor, batch: Optional[Tensor], num_graphs: Optional[int] = None) -> Tensor:
        pos = pos.float()
        if batch is None:                                   # ist_encoder.py:62-64 (no epsilon)
            pos = pos - pos.min(dim=0).values
            return pos / pos.max(dim=0).values
        if num_graphs is None:
            num_graphs = int(batch.max()) + 1 if batch.numel() else 0
        mins, maxs = ops.segment_minmax(pos, batch, num_graphs)     # one HIP pass, no per-graph sync
        lo, hi = mins[batch.long()], maxs[batch.long()]
        return (pos - lo) / (hi - lo + 1e-8)                # ist_encoder.py:74

    def forward(self, pos: Tensor, batch: Optional[Tensor] = None, *, num_graphs: Optional[int] = None,
                dtype: torch.dtype = torch.float32) -> Tensor:
        return self._embed(pos, batch, num_graphs, dtype).out

    def route(self, *, on_gpu: bool, batched: bool, dtype: torch.dtype, rows: int, pos_grad: bool = False) -> EmbedRoute:
        """The route of one :meth:`_embed` call from shapes, dtypes and the switches of ``ops``: nothing is launched.
        ``batched``: there is a batch vector; ``rows``: the number of positions; ``pos_grad``: they require a gradient."""
        fd, dim, l0, l2 = self.frequency_embedding_size, self.dim, self.mlp[0], self.mlp[2]
        biased = l0.bias is not None and l2.bias is not None
        if not ((batched or on_gpu) and fd % 16 == 0):
            # (the fp32 nodes below are GPU kernels for widths that are multiples of 16: none of them applies here)
            return EmbedRoute("torch", "composed")
        if ops.FUSED_POSMLP and on_gpu and biased and ops.posmlp_supported(fd, dim, dtype):
            return EmbedRoute("none", "fused16")
        # fp32 storage: the MLP behind ONE autograd node, over at least one row
        f32_node = dtype == torch.float32 and ops.F32_GATE_EPILOGUE and biased and on_gpu and rows > 0
        if (f32_node and not pos_grad and l0.weight.dtype == l2.weight.dtype == torch.float32
                and ops.pos_poly_f32_covers(fd, dim)):
            return EmbedRoute("none", "poly_f32")
        # (segger_posfreq's features are constants for autograd, whatever the positions require)
        return EmbedRoute("posfreq", "mlp_f32" if f32_node and ops.mlp_silu_f32_covers(fd, dim, dim) else "composed")

    def _embed(self, pos: Tensor, batch: Optional[Tensor], num_graphs: Optional[int], dtype: torch.dtype, *,
               gelu: bool = False, want_pre: bool = False, minmax=None) -> PosEmbedding:
        """``gelu`` (not in the reference): also apply the GELU that ISTEncoder puts on its concatenated input;
        ``want_pre`` (with ``gelu``): hand the GELU's derivative to the consumer (``PosEmbedding.pre``) on the routes that
        can; the others keep the GELU in autograd and return ``pre = None``."""
        n, fd, l0, l2 = pos.shape[0], self.frequency_embedding_size, self.mlp[0], self.mlp[2]
        w = (l0.weight, l0.bias, l2.weight, l2.bias)
        want_pre = want_pre and gelu
        route = self.route(on_gpu=pos.is_cuda, batched=batch is not None, dtype=dtype, rows=n, pos_grad=pos.requires_grad)
        if route.features == "torch":
            pos = self.normalize(pos, batch, num_graphs)
            freq = sinusoidal_embedding(pos.flatten(), fd, max_period=10000).reshape(n, 2, fd).to(dtype)
        else:
            # per-graph min/max (one pass); the kernels normalise with them and only look up the graphs of existing nodes: no
            # (0, 0) fix-up for empty ones.  No batch vector = one graph, normalised WITHOUT the epsilon (ist_encoder.py:62-64)
            if batch is None or num_graphs is None:
                num_graphs = 1 if batch is None else int(batch.max()) + 1 if batch.numel() else 0
            mins, maxs = ops.segment_minmax(pos, batch, num_graphs, keep_empty=True, out=minmax)
            eps_n = 1e-8 if batch is not None else 0.0
            if route.features == "posfreq":                  # normalise + sinusoid written straight in `dtype`
                freq = ops.posfreq(pos, batch, mins, maxs, fd, dtype, eps_n, 10000.0, num_graphs)
        # h: the embedder's output; act: gelu(h) where the route's own kernel made it (with `want_pre` a constant for autograd)
        act = None
        if route.mlp == "fused16":
            # sinusoid + Linear + SiLU + Linear in one kernel: the [2n, 256] feature matrix is generated in registers
            # (and stored once for the weight gradient when training) instead of written and re-read
            r = ops.posmlp(pos, batch, mins, maxs, *w, dtype, eps_n, 10000.0, gelu, want_pre, num_graphs)
            act, h = r if want_pre else (r, None) if gelu else (None, r)
        elif route.mlp == "composed":
            h = ops.linear(F.silu(ops.linear(freq, l0.weight, l0.bias)), l2.weight, l2.bias).flatten(-2)
        else:                    # fp32 storage: the MLP (+ the GELU that follows) behind one autograd node, as [2n, dim] rows
            if route.mlp == "poly_f32":
                # the first Linear as a polynomial of the normalised coordinate (no feature matrix, no K = 256 GEMM:
                # csrc/posenc_poly.hip), SiLU and the 64-wide second Linear
                r = ops.pos_poly_mlp_f32(pos, batch, mins, maxs, *w, eps=eps_n, max_period=10000.0, gelu_out=want_pre,
                                         num_graphs=num_graphs)
            else:                # SiLU in the GEMMs' epilogues, its derivative in the data-gradient GEMM's epilogue
                r = ops.mlp_silu_f32(freq.reshape(-1, fd), *w, gelu_out=want_pre)
            h, act = (t.reshape(n, -1) for t in r) if want_pre else (r.reshape(n, -1), None)
        if gelu and act is None:
            # fp32 storage: gelu'(h) in the epilogue of the consumer's data-gradient GEMM instead of a gelu_backward pass
            want_pre = want_pre and dtype == torch.float32 and h.is_cuda and ops.F32_GATE_EPILOGUE
            act = F.gelu(h).detach() if want_pre else F.gelu(h)
        return PosEmbedding(act if gelu else h, h if want_pre else None, gelu)


def _pair_node_applies(emb: "Positional2dEmbedder", on_gpu: bool, batched: bool, dtype: torch.dtype) -> bool:
    """``ops.posmlp_pair`` covers: the fused 16-bit embedder (``emb.route``), batch vectors + a graph count, training."""
    l0, l2 = emb.mlp[0], emb.mlp[2]
    return bool(ops.POS_PAIR_NODE and batched and emb.route(on_gpu=on_gpu, batched=batched, dtype=dtype, rows=1).mlp == "fused16"
                and ops.posmlp_pair_supported(l0.weight, l0.bias, l2.weight, l2.bias, dtype))


def _pair_node(emb: "Positional2dEmbedder", pos_a, batch_a, pos_b, batch_b, num_graphs, dtype):
    """``((gelu(pe_a), pe_a), pe_b)`` from ONE autograd node (``ops.posmlp_pair``), or None where that route does not
    apply -- then the caller embeds each node type by its own call."""
    batched = batch_a is not None and batch_b is not None and num_graphs is not None
    if not _pair_node_applies(emb, pos_a.is_cuda, batched, dtype):
        return None
    l0, l2 = emb.mlp[0], emb.mlp[2]
    mm_a = ops.segment_minmax(pos_a, batch_a, num_graphs, keep_empty=True)
    mm_b = ops.segment_minmax(pos_b, batch_b, num_graphs, keep_empty=True)
    return ops.posmlp_pair(pos_a, batch_a, mm_a[0], mm_a[1], pos_b, batch_b, mm_b[0], mm_b[1], l0.weight, l0.bias, l2.weight,
                           l2.bias, dtype, eps=1e-8, max_period=10000.0, num_graphs=num_graphs)


class _SplitRows(torch.autograd.Function):
    """[n_a + n_b, D] -> ([n_a, D], [n_b, D]) as views; backward = one ``cat`` (autograd's own slicing would zero-fill
    and add a full-size matrix per slice)."""

    @staticmethod
    def forward(ctx, x, n_a):
        ctx.n = (int(n_a), int(x.shape[0]) - int(n_a))
        return x[:n_a], x[n_a:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        ref = ga if ga is not None else gb
        if ga is None:
            ga = ref.new_zeros((ctx.n[0],) + tuple(ref.shape[1:]))
        if gb is None:
            gb = ref.new_zeros((ctx.n[1],) + tuple(ref.shape[1:]))
        return torch.cat((ga, gb), 0), None


class FrontPlan(NamedTuple):
    """The route of a step's input stage, decided by :meth:`ISTEncoder.front_plan` before anything is launched."""
    positional: bool = False   # positions are embedded at all
    table: bool = False        # transcripts through the gene-table kernels (embed_gelu / front_join / embed_linear), not torch
    split: bool = False        # first layer as per-gene table + positional GEMM: x_tx stays an ops.EmbedInput
    join: bool = False         # ops.front_join assembles the inputs: both node types when `merged`, else the boundaries
    merged: bool = False       # one embedder call for both node types
    pair_node: bool = False    # one embedder call per type, both behind one autograd node (ops.posmlp_pair)


class PosPair(NamedTuple):
    """Both node types' positional embeddings: ``joint`` (un-split [n_tx + n_bd, D], for ``ops.front_join``) or ``tx`` / ``bd``.
    ``tx_pre`` as ``PosEmbedding.pre``; ``bd_gelu_applied``: else whoever concatenates ``bd`` owes the GELU of ist_encoder.py:320."""
    tx: Optional[Tensor] = None
    tx_pre: Optional[Tensor] = None
    bd: Optional[Tensor] = None
    joint: Optional[Tensor] = None
    bd_gelu_applied: bool = False


class StagedInputs(NamedTuple):
    """What a captured step (train_step_graph.py) prepared in its static buffers instead of the forward."""
    by_gene: Optional[EdgeCSR] = None        # rows grouped by gene id (:func:`rows_by_gene`)
    pos_all: Optional[Tensor] = None         # positions of both node types, concatenated
    batch_all: Optional[Tensor] = None       # ... and their graph ids (the boundaries' offset by num_graphs)
    minmax: Optional[tuple] = None           # where the per-graph minima / maxima go
    draws: Optional[tuple] = None            # (dropout bit planes | None, constant added to every seed): ops.step_draws


def rows_by_gene(ids: Tensor, n_genes: int, cache: Optional[dict], staged: Optional[EdgeCSR] = None) -> EdgeCSR:
    """``ops.rows_by_id`` of a batch's gene ids (one sort): the view a captured step staged; else the one kept by the store
    that batches of a resident partition share across epochs (tiles.TilePartition: ``cache["persistent"]``) or, without
    such a store, by the batch's own cache -- built when missing or when it belongs to other rows."""
    if staged is not None:
        return staged
    keep, key = cache, ("by_gene", ids.data_ptr(), int(ids.shape[0]))
    if cache is not None and cache.get("persistent") is not None:
        keep, key = cache["persistent"], "tx_by_gene"
    hit = keep.get(key) if keep is not None else None
    if hit is None or hit.n_rows != n_genes or hit.n_edges != ids.shape[0]:
        hit = ops.rows_by_id(ids, n_genes)
        if keep is not None:
            keep[key] = hit
    return hit


class GATv2Conv(Module):
    """Parameter holder with torch_geometric.nn.GATv2Conv's names and shapes
    (``lin_l``, ``lin_r``: [H*C, in] + bias; ``att``: [1, H, C]; ``bias``: [H*C]).
    The arithmetic lives in :func:`segger_amd.ops.gatv2_aggregate`."""

    def __init__(self, in_channels: Tuple[int, int], out_channels: int, heads: int,
                 negative_slope: float = NEGATIVE_SLOPE, dropout: float = GAT_DROPOUT):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.negative_slope, self.dropout = negative_slope, dropout
        self.lin_l = Linear(in_channels[0], heads * out_channels, bias=True)
        self.lin_r = Linear(in_channels[1], heads * out_channels, bias=True)
        self.att = Parameter(torch.empty(1, heads, out_channels))
        self.bias = Parameter(torch.empty(heads * out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        # PyG: glorot for lin weights and att, zeros for biases
        for lin in (self.lin_l, self.lin_r):
            torch.nn.init.xavier_uniform_(lin.weight)
            torch.nn.init.zeros_(lin.bias)
        a = math.sqrt(6.0 / (self.att.size(-2) + self.att.size(-1)))
        torch.nn.init.uniform_(self.att, -a, a)
        torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tuple[Tensor, Tensor], graph: EdgeGraph, *, apply_gelu: bool = False, seed: int = 0,
                return_attention_weights: bool = False):
        x_src, x_dst = x
        xl = ops.linear(x_src, self.lin_l.weight, self.lin_l.bias)
        xr = ops.linear(x_dst, self.lin_r.weight, self.lin_r.bias)
        p = self.dropout if self.training else 0.0
        return ops.gatv2_aggregate(xl, xr, self.att, self.bias, graph, self.heads, self.out_channels,
                                   apply_gelu=apply_gelu, negative_slope=self.negative_slope,
                                   dropout_p=p, seed=seed, return_alpha=return_attention_weights)


class _HeteroConv(Module):
    """Holds ``convs`` under PyG's mangled keys so ``state_dict`` matches HeteroConv."""

    def __init__(self, convs: Dict[EdgeType, Module]):
        super().__init__()
        self.convs = ModuleDict({pyg_key(k): v for k, v in convs.items()})

    def __getitem__(self, et: EdgeType) -> Module:
        return self.convs[pyg_key(et)]


class SkipGAT(Module):
    """One hetero GATv2 layer over tx-neighbors-tx and tx-belongs-bd
    (ist_encoder.py:82-211) + the GELU that follows it in ISTEncoder (``:325``),
    fused.  ``attention_weights`` holds tx-neighbors-tx coefficients of the last
    forward when ``store_attention`` is set (the reference's forward hook)."""

    def __init__(self, in_channels: Tuple[int, int], out_channels: int, n_heads: int,
                 add_self_loops_tx: bool = False):
        super().__init__()
        if add_self_loops_tx:
            raise NotImplementedError("add_self_loops_tx=True is never used by segger (ist_encoder.py:104)")
        self.out_channels, self.n_heads = out_channels, n_heads
        self.conv = _HeteroConv({
            TX_TX: GATv2Conv((in_channels[0], in_channels[0]), out_channels, n_heads),
            TX_BD: GATv2Conv((in_channels[0], in_channels[1]), out_channels, n_heads),
        })
        self.store_attention = False
        self._attn_weights: Dict[EdgeType, Tensor] = {}

    def forward(self, x_dict: Dict[str, Tensor], edge_index_dict: Dict[EdgeType, Tensor], *,
                graphs: Optional[Dict[EdgeType, EdgeGraph]] = None, apply_gelu: bool = False,
                seed=0, keep_bits: Optional[Dict[EdgeType, tuple]] = None) -> Dict[str, Tensor]:
        for et in (TX_TX, TX_BD):
            if et not in edge_index_dict:
                raise KeyError(f"edge type {et} missing from edge_index_dict: segger's HeteroConv would "
                               f"drop node type '{et[2]}' and fail in the next layer")
        x_tx, x_bd = x_dict["tx"], x_dict["bd"]
        if graphs is None:
            graphs = {et: edge_graph(None, et, edge_index_dict[et], x_dict[et[0]].shape[0], x_dict[et[2]].shape[0],
                                     validate="deferred")
                      for et in (TX_TX, TX_BD)}
        tt, tb = self.conv[TX_TX], self.conv[TX_BD]
        # one fused projection for the three linear maps that read x_tx (stacked and cast once per optimizer step)
        w_tx, b_tx = (tt.lin_l.weight, tt.lin_r.weight, tb.lin_l.weight), (tt.lin_l.bias, tt.lin_r.bias, tb.lin_l.bias)
        if isinstance(x_tx, ops.EmbedInput):
            xp_tx = ops.embed_linear(x_tx, w_tx, b_tx)
            xp_bd = ops.linear(x_bd, tb.lin_r.weight, tb.lin_r.bias)
        else:                    # both node types' projections in one launch (the boundary side rides in the grid)
            xp_tx, xp_bd = ops.linear_pair(x_tx, w_tx, b_tx, x_bd, tb.lin_r.weight, tb.lin_r.bias)
        p = tt.dropout if self.training else 0.0
        y_tx, y_bd, alpha = ops.hetero_gat_layer(
            xp_tx, xp_bd, tt.att, tt.bias, tb.att, tb.bias, graphs[TX_TX], graphs[TX_BD],
            self.n_heads, self.out_channels, apply_gelu=apply_gelu, negative_slope=tt.negative_slope,
            dropout_p=p, seed_tt=_layer_seed(seed, 0), seed_tb=_layer_seed(seed, 1), return_alpha=self.store_attention,
            bits_tt=None if keep_bits is None else keep_bits.get(TX_TX),
            bits_tb=None if keep_bits is None else keep_bits.get(TX_BD))
        if self.store_attention:
            self._attn_weights[TX_TX] = alpha
        return {"tx": y_tx, "bd": y_bd}

    @property
    def attention_weights(self) -> Dict[EdgeType, Tensor]:
        if not self._attn_weights:
            raise AttributeError("Attention weights are empty. Please perform a forward pass.")
        return self._attn_weights


class _HeteroDictLinear(Module):
    """``lins.{type}`` naming of torch_geometric.nn.HeteroDictLinear."""

    def __init__(self, in_channels: int, out_channels: int, types=("tx", "bd")):
        super().__init__()
        self.lins = ModuleDict({t: Linear(in_channels, out_channels, bias=True) for t in types})

    def forward(self, x_dict: Dict[str, Tensor]) -> Dict[str, Tensor]:
        out = {}
        if len(x_dict) == 2:     # lin_last of both node types: one launch
            (ka, xa), (kb, xb) = x_dict.items()
            la, lb = self.lins[ka], self.lins[kb]
            out[ka], out[kb] = ops.linear_pair(xa, la.weight, la.bias, xb, lb.weight, lb.bias)
            return out
        for k, x in x_dict.items():
            lin = self.lins[k]
            out[k] = ops.linear(x, lin.weight, lin.bias)
        return out


class ISTEncoder(Module):
    """Same constructor and ``forward(x_dict, edge_index_dict, pos_dict, batch_dict)``
    as the reference (ist_encoder.py:219-333).

    Extra keyword-only knobs (not in the reference): ``bd_in_channels`` (the
    reference's lazy ``Linear(-1, in)`` is materialised on first forward when
    this is None), ``compute_dtype`` (activations; parameters stay fp32).
    """

    def __init__(self, n_genes: int, in_channels: int = 16, hidden_channels: int = 32, out_channels: int = 32,
                 n_mid_layers: int = 3, n_heads: int = 3, normalize_embeddings: bool = True,
                 use_positional_embeddings: bool = True, *, bd_in_channels: Optional[int] = None,
                 compute_dtype: torch.dtype = torch.float32):
        super().__init__()
        self.normalize_embeddings = normalize_embeddings
        self.use_positional_embeddings = use_positional_embeddings
        self.compute_dtype = compute_dtype
        self.hparams = dict(n_genes=n_genes, in_channels=in_channels, hidden_channels=hidden_channels,
                            out_channels=out_channels, n_mid_layers=n_mid_layers, n_heads=n_heads,
                            normalize_embeddings=normalize_embeddings,
                            use_positional_embeddings=use_positional_embeddings)
        self.in_channels, self.n_heads = in_channels, n_heads
        self.lin_first = ModuleDict({"tx": Embedding(n_genes, in_channels)})
        if bd_in_channels is not None:
            self.lin_first["bd"] = Linear(bd_in_channels, in_channels)
        self.pos_emb = Positional2dEmbedder(in_channels)
        f0 = 2 * in_channels if use_positional_embeddings else in_channels
        self.conv_layers = ModuleList()
        self.conv_layers.append(SkipGAT((f0, f0), hidden_channels, n_heads))
        for _ in range(n_mid_layers):
            self.conv_layers.append(SkipGAT((hidden_channels * n_heads,) * 2, hidden_channels, n_heads))
        last_in = hidden_channels * n_heads
        self.conv_layers.append(SkipGAT((last_in, last_in), out_channels, n_heads))
        self.lin_last = _HeteroDictLinear(out_channels * n_heads, out_channels, types=("tx", "bd"))
        # dropout stream: effective seed of (layer, edge type, step) = 2*layer + type + *_step_dev; the counter
        # lives on the device and advances by 256 per training forward, so captured graphs see fresh masks
        self.register_buffer("_step_dev", torch.zeros(1, dtype=torch.int64), persistent=False)
        self.register_load_state_dict_pre_hook(ISTEncoder._adopt_reference_state_dict)

    @staticmethod
    def _adopt_reference_state_dict(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                    error_msgs) -> None:
        """Makes a reference checkpoint load with ``strict=True``: the reference's lazy ``Linear(-1, in)`` for
        boundaries (ist_encoder.py:261) is materialised from the shape of the incoming ``lin_first.bd.weight``
        (instead of being fabricated at random by the first forward), and the entries of the never-initialised
        ``('bd','contains','tx')`` conv (lazy placeholders, no trained values) are dropped."""
        w = state_dict.get(prefix + "lin_first.bd.weight")
        if w is not None and "bd" not in module.lin_first and getattr(w, "dim", lambda: 0)() == 2:
            ref = module.lin_first["tx"].weight
            module.lin_first["bd"] = Linear(int(w.shape[1]), int(w.shape[0])).to(device=ref.device)
        for k in [k for k in state_dict if k.startswith(prefix) and "<bd___contains___tx>" in k]:
            del state_dict[k]

    def plane_views(self, graphs, seed_offset: int = 0):
        """The CSR views whose attention-dropout masks a training step needs as bit planes: [(edge type, side, csr, seeds)]
        (side 0 = by destination, 1 = by source), or None when the planes do not apply."""
        n_layers = len(self.conv_layers)
        first = self.conv_layers[0]
        if n_layers > 16 or self.n_heads > 8 or not (first.conv[TX_TX].dropout > 0):
            return None
        views = []
        for which, et in ((0, TX_TX), (1, TX_BD)):
            g = graphs.get(et)
            if g is None or g.by_dst is None:
                continue
            seeds = [2 * li + which + int(seed_offset) for li in range(n_layers)]
            views += [(et, 0, g.by_dst, seeds)] + ([(et, 1, g.by_src, seeds)] if g.by_src is not None else [])
        return views

    @staticmethod
    def planes_of(views, bits) -> dict:
        out = {}
        for (et, side, _, _), b in zip(views, bits):
            out.setdefault(et, [None, None])[side] = b
        return {et: tuple(v) for et, v in out.items()}

    def _dropout_planes(self, graphs, step):
        """The attention-dropout masks of all layers as bit planes per CSR view (``ops.dropout_bits_many``): one launch
        per step; the 12 aggregation launches of the step then test a bit per (edge, head) instead of hashing."""
        views = self.plane_views(graphs)
        if views is None:
            return None
        p = self.conv_layers[0].conv[TX_TX].dropout
        return self.planes_of(views, ops.dropout_bits_many([(c, sd) for _, _, c, sd in views], self.n_heads, p, step))

    def front_plan(self, n_tx: int, *, on_gpu: bool, batched: bool, staged_pos: bool = False) -> FrontPlan:
        """The input stage's route for ``n_tx`` transcripts, from shapes, dtypes, grad mode and the switches of ``ops``: nothing
        is launched.  ``batched``: both node types have a batch vector and the graph count is known; ``staged_pos``: the
        caller (a captured step) concatenated the two types' positions itself."""
        if not self.use_positional_embeddings:
            return FrontPlan()
        dt = self.compute_dtype
        table = self.in_channels % 32 == 0 and self.lin_first["tx"].weight.dtype == torch.float32
        split = False
        if table and ops.SPLIT_FIRST_LAYER and on_gpu:
            first = self.conv_layers[0].conv
            m_first = sum(int(w.shape[0]) for w in (first[TX_TX].lin_l.weight, first[TX_TX].lin_r.weight,
                                                    first[TX_BD].lin_l.weight))
            min_rows = ops.SPLIT_FIRST_LAYER_MIN_ROWS_F32 if dt == torch.float32 else ops.SPLIT_FIRST_LAYER_MIN_ROWS
            split = n_tx >= min_rows and ops.embed_linear_supported(self.in_channels, m_first, dt)
        join = table and ops.FRONT_JOIN
        # ONE embedder call for both node types (the reference calls it per type, ist_encoder.py:314-318): graph ids
        # of the boundaries are offset by num_graphs, so the per-graph min / max stay per type.  Half the launches
        # of the front end, and the embedder's parameters receive ONE gradient each (what lets a captured step
        # postpone its partial sums, ops.deferred_reductions).  `split` (large batches) keeps one call per type: the
        # launches do not matter there, and joining the two gradients of the embedder's output would copy [n_tx, D].
        merged = staged_pos or (ops.MERGED_POS_EMBED and not split and batched)
        pair_node = split and join and not merged and _pair_node_applies(self.pos_emb, on_gpu, batched, dt)
        return FrontPlan(True, table, split, join, merged, pair_node)

    def _pos_embed_pair(self, plan: FrontPlan, pos_dict, batch_dict, num_graphs, staged: StagedInputs) -> PosPair:
        """``pos_emb`` of both node types as ``plan`` says.  `split`: the GELU of ist_encoder.py:320 comes applied to the
        transcripts' half (gelu(cat(a, b)) = cat(gelu(a), gelu(b))), and to the boundaries' unless ``ops.front_join``
        applies it (``plan.join`` with one call per type)."""
        dt, emb = self.compute_dtype, self.pos_emb
        if plan.pair_node:
            (act, pre), pe_bd = _pair_node(emb, pos_dict["tx"], batch_dict["tx"], pos_dict["bd"], batch_dict["bd"], num_graphs, dt)
            return PosPair(act, pre, pe_bd)
        if not plan.merged:
            tx = emb._embed(pos_dict["tx"], batch_dict.get("tx"), num_graphs, dt, gelu=plan.split, want_pre=True)
            bd = emb._embed(pos_dict["bd"], batch_dict.get("bd"), num_graphs, dt, gelu=plan.split and not plan.join)
            return PosPair(tx.out, tx.pre, bd.out, None, bd.gelu_applied)
        if staged.pos_all is not None:
            pos_all, batch_all = staged.pos_all, staged.batch_all
        else:
            pos_all = torch.cat((pos_dict["tx"].float(), pos_dict["bd"].float()), 0)
            batch_all = torch.cat((batch_dict["tx"].long(), batch_dict["bd"].long() + int(num_graphs)), 0)
        pe = emb._embed(pos_all, batch_all, 2 * int(num_graphs), dt, gelu=plan.split, minmax=staged.minmax)
        if plan.join and not plan.split:
            return PosPair(joint=pe.out)
        pe_tx, pe_bd = _SplitRows.apply(pe.out, int(pos_dict["tx"].shape[0]))
        return PosPair(pe_tx, None, pe_bd, None, pe.gelu_applied)

    def _materialize_bd(self, d_in: int, device) -> None:
        if "bd" not in self.lin_first:
            self.lin_first["bd"] = Linear(d_in, self.in_channels).to(device)

    def _front_end(self, x_dict, pos_dict, batch_dict, num_graphs, cache, staged: StagedInputs) -> Dict[str, Tensor]:
        """The layers' input (ist_encoder.py:312-320): ``gelu(cat(lin_first(x), pos_emb(pos)))`` per node type."""
        dt = self.compute_dtype
        self._materialize_bd(x_dict["bd"].shape[-1], x_dict["bd"].device)
        bd_lin, emb, ids = self.lin_first["bd"], self.lin_first["tx"], x_dict["tx"]
        x_bd = ops.linear(x_dict["bd"].to(dt), bd_lin.weight, bd_lin.bias)
        batched = batch_dict.get("tx") is not None and batch_dict.get("bd") is not None and num_graphs is not None
        plan = self.front_plan(int(ids.shape[0]), on_gpu=x_bd.is_cuda, batched=batched, staged_pos=staged.pos_all is not None)
        if not plan.positional:
            return {"bd": F.gelu(x_bd), "tx": F.gelu(emb(ids.long()).to(dt))}
        pe = self._pos_embed_pair(plan, pos_dict, batch_dict, num_graphs, staged)
        if pe.joint is None:
            if pe.bd_gelu_applied:
                x_bd = torch.cat((F.gelu(x_bd), pe.bd), -1)
            elif plan.join:      # the boundary side alone through the join (no transcript rows, no table gradient)
                _, x_bd = ops.front_join(emb.weight.detach(), ids[:0], x_bd, pe.bd, None)
            else:
                x_bd = F.gelu(torch.cat((x_bd, pe.bd), -1))
        if not plan.table:
            return {"tx": F.gelu(torch.cat((emb(ids.long()).to(dt), pe.tx), -1)), "bd": x_bd}
        # gather + concat + GELU in one kernel; its table gradient sums over rows grouped by gene id: one sort per
        # batch (not needed without grad), cached with the batch or staged
        need = staged.by_gene is not None or (torch.is_grad_enabled() and emb.weight.requires_grad)
        by_gene = rows_by_gene(ids, emb.weight.shape[0], cache, staged.by_gene) if need else None
        if pe.joint is not None:
            # both node types in one launch, and back in one (no torch cat + GELU on 'bd', no cat of the two slices' gradients)
            x_tx, x_bd = ops.front_join(emb.weight, ids, x_bd, pe.joint, by_gene)
        elif plan.split:
            # keep gelu(cat(E[g], pe)) as its parts: the first layer projects it as T[g] + W_pe gelu(pe)
            x_tx = ops.EmbedInput(emb.weight, ids.to(torch.int32).contiguous(), pe.tx, by_gene, pe.tx_pre)
        else:
            x_tx = ops.embed_gelu(emb.weight, ids, pe.tx, by_gene)
        return {"tx": x_tx, "bd": x_bd}

    def forward(self, x_dict: Dict[str, Tensor], edge_index_dict: Dict[EdgeType, Tensor],
                pos_dict: Dict[str, Tensor], batch_dict: Dict[str, Tensor], *,
                num_graphs: Optional[int] = None, cache: Optional[dict] = None,
                graphs: Optional[Dict[EdgeType, EdgeGraph]] = None,
                staged: StagedInputs = StagedInputs()) -> Dict[str, Tensor]:
        x = self._front_end(x_dict, pos_dict, batch_dict, num_graphs, cache, staged)
        if graphs is None:       # sorted views of the edge stores: built once per batch, shared by all layers
            # the by-source view only serves the backward: inference sorts each edge store once, not twice
            # tx-belongs-bd: a transcript lies in at most one boundary (heterodata.py:147), so its backward needs no
            # by-source view; "lazy" verifies that on the device and sorts only if it does not hold (graph.EdgeGraph)
            by_src = {TX_TX: True, TX_BD: "lazy"} if torch.is_grad_enabled() else {TX_TX: False, TX_BD: False}
            graphs = {et: edge_graph(cache, et, edge_index_dict[et], x[et[0]].shape[0], x[et[2]].shape[0],
                                     need_by_src=by_src[et],
                                     validate="deferred")     # checked without a host sync (graph.py)
                      for et in (TX_TX, TX_BD) if et in edge_index_dict}
        planes, step, seed_off = None, self._step_dev, 0
        if self.training and staged.draws is not None:
            # a captured step made all of its draws up front in one launch (ops.step_draws) from the counter as it stands
            # and advances it at its end: (planes | None, constant added to every seed)
            planes, seed_off = staged.draws
        elif self.training:
            # every training forward gets its own snapshot of the advanced counter: its backward re-reads THAT word,
            # so a second forward before the first backward (two views, checkpointing, a logging pass) cannot change
            # the masks the first backward regenerates.  Capture-safe: the clone lives in the graph's pool.
            if self._step_dev.is_cuda:
                step = ops.step_advance(self._step_dev, 256)
            else:
                self._step_dev.add_(256)
                step = self._step_dev.clone()
            planes = self._dropout_planes(graphs, step)
        for li, layer in enumerate(self.conv_layers):
            kb = None if planes is None else {et: (d[li], None if s_ is None else s_[li]) for et, (d, s_) in planes.items()}
            x = layer(x, edge_index_dict, graphs=graphs, apply_gelu=True, seed=(li, step, seed_off), keep_bits=kb)   # conv + GELU (:324-325)

        x = self.lin_last(x)
        if self.normalize_embeddings:
            x = ops.l2_normalize_many(x)                     # both node types in one launch
        return x
