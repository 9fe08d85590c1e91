"""Fragment cells on the device: what happens to the transcripts a segmentation leaves with ``cell_encoding = -1``.

Upstream segger calls it "fragment mode" (``use_cc``): unassigned transcripts that are neighbours in the transcript graph and
whose embeddings agree are grouped into connected components, and components of a minimum size become extra cells.  The
reference snapshot this project follows does NOT contain that code, so the contract is this project's own (``include/
segger_amd.h``) and is UNPINNED by any reference run; ``tests/fragment_cases.py`` restates it sequentially.

A directed edge ``(s, d)`` of a batch is **live** when ``mask[s]`` is true (the tile that owns the source scores the edge, so
overlapping prediction tiles count each directed edge once), both ``unassigned[tx_index[s]]`` and ``unassigned[tx_index[d]]``
are true, and the two transcripts differ.  A live edge is **kept** when ``sim(s, d) >= min_similarity`` (inclusive; ``sim`` is
``torch.cosine_similarity``'s form with ``eps = 1e-8`` in correctly rounded fp32, or the caller's own per-edge value).  Kept
edges count as undirected.  **Fragments** are the connected components of the kept edges with at least ``min_size`` members,
numbered by their smallest transcript, ascending: the labels are a function of the SET of kept edges -- not of the order of
the edges, the batches, the chunking or the atomics, bit for bit.

:class:`FragmentAccumulator` is the streaming form (``csrc/fragments.hip``: one launch per batch that never waits for the
device; 4 bytes of state per transcript), :func:`fragment_cells` the one-shot form, :func:`connected_components` the bare
min-id labelling for callers with their own edge filter; :func:`unassigned_mask` and :func:`merge_fragments` connect it to
``SegmentationAccumulator.segmentation()`` on one side and to ``expression_matrix`` / ``segmentation_boundaries`` /
``segmentation_outlines`` on the other.

The defaults ``min_similarity = 0.5`` and ``min_size = 5`` are upstream's habit, not a measurement of this project.

NOT BUILT: capturing ``update`` into the graphed predictor; more than one GPU; a CPU path (the oracle in
``tests/fragment_cases.py`` is test infrastructure)."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib as L
from .hetero import TX_TX

__all__ = ["FragmentAccumulator", "fragment_cells", "connected_components", "unassigned_mask", "merge_fragments",
           "similarity_error_bound", "COUNTER_NAMES", "MAX_CHANNELS"]

COUNTER_NAMES = ("n_edges", "n_live_edges", "n_kept_edges", "n_bad", "n_candidates", "n_components", "n_fragments", "n_bad_parent")
MAX_CHANNELS = L.FRAGMENTS_MAX_CHANNELS
_HINT = "tests/fragment_cases.py holds the CPU oracle"
_Z_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def similarity_error_bound(channels: int, dtype: torch.dtype = torch.float32) -> float:
    """An upper bound on ``|sim_fp32 - sim_exact|`` of the device cosine over rows of ``channels`` stored values (no
    overflow or underflow, both norms above ``eps``): ``(2 C + 6) 2^-24`` for fp32 rows and ``(2 C + 4) 2^-24`` for bf16 / fp16
    rows, whose products are exact in fp32 (DESIGN 3.5p has the derivation).  A live edge whose exact cosine is farther than
    this from ``min_similarity`` is decided as exact arithmetic decides it."""
    c = int(channels)
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"similarity_error_bound: channels must be in [1, {MAX_CHANNELS}], got {c}")
    if dtype not in _Z_DTYPES:
        raise ValueError(f"similarity_error_bound: dtype must be one of {_Z_DTYPES}, got {dtype}")
    return (2 * c + (6 if dtype == torch.float32 else 4)) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ validation ---
def _check_n(who: str, n_transcripts) -> int:
    n = int(n_transcripts)
    if not 1 <= n < (1 << 31):
        raise ValueError(f"{who}: n_transcripts must be in [1, 2^31), got {n}")
    return n


def _check_unassigned(who: str, unassigned, n: int) -> None:
    if not isinstance(unassigned, Tensor) or unassigned.dtype != torch.bool or unassigned.dim() != 1:
        raise ValueError(f"{who}: unassigned is a 1-D bool tensor")
    if int(unassigned.numel()) != n:
        raise ValueError(f"{who}: unassigned has {int(unassigned.numel())} entries, n_transcripts is {n}")


def _check_min_similarity(who: str, min_similarity) -> float:
    m = float(min_similarity)
    if math.isnan(m):
        raise ValueError(f"{who}: min_similarity is NaN")
    return m


def _check_result_args(who: str, min_size, first_id) -> None:
    if isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 1:
        raise ValueError(f"{who}: min_size must be an integer >= 1, got {min_size!r}")
    if isinstance(first_id, bool) or not isinstance(first_id, int) or not 0 <= first_id < (1 << 62):
        raise ValueError(f"{who}: first_id must be an integer in [0, 2^62), got {first_id!r}")


def _check_batch(who: str, n_transcripts: int, z, edge_index, tx_index, mask, similarity, keep) -> int:
    """Every refusal of one batch that needs no device; returns the number of local nodes."""
    if not isinstance(edge_index, Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2 or \
            edge_index.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{who}: edge_index is an int64 (or int32) [2, e] tensor")
    e = int(edge_index.shape[1])
    if z is not None and similarity is not None:
        raise ValueError(f"{who}: give z or similarity, not both")
    if z is not None:
        if not isinstance(z, Tensor) or z.dim() != 2 or z.dtype not in _Z_DTYPES:
            raise ValueError(f"{who}: z is a 2-D fp32, bf16 or fp16 tensor [n, C]")
        if not 1 <= int(z.shape[1]) <= MAX_CHANNELS:
            raise ValueError(f"{who}: z has {int(z.shape[1])} channels, outside [1, {MAX_CHANNELS}]")
        if int(z.shape[0]) >= (1 << 31):
            raise ValueError(f"{who}: z has 2^31 rows or more")
    if similarity is not None:
        if not isinstance(similarity, Tensor) or similarity.dtype != torch.float32 or similarity.dim() != 1 or \
                int(similarity.numel()) != e:
            raise ValueError(f"{who}: similarity is a 1-D fp32 tensor with one value per edge ({e})")
    if keep is not None:
        if not isinstance(keep, Tensor) or keep.dtype != torch.bool or keep.dim() != 1 or int(keep.numel()) != e:
            raise ValueError(f"{who}: keep is a 1-D bool tensor with one value per edge ({e})")
    if tx_index is not None:
        if not isinstance(tx_index, Tensor) or tx_index.dim() != 1 or tx_index.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"{who}: tx_index is a 1-D int64 (or int32) tensor")
    if mask is not None:
        if not isinstance(mask, Tensor) or mask.dim() != 1 or mask.dtype != torch.bool:
            raise ValueError(f"{who}: mask is a 1-D bool tensor")
    sizes = [int(t.shape[0]) for t in (z, tx_index, mask) if t is not None]
    if len(set(sizes)) > 1:
        raise ValueError(f"{who}: z, tx_index and mask disagree on the number of nodes: {sizes}")
    n_nodes = sizes[0] if sizes else n_transcripts
    if n_nodes >= (1 << 31):
        raise ValueError(f"{who}: 2^31 nodes or more in a batch")
    return n_nodes


def _workspace_bytes(n: int) -> int:
    up = lambda x: (x + 255) // 256 * 256                            # noqa: E731
    return up(4 * n) + up(8 * ((n + L.FRAGMENTS_CHUNK - 1) // L.FRAGMENTS_CHUNK + 1))


# ------------------------------------------------------------------------------------------------ the accumulator ---
class FragmentAccumulator:
    """The streaming form: ``update`` one batch at a time, ``result()`` at the end.

    ``n_transcripts`` is the ``row_index`` domain and ``unassigned`` a bool mask over it (:func:`unassigned_mask` derives it
    from a finished segmentation).  The state is a union-find ``parent`` array, 4 bytes per transcript; ``update`` is one
    launch (``segger_fragments_update``) on torch's current stream that never waits for the device.  The result does not
    depend on the order of the edges, of the batches or of the atomics, bit for bit.  A ``tx_index`` or local id outside its
    range is never used as an address; it is counted and ``result()`` raises.

    ``min_similarity`` (default 0.5: upstream's habit, not a measurement) is rounded to fp32; the comparison is inclusive."""

    def __init__(self, n_transcripts: int, unassigned: Tensor, min_similarity: float = 0.5, device="cuda"):
        who = "FragmentAccumulator"
        n = _check_n(who, n_transcripts)
        _check_unassigned(who, unassigned, n)
        self.min_similarity = _check_min_similarity(who, min_similarity)
        self.device = torch.device(device)
        L.need_device(who, self.device, hint=_HINT)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_transcripts = n
        self.unassigned = unassigned.detach().to(self.device).contiguous()
        self.parent = torch.arange(n, dtype=torch.int32, device=self.device)
        self.counters = torch.zeros(L.FRAGMENTS_COUNTERS, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        """Forget every edge (enqueued like an update: no sync).  ``unassigned`` stays."""
        torch.arange(self.n_transcripts, dtype=torch.int32, out=self.parent)
        self.counters.zero_()

    def update(self, z_tx: Optional[Tensor], edge_index: Tensor, tx_index: Optional[Tensor] = None,
               mask: Optional[Tensor] = None) -> None:
        """Feed one batch: ``z_tx`` ``[n, C]`` (fp32, bf16 or fp16; ``1 <= C <= 1024``), ``edge_index`` ``[2, e]`` of local
        ids, ``tx_index`` ``[n]`` (``None``: the identity) and ``mask`` ``[n]`` bool (``None``: all true).  Enqueue only."""
        self._feed("FragmentAccumulator.update", z_tx, edge_index, tx_index, mask, None, None)

    def update_from_batch(self, model, batch) -> None:
        """One batch of the prediction loop: the unit-norm ``model.forward(batch)['tx']``, the ``tx-neighbors-tx`` edge index,
        ``batch['tx']['index']`` and ``batch['tx']['predict_mask']``.  Enqueue only."""
        with torch.no_grad():
            z = model.forward(batch)["tx"]
        self._feed("FragmentAccumulator.update_from_batch", z, batch[TX_TX].edge_index, batch["tx"]["index"],
                   batch["tx"]["predict_mask"], None, None)

    def _feed(self, who, z, edge_index, tx_index, mask, similarity, keep) -> None:
        n_nodes = _check_batch(who, self.n_transcripts, z, edge_index, tx_index, mask, similarity, keep)
        e = int(edge_index.shape[1])
        if e == 0:
            return
        dev = self.device
        ei = edge_index.detach().to(device=dev, dtype=torch.int64).contiguous()
        ti = None if tx_index is None else tx_index.detach().to(device=dev, dtype=torch.int64).contiguous()
        m = None if mask is None else mask.detach().to(dev).contiguous()
        s = None if similarity is None else similarity.detach().to(dev).contiguous()
        k = None if keep is None else keep.detach().to(dev).contiguous()
        ld, channels, code = 0, 0, 0
        if z is not None:
            z = z.detach().to(dev)
            if z.stride(1) != 1 or z.stride(0) < z.shape[1]:
                z = z.contiguous()
            ld, channels, code = int(z.stride(0)), int(z.shape[1]), L.DTYPE_CODE[z.dtype]
        L.call("segger_fragments_update", dev, L.ptr(z), ld, channels, code, L.ptr(s), L.ptr(k), ei[0].data_ptr(),
               ei[1].data_ptr(), e, L.ptr(ti), L.ptr(m), n_nodes, self.unassigned.data_ptr(), self.n_transcripts,
               self.min_similarity, self.parent.data_ptr(), self.counters.data_ptr())

    def result(self, min_size: int = 5, first_id: int = 0) -> Dict[str, Tensor]:
        """The fragments of what has been fed so far, on the device:

        * ``fragment`` int64 ``[n_transcripts]``: ``first_id + rank`` for the members of a component of at least ``min_size``
          (default 5: upstream's habit) transcripts, ``-1`` for everything else; ``rank`` numbers those components by their
          smallest transcript, ascending;
        * ``root`` int64 (that smallest transcript) and ``size`` int64 per fragment, in rank order; ``first_id``;
        * Python ints: ``n_candidates`` (unassigned transcripts), ``n_edges`` (fed), ``n_live_edges``, ``n_kept_edges``,
          ``n_components`` (singletons included), ``n_fragments``, ``n_bad`` (0).

        The one place that waits for the device; raises if an edge had an id outside its range (nothing was written for
        it).  More updates may follow."""
        who = "FragmentAccumulator.result"
        _check_result_args(who, min_size, first_id)
        n, dev = self.n_transcripts, self.device
        cap = n // min_size
        fragment = torch.empty(n, dtype=torch.int64, device=dev)
        root = torch.empty(cap, dtype=torch.int32, device=dev)
        size = torch.empty(cap, dtype=torch.int32, device=dev)
        ws_bytes = _workspace_bytes(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        L.call("segger_fragments_finalize", dev, self.parent.data_ptr(), self.unassigned.data_ptr(), n, min_size, first_id,
               fragment.data_ptr(), L.ptr(root) if cap else None, L.ptr(size) if cap else None, cap, self.counters.data_ptr(),
               ws.data_ptr(), ws_bytes)
        c = dict(zip(COUNTER_NAMES, self.counters.tolist()))             # the one wait for the device
        del ws
        if c["n_bad"] or c["n_bad_parent"]:
            raise L.SeggerAmdError(f"FragmentAccumulator: {c['n_bad']} of {c['n_edges']} edges had a local id or a tx_index "
                                   f"outside its range ({c['n_bad_parent']} corrupt parent chains); nothing was written for them")
        f = c["n_fragments"]
        out = {"fragment": fragment, "root": root[:f].long(), "size": size[:f].long(), "first_id": first_id}
        out.update({k: c[k] for k in COUNTER_NAMES[:-1]})
        return out


# ------------------------------------------------------------------------------------------------ one-shot forms ---
def fragment_cells(edge_index: Tensor, unassigned: Tensor, z: Optional[Tensor] = None, similarity: Optional[Tensor] = None,
                   tx_index: Optional[Tensor] = None, mask: Optional[Tensor] = None, min_similarity: float = 0.5,
                   min_size: int = 5, first_id: int = 0) -> Dict[str, Tensor]:
    """One batch, one result: :class:`FragmentAccumulator` over ``unassigned`` (its length is ``n_transcripts``), one
    ``update``, ``result(min_size, first_id)``.  Exactly one of ``z`` (``[n, C]`` embeddings) and ``similarity`` (fp32, one
    value per edge) is given; with ``similarity`` the comparison with ``min_similarity`` is exact and no row is gathered.
    The defaults 0.5 and 5 are upstream's habit, not a measurement."""
    who = "fragment_cells"
    if not isinstance(unassigned, Tensor):
        raise ValueError(f"{who}: unassigned is a 1-D bool tensor")
    n = _check_n(who, unassigned.numel())
    _check_unassigned(who, unassigned, n)
    if (z is None) == (similarity is None):
        raise ValueError(f"{who}: give exactly one of z and similarity")
    _check_min_similarity(who, min_similarity)
    _check_result_args(who, min_size, first_id)
    _check_batch(who, n, z, edge_index, tx_index, mask, similarity, None)
    L.need_device(who, unassigned, edge_index, z, similarity, tx_index, mask, hint=_HINT)
    acc = FragmentAccumulator(n, unassigned, min_similarity, unassigned.device)
    acc._feed(who, z, edge_index, tx_index, mask, similarity, None)
    return acc.result(min_size, first_id)


def connected_components(edge_index: Tensor, n: int, keep: Optional[Tensor] = None) -> Tensor:
    """The bare labelling: ``labels`` int64 ``[n]``, the smallest node of each node's connected component over the edges of
    ``edge_index`` ``[2, e]`` (those with ``keep`` true, when given), taken as undirected.  Self loops and duplicates change
    nothing.  Waits for the device once; raises if an edge names a node outside ``[0, n)``."""
    who = "connected_components"
    n = _check_n(who, n)
    _check_batch(who, n, None, edge_index, None, None, None, keep)
    L.need_device(who, edge_index, keep, hint=_HINT)
    dev = edge_index.device
    acc = FragmentAccumulator(n, torch.ones(n, dtype=torch.bool, device=dev), 0.0, dev)
    acc._feed(who, None, edge_index, None, None, None, keep)
    acc.result(1, 0)                                                     # flattens parent, raises on a bad edge
    return acc.parent.long()


# ------------------------------------------------------------------------------------------------ the joints ---
_SEG_KEYS = ("row_index", "cell_encoding", "similarity", "similarity_threshold")


def _seg_columns(who: str, segmentation) -> list:
    try:
        cols = [segmentation[k] for k in _SEG_KEYS]
    except (KeyError, TypeError):
        raise ValueError(f"{who}: segmentation is the dict SegmentationAccumulator.segmentation() returns (keys {_SEG_KEYS})") from None
    n = int(cols[0].numel())
    if any(not isinstance(t, Tensor) or int(t.numel()) != n for t in cols):
        raise ValueError(f"{who}: columns of different lengths")
    return cols


def unassigned_mask(segmentation: Dict[str, Tensor], n_transcripts: int) -> Tensor:
    """bool ``[n_transcripts]``: true for every transcript that ``expression_matrix`` would NOT count -- ``cell_encoding < 0``,
    or ``similarity < similarity_threshold``, or a NaN on either side -- and for every transcript without a row in the
    segmentation.  Runs wherever the columns live (torch plumbing); no wait for the device."""
    who = "unassigned_mask"
    n = _check_n(who, n_transcripts)
    row, cell, sim, thr = _seg_columns(who, segmentation)
    counted = (cell >= 0) & (sim.double() >= thr.double())
    out = torch.ones(n, dtype=torch.bool, device=row.device)
    out[row.long()[counted]] = False
    return out


def merge_fragments(segmentation: Dict[str, Tensor], fragments: Dict[str, Tensor], n_cells: int) -> Dict[str, Tensor]:
    """A dict of the shape of ``segmentation`` in which the rows of fragment members carry ``cell_encoding = n_cells + rank``
    (``rank = fragment - first_id``), ``similarity_threshold = -inf`` and a NaN similarity replaced by 0, so that
    ``expression_matrix``, ``segmentation_boundaries`` and ``segmentation_outlines`` count them and take the dict
    unchanged; every other row and key is the input's.  ``n_cells`` is the cell id domain of the segmentation (fragment
    cells are numbered behind it).  A fragment member without a row in the segmentation (never predicted) stays out."""
    who = "merge_fragments"
    row, cell, sim, thr = _seg_columns(who, segmentation)
    if isinstance(n_cells, bool) or not isinstance(n_cells, int) or n_cells < 0:
        raise ValueError(f"{who}: n_cells must be an integer >= 0, got {n_cells!r}")
    try:
        frag, first_id = fragments["fragment"], int(fragments["first_id"])
    except (KeyError, TypeError):
        raise ValueError(f"{who}: fragments is the dict FragmentAccumulator.result() returns") from None
    if n_cells + int(fragments.get("n_fragments", 0)) >= (1 << 31):
        raise ValueError(f"{who}: n_cells + n_fragments reaches 2^31 (cell encodings are kept as int32 downstream)")
    f = frag.to(row.device)[row.long()]
    member = f >= 0
    out = dict(segmentation)
    out["cell_encoding"] = torch.where(member, (f - first_id + n_cells).to(cell.dtype), cell)
    out["similarity_threshold"] = torch.where(member, torch.full_like(thr, float("-inf")), thr)
    out["similarity"] = torch.where(member & sim.isnan(), torch.zeros_like(sim), sim)
    return out
