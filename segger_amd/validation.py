"""Contamination scoring of a segmentation, on the device: the reference's ``src/segger/validation/contamination.py``
from the tensors :func:`segger_amd.postprocess.expression_matrix` returns and a cell-type label per cell (for instance the
clusters of :func:`segger_amd.phenograph.phenograph`).  Tensors in, tensors out: no AnnData, polars or pandas.

* :func:`neighbor_frequencies` -- ``get_neighbor_frequencies``: the type frequencies of every cell's spatial neighbours
  (``neighbors.knn_grid`` + ``segger_neighbor_frequencies``).
* :func:`reference_table` -- ``expression_summary_from_anndata``: the per-(type, gene) table ``n``, ``me``, ``pc`` of an
  annotated count matrix.  Plain device torch: it runs once over a small atlas, it is plumbing and not a kernel.
* :func:`calculate_contamination` -- the three-way posterior (own type, neighbouring type, background) of every stored
  (cell, gene) count and ``percent_contamination`` per cell (``segger_contamination_posterior``).  The reference
  materialises ``neigh[rows]``, ``L[:, gene_idx].T`` and their product, three ``nnz x T`` matrices; here nothing of that
  size is built -- a wave owns a row and sums over the types in registers.
* :func:`contamination_flow` -- the donor -> host table, through ``features.sparse_project``.

Arithmetic is float64 (the reference multiplies and sums ``neigh * L`` in float32), each ``q`` layer rounded once to
float32.  Two deliberate deviations from the reference:

* a cell with no type (label -1): the reference indexes ``L[-1, g]``, numpy's wrap-around to the LAST type; here such a
  cell gets ``P_self = eps`` and all types count as neighbouring types;
* an unlabelled neighbour makes the reference's ``csr_matrix`` raise (column -1); here it is skipped.

Not built: ``group_reference`` (a regrouping of the table a caller does on the host).  There is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .features import csr_row_sums, deterministic_sums, sparse_project
from .neighbors import knn_grid

__all__ = ["neighbor_frequencies", "reference_table", "contamination_posterior", "calculate_contamination", "contamination_flow"]


_CPU_HINT = "tests/contamination_cases.py holds the CPU oracle"


def _n_types(n_types: int) -> int:
    n_types = int(n_types)
    if not 1 <= n_types <= L.CONTAM_MAX_TYPES:
        raise ValueError(f"n_types = {n_types} outside 1 .. {L.CONTAM_MAX_TYPES}")
    return n_types


def _gene_map(expr: Dict[str, Tensor], gene_map: Optional[Tensor], n_ref: int) -> Tensor:
    """table column of every CSR column, -1 where the table lacks the gene; by default the gene ids ARE the columns"""
    gm = (expr["gene_ids"] if gene_map is None else gene_map).to(device=expr["indptr"].device, dtype=torch.int64).view(-1)
    return torch.where((gm >= 0) & (gm < n_ref), gm, torch.full_like(gm, -1)).to(torch.int32).contiguous()


def neighbor_frequencies(xy: Tensor, labels: Tensor, k: int, n_types: int, max_distance: Optional[float] = None,
                         normalize: bool = True, knn: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
    """``get_neighbor_frequencies``: for every cell the types of its ``k`` nearest cells, ITSELF INCLUDED (cuML's
    ``kneighbors`` on its own training set).  ``xy`` ``[n, 2]``, ``labels`` ``[n]`` in ``[0, n_types)`` or -1.  A neighbour
    counts iff its distance is ``<= max_distance`` (``None``: no limit -- the test is the reference's own, on the distance
    table, not ``knn_grid``'s search radius) and it has a label.  Returns ``(freq, counts)``: ``counts`` int32
    ``[n, n_types]`` and ``freq`` float32, each row of ``counts`` times ``1.0 / sum`` in float64 and rounded (zeros when the
    sum is 0); with ``normalize=False`` ``freq`` is ``counts`` as float32.  ``knn`` = ``(nbr, dist)`` uses a neighbour table
    computed elsewhere, in ``knn_grid``'s format, instead of searching.  Waits for the device once, inside ``knn_grid``."""
    L.need_device("neighbor_frequencies", xy, labels, hint=_CPU_HINT)
    n_types = _n_types(n_types)
    dev = xy.device
    n = int(xy.shape[0])
    labels = labels.detach().to(device=dev, dtype=torch.int32).contiguous().view(-1)
    if int(labels.numel()) != n:
        raise ValueError("neighbor_frequencies: one label per point")
    max_distance = math.inf if max_distance is None else float(max_distance)
    nbr, dist = knn_grid(xy, int(k), return_dist=True) if knn is None else knn
    L.need_device("neighbor_frequencies", nbr, dist, hint=_CPU_HINT)
    nbr = nbr.detach().to(torch.int32).contiguous()
    dist = dist.detach().to(torch.float32).contiguous()
    if nbr.dim() != 2 or nbr.shape != dist.shape or int(nbr.shape[0]) != n:
        raise ValueError("neighbor_frequencies: nbr and dist are [n, k]")
    counts = torch.empty(n, n_types, dtype=torch.int32, device=dev)
    freq = torch.empty(n, n_types, dtype=torch.float32, device=dev)
    L.call("segger_neighbor_frequencies", dev, nbr.data_ptr(), dist.data_ptr(), labels.data_ptr(), n, int(nbr.shape[1]),
           n_types, max_distance, counts.data_ptr(), freq.data_ptr())
    return (freq if normalize else counts.float()), counts


def reference_table(indptr: Tensor, indices: Tensor, counts: Tensor, cell_type: Tensor, n_types: int, min_counts: int = 2,
                    n_genes: Optional[int] = None) -> Dict[str, Tensor]:
    """``expression_summary_from_anndata`` of an annotated count matrix (canonical CSR, ``cell_type`` ``[n_cells]`` in
    ``[0, n_types)`` or -1 for a cell that takes no part), float64: ``normalize_total(1e4)`` (every count over
    ``row_total / 1e4``), ``log1p``; the entries whose RAW count is ``>= min_counts`` are kept; per (type, gene) ``n`` =
    the kept entries, ``me`` = their mean, ``pc = n / n_cells`` and ``weight = pc * me`` (0 where ``n = 0``), the table
    :func:`calculate_contamination` takes.  Returns ``n`` int64 ``[n_types, n_genes]``, ``me``, ``pc``, ``weight`` float64
    of that shape and ``n_cells`` int64 ``[n_types]``.  ``n_genes`` defaults to ``indices.max() + 1`` (one wait).

    Device torch under :func:`~segger_amd.features.deterministic_sums`: this runs once over a small annotated atlas -- it is
    plumbing, not a kernel."""
    L.need_device("reference_table", indptr, indices, counts, cell_type, hint=_CPU_HINT)
    n_types = _n_types(n_types)
    dev = indptr.device
    if n_genes is None:
        n_genes = int(indices.max()) + 1 if indices.numel() else 1
    n_genes = int(n_genes)
    n_cells = int(indptr.numel()) - 1
    cell_type = cell_type.to(device=dev, dtype=torch.int64).view(-1)
    rows = torch.repeat_interleave(torch.arange(n_cells, device=dev), indptr.diff(), output_size=int(indices.numel()))
    total = csr_row_sums(indptr, counts).double()
    value = torch.log1p(counts.double() / (total / 1e4)[rows])
    kind = cell_type[rows]
    keep = (counts >= int(min_counts)) & (kind >= 0) & (kind < n_types) & (value > 0)
    key = (kind * n_genes + indices.long())[keep]
    with deterministic_sums():
        n = torch.zeros(n_types * n_genes, dtype=torch.int64, device=dev).index_add_(0, key, torch.ones_like(key))
        s = torch.zeros(n_types * n_genes, dtype=torch.float64, device=dev).index_add_(0, key, value[keep])
    n, s = n.view(n_types, n_genes), s.view(n_types, n_genes)
    labelled = cell_type[(cell_type >= 0) & (cell_type < n_types)]
    cells = torch.bincount(labelled, minlength=n_types)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    me = torch.where(n > 0, s / n.clamp_min(1).double(), zero)
    pc = torch.where(n > 0, n.double() / cells.clamp_min(1).double()[:, None], zero)
    return {"n": n, "me": me, "pc": pc, "n_cells": cells, "weight": pc * me}


def _likelihood(weight: Tensor, host: Tensor, T: int, eps: float) -> Tuple[Tensor, Tensor]:
    """``L = float32(weight) + eps`` gene-major and padded to four types (the one transpose), and ``back = A @ L`` with ``A``
    the share of each type among the labelled cells"""
    dev = weight.device
    lik = weight.detach().to(torch.float32) + eps                                        # the reference's float32 L
    lik_t = torch.zeros(int(weight.shape[1]), (T + 3) // 4 * 4, dtype=torch.float32, device=dev)
    lik_t[:, :T] = lik.T
    slot = torch.where((host >= 0) & (host < T), host, torch.full_like(host, -1)).long() + 1       # 0: no label
    share = torch.zeros(T + 1, dtype=torch.int64, device=dev).index_add_(0, slot, torch.ones_like(slot))[1:].double()
    share = share / share.sum().clamp_min(1.0)                                           # integer counts: no wait, any order
    return lik_t, (share[:, None] * lik.double()).sum(dim=0).contiguous()                # A @ L: T x G_ref, an ordered sum


def contamination_posterior(indptr: Tensor, indices: Tensor, counts: Tensor, gene_map: Tensor, host_type: Tensor, freq: Tensor,
                            lik_t: Tensor, back: Tensor, n_types: int, alpha_self: float = 0.8, alpha_neighbor: float = 0.15,
                            alpha_background: float = 0.05, eps: float = 1e-6, contam_cutoff: float = 0.5) -> Dict[str, Tensor]:
    """``segger_contamination_posterior`` on prepared tensors, one launch and nothing else (what
    :func:`calculate_contamination` ends in): the CSR, ``gene_map`` int32 per CSR column, ``host_type`` int32 per row,
    ``freq`` float32 ``[n, n_types]``, ``lik_t`` float32 ``[G_ref, ld]`` -- the likelihood table GENE-MAJOR, ``ld`` a multiple
    of 4 and ``>= n_types`` -- and ``back`` float64 ``[G_ref]``.  Returns the seven kernel outputs."""
    L.need_device("contamination_posterior", indptr, indices, counts, gene_map, host_type, freq, lik_t, back, hint=_CPU_HINT)
    dev = indptr.device
    T = _n_types(n_types)
    indptr = indptr.detach().to(torch.int64).contiguous()
    indices = indices.detach().to(torch.int32).contiguous()
    counts = counts.detach().to(torch.int32).contiguous()
    gene_map = gene_map.detach().to(torch.int32).contiguous()
    host_type = host_type.detach().to(torch.int32).contiguous()
    freq = freq.detach().to(torch.float32).contiguous()
    lik_t = lik_t.detach().to(torch.float32).contiguous()
    back = back.detach().to(torch.float64).contiguous()
    n, nnz = int(indptr.numel()) - 1, int(indices.numel())
    if lik_t.dim() != 2 or tuple(freq.shape) != (n, T) or int(host_type.numel()) != n or int(back.numel()) != int(lik_t.shape[0]):
        raise ValueError("contamination_posterior: freq is [n, n_types], host_type [n], lik_t [G_ref, ld], back [G_ref]")
    G_ref, ld = int(lik_t.shape[0]), int(lik_t.shape[1])
    out = {"q_self": torch.empty(nnz, dtype=torch.float32, device=dev),
           "q_neighbor": torch.empty(nnz, dtype=torch.float32, device=dev),
           "q_background": torch.empty(nnz, dtype=torch.float32, device=dev),
           "contamination": torch.empty(nnz, dtype=torch.int32, device=dev)}
    per_cell = torch.zeros if nnz == 0 else torch.empty                                  # no entries: the kernel writes nothing
    out["contaminated"] = per_cell(n, dtype=torch.int64, device=dev)
    out["total"] = per_cell(n, dtype=torch.int64, device=dev)
    out["percent_contamination"] = per_cell(n, dtype=torch.float64, device=dev)
    L.call("segger_contamination_posterior", dev,
           indptr.data_ptr(), indices.data_ptr(), counts.data_ptr(), n, int(gene_map.numel()), nnz, gene_map.data_ptr(),
           host_type.data_ptr(), freq.data_ptr(), lik_t.data_ptr(), ld, back.data_ptr(), T, G_ref, float(alpha_self),
           float(alpha_neighbor), float(alpha_background), float(eps), float(contam_cutoff), out["q_self"].data_ptr(),
           out["q_neighbor"].data_ptr(), out["q_background"].data_ptr(), out["contamination"].data_ptr(),
           out["contaminated"].data_ptr(), out["total"].data_ptr(), out["percent_contamination"].data_ptr())
    return out


def calculate_contamination(expr: Dict[str, Tensor], cell_type: Tensor, weight: Tensor, gene_map: Optional[Tensor] = None, *,
                            n_neighbors: int = 10, max_neighbor_distance: Optional[float] = 20.0, alpha_self: float = 0.8,
                            alpha_neighbor: float = 0.15, alpha_background: float = 0.05, eps: float = 1e-6,
                            contam_cutoff: float = 0.5, knn: Optional[Tuple[Tensor, Tensor]] = None) -> Dict[str, Tensor]:
    """The reference's ``calculate_contamination``.  ``expr`` is what ``expression_matrix(..., xy=)`` returns (it must hold
    ``centroid``); ``cell_type`` ``[n_cells_present]`` in ``[0, T)`` or -1; ``weight`` ``[T, G_ref]`` the ``pc * me`` table
    (:func:`reference_table`), ``L = float32(weight) + eps``; ``gene_map`` the table column of every CSR column (-1: the
    table lacks the gene), by default ``expr["gene_ids"]`` themselves where they are below ``G_ref``.

    For every stored entry (cell r, gene g, count v), in float64: ``P_self = L[type_r, g]``; ``P_neigh = sum_{t != type_r}
    freq[r, t] L[t, g] + eps``; ``P_back = (A @ L)[g] + eps`` with ``A`` the share of each type among the labelled cells;
    ``q_x = alpha_x P_x / sum``.  An entry whose gene the table lacks gets three zeros and is never flagged.

    Returns ``q_self``, ``q_neighbor``, ``q_background`` float32 ``[nnz]`` (layers over the CSR of ``expr``),
    ``contamination`` int32 ``[nnz]`` (``v`` where ``q_self < contam_cutoff``), ``contaminated`` and ``total`` int64 per
    cell, ``percent_contamination`` float64 per cell and ``neighbor_frequencies`` float32 ``[n_cells, T]``.  The same bits
    from call to call.  Waits for the device no more than ``knn_grid`` does (once)."""
    if "centroid" not in expr:
        raise ValueError("calculate_contamination: expr holds no centroid -- call expression_matrix(..., xy=)")
    indptr, indices, counts, xy = expr["indptr"], expr["indices"], expr["counts"], expr["centroid"]
    L.need_device("calculate_contamination", indptr, indices, counts, xy, cell_type, weight, hint=_CPU_HINT)
    if weight.dim() != 2:
        raise ValueError("calculate_contamination: weight is [n_types, n_ref_genes]")
    dev = indptr.device
    T, G_ref = _n_types(weight.shape[0]), int(weight.shape[1])
    n, nnz = int(indptr.numel()) - 1, int(indices.numel())
    host = cell_type.detach().to(device=dev, dtype=torch.int32).contiguous().view(-1)
    if int(host.numel()) != n:
        raise ValueError("calculate_contamination: one cell type per row of expr")
    gmap = _gene_map(expr, gene_map, G_ref)
    freq, _ = neighbor_frequencies(xy, host, n_neighbors, T, max_neighbor_distance, True, knn)
    lik_t, back = _likelihood(weight, host, T, float(eps))
    out = contamination_posterior(indptr, indices, counts, gmap, host, freq, lik_t, back, T, alpha_self, alpha_neighbor,
                                  alpha_background, eps, contam_cutoff)
    out["neighbor_frequencies"] = freq
    return out


def contamination_flow(expr: Dict[str, Tensor], contamination: Tensor, cell_type: Tensor, weight: Tensor,
                       gene_map: Optional[Tensor] = None, n_host_types: Optional[int] = None) -> Tensor:
    """The reference's ``contamination_flow``: ``[D, H]`` float64, entry ``(d, h)`` the mean over the cells of host type
    ``h`` of the percentage of the cell's counts that are flagged and attributed to donor type ``d``.  ``contamination`` is
    the layer :func:`calculate_contamination` returns; ``weight`` ``[D, G_ref]``; a flagged count of gene g is split over
    the donors by ``W[g, :]`` = column g of ``weight`` normalised to sum 1 (a gene no donor expresses stays zero).  The
    per-cell percentages are ``sparse_project`` of the flagged counts with the row weight ``100 / max(libsize, 1)``; genes
    the table lacks are dropped, and ``ValueError`` is raised when none is shared (one wait).  Unlabelled cells belong to
    no host type.  ``n_host_types`` defaults to ``D``.  Float64 (the reference's ``W`` is float32), a fixed order."""
    indptr, indices, counts = expr["indptr"], expr["indices"], expr["counts"]
    L.need_device("contamination_flow", indptr, indices, counts, contamination, cell_type, weight, hint=_CPU_HINT)
    dev = indptr.device
    D, G_ref = int(weight.shape[0]), int(weight.shape[1])
    H = D if n_host_types is None else int(n_host_types)
    gmap = _gene_map(expr, gene_map, G_ref)
    if not bool((gmap >= 0).any()):
        raise ValueError("No shared genes between the count matrix and the reference table")
    W = weight.detach().double().T.contiguous()
    row_sum = W.sum(dim=1, keepdim=True)
    W = W / torch.where(row_sum == 0, torch.ones_like(row_sum), row_sum)
    libsize = csr_row_sums(indptr, counts)
    kept = gmap[indices.long()]                                        # -1 for a dropped gene: sparse_project skips it
    percent = sparse_project(indptr, kept, contamination, 100.0 / libsize.clamp_min(1).double(), W,
                             torch.zeros(D, dtype=torch.float64, device=dev), torch.float64)
    host = cell_type.to(device=dev, dtype=torch.int64).view(-1)
    known = (host >= 0) & (host < H)
    with deterministic_sums():
        sums = torch.zeros(H, D, dtype=torch.float64, device=dev).index_add_(0, host[known], percent[known])
    cells = torch.bincount(host[known], minlength=H).clamp_min(1).double()
    return (sums / cells[:, None]).T.contiguous()
