"""Boundary and gene features of a count matrix, on the device: the reference's ``setup_anndata``
(``src/segger/data/utils/anndata.py:184-259``) from the CSR that :func:`segger_amd.postprocess.expression_matrix` returns.

``expression_features`` gives the cell PCA (``X_pca``, what the reference stores as ``bd.x``), the gene embedding
(``X_corr``, the PCA of the gene-gene correlation matrix) and the intermediate numbers; ``cluster_cosine_similarity``
gives a cluster-similarity table the triplet loss samples from; ``anndata_features`` adds the phenograph clusters of the
cells and the genes (:mod:`segger_amd.phenograph`) and both tables (``anndata.py:261-291``).

Both the correlation matrix and the covariance the cell PCA needs are ONE ``G x G`` second-moment matrix of the weighted
sparse rows (``segger_sparse_gram``, float64 MFMA over row blocks densified in LDS); the cells are projected onto the
components by a CSR x dense product (``segger_sparse_project``).  Nothing dense of size ``n_cells x n_genes`` is ever
built.  Everything around the two kernels -- integer sums, the median, ``torch.linalg.eigh`` on ``G x G``, sign flips --
is torch on the device.  There is no CPU path.

The phenograph clustering (kNN -> Jaccard -> Louvain) is :mod:`segger_amd.phenograph`: cluster labels are computed on
the device, by a deterministic Louvain that is cuGraph's in objective, not in move order.  The morphology features of the
boundary polygons (``X_morphology``, the other ``cells_representation``) are :mod:`segger_amd.morphology`;
``anndata_features`` adds them when it is given the rings.  Not built: sklearn's randomized solver, which sklearn's ``auto`` policy picks when ``G > 500`` -- the exact PCA is computed for
every ``G``; cuML's own sign convention for ``X_pca`` -- sklearn's is used for both embeddings.  scanpy's
``normalize_total`` casts integer counts to float32 first; here the normalised values are float64 throughout.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L

__all__ = ["expression_features", "sparse_gram", "sparse_project", "cluster_cosine_similarity", "anndata_features"]


def _csr(indptr: Tensor, indices: Tensor, values: Tensor, row_weight: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, int, int]:
    L.need_device("sparse_gram / sparse_project", indptr, indices, values, row_weight)
    indptr = indptr.detach().to(torch.int64).contiguous().view(-1)
    indices = indices.detach().to(torch.int32).contiguous().view(-1)
    values = values.detach().to(torch.int32).contiguous().view(-1)
    row_weight = row_weight.detach().to(torch.float64).contiguous().view(-1)
    n_rows = int(indptr.numel()) - 1
    nnz = int(indices.numel())
    if n_rows < 0 or int(row_weight.numel()) != n_rows or int(values.numel()) != nnz:
        raise ValueError("sparse CSR: indptr has n_rows + 1 entries, row_weight n_rows, indices and values nnz")
    return indptr, indices, values, row_weight, n_rows, nnz


def csr_row_sums(indptr: Tensor, values: Tensor) -> Tensor:
    """exact int64 row sums of a CSR: differences of one running sum at the row pointers"""
    running = torch.zeros(int(values.numel()) + 1, dtype=torch.int64, device=values.device)
    torch.cumsum(values.long(), 0, out=running[1:])
    return running[indptr[1:]] - running[indptr[:-1]]


def sparse_gram(indptr: Tensor, indices: Tensor, values: Tensor, row_weight: Tensor, n_cols: int) -> Tuple[Tensor, Tensor]:
    """``S = sum_r w_r^2 x_r x_r^T`` ``[n_cols, n_cols]`` and ``s = sum_r w_r x_r`` ``[n_cols]``, float64, over the rows of
    a CSR matrix (``indices`` strictly ascending inside a row, integer ``values``); a row of weight 0 takes no part.
    ``S`` is bit-symmetric and both outputs have the same bits from call to call (``segger_sparse_gram``).  A
    gene-correlation reference matrix (``gene_corr_reference``) goes through the same call."""
    indptr, indices, values, row_weight, n_rows, nnz = _csr(indptr, indices, values, row_weight)
    dev = indptr.device
    n_cols = int(n_cols)
    ws, ws_bytes = L.workspace("segger_features_workspace_bytes", dev, n_rows, n_cols)   # never empty: one slab at least
    S = torch.empty(n_cols, n_cols, dtype=torch.float64, device=dev)
    s = torch.empty(n_cols, dtype=torch.float64, device=dev)
    L.call("segger_sparse_gram", dev, indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), row_weight.data_ptr(), n_rows,
           n_cols, nnz, S.data_ptr(), s.data_ptr(), ws.data_ptr(), ws_bytes)
    return S, s


def sparse_project(indptr: Tensor, indices: Tensor, values: Tensor, row_weight: Tensor, V: Tensor, offset: Tensor,
                   out_dtype: torch.dtype = torch.float32) -> Tensor:
    """``out[r, :] = w_r * sum_j x_rj V[j, :] - offset`` for every row of a CSR matrix: ``V`` ``[n_cols, k]`` and ``offset``
    ``[k]`` float64, ``1 <= k <= 256``, ``out`` float32 or float64.  Accumulated in float64 in CSR order and rounded once;
    a row of weight 0 gives exactly ``-offset`` (``segger_sparse_project``)."""
    indptr, indices, values, row_weight, n_rows, nnz = _csr(indptr, indices, values, row_weight)
    L.need_device("sparse_project", V, offset)
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError("sparse_project: out_dtype is torch.float32 or torch.float64")
    if V.dim() != 2 or offset.numel() != V.shape[1]:
        raise ValueError("sparse_project: V is [n_cols, k] and offset [k]")
    dev = indptr.device
    V = V.detach().to(torch.float64).contiguous()
    offset = offset.detach().to(torch.float64).contiguous().view(-1)
    n_cols, k = int(V.shape[0]), int(V.shape[1])
    out = torch.empty(n_rows, k, dtype=out_dtype, device=dev)
    L.call("segger_sparse_project", dev, indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), row_weight.data_ptr(),
           n_rows, n_cols, nnz, V.data_ptr(), offset.data_ptr(), k, out.data_ptr(), int(out_dtype == torch.float64))
    return out


def _flip_signs(V: Tensor) -> Tensor:
    """sklearn's ``svd_flip(u_based_decision=False)`` on components stored as COLUMNS: the largest-magnitude loading of
    each component becomes positive (the first one on a tie, as ``argmax`` picks)."""
    top = V.abs().argmax(dim=0)
    sign = torch.sign(V[top, torch.arange(V.shape[1], device=V.device)])
    return V * torch.where(sign == 0, torch.ones_like(sign), sign)


def _top_eigenvectors(M: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """the ``k`` largest eigenpairs of a symmetric matrix, descending, signs fixed by :func:`_flip_signs`"""
    evals, evecs = torch.linalg.eigh(M)
    return evals.flip(0)[:k].contiguous(), _flip_signs(evecs.flip(1)[:, :k]).contiguous()


def expression_features(expr: Dict[str, Tensor], embedding_size: int = 128, cells_min_counts: int = 10,
                        genes_min_counts: int = 100, out_dtype: torch.dtype = torch.float32) -> Dict[str, Tensor]:
    """``setup_anndata``'s numbers from ``expr``, the dict :func:`~segger_amd.postprocess.expression_matrix` returns.

    Step by step as the reference: gene totals (exact int64), genes with ``>= genes_min_counts`` are kept; ``n_counts``
    = each cell's sum over the kept genes; ``filtered = n_counts >= cells_min_counts``; ``target_sum`` = numpy's median
    of ``n_counts`` over the filtered cells; ``normalize_total`` as the row weight ``target_sum / n_counts`` (0 for an
    empty cell); the Gram of the FILTERED rows; ``cov = (S - s s^T / n) / (n - 1)``; ``corr`` as ``np.corrcoef`` (clipped
    to [-1, 1]) then ``nan_to_num`` (NaN -> 0, +-inf -> 1); ``X_corr`` = the exact PCA scores ``U Sigma`` of ``corr``
    (columns centred, top ``embedding_size``); ``X_pca`` = ``(norm - mean) V`` of ALL cells, ``V`` the top eigenvectors
    of ``cov``.  Both embeddings carry sklearn's signs (``svd_flip(u_based_decision=False)``).

    Returns device tensors: ``X_pca`` ``[n_cells_present, k]`` ``out_dtype``, ``X_corr`` ``[n_genes_kept, k]`` float64,
    ``corr`` ``[n_genes_kept, n_genes_kept]`` float64, ``gene_keep`` bool over ``expr["gene_ids"]``, ``n_counts`` int64,
    ``filtered`` bool, ``target_sum`` float64 scalar, ``explained_variance`` ``[k]`` (of the cell PCA) and
    ``corr_explained_variance`` ``[k]``.  Raises ``ValueError`` when ``embedding_size > min(n_genes_kept, n_filtered)``,
    where sklearn's exact solver refuses.  Waits for the device once (the two counts)."""
    indptr, indices, counts = expr["indptr"], expr["indices"], expr["counts"]
    L.need_device("expression_features", indptr, indices, counts, hint="tests/features_cases.py holds the CPU oracle")
    dev = indptr.device
    k = int(embedding_size)
    n_cells, n_genes = int(indptr.numel()) - 1, int(expr["gene_ids"].numel())
    cols = indices.long()
    gene_total = torch.zeros(n_genes, dtype=torch.int64, device=dev).index_add_(0, cols, counts.long())
    gene_keep = gene_total >= int(genes_min_counts)
    n_counts = csr_row_sums(indptr, counts.long() * gene_keep[cols])       # over the kept genes
    filtered = n_counts >= int(cells_min_counts)
    n_kept_genes, n_filtered = torch.stack([gene_keep.sum(), filtered.sum()]).tolist()          # the one wait
    if k < 1 or k > min(n_kept_genes, n_filtered):
        raise ValueError(f"expression_features: embedding_size={k} must be between 1 and min(n_samples, n_features)="
                         f"{min(n_kept_genes, n_filtered)} with svd_solver='full' ({n_filtered} filtered cells, "
                         f"{n_kept_genes} kept genes)")
    ordered = n_counts[filtered].sort().values                        # numpy's median: the mean of the two middle values
    target_sum = (ordered[(n_filtered - 1) // 2] + ordered[n_filtered // 2]).double() / 2.0
    weight = torch.where(n_counts > 0, target_sum / n_counts.double(), torch.zeros((), dtype=torch.float64, device=dev))
    # dropped genes stay columns of the kernels' matrix and leave through the sub-selection of S, s and the rows of V
    S, s = sparse_gram(indptr, indices, counts, torch.where(filtered, weight, torch.zeros_like(weight)), n_genes)
    S, s = S[gene_keep][:, gene_keep], s[gene_keep]
    n = float(n_filtered)
    mean = s / n
    cov = (S - torch.outer(s, s) / n) / (n - 1.0)
    std = cov.diagonal().sqrt()
    corr = (cov / std[:, None] / std[None, :]).clamp(-1.0, 1.0)      # a 0 / 0 is NaN and stays NaN through the clamp
    corr = torch.nan_to_num(corr, nan=0.0, posinf=1.0, neginf=1.0)
    centred = corr - corr.mean(dim=0, keepdim=True)
    ev_corr, v_corr = _top_eigenvectors(centred.T @ centred, k)
    X_corr = centred @ v_corr
    ev_cov, v_cov = _top_eigenvectors(cov, k)
    v_full = torch.zeros(n_genes, k, dtype=torch.float64, device=dev)
    v_full[gene_keep] = v_cov
    X_pca = sparse_project(indptr, indices, counts, weight, v_full, mean @ v_cov, out_dtype)
    return {"X_pca": X_pca, "X_corr": X_corr, "corr": corr, "gene_keep": gene_keep, "n_counts": n_counts, "filtered": filtered,
            "target_sum": target_sum, "explained_variance": ev_cov,
            "corr_explained_variance": ev_corr.clamp_min(0.0) / max(n_kept_genes - 1, 1)}


def cluster_cosine_similarity(embedding: Tensor, clusters: Tensor) -> Tensor:
    """The reference's ``get_cluster_cosine_similarity``: L2-normalise every row (``eps = 1e-8``), average per cluster,
    ``means @ means.T``.  Rows and columns follow the ascending cluster labels (-1, the label of a removed cell, is a
    cluster like any other, as in the reference).  Plain torch on the embedding's device; no kernel."""
    unique, inverse = clusters.unique(sorted=True, return_inverse=True)
    n = unique.numel()
    sums = torch.zeros(n, embedding.size(1), dtype=embedding.dtype, device=embedding.device)
    sums.index_add_(0, inverse, torch.nn.functional.normalize(embedding, p=2, dim=1, eps=1e-8))
    means = sums / torch.bincount(inverse, minlength=n).unsqueeze(1)
    return means @ means.T


@contextlib.contextmanager
def deterministic_sums():
    """torch's deterministic algorithms for the block: ``cluster_cosine_similarity`` sums rows with ``index_add_``, whose
    default route on the device is floating-point atomics -- the same table to the last bit needs the ordered route."""
    enabled, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(enabled, warn_only=warn_only)


def anndata_features(expr: Dict[str, Tensor], embedding_size: int = 128, cells_min_counts: int = 10, genes_min_counts: int = 100,
                     cells_clusters_n_neighbors: int = 10, cells_clusters_resolution: float = 2.0,
                     genes_clusters_n_neighbors: int = 5, genes_clusters_resolution: float = 2.0,
                     out_dtype: torch.dtype = torch.float32,
                     boundaries: Optional[Tuple[Tensor, Tensor]] = None) -> Dict[str, Tensor]:
    """Everything :func:`expression_features` returns plus the reference's clusters (``anndata.py:261-291``, the defaults
    of ``data_module.py:138-144``): ``cell_clusters`` int64 over the cells -- the phenograph of ``X_pca`` of the FILTERED
    cells with ``min_size=100``, -1 for a removed cell; ``gene_clusters`` int64 over the kept genes -- the phenograph of
    ``X_corr`` with ``min_size=-1``; ``cell_cluster_similarities`` and ``gene_cluster_similarities`` from
    :func:`cluster_cosine_similarity` (-1 is a cluster like any other there, as in the reference), summed in a fixed order
    (:func:`deterministic_sums`): the whole result has the same bits from call to call.

    ``boundaries = (ring_offsets, xy)``, the polygons of the ``expr`` cells in the order of its rows, adds ``X_morphology``
    ``[n_cells_present, 4]`` ``out_dtype`` (:func:`segger_amd.morphology.morphology_features`, the reference's
    ``anndata.py:296-311``); without it the result is what it was, key for key."""
    from .phenograph import phenograph
    out = expression_features(expr, embedding_size, cells_min_counts, genes_min_counts, out_dtype)
    filtered, X_pca, X_corr = out["filtered"], out["X_pca"], out["X_corr"]
    cell_clusters = torch.full((int(filtered.numel()),), -1, dtype=torch.int64, device=filtered.device)
    cell_clusters[filtered] = phenograph(X_pca[filtered], cells_clusters_n_neighbors, cells_clusters_resolution, min_size=100)
    out["cell_clusters"] = cell_clusters
    out["gene_clusters"] = phenograph(X_corr, genes_clusters_n_neighbors, genes_clusters_resolution, min_size=-1)
    with deterministic_sums():                                        # the same tables from call to call
        out["cell_cluster_similarities"] = cluster_cosine_similarity(X_pca, cell_clusters)
        out["gene_cluster_similarities"] = cluster_cosine_similarity(X_corr, out["gene_clusters"])
    if boundaries is not None:
        from .morphology import morphology_features
        X_morphology = morphology_features(boundaries[0], boundaries[1], out_dtype)
        if int(X_morphology.shape[0]) != int(filtered.numel()):
            raise ValueError(f"anndata_features: {int(X_morphology.shape[0])} boundary rings for {int(filtered.numel())} cells")
        out["X_morphology"] = X_morphology
    return out
