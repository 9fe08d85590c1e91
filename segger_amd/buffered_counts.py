"""Buffered-boundary count matrices on the device: the reference's ``src/segger/metrics/segment.py`` --
``get_buffered_counts`` -> ``buffer_polygons`` -> ``get_expression_matrix`` (the polygon x gene count matrix of boundaries
grown by a distance: the NUCLEUS-EXPANSION BASELINE every segger segmentation is compared against), ``filter_boundaries``
(the rule that keeps a boundary in exactly one region of a tiled slide) and ``get_buffered_counts_distributed`` (the sum
over regions).  The reference computes the matrix with three cuSpatial calls that do not exist on ROCm; this is
``segger_buffered_counts_count`` / ``segger_buffered_counts_fill`` (csrc/buffered_counts.hip; include/segger_amd.h has the
contract): the polygon join and the gene histogram fused, one wave per polygon, no pair list.  There is no CPU path.

The predicate is :func:`segger_amd.geometry.points_in_polygons`' bit for bit (both kernels compile
csrc/ring_predicate.h); that module's docstring defines it and says how the exact offset differs from GEOS's polyline
buffer.  A transcript inside several grown polygons is counted in each ("transcripts can be doubly-counted", as the
reference notes).

NOT BUILT: parquet reading, the ``qv`` filter, the gene-panel reordering, dask, and the reference's ``row_ind - 1`` id
arithmetic (rows here are the polygons in the order given); panels above ``SEGGER_BCOUNT_MAX_GENES`` genes (a key-sort
route); a histogram sized by ``n_genes`` instead of by its tier's cap (dynamic LDS, or a tier between 2048 and the cap):
every panel above 2048 genes runs one wave a workgroup today, which is why such panels are slower than the composition.  UNPINNED: cuSpatial, cudf, shapely and GEOS cannot be run where this was written, so the reference module was
never executed; what IS checked is equality with the CPU oracle of tests/buffered_count_cases.py, which asks the join's
float64 and exact-rational predicate oracles.  The reference's ``filter_boundaries`` runs on cudf only; its arithmetic is
restated here, never compared with a run.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Union

import torch
from torch import Tensor

from . import _lib as L
from .geometry import join_inputs
from .rings import raise_ring_errors, ring_csr

__all__ = ["COUNTER_NAMES", "buffered_counts", "buffered_counts_to_scipy", "filter_boundaries", "buffered_counts_regions"]

COUNTER_NAMES = ("n_pairs", "nnz", "n_bad", "n_overflow_rows", "n_large_tier")


def _check_genes(who: str, points: Tensor, gene: Tensor, n_genes: int) -> int:
    if isinstance(n_genes, bool) or not isinstance(n_genes, int) or n_genes < 1:
        raise ValueError(f"{who}: n_genes is a positive int")
    if n_genes > L.BCOUNT_MAX_GENES:
        raise ValueError(f"{who}: n_genes = {n_genes} is above SEGGER_BCOUNT_MAX_GENES = {L.BCOUNT_MAX_GENES} (the histogram of a "
                         f"polygon lives in LDS; a key-sort route for larger panels is not built)")
    if (not isinstance(gene, Tensor) or gene.dim() != 1 or gene.is_floating_point() or gene.is_complex() or gene.dtype == torch.bool
            or not isinstance(points, Tensor) or points.dim() != 2 or gene.numel() != points.shape[0]):
        raise ValueError(f"{who}: gene is an integer [n_points] tensor")
    if gene.device != points.device:
        raise ValueError(f"{who}: gene and points are on different devices")
    return n_genes


def _gene_codes(gene: Tensor, n_genes: int) -> Tensor:
    """``gene`` of any integer dtype as the int32 the kernel reads: everything outside ``[0, n_genes)`` becomes -1.  Widened
    to int64 BEFORE the comparison: in a narrow dtype ``n_genes`` and the -1 themselves would wrap (int8 turns 500 into -12,
    uint8 turns -1 into 255)."""
    g = gene.detach().to(torch.int64)
    return torch.where((g < 0) | (g >= n_genes), torch.full_like(g, -1), g).to(torch.int32).contiguous()


def _empty_result(n_polygons: int, n_genes: int, device) -> Dict[str, Tensor]:
    i32 = dict(dtype=torch.int32, device=device)
    return {"indptr": torch.zeros(n_polygons + 1, dtype=torch.int64, device=device), "indices": torch.empty(0, **i32),
            "counts": torch.empty(0, **i32), "cell_count": torch.zeros(n_polygons, dtype=torch.int64, device=device),
            "counters": torch.zeros(len(COUNTER_NAMES), dtype=torch.int64, device=device),
            "cell_ids": torch.arange(n_polygons, **i32), "gene_ids": torch.arange(n_genes, **i32)}


def buffered_counts(points: Tensor, gene: Tensor, ring_offsets: Tensor, xy: Tensor, n_genes: int,
                    buffer: Union[None, float, Tensor] = None, predicate: str = "contains",
                    points_per_cell: float = 2.0) -> Dict[str, Tensor]:
    """The polygon x gene count matrix of the polygons grown by ``buffer``: entry ``(p, g)`` is the number of points of
    gene ``g`` in polygon ``p`` grown by its distance.

    ``points`` ``[N, 2]``, ``ring_offsets`` ``[P + 1]``, ``xy`` ``[V, 2]``, ``buffer`` (``None``, a float, a ``[P]`` tensor),
    ``predicate`` and ``points_per_cell`` are :func:`segger_amd.geometry.points_in_polygons`'; the checks and their messages
    are that function's.  ``gene`` is an integer ``[N]`` tensor of any integer dtype; ``n_genes`` is the panel size,
    ``1 .. SEGGER_BCOUNT_MAX_GENES`` (24064; above it ``ValueError`` names the cap).

    Returns a dict of device tensors, the same bytes from call to call, for any ``points_per_cell`` and any order of the
    points:

    * ``indptr`` int64 ``[P + 1]``: one row per polygon, in the order given; a polygon without hits has an empty row;
    * ``indices`` int32 ``[nnz]``: the gene id, strictly ascending inside a row;  ``counts`` int32 ``[nnz]``;
    * ``cell_count`` int64 ``[P]``: the sum of the row;
    * ``counters`` int64, named by ``COUNTER_NAMES``: ``n_pairs`` (matched (point, polygon) pairs), ``nnz``, ``n_bad``
      (matched pairs whose gene lies outside ``[0, n_genes)``: counted here and nowhere else, never an index),
      ``n_overflow_rows`` (polygons with more than ``SEGGER_BCOUNT_TOUCHED`` distinct genes: the ordered-scan path),
      ``n_large_tier`` (polygons that ran with the whole-LDS histogram: ``n_genes > SEGGER_BCOUNT_SMALL_GENES``);
    * ``cell_ids`` and ``gene_ids`` int32, ``arange(P)`` and ``arange(n_genes)``: with them the dict is what
      :func:`segger_amd.features.expression_features` and :func:`segger_amd.validation.calculate_contamination` take from
      :func:`segger_amd.postprocess.expression_matrix` (the latter also wants a ``centroid`` ``[P, 2]``, the caller's).

    Empty points or polygons return the all-empty CSR (``indptr`` zeros) and launch nothing; CPU tensors raise
    ``SeggerAmdError``.  Waits for the device four times: the longest ring (the shared ring validation), the extent of the
    points and the rings with the finiteness checks, ``nnz``, and the error word."""
    who = "buffered_counts"
    n_genes = _check_genes(who, points, gene, n_genes)
    j = join_inputs(who, points, ring_offsets, xy, buffer, predicate, points_per_cell, others=(gene,),
                    hint="tests/buffered_count_cases.py holds the CPU oracle")
    dev = xy.device
    if j is None:
        return _empty_result(int(ring_offsets.numel()) - 1, n_genes, dev)
    pts, ring_offsets, xy, buf, n_points, n_polygons, n_vertices = j[:7]
    g = _gene_codes(gene, n_genes)
    ws, ws_bytes = L.workspace("segger_buffered_counts_workspace_bytes", dev, n_points, n_polygons, n_genes, j.grid[3], j.grid[4])
    indptr = torch.empty(n_polygons + 1, dtype=torch.int64, device=dev)
    cell_count = torch.empty(n_polygons, dtype=torch.int64, device=dev)
    counters = torch.empty(len(COUNTER_NAMES), dtype=torch.int64, device=dev)
    head = (pts.data_ptr(), n_points, g.data_ptr(), n_genes, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices,
            L.ptr(buf), j.predicate, *j.grid, indptr.data_ptr())
    L.call("segger_buffered_counts_count", dev, *head, cell_count.data_ptr(), counters.data_ptr(), ws.data_ptr(), ws_bytes)
    nnz = int(indptr[-1])                                            # the third wait
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    counts = torch.empty(nnz, dtype=torch.int32, device=dev)
    if nnz > 0:
        L.call("segger_buffered_counts_fill", dev, *head, cell_count.data_ptr(), indices.data_ptr(), counts.data_ptr(), nnz,
               ws.data_ptr(), ws_bytes)
    raise_ring_errors(who, int(ws[:4].view(torch.int32)), ring_offsets, n_vertices)          # the fourth
    i32 = dict(dtype=torch.int32, device=dev)
    return {"indptr": indptr, "indices": indices, "counts": counts, "cell_count": cell_count, "counters": counters,
            "cell_ids": torch.arange(n_polygons, **i32), "gene_ids": torch.arange(n_genes, **i32)}


def buffered_counts_to_scipy(result: Dict[str, Tensor], n_genes: int):
    """``scipy.sparse.csr_matrix`` ``[P, n_genes]`` of dtype uint32 -- the reference's ``get_expression_matrix`` dtype --
    from what :func:`buffered_counts` returns (canonical: sorted indices, no duplicates)."""
    import numpy as np
    import scipy.sparse as sp
    indptr = result["indptr"].cpu().numpy()
    return sp.csr_matrix((result["counts"].cpu().numpy().astype(np.uint32), result["indices"].cpu().numpy(), indptr),
                         shape=(indptr.size - 1, int(n_genes)))


def _box(who: str, name: str, box) -> tuple:
    vals = tuple(float(v) for v in (box.tolist() if isinstance(box, Tensor) else box))
    if len(vals) != 4 or not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{who}: {name} is four finite numbers")
    return vals


def filter_boundaries(ring_offsets: Tensor, xy: Tensor, inset: Sequence[float], outset: Sequence[float]) -> Tensor:
    """The reference's ``filter_boundaries`` (``src/segger/metrics/segment.py:125-156``): a bool ``[P]`` keep-mask that
    puts every boundary of a tiled slide into exactly one region.  ``inset = (x2, y2, x3, y3)`` is the region,
    ``outset = (x1, y1, x4, y4)`` the region grown by the overlap; every test is inclusive on both ends (``between``).
    Per ring, over ALL its stored vertices (a closing duplicate included, as the reference's vertex table has it):

    * ``center``: vertices in the inset box;  ``top``: ``x in [x1, x4], y in [y1, y2]``;  ``left``: ``x in [x1, x2],
      y in [y1, y4]``;  ``right``: ``x in [x3, x4], y in [y1, y4]``;  ``bottom``: ``x in [x1, x4], y in [y3, y4]``;
    * ``keep = (center == total) | (center > 0 & left > 0 & bottom == 0) | (center > 0 & top > 0 & right == 0)``.

    The reference's names do not match the y direction -- its "top" strip is the one at the LOW y end -- and its
    arithmetic is kept as it is: the rule is symmetric in what it needs (a ring straddling two regions is kept by one of
    them), whatever the strips are called.  Plain torch on the device: five segmented sums, no kernel.  A ring without
    vertices has ``center == total == 0`` and is kept, as in the reference.  Waits for the device twice (the longest ring in
    the shared ring validation, the offsets).  UNPINNED: the reference runs on cudf only."""
    who = "filter_boundaries"
    ring_offsets, xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    x2, y2, x3, y3 = _box(who, "inset", inset)
    x1, y1, x4, y4 = _box(who, "outset", outset)
    L.need_device(who, ring_offsets, xy, hint="tests/buffered_count_cases.py holds the numpy restatement")
    dev = xy.device
    if n_polygons == 0:
        return torch.zeros(0, dtype=torch.bool, device=dev)
    _check_offsets(who, ring_offsets, n_vertices)                    # the second wait (the first: the longest ring)
    return _keep_mask(ring_offsets, xy, (x2, y2, x3, y3), (x1, y1, x4, y4))


def _check_offsets(who: str, ring_offsets: Tensor, n_vertices: int) -> None:
    if bool(((ring_offsets < 0) | (ring_offsets > n_vertices)).any() | (ring_offsets[1:] < ring_offsets[:-1]).any()):      # one wait
        raise ValueError(f"{who}: ring_offsets are negative, descending or beyond the {n_vertices} vertices")


def _keep_mask(ring_offsets: Tensor, xy: Tensor, inset: tuple, outset: tuple) -> Tensor:
    """:func:`filter_boundaries` on a validated CSR: enqueues only, never waits for the device"""
    x2, y2, x3, y3 = inset
    x1, y1, x4, y4 = outset
    dev, n_vertices = xy.device, int(xy.shape[0])
    x, y = xy[:, 0], xy[:, 1]

    def between(v, lo, hi):
        return (v >= lo) & (v <= hi)

    in_x, in_y = between(x, x1, x4), between(y, y1, y4)
    flags = torch.stack([between(x, x2, x3) & between(y, y2, y3), in_x & between(y, y1, y2), between(x, x1, x2) & in_y,
                         between(x, x3, x4) & in_y, in_x & between(y, y3, y4)], dim=1).to(torch.int64)
    sums = torch.zeros(n_vertices + 1, 5, dtype=torch.int64, device=dev)
    torch.cumsum(flags, 0, out=sums[1:])
    per_ring = sums[ring_offsets[1:]] - sums[ring_offsets[:-1]]
    center, top, left, right, bottom = per_ring.unbind(1)
    total = ring_offsets[1:] - ring_offsets[:-1]
    return (center == total) | ((center > 0) & (left > 0) & (bottom == 0)) | ((center > 0) & (top > 0) & (right == 0))


def buffered_counts_regions(points: Tensor, gene: Tensor, ring_offsets: Tensor, xy: Tensor, n_genes: int, regions,
                            buffer: Union[None, float, Tensor] = None, overlap: float = 100.0, predicate: str = "contains",
                            points_per_cell: float = 2.0) -> Dict[str, Tensor]:
    """``get_buffered_counts`` summed over regions, as the reference's ``get_buffered_counts_distributed`` does.
    ``regions`` is ``[R, 4]`` of ``(xmin, ymin, xmax, ymax)``.  For each region: the points STRICTLY inside the region grown
    by ``overlap`` (the reference filters with ``>`` and ``<``), the polygons :func:`filter_boundaries` keeps for
    ``(region, grown region)``, :func:`buffered_counts` on those, the rows mapped back to the given polygon ids; the
    results are added into one CSR of ``P`` rows (plain torch on ``row * n_genes + gene`` keys, a stable sort only).

    Returns ``indptr``, ``indices``, ``counts``, ``cell_count``, ``counters`` (summed over the regions), ``cell_ids`` and
    ``gene_ids`` as :func:`buffered_counts`, and ``kept`` int64 ``[P]``: in how many regions a polygon was kept (1 on a
    tiling whose overlap exceeds the largest boundary).  Waits for the device three times up front (the longest ring, the
    offsets, the buffer's range when it is a tensor), then per region seven times -- the kept polygons, the selected points,
    the vertices of the kept rings, and :func:`buffered_counts`' own four -- and once at the end (the number of distinct
    keys).  NOT BUILT: parquet reading, the ``qv`` filter, the gene-panel
    reordering, dask and the ``row_ind - 1`` id arithmetic of the reference."""
    who = "buffered_counts_regions"
    n_genes = _check_genes(who, points, gene, n_genes)
    offs, ring_xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    regions = torch.as_tensor(regions, dtype=torch.float64).reshape(-1, 4).cpu()
    if not (float(overlap) >= 0.0 and math.isfinite(float(overlap))) or not bool(regions.isfinite().all()):
        raise ValueError(f"{who}: overlap must be finite and >= 0 and regions finite")
    if isinstance(buffer, Tensor) and (buffer.dim() != 1 or buffer.numel() != n_polygons or not buffer.is_floating_point()):
        raise ValueError(f"{who}: buffer is None, a float or a floating-point [n_polygons] tensor")
    L.need_device(who, points, gene, offs, ring_xy, buffer if isinstance(buffer, Tensor) else None,
                  hint="tests/buffered_count_cases.py holds the CPU oracle")
    dev = ring_xy.device
    if n_polygons:
        _check_offsets(who, offs, n_vertices)
    if isinstance(buffer, Tensor) and n_polygons and not bool(((buffer >= 0) & buffer.isfinite()).all()):
        raise ValueError(f"{who}: buffer must be finite and >= 0")
    ov = float(overlap)
    lengths = offs[1:] - offs[:-1]
    keys, vals = [], []
    cell_count = torch.zeros(n_polygons, dtype=torch.int64, device=dev)
    counters = torch.zeros(len(COUNTER_NAMES), dtype=torch.int64, device=dev)
    kept = torch.zeros(n_polygons, dtype=torch.int64, device=dev)
    for xmin, ymin, xmax, ymax in regions.tolist():
        outset = (xmin - ov, ymin - ov, xmax + ov, ymax + ov)
        keep = _keep_mask(offs, ring_xy, (xmin, ymin, xmax, ymax), outset)
        rows = keep.nonzero().view(-1)
        kept += keep
        inside = (points[:, 0] > outset[0]) & (points[:, 0] < outset[2]) & (points[:, 1] > outset[1]) & (points[:, 1] < outset[3])
        sel = inside.nonzero().view(-1)
        if rows.numel() == 0 or sel.numel() == 0:
            continue
        sub_len = lengths[rows]
        sub_off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(sub_len, 0, out=sub_off[1:])
        n_sub = int(sub_off[-1])
        vert = torch.repeat_interleave(offs[rows] - sub_off[:-1], sub_len, output_size=n_sub) + torch.arange(n_sub, device=dev)
        r = buffered_counts(points[sel], gene[sel], sub_off, ring_xy[vert], n_genes,
                            buffer[rows] if isinstance(buffer, Tensor) else buffer, predicate, points_per_cell)
        row_of = torch.repeat_interleave(rows, r["indptr"][1:] - r["indptr"][:-1], output_size=int(r["indices"].numel()))
        keys.append(row_of * n_genes + r["indices"].long())
        vals.append(r["counts"].long())
        cell_count[rows] += r["cell_count"]
        counters += r["counters"]
    out = _empty_result(n_polygons, n_genes, dev)
    out["kept"] = kept
    if keys:
        key, order = torch.sort(torch.cat(keys), stable=True)
        uniq, inverse = torch.unique_consecutive(key, return_inverse=True)
        summed = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).index_add_(0, inverse, torch.cat(vals)[order])
        row = torch.div(uniq, n_genes, rounding_mode="floor")
        out["indptr"][1:] = torch.cumsum(torch.bincount(row, minlength=n_polygons), 0)
        out["indices"] = (uniq - row * n_genes).to(torch.int32)
        out["counts"] = summed.to(torch.int32)
        counters[COUNTER_NAMES.index("nnz")] = uniq.numel()
    out["cell_count"], out["counters"] = cell_count, counters
    return out
