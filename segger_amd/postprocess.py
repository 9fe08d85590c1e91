"""What consumes the ``predict_step`` 4-tuples: the final transcript -> cell table.

Restates ``ISTSegmentationWriter.assign_transcripts_to_cells`` (reference ``src/segger/data/writer.py:131-259``)
as segmented tensor operations that run wherever the tensors live (on the MI355X for a 100 M-transcript slide:
two stable sorts, one 2-D histogram, one vectorised fixed-point iteration -- no per-gene Python loop, no polars;
:func:`gene_thresholds` is the same threshold step as HIP kernels over one keys-only sort, ``thresholds="kernel"``):

* best row per transcript over overlapping prediction tiles (``:186-190``: sort by row_index, similarity
  descending, keep the first);
* per-gene similarity threshold over ASSIGNED transcripts = ``min(threshold_yen, threshold_li)`` (``:196-235``):
  Yen's maximum-correlation criterion on a 256-bin histogram and Li's iterative minimum cross entropy (the
  algorithms of scikit-image 0.26 the reference calls; ``threshold_li_custom``, ``data/utils/threshold.py:3-11``,
  gives up after 250 callbacks), all genes at once;
* genes whose Li iteration does not converge take the median of the converged thresholds (``:238-241``).

Differences from the reference, both documented in oracle/postprocess_oracle.py: no 10 M-value subsampling of
large genes (every value is used), and similarity ties in the dedup go to the first row of the concatenation.

:class:`SegmentationAccumulator` is the streaming form of the first step: it keeps the best row per transcript on
the device while the batches arrive (``csrc/assign.hip``: one 64-bit atomic max per row, no sort), so a slide's
prediction rows never have to exist at once.

:func:`expression_matrix` is the second artefact of ``segger segment``, ``segger_anndata.h5ad`` (``writer.py:91-129``,
``data/utils/anndata.py:18-102``): the cell x gene counts of the segmented transcripts in canonical CSR, the per-pair mean
similarity and the per-cell mean position, built on the device (``csrc/expression.hip``); :func:`expression_to_scipy`
hands it to scipy / AnnData.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

N_BINS = 256


def best_assignment(predictions: Sequence[Sequence[Tensor]], device=None) -> Dict[str, Tensor]:
    """Concatenate ``(tx_index, seg_idx, max_sim, gene_id)`` tuples and keep, per ``tx_index``, the row of
    highest similarity.  Rows come back sorted by ``row_index``."""
    if len(predictions) == 0:
        raise ValueError("no predictions")
    dev = torch.device(device) if device is not None else predictions[0][0].device
    idx = torch.cat([p[0].to(dev) for p in predictions]).long()
    seg = torch.cat([p[1].to(dev) for p in predictions]).long()
    sim = torch.cat([p[2].to(dev) for p in predictions]).float()
    gene = torch.cat([p[3].to(dev) for p in predictions]).long()
    o1 = torch.sort(sim, descending=True, stable=True).indices
    o2 = torch.sort(idx[o1], stable=True).indices
    order = o1[o2]
    si = idx[order]
    first = torch.ones_like(si, dtype=torch.bool)
    first[1:] = si[1:] != si[:-1]
    keep = order[first]
    return {"row_index": idx[keep], "cell_encoding": seg[keep], "similarity": sim[keep], "gene": gene[keep]}


def _edges(i: Tensor, lo: Tensor, hi: Tensor, step: Tensor) -> Tensor:
    """numpy.linspace(lo, hi, N_BINS + 1)[i]: lo + i * step, with the last edge pinned to hi."""
    return torch.where(i == N_BINS, hi, lo + i.double() * step)


def per_gene_thresholds(similarity: Tensor, gene: Tensor, assigned: Tensor, max_iter: int = 250):
    """-> (genes [G] sorted, threshold [G] f64, converged [G] bool, global_threshold float)."""
    v = similarity[assigned].double()
    genes, inv, counts = torch.unique(gene[assigned], return_inverse=True, return_counts=True)
    ng = int(genes.numel())
    dev = v.device
    if ng == 0:
        return genes, v.new_zeros(0), torch.zeros(0, dtype=torch.bool, device=dev), float("nan")
    o1 = torch.sort(v, stable=True).indices
    o2 = torch.sort(inv[o1], stable=True).indices
    order = o1[o2]
    vs, gs = v[order], inv[order]                          # grouped by gene, ascending inside a gene
    ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    beg, end = ptr[:-1], ptr[1:]
    vmin, vmax = vs[beg], vs[end - 1]
    flat = vmin == vmax

    # ---- Yen: 256-bin histogram over [min, max] per gene (numpy.histogram's uniform-bin indexing) ---------
    lo = torch.where(flat, vmin - 0.5, vmin)
    hi = torch.where(flat, vmax + 0.5, vmax)
    step = (hi - lo) / N_BINS
    glo, ghi, gstep = lo[gs], hi[gs], step[gs]
    ind = (((vs - glo) / (ghi - glo)) * N_BINS).long()
    ind = torch.where(ind == N_BINS, ind - 1, ind)
    ind = ind - (vs < _edges(ind, glo, ghi, gstep)).long()
    ind = ind + ((vs >= _edges(ind + 1, glo, ghi, gstep)) & (ind != N_BINS - 1)).long()
    hist = torch.bincount(gs * N_BINS + ind, minlength=ng * N_BINS).view(ng, N_BINS).double()
    pmf = hist / hist.sum(1, keepdim=True)
    p1 = pmf.cumsum(1)
    p1_sq = (pmf * pmf).cumsum(1)
    p2_sq = (pmf * pmf).flip(1).cumsum(1).flip(1)
    crit = torch.log((p1_sq[:, :-1] * p2_sq[:, 1:]).reciprocal() * (p1[:, :-1] * (1.0 - p1[:, :-1])) ** 2)
    crit = torch.where(torch.isnan(crit), torch.full_like(crit, float("inf")), crit)     # numpy.argmax: nan wins
    k = crit.argmax(1)
    yen = (_edges(k, lo, hi, step) + _edges(k + 1, lo, hi, step)) / 2.0

    # ---- Li: t <- (mean_back - mean_fore) / (log mean_back - log mean_fore) on values shifted to min 0 -----
    a = vs - vmin[gs]
    d = a[1:] - a[:-1]
    ok = (gs[1:] == gs[:-1]) & (d > 0)
    gap = torch.full((ng,), float("inf"), dtype=torch.float64, device=dev)
    gap = gap.scatter_reduce(0, gs[1:][ok], d[ok], reduce="amin", include_self=True)
    tol = gap / 2.0
    cs = torch.cat([a.new_zeros(1), a.cumsum(0)])
    n_all = counts.double()
    t_next = (cs[end] - cs[beg]) / n_all
    t_curr = -2.0 * tol
    key = gs.double() * 4.0 + a                           # a in [0, 2]: one ascending key over all genes
    base = torch.arange(ng, device=dev, dtype=torch.float64) * 4.0
    calls = torch.ones(ng, dtype=torch.long, device=dev)
    failed = torch.zeros(ng, dtype=torch.bool, device=dev)
    active = ~flat & ((t_next - t_curr).abs() > tol)
    for _ in range(max_iter):
        if not bool(active.any()):
            break
        t_curr = torch.where(active, t_next, t_curr)
        pos = torch.searchsorted(key, base + t_curr, right=True)
        pos = torch.minimum(torch.maximum(pos, beg), end)
        n_back = (pos - beg).double()
        mean_back = (cs[pos] - cs[beg]) / n_back
        mean_fore = (cs[end] - cs[pos]) / (n_all - n_back)
        upd = active & ~(mean_back == 0)
        new_t = (mean_back - mean_fore) / (torch.log(mean_back) - torch.log(mean_fore))
        t_next = torch.where(upd, new_t, t_next)
        calls = calls + upd.long()
        fail = upd & (calls > max_iter)
        failed |= fail
        active = upd & ~fail & ((t_next - t_curr).abs() > tol)
    li = torch.where(flat, vmin, t_next + vmin)

    thr = torch.where(li < yen, li, yen)                   # python min(tye, tli): tye unless tli is smaller
    converged = ~failed
    glob = float(torch.quantile(thr[converged], 0.5)) if bool(converged.any()) else float("nan")
    thr = torch.where(converged, thr, torch.full_like(thr, glob))
    return genes, thr, converged, glob


THRESHOLD_ROUTES = ("torch", "kernel")
THRESHOLDS_COUNTERS = ("n_assigned", "n_genes_present", "n_bad", "n_nan")


def _check_route(thresholds: str) -> None:
    if thresholds not in THRESHOLD_ROUTES:
        raise ValueError(f"thresholds must be one of {THRESHOLD_ROUTES}, got {thresholds!r}")


def gene_thresholds(similarity: Tensor, gene: Tensor, cell_encoding: Tensor, n_genes: Optional[int] = None,
                    max_iter: int = 250) -> Dict[str, Tensor]:
    """``per_gene_thresholds`` on the device (``segger_thresholds_build``, ``csrc/thresholds.hip``): ``min(Yen, Li)`` per
    gene over the rows with ``cell_encoding >= 0``, from one keys-only radix sort of ``(gene, similarity)`` -- 16 bytes of
    workspace per row plus the sort's storage, where the torch route keeps over 60.

    ``n_genes`` is the gene id domain (ids must fit int32); it defaults to ``max(gene) + 1`` (one more wait for the
    device).  Returns tensors on the device, dense over the gene ids, ``[n_genes]``:

    * ``threshold`` float64: ``min(yen, li)``, the median of the converged genes' thresholds for a gene whose Li iteration
      failed, NaN for a gene without an assigned row;
    * ``yen``, ``li`` float64: the two thresholds on their own (``li`` of a failed gene is its last iterate);
    * ``count`` int64: assigned rows of the gene; ``converged`` bool (true for a gene without a row);
    * ``global_threshold`` (a Python float, NaN when no gene has a threshold) and ``failed_genes`` int64, ascending.

    Every value is used: the reference's 10 M-per-gene subsampling is not reproduced.  The same bits from run to run and
    for any order of the rows.  Waits for the device once, to read the counters and the median (and once more when a
    gene failed, to list it); raises if an assigned row has a gene id outside ``[0, n_genes)`` or a NaN similarity
    (neither is ever used as an index)."""
    from . import _lib as L
    cols = [similarity, gene, cell_encoding]
    L.need_device("gene_thresholds", *cols, hint="per_gene_thresholds is the CPU form")
    dev = cols[0].device
    n = int(cols[0].numel())
    if any(int(t.numel()) != n for t in cols):
        raise ValueError("gene_thresholds: columns of different lengths")
    if n >= (1 << 31):
        raise ValueError("gene_thresholds: 2^31 rows or more")
    sim = similarity.detach().to(torch.float32).contiguous().view(-1)
    g32 = gene.detach().to(torch.int32).contiguous().view(-1)
    cell = cell_encoding.detach().view(-1)
    if cell.dtype != torch.int32:                            # only the sign is read: wider encodings must not wrap
        cell = (cell >= 0).to(torch.int32) - 1
    cell = cell.contiguous()
    if n_genes is None:
        n_genes = max(int(g32.max()) + 1, 1) if n else 1
    n_genes = int(n_genes)
    ws, ws_bytes = L.workspace("segger_thresholds_workspace_bytes", dev, n, n_genes)
    if not n:                                                # no row pointer and no workspace is looked at
        ws, ws_bytes = None, 0
    f64 = dict(dtype=torch.float64, device=dev)
    thr, yen, li = torch.empty(n_genes, **f64), torch.empty(n_genes, **f64), torch.empty(n_genes, **f64)
    count = torch.empty(n_genes, dtype=torch.int64, device=dev)
    conv = torch.empty(n_genes, dtype=torch.uint8, device=dev)
    counters = torch.zeros(len(THRESHOLDS_COUNTERS), dtype=torch.int64, device=dev)
    L.call("segger_thresholds_build", dev, L.ptr(sim) if n else None, L.ptr(g32) if n else None, L.ptr(cell) if n else None,
           n, n_genes, int(max_iter), thr.data_ptr(), yen.data_ptr(), li.data_ptr(), count.data_ptr(), conv.data_ptr(),
           counters.data_ptr(), L.ptr(ws), ws_bytes)
    del ws
    converged = conv.bool()
    # median of the converged present genes' thresholds and the back-fill: [n_genes] torch ops (plumbing)
    voted = converged & (count > 0)
    glob = torch.nanquantile(torch.where(voted, thr, torch.full_like(thr, float("nan"))), 0.5)
    glob = torch.where((voted & thr.isnan()).any(), torch.full_like(glob, float("nan")), glob)     # quantile: a NaN wins
    n_failed = (~converged).sum()
    stats = torch.cat([counters.double(), n_failed.double().view(1), glob.view(1)]).tolist()       # the one wait
    n_bad, n_nan, n_failed, glob_f = int(stats[2]), int(stats[3]), int(stats[4]), float(stats[5])
    if n_bad or n_nan:
        raise L.SeggerAmdError(f"gene_thresholds: {n_bad} assigned rows have a gene id outside [0, {n_genes}) and {n_nan} "
                               f"a NaN similarity; they took part in nothing")
    failed = (~converged).nonzero().squeeze(1) if n_failed else torch.empty(0, dtype=torch.int64, device=dev)
    return {"threshold": torch.where(converged, thr, glob), "yen": yen, "li": li, "count": count, "converged": converged,
            "global_threshold": glob_f, "failed_genes": failed}


def assign_transcripts_to_cells(predictions: Sequence[Sequence[Tensor]], device=None,
                                max_iter: int = 250, thresholds: str = "torch") -> Dict[str, Tensor]:
    """-> ``row_index`` (unique, ascending), ``cell_encoding`` (-1 = unassigned), ``similarity``, ``gene``,
    ``similarity_threshold`` (nan for genes without an assigned transcript), plus ``global_threshold`` and
    ``failed_genes``.  A transcript counts as segmented when ``similarity >= similarity_threshold``
    (``writer.py:96-99``).  ``thresholds="kernel"`` computes the per-gene thresholds with :func:`gene_thresholds`
    (device tensors only) instead of :func:`per_gene_thresholds`."""
    _check_route(thresholds)
    return _thresholds_and_join(best_assignment(predictions, device), max_iter, thresholds)


def _thresholds_and_join(out: Dict[str, Tensor], max_iter: int, thresholds: str = "torch") -> Dict[str, Tensor]:
    """The tail both entry points share: per-gene thresholds over the deduplicated rows, joined back by gene."""
    _check_route(thresholds)
    if thresholds == "kernel":                               # dense over the gene ids: the join is a gather
        res = gene_thresholds(out["similarity"], out["gene"], out["cell_encoding"], None, max_iter)
        out["similarity_threshold"] = res["threshold"][out["gene"].long()]
        out["global_threshold"] = res["global_threshold"]
        out["failed_genes"] = res["failed_genes"]
        return out
    genes, thr, converged, glob = per_gene_thresholds(out["similarity"], out["gene"], out["cell_encoding"] >= 0, max_iter)
    t = torch.full(out["gene"].shape, float("nan"), dtype=torch.float64, device=out["gene"].device)
    if genes.numel():
        j = torch.searchsorted(genes, out["gene"]).clamp_(max=genes.numel() - 1)
        hit = genes[j] == out["gene"]
        t = torch.where(hit, thr[j], t)
    out["similarity_threshold"] = t
    out["global_threshold"] = glob
    out["failed_genes"] = genes[~converged]
    return out


SEQ_LIMIT = 1 << 32          # sequence numbers (positions in the concatenation of everything fed) are 32 bits


class SegmentationAccumulator:
    """``best_assignment`` as a stream: ``update`` one batch of ``(tx_index, seg_idx, max_sim, gene_id)`` rows at a time,
    ``result()`` at the end.  The state is 16 bytes per transcript of the slide (a packed ``(similarity, arrival order)``
    key, the winning cell, its gene) whatever the number of rows or the tile overlap; ``update`` is two passes over the
    batch (``segger_assign_update``) that never wait for the device, on torch's current stream.

    The result equals ``best_assignment`` over the concatenation of the same batches in the same order -- and does not
    depend on the order or the chunking, bit for bit -- with three differences:

    * a winning similarity of -0.0 comes back as +0.0;
    * any winning NaN comes back as the canonical NaN (``0x7FC00000``; NaN wins, as in ``torch.sort``);
    * cell encodings must be < 2^31 (they are kept as int32).

    ``n_transcripts`` is the ``row_index`` domain: every ``tx_index`` must lie in ``[0, n_transcripts)``.  Rows outside
    it are never written anywhere; they are counted on the device and ``result()`` raises."""

    def __init__(self, n_transcripts: int, device="cuda"):
        from . import _lib
        n = int(n_transcripts)
        if not 1 <= n < (1 << 31):
            raise ValueError(f"n_transcripts must be in [1, 2^31), got {n}")
        self.device = torch.device(device)
        _lib.need_device("SegmentationAccumulator", self.device, hint="best_assignment is the CPU form")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _lib
        self.n_transcripts = n
        self.best_key = torch.zeros(n, dtype=torch.int64, device=self.device)       # uint64 bit patterns
        self.cell = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.gene = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.counters = torch.zeros(2, dtype=torch.int64, device=self.device)       # rows seen, rows dropped
        self.rows_fed = 0

    def reset(self) -> None:
        """Forget every row (enqueued like an update: no sync)."""
        self.best_key.zero_()
        self.counters.zero_()
        self.rows_fed = 0

    def _col(self, t: Tensor, dtype) -> Tensor:
        return t.detach().to(device=self.device, dtype=dtype).contiguous().view(-1)

    def update(self, tx_index: Tensor, seg_idx: Tensor, max_sim: Tensor, gene_id: Tensor, mask: Optional[Tensor] = None) -> None:
        """Feed one batch: CPU tensors (what ``predict_step`` returns) or device tensors of any integer / float dtype.
        ``mask`` (bool, optional) keeps the rows where it is true, as ``tensor[mask]`` would before the call -- but a
        masked-out row still takes a sequence number, which changes nothing in the result.  Enqueue only: device tensors
        of the right dtype (int64, int64, float32, int32, bool) are read in place, anything else is converted or copied
        to the device first.  (An update captured in a hipGraph is counted in ``rows_fed`` once, at capture; the 2^32 bound
        on replays is kept by the device, which drops and counts rows past it.)"""
        n = int(tx_index.numel())
        if not (int(seg_idx.numel()) == int(max_sim.numel()) == int(gene_id.numel()) == n) or (
                mask is not None and int(mask.numel()) != n):
            raise ValueError("SegmentationAccumulator.update: columns of different lengths")
        if self.rows_fed + n >= SEQ_LIMIT:
            raise OverflowError(f"SegmentationAccumulator: {self.rows_fed} + {n} rows reach 2^32 (32-bit sequence numbers)")
        if n == 0:
            return
        idx, seg = self._col(tx_index, torch.int64), self._col(seg_idx, torch.int64)
        sim, gene = self._col(max_sim, torch.float32), self._col(gene_id, torch.int32)
        m = None if mask is None else self._col(mask, torch.bool)
        L = self._lib
        L.call("segger_assign_update", self.device, idx.data_ptr(), seg.data_ptr(), sim.data_ptr(), gene.data_ptr(), L.ptr(m), n,
               self.best_key.data_ptr(), self.cell.data_ptr(), self.gene.data_ptr(), self.counters.data_ptr(), self.n_transcripts)
        self.rows_fed += n

    def result(self) -> Dict[str, Tensor]:
        """The dict ``best_assignment`` returns (``row_index`` ascending, ``cell_encoding``, ``similarity``, ``gene``), on
        the device.  The one place that waits for the device; raises if any row was dropped."""
        L = self._lib
        sim = torch.empty(self.n_transcripts, dtype=torch.float32, device=self.device)
        seen = torch.empty(self.n_transcripts, dtype=torch.bool, device=self.device)
        L.call("segger_assign_finalize", self.device, self.best_key.data_ptr(), self.n_transcripts, sim.data_ptr(),
               seen.data_ptr())
        rows, dropped = self.counters.tolist()
        if dropped:
            raise L.SeggerAmdError(f"SegmentationAccumulator: {dropped} of {rows} rows were dropped (tx_index outside "
                                   f"[0, {self.n_transcripts}), or more than 2^32 rows fed); nothing was written for them")
        row = seen.nonzero().squeeze(1)                      # the compaction to ascending row_index is plumbing
        return {"row_index": row, "cell_encoding": self.cell[row].long(), "similarity": sim[row], "gene": self.gene[row].long()}

    def segmentation(self, max_iter: int = 250, thresholds: str = "torch") -> Dict[str, Tensor]:
        """The dict ``assign_transcripts_to_cells`` returns, through the same thresholds-and-join tail
        (``thresholds="kernel"``: :func:`gene_thresholds`)."""
        _check_route(thresholds)
        return _thresholds_and_join(self.result(), max_iter, thresholds)

    def expression(self, xy: Optional[Tensor] = None, max_iter: int = 250, thresholds: str = "torch") -> Dict[str, Tensor]:
        """``expression_matrix(self.segmentation(max_iter, thresholds), xy)``: the count matrix of what has been fed so far."""
        return expression_matrix(self.segmentation(max_iter, thresholds), xy)

    def boundaries(self, xy: Tensor, max_iter: int = 250, thresholds: str = "torch", **kw) -> Dict[str, Tensor]:
        """``segmentation_boundaries(self.segmentation(max_iter, thresholds), xy, **kw)``: one boundary polygon per cell of
        what has been fed so far, from the transcripts :meth:`expression` counts (:mod:`segger_amd.boundaries`)."""
        from .boundaries import segmentation_boundaries
        return segmentation_boundaries(self.segmentation(max_iter, thresholds), xy, **kw)

    def outlines(self, xy: Tensor, max_iter: int = 250, thresholds: str = "torch", **kw) -> Dict[str, Tensor]:
        """``segmentation_outlines(self.segmentation(max_iter, thresholds), xy, **kw)``: the concave outline per cell, the
        reference's default ``method="delaunay"`` (:func:`segger_amd.boundaries.cell_outlines`; ``kw`` is its ``connectivity``,
        ``smoothing`` and ``large_cells``)."""
        from .boundaries import segmentation_outlines
        return segmentation_outlines(self.segmentation(max_iter, thresholds), xy, **kw)


EXPRESSION_COUNTERS = ("n_kept", "nnz", "n_cells_present", "n_genes_present", "n_bad")


def expression_matrix(result: Dict[str, Tensor], xy: Optional[Tensor] = None, n_cells: Optional[int] = None,
                      n_genes: Optional[int] = None) -> Dict[str, Tensor]:
    """The cell x gene count matrix of the segmented transcripts of ``result`` (what ``assign_transcripts_to_cells`` or
    ``SegmentationAccumulator.segmentation()`` returns), on the device (``segger_expression_build``).

    A transcript is counted iff ``cell_encoding >= 0`` and ``similarity >= similarity_threshold`` (NaN on either side:
    not counted; equality: counted).  ``xy`` is ``[n_transcripts_of_the_slide, 2]``, indexed by ``row_index``.
    ``n_cells`` / ``n_genes`` are the id domains; they default to ``max + 1`` of the columns (one more wait for the
    device).  Returns device tensors sliced to their real sizes:

    * ``cell_ids`` int32, ``gene_ids`` int32: ascending ids that own at least one counted transcript;
    * ``indptr`` int64, ``indices`` int32 (positions in ``gene_ids``, strictly ascending inside a row), ``counts`` int32:
      canonical CSR, what ``coo_matrix(...).tocsr()`` + ``sort_indices()`` gives;
    * ``mean_similarity`` float64 per stored entry, ``cell_count`` int64 per row;
    * ``centroid`` float64 ``[n_cells_present, 2]``, only when ``xy`` is given;
    * ``n_kept``: the number of counted transcripts (a Python int).

    Sums are float64 in an order fixed by the row positions: every output has the same bits from run to run and however
    the rows were fed.  Waits for the device exactly once, to read the five sizes; raises if a counted transcript has a
    cell or gene id outside its domain (it is never used as an index)."""
    from . import _lib as L
    cols = [result[k] for k in ("cell_encoding", "gene", "similarity", "similarity_threshold")]
    L.need_device("expression_matrix", *cols, hint="tests/expression_cases.py holds the CPU oracle")
    dev = cols[0].device
    n = int(cols[0].numel())
    if any(int(t.numel()) != n for t in cols):
        raise ValueError("expression_matrix: columns of different lengths")
    if n >= (1 << 31):
        raise ValueError("expression_matrix: 2^31 rows or more")
    cell = cols[0].detach().to(torch.int32).contiguous().view(-1)
    gene = cols[1].detach().to(torch.int32).contiguous().view(-1)
    sim = cols[2].detach().to(torch.float32).contiguous().view(-1)
    thr = cols[3].detach().to(torch.float64).contiguous().view(-1)
    pts = None
    if xy is not None:                                       # the gather by row_index is plumbing
        pts = xy.detach().to(device=dev, dtype=torch.float32)[result["row_index"].to(dev)].contiguous()
    if n_cells is None or n_genes is None:
        top = torch.stack([cell.max(), gene.max()]).tolist() if n else [-1, -1]          # one sync, like result()
        n_cells = max(int(top[0]) + 1, 1) if n_cells is None else n_cells
        n_genes = max(int(top[1]) + 1, 1) if n_genes is None else n_genes
    n_cells, n_genes = int(n_cells), int(n_genes)
    ws, ws_bytes = L.workspace("segger_expression_workspace_bytes", dev, n, n_cells, n_genes)
    cap_c, cap_g = min(n, n_cells), min(n, n_genes)
    i32 = dict(dtype=torch.int32, device=dev)
    cell_ids, gene_ids = torch.empty(cap_c, **i32), torch.empty(cap_g, **i32)
    indices, counts = torch.empty(n, **i32), torch.empty(n, **i32)
    indptr = torch.empty(cap_c + 1, dtype=torch.int64, device=dev) if n else torch.zeros(1, dtype=torch.int64, device=dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    cell_count = torch.empty(cap_c, dtype=torch.int64, device=dev)
    centroid = torch.empty(cap_c, 2, dtype=torch.float64, device=dev) if pts is not None else None
    counters = torch.zeros(len(EXPRESSION_COUNTERS), dtype=torch.int64, device=dev)
    L.call("segger_expression_build", dev, cell.data_ptr(), gene.data_ptr(), sim.data_ptr(), thr.data_ptr(), L.ptr(pts), n,
           n_cells, n_genes, cell_ids.data_ptr(), gene_ids.data_ptr(), indptr.data_ptr(), indices.data_ptr(),
           counts.data_ptr(), mean.data_ptr(), cell_count.data_ptr(), L.ptr(centroid), counters.data_ptr(), ws.data_ptr(),
           ws_bytes)
    n_kept, nnz, n_c, n_g, n_bad = counters.tolist()         # the one wait for the device
    if n_bad:
        raise L.SeggerAmdError(f"expression_matrix: {n_bad} segmented transcripts have a cell id outside [0, {n_cells}) or "
                               f"a gene id outside [0, {n_genes}); they were counted nowhere")
    out = {"cell_ids": cell_ids[:n_c], "gene_ids": gene_ids[:n_g], "indptr": indptr[:n_c + 1], "indices": indices[:nnz],
           "counts": counts[:nnz], "mean_similarity": mean[:nnz], "cell_count": cell_count[:n_c], "n_kept": n_kept}
    if centroid is not None:
        out["centroid"] = centroid[:n_c]
    return out


def expression_to_scipy(expr: Dict[str, Tensor], obs=None, cell_id: str = "cell_id", cell_encoding: str = "cell_encoding"):
    """-> ``(X, scores, obs_names, var_ids, X_spatial)``, the pieces ``AnnData(X=X, obs=..., var=..., layers={"scores":
    scores}, obsm={"X_spatial": X_spatial})`` takes: ``X`` the counts and ``scores`` the mean similarities as
    ``scipy.sparse.csr_matrix`` of one sparsity pattern (canonical: sorted, no duplicates), ``obs_names`` the cell ids
    looked up in ``obs[[cell_id, cell_encoding]]`` as :func:`to_frame` does (the encodings themselves when ``obs`` is
    None), ``var_ids`` the gene ids of the columns, ``X_spatial`` the centroids (None without ``xy``)."""
    import numpy as np
    import scipy.sparse as sp
    enc = expr["cell_ids"].cpu().numpy()
    var_ids = expr["gene_ids"].cpu().numpy()
    indptr, indices = expr["indptr"].cpu().numpy(), expr["indices"].cpu().numpy()
    shape = (enc.size, var_ids.size)
    X = sp.csr_matrix((expr["counts"].cpu().numpy(), indices, indptr), shape=shape)
    scores = sp.csr_matrix((expr["mean_similarity"].cpu().numpy(), indices.copy(), indptr.copy()), shape=shape)
    if obs is not None:
        import pandas as pd
        lut = pd.Series(obs[cell_id].to_numpy(), index=obs[cell_encoding].to_numpy().astype(np.int64))
        obs_names = lut.reindex(enc.astype(np.int64)).to_numpy()
    else:
        obs_names = enc
    X_spatial = expr["centroid"].cpu().numpy() if "centroid" in expr else None
    return X, scores, obs_names, var_ids, X_spatial


def to_frame(result: Dict[str, Tensor], obs=None, cell_id: str = "cell_id", cell_encoding: str = "cell_encoding"):
    """The columns of ``segger_segmentation.parquet`` as a pandas frame: ``row_index``, ``segger_cell_id``
    (from ``obs[[cell_id, cell_encoding]]``; the integer encoding itself when ``obs`` is None), ``segger_similarity``,
    ``similarity_threshold``."""
    import numpy as np
    import pandas as pd
    enc = result["cell_encoding"].cpu().numpy()
    if obs is not None:
        lut = pd.Series(obs[cell_id].to_numpy(), index=obs[cell_encoding].to_numpy().astype(np.int64))
        ids = lut.reindex(enc).to_numpy()
    else:
        ids = pd.array(np.where(enc >= 0, enc, 0), dtype="Int64")
        ids[enc < 0] = pd.NA
    return pd.DataFrame({
        "row_index": result["row_index"].cpu().numpy(),
        "segger_cell_id": ids,
        "segger_similarity": result["similarity"].cpu().numpy(),
        "similarity_threshold": result["similarity_threshold"].cpu().numpy(),
    })
