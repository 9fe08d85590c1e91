"""Polygon overlap join on the device: which polygons of one ring CSR meet which of another, and by how much.

The reference's ``segger.geometry`` exports two joins; ``points_in_polygons`` is :func:`segger_amd.points_in_polygons`,
and ``polygons_in_polygons`` (``src/segger/geometry/query.py:244-285``, a CPU ``gpd.sjoin``, called from
``data/tiling.py:134``) is :func:`polygons_in_polygons` here.  :func:`polygon_overlaps` also sizes every intersection, and
:func:`match_polygons` turns that into the comparison a user makes first with a segmentation: which vendor cell each outline
corresponds to and how well the two agree (IoU / Jaccard per cell).  The intake's two polygon-against-polygon problems --
CosMx's "cell mask A overlaps with nuclear mask for cell B" (``io/cosmx.py:16-18``) and Xenium's nucleus as the
intersection of its cell and nucleus polygons (``io/preprocessor.py:493-495``) -- are detected and sized by the same join.
The kernels are csrc/polygon_overlap.hip; include/segger_amd.h has the contract and DESIGN 3.5n the reasoning.

The contract.  Polygons are single exterior rings, as everywhere else in the project: either orientation, a closing
duplicate of the first vertex dropped bit for bit, rings above ``SEGGER_MORPH_MAX_VERTS`` refused (naming the set and the
polygon), a ring with fewer than 3 open vertices pairs with nothing.

* **Intersection area**, measure-theoretically, so that shared edges, collinear overlaps, nesting and self-overlap need no
  special cases.  For ring ``A`` with orientation sign ``sA`` (the sign of its shoelace area) and an edge ``e = (p -> q)`` with
  ``p.x != q.x`` let ``sigma_e = sA * sign(p.x - q.x)``.  With a baseline ``y0`` not above any vertex of the pair,
  ``1_A(x, y) = sum_e sigma_e [x in the half-open x-range of e] [y0 <= y < y_e(x)]`` almost everywhere (vertical edges
  contribute nothing), hence ``area(A & B) = sum_{e in A} sum_{f in B} sigma_e sigma_f I(e, f)`` with ``I(e, f)`` the integral
  of ``min(y_e(x), y_f(x)) - y0`` over the overlap of the two x-ranges: one trapezoid, or two split at the single crossing
  of the two lines.  float64, FMA contraction off, both rings translated to the first vertex of ring ``A`` before any
  product, ``y0`` the lowest translated ``y`` of the pair, the result clamped into ``[0, min(area_a, area_b)]``.  Within
  ``2^-52 (T S + 16 T W H)`` of the exact value (``T`` non-zero terms of summed magnitude ``S``, ``W x H`` the pair's extent).
* **intersects(A, B)**: the closed polygons share a point -- some edge of ``A`` and some edge of ``B`` share a point (closed
  segments: ``rings_simple``'s touch without its shared-endpoint exemption), or vertex 0 of ``A`` is inside ``B`` by
  ``points_in_polygons``' half-open parity rule, or vertex 0 of ``B`` is inside ``A``.  Exact for integer coordinates below
  ``2^25`` in magnitude, as the project's other predicates are.  This is the reference's ``predicate='intersects'``.

CHECKED: tests/overlap_cases.py holds the formula in exact rationals, an independent exact clipping oracle
(Sutherland-Hodgman for a convex ``B``), the exact integer predicate and brute-force bounding-box pairs.

UNPINNED: neither shapely nor GEOS could be imported where this was written and the reference was never run: what GEOS's
``intersects`` answers for invalid (self-touching, self-crossing) rings is not known here.

NOT BUILT: ``predicate='contains'`` (deciding it exactly needs the sub-segments of a query edge between boundary touches,
and the reference never reaches it with polygons), the intersection polygon itself (the Xenium nucleus clip is sized, not
constructed), holes, multi-part polygons."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib as L
from .rings import raise_ring_errors, ring_csr

__all__ = ["polygon_overlaps", "polygons_in_polygons", "match_polygons", "COUNTER_NAMES"]

COUNTER_NAMES = ("n_candidates", "n_intersecting", "n_lds_pairs", "n_wide")
_ROUTES = {None: (64, L.OVERLAP_SMALL_VERTS), "auto": (64, L.OVERLAP_SMALL_VERTS), "large": (0, 0)}
_WORD_FLAG_A, _WORD_WIDE_A, _WORD_FLAG_B, _WORD_WIDE_B, _WORD_LDS_PAIRS = 0, 2, 8, 10, 16       # csrc/polygon_overlap.hip


def _empty(dev, area_a: Tensor, area_b: Tensor) -> Dict[str, Tensor]:
    return {"pairs": torch.empty(2, 0, dtype=torch.int64, device=dev), "area": torch.empty(0, dtype=torch.float64, device=dev),
            "area_a": area_a, "area_b": area_b, "counters": torch.zeros(len(COUNTER_NAMES), dtype=torch.int64, device=dev)}


def _areas(who: str, ring_offsets: Tensor, xy: Tensor, n_polygons: int, n_vertices: int) -> Tensor:
    """``polygon_props``' areas of a CSR that ``ring_csr`` has passed, without its waits: the offsets the device finds out
    of range are the ones the overlap kernels report in their own word."""
    props = torch.empty(n_polygons, L.MORPH_COLS, dtype=torch.float64, device=xy.device)
    if n_polygons > 0:
        ws, ws_bytes = L.workspace("segger_morphology_workspace_bytes", xy.device, n_polygons)
        L.call("segger_polygon_props", xy.device, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, props.data_ptr(),
               ws.data_ptr(), ws_bytes)
    return props[:, 0].contiguous()


def polygon_overlaps(ring_offsets_a: Tensor, xy_a: Tensor, ring_offsets_b: Tensor, xy_b: Tensor, *, cells_per_polygon: float = 1.0,
                     _route: Optional[str] = None) -> Dict[str, Tensor]:
    """Every pair of a polygon of set ``A`` and a polygon of set ``B`` that intersect, with the area of the intersection.

    Both sets are ring CSRs on the device as ``polygon_props`` takes them (``ring_offsets`` ``[P + 1]``, ``xy`` ``[V, 2]``).

    Returns a dict of device tensors: ``pairs`` int64 ``[2, E]``, every intersecting ``(a, b)`` sorted by ``(a, b)``; ``area``
    float64 ``[E]``, the area of each intersection (the module docstring defines it and the predicate; a pair that only
    touches has area 0); ``area_a`` ``[Pa]`` and ``area_b`` ``[Pb]``, ``polygon_props``' areas; ``counters`` int64
    (:data:`COUNTER_NAMES`: pairs whose closed bounding boxes overlap, intersecting pairs, candidate pairs evaluated on an
    LDS tier -- a ring above 64 vertices --, polygons on the wide list).

    The same bytes from call to call, for any order of the polygons within either set (ids mapped back) and for any
    ``cells_per_polygon``: the uniform grid that finds the candidate pairs -- about ``cells_per_polygon * max(Pa, Pb)`` cells
    over the union extent; a polygon whose box covers more than ``SEGGER_OVERLAP_WIDE_CELLS`` of them is tested against the
    whole other set instead -- decides the speed and nothing else.  Only the last counter depends on it.

    ``_route`` (tests and timing only): ``"large"`` sends every pair through the 4096-vertex LDS tier; the bytes are the same.

    Waits for the device five times: the longest ring of each set, the extents together with the finiteness check, the
    candidate total (it sizes three arrays), and the workspace's words (errors and counters).  An empty set on either side
    returns ``[2, 0]`` and launches nothing.  Raises ``ValueError`` for bad shapes, dtypes or devices, non-finite
    coordinates, a ring above ``SEGGER_MORPH_MAX_VERTS`` (naming the set and the polygon) or offsets the device found out of
    range, and ``SeggerAmdError`` for CPU tensors: there is no CPU fallback."""
    who = "polygon_overlaps"
    try:
        reg_max, small_max = _ROUTES[_route]
    except (KeyError, TypeError):
        raise ValueError(f"{who}: _route is None, 'auto' or 'large', got {_route!r}") from None
    if isinstance(cells_per_polygon, bool) or not isinstance(cells_per_polygon, (int, float)) or not (
            cells_per_polygon > 0 and math.isfinite(cells_per_polygon)):
        raise ValueError(f"{who}: cells_per_polygon must be positive and finite")
    off_a, xy_a, n_a, v_a = ring_csr(f"{who}: set A", ring_offsets_a, xy_a)
    off_b, xy_b, n_b, v_b = ring_csr(f"{who}: set B", ring_offsets_b, xy_b)
    if xy_a.device != xy_b.device:
        raise ValueError(f"{who}: the two sets are on different devices")
    L.need_device(who, off_a, xy_a, off_b, xy_b, hint="tests/overlap_cases.py holds the CPU oracles")
    dev = xy_a.device
    for name, off, n_v in (("A", off_a, v_a), ("B", off_b, v_b)):
        if n_v == 0 and off.numel() > 1 and bool((off != 0).any()):
            raise ValueError(f"{who}: set {name}: ring_offsets of polygon {int((off[1:] != 0).nonzero()[0])} are negative, "
                             f"descending or beyond the 0 vertices")
    if n_a == 0 or n_b == 0 or v_a == 0 or v_b == 0:
        nan_a, nan_b = (torch.full((n,), math.nan, dtype=torch.float64, device=dev) for n in (n_a, n_b))
        return _empty(dev, nan_a if v_a == 0 else _areas(who, off_a, xy_a, n_a, v_a), nan_b if v_b == 0 else _areas(who, off_b, xy_b, n_b, v_b))

    # one synchronisation: both extents; a NaN anywhere is a NaN in its minimum and maximum, an infinity is one of the two
    ext = torch.cat([xy_a.min(0).values, xy_a.max(0).values, xy_b.min(0).values, xy_b.max(0).values]).tolist()
    for name, e in (("A", ext[:4]), ("B", ext[4:])):
        if not all(math.isfinite(v) for v in e):
            raise ValueError(f"{who}: set {name}: xy holds a non-finite coordinate")
    x0, y0 = min(ext[0], ext[4]), min(ext[1], ext[5])
    w, h = max(max(ext[2], ext[6]) - x0, 1e-6), max(max(ext[3], ext[7]) - y0, 1e-6)
    cell = math.sqrt(w * h / (cells_per_polygon * max(n_a, n_b)))
    cell = max(cell, math.sqrt(w * h / (64.0 * max(n_a, n_b))), max(w, h) / 30000.0)   # <= 64 cells a polygon, < 2^31 cells
    nx, ny = int(w / cell) + 1, int(h / cell) + 1

    area_a, area_b = _areas(who, off_a, xy_a, n_a, v_a), _areas(who, off_b, xy_b, n_b, v_b)
    ws, ws_bytes = L.workspace("segger_polygon_overlap_workspace_bytes", dev, n_a, n_b, nx, ny)
    total_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    args = (off_a.data_ptr(), xy_a.data_ptr(), n_a, v_a, off_b.data_ptr(), xy_b.data_ptr(), n_b, v_b, x0, y0, cell, nx, ny)
    L.call("segger_polygon_overlap_candidates", dev, *args, total_dev.data_ptr(), ws.data_ptr(), ws_bytes)
    total = int(total_dev)                                           # the wait that sizes the result
    cand = torch.empty(total, dtype=torch.int64, device=dev)
    hit = torch.empty(total, dtype=torch.uint8, device=dev)
    area = torch.empty(total, dtype=torch.float64, device=dev)
    if total > 0:
        L.call("segger_polygon_overlap_pairs", dev, *args, area_a.data_ptr(), area_b.data_ptr(), total_dev.data_ptr(), cand.data_ptr(),
               hit.data_ptr(), area.data_ptr(), total, reg_max, small_max, ws.data_ptr(), ws_bytes)
    words = ws[:256].view(torch.int32).tolist()                      # the last wait: both error words, the counters
    raise_ring_errors(f"{who}: set A", words[_WORD_FLAG_A], off_a, v_a)
    raise_ring_errors(f"{who}: set B", words[_WORD_FLAG_B], off_b, v_b)
    keep = hit.bool()
    keys, order = torch.sort(cand[keep])                             # the keys are distinct: one order
    counters = torch.tensor([total, int(keys.numel()), words[_WORD_LDS_PAIRS], words[_WORD_WIDE_A] + words[_WORD_WIDE_B]],
                            dtype=torch.int64, device=dev)
    return {"pairs": torch.stack([keys >> 32, keys & 0xffffffff]), "area": area[keep][order], "area_a": area_a, "area_b": area_b,
            "counters": counters}


def polygons_in_polygons(query_offsets: Tensor, query_xy: Tensor, index_offsets: Tensor, index_xy: Tensor,
                         predicate: str = "intersects") -> Tensor:
    """The reference's ``polygons_in_polygons(query_polygons, index_polygons, predicate)``: an int64 ``[2, E]`` device tensor,
    row 0 ``index_query`` and row 1 ``index_match``, every (query polygon, index polygon) pair whose closed polygons share a
    point, sorted by (query, match).  Both sets are ring CSRs; it is ``polygon_overlaps(...)["pairs"]`` and raises as that does.
    ``predicate='contains'`` is not built and raises ``ValueError``."""
    who = "polygons_in_polygons"
    if predicate == "contains":
        raise ValueError(f"{who}: predicate 'contains' is not built: deciding it exactly needs the sub-segments of a query edge "
                         f"between boundary touches, and the reference never reaches it with polygons; use 'intersects'")
    if predicate != "intersects":
        raise ValueError(f"{who}: predicate {predicate!r} is neither 'contains' nor 'intersects'")
    return polygon_overlaps(query_offsets, query_xy, index_offsets, index_xy)["pairs"]


def match_polygons(overlaps: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """The segmentation-against-vendor comparison from :func:`polygon_overlaps`' result: plain torch on the sparse triplets.

    Returns ``iou`` ``[E]`` = ``area / (area_a + area_b - area)`` per pair, and for each polygon of ``A`` ``best_b`` int64
    (``-1`` where nothing intersects), ``best_iou`` float64 (0 there) and ``n_overlapping`` int64; ``best_a``, ``best_iou_b``
    and ``n_overlapping_b`` likewise for each polygon of ``B``.  Ties in IoU go to the lowest id.  Deterministic: stable
    sorts only.  Two rings of zero area that touch give ``nan``."""
    pairs, area, area_a, area_b = (overlaps[k] for k in ("pairs", "area", "area_a", "area_b"))
    if pairs.dim() != 2 or pairs.shape[0] != 2 or area.shape != (pairs.shape[1],):
        raise ValueError("match_polygons: overlaps is the dict polygon_overlaps returns")
    a, b = pairs[0], pairs[1]
    iou = area / (area_a[a] + area_b[b] - area)
    out = {"iou": iou}
    by_iou = torch.sort(iou, descending=True, stable=True).indices   # within equal IoU the (a, b) order stays
    for own, other, n, names in ((a, b, area_a.numel(), ("best_b", "best_iou", "n_overlapping")),
                                 (b, a, area_b.numel(), ("best_a", "best_iou_b", "n_overlapping_b"))):
        order = by_iou[torch.sort(own[by_iou], stable=True).indices]  # by own id, then IoU descending, then the other id
        ids = own[order]
        first = torch.ones_like(ids, dtype=torch.bool)
        first[1:] = ids[1:] != ids[:-1]
        best = torch.full((n,), -1, dtype=torch.int64, device=pairs.device)
        best_iou = torch.zeros(n, dtype=torch.float64, device=pairs.device)
        best[ids[first]] = other[order][first]
        best_iou[ids[first]] = iou[order][first]
        out[names[0]], out[names[1]], out[names[2]] = best, best_iou, torch.bincount(own, minlength=n)
    return out
