"""Label images from boundary polygons on the device: the transform opposite to :func:`segger_amd.contours.label_contours`.
A user who has run ``segmentation_outlines`` or ``segmentation_boundaries`` gets what the image-based world consumes -- a
label mask for napari or SpatialData ``labels``, a mask to compare with Cellpose or CosMx label images, pixel areas -- and
the CosMx intake closes into a round trip (image -> rings -> image).  This is ``segger_rasterize_rings``
(csrc/rasterize.hip; include/segger_amd.h has the contract).  There is no CPU path.

NO REFERENCE COUNTERPART EXISTS: the reference reads label images and never writes one, so the contract is this project's
own.  A pixel belongs to a polygon when its centre satisfies the predicate of :func:`segger_amd.geometry.points_in_polygons`
at distance 0 (both kernels compile csrc/ring_predicate.h, so the pixels of polygon ``p`` are, bit for bit, the pairs that
function lists for ``p`` over the pixel centres).  ``cv2.fillPoly`` and ``skimage.draw.polygon`` follow other pixel rules
and could not be run where this was written: UNPINNED against either.  What IS checked: equality with the numpy oracle of
tests/rasterize_cases.py, which asks the join's float64 and exact-rational predicate oracles.

NOT BUILT: holes and multi-part polygons; anti-aliased (fractional) coverage; TIFF writing; capture into a graph.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .rings import raise_ring_errors, ring_csr

__all__ = ["COUNTER_NAMES", "DEFAULT_BLOCK", "rasterize_rings"]

COUNTER_NAMES = ("n_pixels_set", "n_overlaps", "n_empty", "n_clipped", "n_degenerate", "n_large_tier", "n_blocks_filled")
DEFAULT_BLOCK = 8                # chosen by measurement: profiles/rasterize_pixels_per_s.json records 4, 8 and 16
_PREDICATES = {"contains": L.RASTER_CONTAINS, "intersects": L.RASTER_INTERSECTS}
_OVERLAPS = {"lowest": L.RASTER_LOWEST, "highest": L.RASTER_HIGHEST}
_ROUTES = {None: 64, "auto": 64, "large": 0}
_HINT = "tests/rasterize_cases.py holds the CPU oracle"


def _pair(who: str, name: str, value) -> Tuple[float, float]:
    try:
        vals = tuple(float(v) for v in (value.tolist() if isinstance(value, Tensor) else value))
    except (TypeError, ValueError):
        vals = ()
    if len(vals) != 2 or not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{who}: {name} is two finite numbers")
    return vals


def rasterize_rings(ring_offsets: Tensor, xy: Tensor, shape: Sequence[int], *, scale=(1.0, 1.0), translation=(0.0, 0.0),
                    labels: Optional[Tensor] = None, predicate: str = "intersects", overlap: str = "lowest",
                    _route: Optional[str] = None, _block: Optional[int] = None) -> Dict[str, Tensor]:
    """The ``[H, W]`` int32 label image of a CSR of rings (``ring_offsets`` ``[P + 1]``, ``xy`` ``[V, 2]`` on the device, as
    :func:`segger_amd.morphology.polygon_props` takes them: open or closed, either orientation, at most
    ``SEGGER_MORPH_MAX_VERTS`` vertices).

    ``shape = (H, W)`` with ``H * W < 2**31``.  ``scale = (sx, sy)`` and ``translation = (tx, ty)`` mean what they mean
    in :func:`segger_amd.contours.label_contours`: the pixel in row ``r``, column ``c`` stands for the world point
    ``(c * sx + tx, r * sy + ty)`` -- one multiplication and one addition in float64, not fused -- and that point is tested
    against the ring as given.  ``sx`` and ``sy`` are finite and non-zero; negative values are allowed (the reference's
    frame is ``(1, -1)``).  ``labels`` is an int32 ``[P]`` tensor of values ``>= 1`` (default: polygon index + 1).

    ``predicate``: ``"intersects"`` (default) is the closed set -- a pixel centre on the ring belongs to it -- which makes
    the ``label_contours`` round trip exact, because contour vertices are pixel centres; ``"contains"`` is the open set.
    ``overlap``: a pixel matched by several polygons goes to the ``"lowest"`` or the ``"highest"`` polygon INDEX, never
    the label value.  A ring of fewer than 3 vertices (after a closing duplicate is dropped) matches nothing.

    Returns a dict of device tensors; every one but the two counters named below is the same bytes for any ``_block``, any
    ``_route`` and any run:

    * ``image`` int32 ``[H, W]``, 0 the background;
    * ``n_covered`` int64 ``[P]``: the pixels of the image the polygon matches, before overlaps are resolved;
    * ``n_won`` int64 ``[P]``: the pixels the polygon holds in ``image``;
    * ``counters`` int64, named by ``COUNTER_NAMES``: ``n_pixels_set``, ``n_overlaps`` (``sum n_covered - n_pixels_set``),
      ``n_empty`` (polygons matching no pixel, degenerate ones included), ``n_clipped`` (polygons of 3 or more vertices
      whose bounds leave the closed rectangle of the pixel centres), ``n_degenerate``, ``n_large_tier`` (polygons walked
      with the ring in LDS; depends on ``_route``) and ``n_blocks_filled`` (blocks filled whole; depends on ``_block``).

    ``_block`` (tests and timing only): the side of the pixel blocks that are filled or skipped whole when their centre is
    far from the ring, a power of two up to ``SEGGER_RASTER_MAX_BLOCK``; 1 evaluates every pixel of a polygon's range.
    ``_route`` (tests and timing only): ``"large"`` sends every ring through the 4096-vertex LDS tier.

    Raises ``ValueError`` for bad shapes, dtypes or options before anything is launched, and afterwards for a ring above
    the cap (naming the polygon), offsets the device found out of range, a non-finite vertex or a label below 1;
    ``SeggerAmdError`` for CPU tensors.  No polygons gives the all-background image and launches nothing.  Waits for the
    device twice: the longest ring (the shared ring validation) and the error word, after which the counters are complete."""
    who = "rasterize_rings"
    if predicate not in _PREDICATES:
        raise ValueError(f"{who}: predicate {predicate!r} is neither 'contains' nor 'intersects'")
    if overlap not in _OVERLAPS:
        raise ValueError(f"{who}: overlap {overlap!r} is neither 'lowest' nor 'highest'")
    try:
        reg_max = _ROUTES[_route]
    except (KeyError, TypeError):
        raise ValueError(f"{who}: _route is None, 'auto' or 'large', got {_route!r}") from None
    block = DEFAULT_BLOCK if _block is None else _block
    if isinstance(block, bool) or not isinstance(block, int) or not 1 <= block <= L.RASTER_MAX_BLOCK or block & (block - 1):
        raise ValueError(f"{who}: _block is a power of two in 1 .. {L.RASTER_MAX_BLOCK}, got {_block!r}")
    try:
        dims = tuple(shape)
    except TypeError:
        dims = ()
    if len(dims) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in dims) or min(dims) < 1 or \
            dims[0] * dims[1] >= 2 ** 31:
        raise ValueError(f"{who}: shape is (H, W), two ints >= 1 with H * W < 2^31")
    height, width = dims
    sx, sy = _pair(who, "scale", scale)
    tx, ty = _pair(who, "translation", translation)
    if sx == 0.0 or sy == 0.0:
        raise ValueError(f"{who}: scale must be non-zero")
    ring_offsets, xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    if labels is not None:
        if not isinstance(labels, Tensor) or labels.dtype != torch.int32 or labels.dim() != 1 or labels.numel() != n_polygons:
            raise ValueError(f"{who}: labels is an int32 [n_polygons] tensor ({n_polygons} polygons) or None")
        if labels.device != xy.device:
            raise ValueError(f"{who}: labels and the rings are on different devices")
        labels = labels.detach().contiguous()
    L.need_device(who, ring_offsets, xy, labels, hint=_HINT)
    dev = xy.device
    i64 = dict(dtype=torch.int64, device=dev)
    if n_polygons == 0:
        return {"image": torch.zeros(height, width, dtype=torch.int32, device=dev), "n_covered": torch.zeros(0, **i64),
                "n_won": torch.zeros(0, **i64), "counters": torch.zeros(len(COUNTER_NAMES), **i64)}
    image = torch.empty(height, width, dtype=torch.int32, device=dev)
    n_covered, n_won = torch.empty(n_polygons, **i64), torch.empty(n_polygons, **i64)
    counters = torch.empty(len(COUNTER_NAMES), **i64)
    ws, ws_bytes = L.workspace("segger_rasterize_workspace_bytes", dev, n_polygons)
    L.call("segger_rasterize_rings", dev, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, L.ptr(labels), height,
           width, sx, sy, tx, ty, _PREDICATES[predicate], _OVERLAPS[overlap], block, reg_max, image.data_ptr(),
           n_covered.data_ptr(), n_won.data_ptr(), counters.data_ptr(), ws.data_ptr(), ws_bytes)
    # the second and last wait (ring_csr made the first): the error word; the finiteness of the vertices and the smallest
    # label ride along
    checks = torch.stack([ws[:4].view(torch.int32)[0].to(torch.int64), xy.isfinite().all().to(torch.int64),
                          labels.min().to(torch.int64) if labels is not None else torch.ones((), **i64)]).tolist()
    raise_ring_errors(who, checks[0], ring_offsets, n_vertices)
    if not checks[1]:
        raise ValueError(f"{who}: xy holds a non-finite coordinate")
    if checks[2] < 1:
        raise ValueError(f"{who}: labels must be >= 1 (0 is the background), got {checks[2]}")
    return {"image": image, "n_covered": n_covered, "n_won": n_won, "counters": counters}
